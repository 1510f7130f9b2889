"""The distribution losses on the host (no GPU): the sort-based restatement (tests/_ddl_ref.py) against the reference's own outputs
(tests/golden/ddl.npz, recipe tests/golden/make_golden_ddl.py), the one-pass formulation the kernels of csrc/ddl.hip use against the
sort-based one bit for bit, get_x against the reference's draws, the exported symbols and the refusals."""
import ctypes
import os

import numpy as np
import pytest
import torch

from pnnp_amd import _lib, losses, ops
from tests import _ddl_ref as R

CASES = ['normal', 'distinct', 'ties', 'inside']
SEED = 20240611


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'ddl.npz'))


@pytest.mark.parametrize('case', CASES)
def test_restatement_reproduces_the_reference(golden, case):
    g = golden
    o, t, x = (torch.from_numpy(g[f'{case}_{k}']) for k in ('out', 'gt', 'x'))
    assert np.array_equal(R.ecdf(o, x).numpy().view(np.uint32), g[case + '_cdf_out'].view(np.uint32))
    assert np.array_equal(R.ecdf(t, x).numpy().view(np.uint32), g[case + '_cdf_gt'].view(np.uint32))
    for kind, key in (('cdf', 'cdfloss'), ('kld', 'kld')):
        a, b = o.clone().requires_grad_(True), t.clone().requires_grad_(True)
        loss = R.LOSSES[kind](a, b, x)
        loss.backward()
        # the same ATen operations on the same numbers: as stored
        assert np.float32(loss.item()) == g[f'{case}_{key}'], (kind, loss.item(), g[f'{case}_{key}'])
        assert np.array_equal(a.grad.numpy(), g[f'{case}_g{kind}_out']) and np.array_equal(b.grad.numpy(), g[f'{case}_g{kind}_gt'])


@pytest.mark.parametrize('case', CASES)
def test_one_pass_equals_sort_based_bit_for_bit(golden, case):
    for which in ('out', 'gt'):
        d, x = golden[f'{case}_{which}'], golden[case + '_x']
        cdf, arg_hi, arg_lo, amin, amax = R.ecdf_one_pass(d, x)
        assert np.array_equal(cdf.view(np.uint32), golden[f'{case}_cdf_{which}'].view(np.uint32))
        xc = np.clip(x, d.min(), d.max())
        assert np.all(d[arg_hi] >= xc) and np.all((arg_lo < 0) | (d[np.maximum(arg_lo, 0)] < xc))
        assert d[amin] == d.min() and d[amax] == d.max()


@pytest.mark.parametrize('case', ['distinct', 'inside', 'ties'])
def test_one_pass_gradient_equals_autograd(golden, case):
    """sum_k g[k] cdf[k]: the scattered closed form against autograd through sort / searchsorted / gather / clamp.  With ties autograd
    and the one-pass rule choose different elements of a run of equal values: compare the sums per distinct value."""
    d, x = golden[case + '_out'], golden[case + '_x']
    g = np.random.default_rng(3).normal(size=x.size).astype(np.float32)
    a = torch.from_numpy(d).clone().requires_grad_(True)
    (R.ecdf(a, torch.from_numpy(x)) * torch.from_numpy(g)).sum().backward()
    ref, got = a.grad.numpy().astype(np.float64), R.ecdf_grad_one_pass(d, x, g).astype(np.float64)
    _, inv = np.unique(d, return_inverse=True)
    ref, got = np.bincount(inv, ref), np.bincount(inv, got)
    assert np.abs(ref).max() > 0
    assert np.abs(got - ref).max() <= 2.0 ** -20 * np.abs(ref).max(), np.abs(got - ref).max() / np.abs(ref).max()


def test_get_x_draws_like_the_reference(golden):
    for mode in ('uniform', 'cdf', 'icdf'):
        torch.manual_seed(SEED)
        x = losses.get_x(size=1000, mode=mode)
        assert x.dtype == torch.float32 and not x.is_cuda
        assert np.array_equal(x.numpy(), golden['getx_' + mode]), mode
    torch.manual_seed(SEED)
    assert np.array_equal(losses.get_x(3, 64, 'icdf').numpy(), golden['getx_small'])
    assert np.array_equal(losses.get_x(mode='cdf', random=False).numpy(), np.sort(losses.get_x(mode='cdf', random=False).numpy()))


def test_header_symbols_and_abi_version():
    lib = _lib.lib()
    assert lib.pnnp_abi_version() == 9 == ops.ABI_VERSION
    for name in ('pnnp_ddl_ws_bytes', 'pnnp_ecdf_f32', 'pnnp_ecdf_bwd_f32', 'pnnp_cdf_loss_f32', 'pnnp_kld_loss_f32'):
        assert hasattr(lib, name), name
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'pnnp_hip.h')).read()
    assert '#define PNNP_DDL_MAX_K 4096' in hdr and '#define PNNP_ABI_VERSION 9' in hdr
    assert losses.MAX_K == 4096


def test_entry_limits_before_any_launch():
    """Sizes outside the limits: -2, decided on the host, so this runs without a device."""
    lib = _lib.lib()
    fake = ctypes.c_void_p(4096)
    i64 = ctypes.c_int64
    lib.pnnp_ddl_ws_bytes.restype = ctypes.c_int64
    assert lib.pnnp_ddl_ws_bytes(2, 4096) >= 2 * 4097 * 20
    assert lib.pnnp_ddl_ws_bytes(1, 4097) == -2 and lib.pnnp_ddl_ws_bytes(3, 64) == -1 and lib.pnnp_ddl_ws_bytes(1, 0) == -1
    e, b, c, k = lib.pnnp_ecdf_f32, lib.pnnp_ecdf_bwd_f32, lib.pnnp_cdf_loss_f32, lib.pnnp_kld_loss_f32
    assert e(fake, i64(1024), fake, 4097, fake, fake, fake, None) == -2
    assert e(fake, i64(1024), fake, 0, fake, fake, fake, None) == -2
    assert e(fake, i64(1), fake, 64, fake, fake, fake, None) == -2
    assert e(fake, i64(1 << 31), fake, 64, fake, fake, fake, None) == -2
    assert e(None, i64(1024), fake, 64, fake, fake, fake, None) == -1
    assert b(fake, i64(1024), fake, 4097, fake, fake, None, fake, None) == -2
    assert b(fake, i64(1), fake, 64, fake, fake, None, fake, None) == -2
    assert c(fake, i64(1024), fake, i64(1 << 31), fake, 64, fake, fake, fake, fake, fake, None) == -2
    assert c(fake, i64(1024), fake, i64(512), fake, 4097, fake, fake, fake, fake, fake, None) == -2
    assert k(fake, i64(1024), fake, i64(512), fake, 1, fake, fake, fake, fake, fake, None) == -2
    assert k(fake, i64(1024), fake, i64(512), fake, 64, fake, None, fake, fake, fake, None) == -1


def test_refusals_without_a_gpu():
    d, x = torch.zeros(64), torch.linspace(0, 1, 8)
    with pytest.raises(_lib.PnnpError, match='CPU tensor'):
        losses.CDFPPF(d)
    with pytest.raises(_lib.PnnpError, match='CPU tensor'):
        losses.CDFLoss(d, d, x)
    with pytest.raises(_lib.PnnpError, match='CPU tensor'):
        losses.KLD(d, d, x)
    with pytest.raises(_lib.PnnpError, match='CPU tensor'):
        losses.cdf2pdf(x)
    from pnnp_amd.trainer import NoiseFlowFitStep
    assert callable(NoiseFlowFitStep.ddl)

"""QuantileLoss on the host (no GPU): the sort-based restatement (tests/_quantile_ref.py) against the reference's own outputs
(tests/golden/quantile.npz, recipe tests/golden/make_golden_quantile.py), the exported symbols and the refusals.

The band of a value: BAND = 4 * 2^-24 * max(|s_lo|, |s_hi|) -- the reference's lerp and the unfused formula are each at most three float32
roundings of that magnitude away from the exact interpolation."""
import ctypes
import os

import numpy as np
import pytest
import torch

from pnnp_amd import _lib, losses, ops
from tests import _quantile_ref as R

CASES = ['normal', 'edges', 'ties', 'rows', 'tiny1', 'tiny2', 'tiny3']
TIE_FREE = ['normal', 'edges', 'rows', 'tiny1', 'tiny2', 'tiny3']


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'quantile.npz'))


def rows_of(a):
    return a.reshape(-1, a.shape[-1])


@pytest.mark.parametrize('case', CASES)
def test_ranks_and_weights_are_exact(golden, case):
    """floor, ceil and fraction of the reference's own float32 product q * (N - 1)"""
    q = golden[case + '_q']
    for which in ('out', 'gt'):
        n = golden[f'{case}_{which}'].shape[-1]
        pos = golden[f'{case}_pos_{which}']
        lo, hi, w = R.ranks(q, n)
        assert np.array_equal(lo, np.floor(pos).astype(np.int64)) and np.array_equal(hi, np.ceil(pos).astype(np.int64)), (case, which)
        assert np.array_equal(w.view(np.uint32), (pos - np.floor(pos)).astype(np.float32).view(np.uint32)), (case, which)
        assert lo.min() >= 0 and hi.max() <= n - 1


@pytest.mark.parametrize('case', CASES)
def test_restatement_reproduces_the_reference(golden, case):
    q = golden[case + '_q']
    vals = {}
    for which in ('out', 'gt'):
        d = golden[f'{case}_{which}']
        want = golden[f'{case}_q_{which}']
        got = R.quantile(torch.from_numpy(d), torch.from_numpy(q)).numpy()
        assert got.shape == want.shape, (case, which)
        vals[which] = got
        for r, row in enumerate(rows_of(d)):
            a, b, alo, ahi, w = R.order_stats(row, q)
            assert np.array_equal(row[alo], a) and np.array_equal(row[ahi], b)
            band = 4 * 2.0 ** -24 * np.maximum(np.abs(a), np.abs(b)).astype(np.float64)
            g, t = got.reshape(q.size, -1)[:, r], want.reshape(q.size, -1)[:, r]
            assert np.array_equal(g, R.value_from(a, b, w))
            exact = R.value_from(a, b, w, np.float64)
            print(case, which, r, 'bit-equal to the reference:', int((g == t).sum()), 'of', q.size)
            assert np.all(np.abs(g.astype(np.float64) - t) <= band) and np.all(np.abs(g - exact) <= band) and np.all(np.abs(t - exact) <= band)
    loss = np.abs(vals['out'].astype(np.float64) - vals['gt']).mean()
    assert abs(float(R.quantile_loss(torch.from_numpy(golden[case + '_out']), torch.from_numpy(golden[case + '_gt']), torch.from_numpy(q)))
               - golden[case + '_loss']) <= 2.0 ** -20 * max(loss, 1e-30)
    assert abs(loss - golden[case + '_loss']) <= 2.0 ** -20 * max(loss, 1e-30)


@pytest.mark.parametrize('case', TIE_FREE)
def test_gradient_rule_on_tie_free_data(golden, case):
    """sum g value: the scattered rule against the reference's autograd -- the same elements, the same values"""
    q, g = golden[case + '_q'], golden[case + '_g'].reshape(golden[case + '_q'].size, -1)
    d, want = rows_of(golden[case + '_out']), rows_of(golden[case + '_gq_out'])
    for r in range(d.shape[0]):
        got = R.grad_rule(d[r], q, g[:, r])
        lo, hi, w = R.ranks(q, d.shape[1])
        # (an entry with weight 0 leaves an exact zero in both)
        assert np.array_equal(np.nonzero(got)[0], np.nonzero(want[r])[0]), (case, r)
        assert np.abs(got - want[r]).max() <= 2.0 ** -20 * np.abs(want[r]).max()
    # the loss's own gradient: sign / (K R) scattered by the same rule
    for which in ('out', 'gt'):
        dd, ref = rows_of(golden[f'{case}_{which}']), rows_of(golden[f'{case}_gloss_{which}'])
        diff = (golden[case + '_q_out'] - golden[case + '_q_gt']).reshape(q.size, -1)
        gl = (np.sign(diff) * (1 if which == 'out' else -1) / np.float32(diff.size)).astype(np.float32)
        for r in range(dd.shape[0]):
            got = R.grad_rule(dd[r], q, gl[:, r])
            assert np.array_equal(np.nonzero(got)[0], np.nonzero(ref[r])[0]), (case, which, r)
            assert np.abs(got - ref[r]).max() <= 2.0 ** -20 * np.abs(ref[r]).max()


def test_gradient_rule_on_ties_sums_per_value(golden):
    """With ties torch.sort and the lowest-index rule choose different elements of a run of equal values: the sums per distinct value
    agree, and the rule puts each sum on the lowest index of its value."""
    d, q, g = golden['ties_out'], golden['ties_q'], golden['ties_g']
    got, want = R.grad_rule(d, q, g), golden['ties_gq_out']
    _, inv = np.unique(d, return_inverse=True)
    a, b = np.bincount(inv, got.astype(np.float64)), np.bincount(inv, want.astype(np.float64))
    assert np.abs(b).max() > 0 and np.abs(a - b).max() <= 2.0 ** -20 * np.abs(b).max()
    nz = np.nonzero(got)[0]
    assert np.array_equal(R.first_index_of_value(d)[nz], nz)


def test_header_symbols_and_abi_version():
    lib = _lib.lib()
    assert lib.pnnp_abi_version() == 9 == ops.ABI_VERSION
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'pnnp_hip.h')).read()
    for name in ('pnnp_quantile_ws_bytes', 'pnnp_quantile_f32', 'pnnp_quantile_bwd_f32', 'pnnp_quantile_loss_f32'):
        assert hasattr(lib, name), name
        assert name + '(' in hdr, name
    assert '#define PNNP_QUANTILE_MAX_K 1024' in hdr and '#define PNNP_ABI_VERSION 9' in hdr
    assert losses.QUANTILE_MAX_K == 1024 >= losses.get_x().numel()


def test_entry_limits_before_any_launch():
    """Sizes outside the limits are decided on the host, so this runs without a device."""
    lib = _lib.lib()
    fake = ctypes.c_void_p(4096)
    i64 = ctypes.c_int64
    ws = lib.pnnp_quantile_ws_bytes
    ws.restype = ctypes.c_int64
    ws.argtypes = [ctypes.c_int, i64, i64, ctypes.c_int]
    assert ws(1, 4096, 0, 1000) >= 4096 * 8 and ws(2, 4096, 100, 1000) >= 2 * 4196 * 8 and ws(1, 1, 1, 1) > 0
    assert ws(1, 4096, 0, 0) == -1 and ws(1, 4096, 0, 1025) == -2 and ws(1, 0, 0, 8) == -1 and ws(0, 16, 0, 8) == -1
    assert ws(1, 1 << 31, 0, 8) == -2
    f, b, l = lib.pnnp_quantile_f32, lib.pnnp_quantile_bwd_f32, lib.pnnp_quantile_loss_f32
    assert f(fake, 1, i64(1024), fake, 1025, fake, fake, fake, fake, None) == -2
    assert f(fake, 1, i64(1024), fake, 0, fake, fake, fake, fake, None) == -2
    assert f(fake, 1, i64(0), fake, 8, fake, fake, fake, fake, None) == -2
    assert f(fake, 1, i64(1 << 31), fake, 8, fake, fake, fake, fake, None) == -2
    assert f(None, 1, i64(1024), fake, 8, fake, fake, fake, fake, None) == -1
    assert b(1, i64(0), 8, fake, fake, fake, None, fake, None) == -2
    assert b(1, i64(1024), 1025, fake, fake, fake, None, fake, None) == -2
    assert b(1, i64(1024), 8, None, fake, fake, None, fake, None) == -1
    assert l(fake, i64(1024), fake, i64(1 << 31), 1, fake, 8, fake, fake, fake, fake, fake, fake, None) == -2
    assert l(fake, i64(1024), fake, i64(512), 1, fake, 1025, fake, fake, fake, fake, fake, fake, None) == -2
    assert l(fake, i64(1024), fake, i64(512), 1, fake, 8, fake, fake, fake, fake, None, fake, None) == -1


def test_refusals_without_a_gpu():
    d, q = torch.zeros(64), torch.linspace(0, 1, 8)
    with pytest.raises(_lib.PnnpError, match='CPU tensor'):
        losses.quantile(d, q)
    with pytest.raises(_lib.PnnpError, match='CPU tensor'):
        losses.QuantileLoss(d, d, q)
    from pnnp_amd.trainer import NoiseFlowFitStep
    assert callable(NoiseFlowFitStep.qloss) and callable(NoiseFlowFitStep.qloss_step)

"""The noise-model score on the host (no GPU): the key -> bin table of metrics._kld_bin_lut against np.histogram itself, the numpy
restatement of the algorithm the kernels implement (tests/_kld_np.py) against the reference's own kl_div_norm outputs
(tests/golden/kld.npz, recipe tests/golden/make_golden_kld.py), and the refusals."""
import ctypes
import os

import numpy as np
import pytest
import torch

from pnnp_amd import _lib, metrics
from tests import _kld_np

CASES = ['narrow', 'wide', 'pos', 'posq', 'ties', 'inf', 'nan']


@pytest.mark.parametrize('wp', [16383, 1023, 255])
def test_bin_lut_is_np_histogram(wp):
    lut = metrics._kld_bin_lut(wp)
    edges = metrics._kld_edges(wp)
    assert lut.dtype == np.int32 and lut.shape == (wp + 1,)
    v = np.arange(wp + 1, dtype=np.float32) / np.float32(wp)                # the reference's norm(): float32
    for k in range(wp + 1):
        h, _ = np.histogram(v[k:k + 1], edges)
        assert h.sum() <= 1
        assert lut[k] == (int(np.argmax(h)) if h.sum() else -1), k
    assert np.all(np.diff(lut[lut >= 0]) >= 0)


def test_bin_lut_is_not_the_identity_at_16383():
    lut = metrics._kld_bin_lut(16383)
    nbins = len(metrics._kld_edges(16383)) - 1
    assert nbins == 16383
    moved = int((lut != np.arange(16384)).sum())
    assert moved == 8704, moved                                              # 8703 values below the top + the top one (the closed last bin)
    per_bin = np.bincount(lut[lut >= 0], minlength=nbins)
    assert per_bin.max() == 2 and (per_bin == 0).any() and (lut >= 0).all()
    assert (per_bin[1024:] == 2).sum() > 1000 and (per_bin[1024:] == 0).sum() > 1000
    assert np.all(np.arange(16384) - lut <= 1) and np.all(np.arange(16384) - lut >= 0)


@pytest.mark.parametrize('case', CASES)
def test_restatement_reproduces_the_reference(golden_dir, case):
    g = np.load(os.path.join(golden_dir, 'kld.npz'))
    lut = metrics._kld_bin_lut(16383)
    edges = metrics._kld_edges(16383)
    assert np.array_equal(edges * 16383 - 512, g['edges'])
    p, q = g[case + '_p'], g[case + '_q']
    p0, q0 = p.copy(), q.copy()
    cp, cq, flags, kl, _ = _kld_np.counts_and_kl(p, q, lut, len(edges) - 1)
    assert np.array_equal(p, p0, equal_nan=True) and np.array_equal(q, q0, equal_nan=True)
    assert np.array_equal(cp, g[case + '_cp']) and np.array_equal(cq, g[case + '_cq'])
    assert np.allclose(kl, g[case + '_kl'], rtol=1e-12, atol=0)
    assert (flags == 1) == (case in ('narrow', 'wide', 'ties', 'inf'))       # the shift; 'nan' has negatives AND a NaN: none
    if case == 'nan':
        assert flags == 3 and cp.sum() == p.size - 1 and cq.sum() == q.size


def test_integer_bin_kl_differs_where_the_noise_is_wide(golden_dir):
    """What a port that "simplifies" to bin k would report."""
    g = np.load(os.path.join(golden_dir, 'kld.npz'))
    ident = np.arange(16384, dtype=np.int32)
    for case, same in (('narrow', True), ('wide', False)):
        _, _, _, kl, _ = _kld_np.counts_and_kl(g[case + '_p'], g[case + '_q'], ident, 16384)
        assert np.isclose(kl[0], g[case + '_kl'][0], rtol=1e-9, atol=0) == same, (case, kl[0], g[case + '_kl'][0])


def test_refusals_without_a_gpu():
    x = torch.zeros(4, 8, 8)
    with pytest.raises(_lib.PnnpError, match='bl=None'):
        metrics.kl_div_norm(x, x, bl=None)
    with pytest.raises(_lib.PnnpError, match='CPU tensor'):
        metrics.kl_div_norm(x, x)
    with pytest.raises(_lib.PnnpError, match='CPU tensor'):
        metrics.noise_model_score(x[None], x[None], x[None], bl=512, wp=16383)
    from pnnp_amd.trainer import NoiseFlowFitStep
    assert callable(NoiseFlowFitStep.score)


def test_entry_limits_before_any_launch():
    """n >= 2^32 per crop and wp > 16383: -2; bad arguments: -1 -- decided on the host, so this runs without a device."""
    lib = _lib.lib()
    fake = ctypes.c_void_p(4096)
    kl, ns = lib.pnnp_kl_div_norm_f32, lib.pnnp_noise_score_f32
    i64, f32 = ctypes.c_int64, ctypes.c_float
    assert kl(fake, fake, 1, i64(1 << 32), f32(512), 16383, fake, 16383, fake, fake, fake, None) == -2
    assert kl(fake, fake, 1, i64(1024), f32(512), 16384, fake, 16384, fake, fake, fake, None) == -2
    assert ns(fake, fake, fake, 1, i64(1 << 32), f32(15871), f32(512), 16383, fake, 16383, fake, fake, fake, None) == -2
    assert kl(fake, fake, 0, i64(1024), f32(512), 16383, fake, 16383, fake, fake, fake, None) == -1
    assert kl(None, fake, 1, i64(1024), f32(512), 16383, fake, 16383, fake, fake, fake, None) == -1
    assert kl(fake, fake, 1, i64(1024), f32(512), 16383, None, 16383, fake, fake, fake, None) == -1
    lib.pnnp_noise_score_ws_bytes.restype = ctypes.c_int64
    assert lib.pnnp_noise_score_ws_bytes(2, i64(4096)) >= 2 * (4 + 2 * 16384 * 4 + 32)
    assert lib.pnnp_noise_score_ws_bytes(0, i64(4096)) == -1

"""The float-edge histogram KL on the host (no GPU): the numpy restatement of the algorithm the kernels implement (tests/_kl_data_np.py)
against the reference's own get_histogram / kl_div_3_data / kl_div_norm(bl=None) outputs (tests/golden/kl_data.npz, recipe
tests/golden/make_golden_kl_data.py) and against np.histogram itself, the validation of the edges, and the refusals of the C entries."""
import ctypes
import os

import numpy as np
import pytest
import torch

from pnnp_amd import _lib, metrics
from tests import _kl_data_np as K


@pytest.fixture(scope='module')
def gold(golden_dir):
    g = np.load(os.path.join(golden_dir, 'kl_data.npz'))
    assert [str(c) for c in g['cases']] == K.CASES and [str(c) for c in g['range_cases']] == K.RANGE_CASES
    return g


def _close(kl, ref, ab):
    """within 1e-12 relative of sum |terms|"""
    return (abs(kl[0] - ref[0]) <= 1e-12 * ab[0] and abs(kl[1] - ref[1]) <= 1e-12 * ab[1] and
            abs(kl[2] - ref[2]) <= 1e-12 * (ab[0] + ab[1]) / 2)


@pytest.mark.parametrize('case', K.CASES)
@pytest.mark.parametrize('hinted', [False, True])
def test_restatement_reproduces_the_reference(gold, case, hinted):
    p, q, e, from_arange = K.load_case(gold, case)
    p0, q0 = p.copy(), q.copy()
    cp, cq, kl, ab = K.counts_and_kl(p, q, e, K.hint_of(e) if hinted else None)      # (a hint on edges that are no arange: still exact)
    assert np.array_equal(p, p0, equal_nan=True) and np.array_equal(q, q0, equal_nan=True)
    assert np.array_equal(cp, gold[case + '_cp']) and np.array_equal(cq, gold[case + '_cq'])
    assert _close(kl, gold[case + '_kl'], ab), (kl, gold[case + '_kl'])
    if case in ('allout', 'halfout'):
        assert kl == (0.0, 0.0, 0.0) and cp.sum() == 0


@pytest.mark.parametrize('case', K.RANGE_CASES)
def test_restatement_reproduces_bl_none(gold, case):
    p, q, wp = K.load_range_case(gold, case)
    e = K.range_edges(p.reshape(-1), q.reshape(-1), wp)
    x = gold[case + '_x']
    assert e.dtype == x.dtype and np.array_equal(e * wp - 0, x), (np.__version__, str(gold['numpy_version']))      # (the float32 scalar arithmetic is numpy's)
    assert len(e) - wp in (1, 2)
    cp, cq, kl, ab = K.counts_and_kl(p, q, e, K.hint_of(e))
    assert np.array_equal(cp, gold[case + '_cp']) and np.array_equal(cq, gold[case + '_cq'])
    assert _close(kl, gold[case + '_kl'], ab), (kl, gold[case + '_kl'])


def test_goldens_hold_both_edge_counts(gold):
    extra = {(gold['data_' + str(gold[c + '_pq'][0])].dtype.name, len(gold[c + '_x']) - int(gold[c + '_wp'])) for c in K.RANGE_CASES}
    assert ('float32', 1) in extra and ('float32', 2) in extra and ('float64', 1) in extra
    assert {int(gold[c + '_wp']) for c in K.RANGE_CASES} == {16383, 1000, 255}


@pytest.mark.parametrize('case', K.EDGE_VALUE_CASES)
def test_restatement_is_np_histogram_on_edge_values(gold, case):
    p, q, e, from_arange = K.load_case(gold, case)
    for x in (p, q):
        ref, _ = np.histogram(x, e)
        assert np.array_equal(K.counts_of(x, e), ref)
        if e[-1] > e[0]:
            assert np.array_equal(K.counts_of(x, e, K.hint_of(e)), ref)


def test_float32_edge_values_fall_below_their_edge():
    """What a kernel that bins with float32 arithmetic gets wrong: many float32(e[k]) lie below the float64 edge e[k], in bin k - 1."""
    e = K.default_edges()
    b = K.bins_of(e.astype(np.float32), e, K.hint_of(e))
    below = int((b[:-1] == np.arange(1000) - 1).sum())
    assert 400 < below < 600, below
    assert below == int((e.astype(np.float32).astype(np.float64) < e).sum())
    assert np.all((b[:-1] == np.arange(1000)) | (b[:-1] == np.arange(1000) - 1))


def test_edge_validation():
    x = torch.zeros(4, 8, 8)                                                 # a CPU tensor: the edges are judged first
    for bad in ([0.0, 0.5, 0.4, 1.0], [0.0, np.nan, 1.0], [0.0, 1.0, np.inf], [-np.inf, 0.0, 1.0], np.zeros((2, 2)), [0.5]):
        with pytest.raises(_lib.PnnpError, match='bin_edges'):
            metrics.get_histogram(x, bin_edges=bad)
        with pytest.raises(_lib.PnnpError, match='bin_edges'):
            metrics.kl_div_3_data(x, x, bin_edges=bad)
    with pytest.raises(_lib.PnnpError, match='at most 16384'):
        metrics.kl_div_3_data(x, x, bin_edges=np.linspace(0, 1, 16386))
    with pytest.raises(_lib.PnnpError, match='at most 16384'):
        metrics.get_histogram(x, n_bins=20000)
    for ok in ([0.0, 0.5, 0.5, 1.0], np.linspace(0, 1, 16385), torch.tensor([0.0, 1.0]), [0, 1, 2]):
        with pytest.raises(_lib.PnnpError, match='CPU tensor'):              # equal neighbours and 16384 bins pass
            metrics.kl_div_3_data(x, x, bin_edges=ok)


def test_cpu_tensors_are_refused():
    x = torch.zeros(4, 8, 8)
    with pytest.raises(_lib.PnnpError, match='CPU tensor'):
        metrics.get_histogram(x)
    with pytest.raises(_lib.PnnpError, match='CPU tensor'):
        metrics.kl_div_3_data(x, x)
    with pytest.raises(_lib.PnnpError, match='CPU tensor'):
        metrics.kl_div_range(x, x)
    with pytest.raises(_lib.PnnpError, match='CPU tensor'):
        metrics.kl_div_3(x.reshape(-1), x.reshape(-1))
    with pytest.raises(_lib.PnnpError, match='wp = 16384'):
        metrics.kl_div_range(x, x, wp=16384)
    from pnnp_amd.trainer import NoiseFlowFitStep
    assert callable(NoiseFlowFitStep.kl3)
    e = metrics.noise_flow_edges()
    assert e.shape == (103,) and e[0] == -1000.0 and e[-1] == 1000.0 and np.all(np.diff(e) > 0)


def test_kl_div_norm_without_bl_still_raises():
    x = torch.zeros(4, 8, 8)
    with pytest.raises(_lib.PnnpError, match='is not provided'):
        metrics.kl_div_norm(x, x, bl=None)


def test_entry_limits_before_any_launch():
    """Bad arguments: -1; more than 16384 bins and n >= 2^32 per crop: -2 -- decided on the host, so this runs without a device."""
    lib = _lib.lib()
    fake = ctypes.c_void_p(4096)
    i64, f64 = ctypes.c_int64, ctypes.c_double
    run = lambda p=fake, q=fake, f=0, B=1, n_p=1024, n_q=1024, e=fake, nb=1000, hs=0.0, ws=fake, hist=fake, kl=fake: \
        lib.pnnp_hist_edges_f64(p, q, f, B, i64(n_p), i64(n_q), e, nb, f64(0.0), f64(hs), ws, hist, kl, None)
    assert run(p=None) == -1 and run(e=None) == -1 and run(ws=None) == -1 and run(hist=None) == -1 and run(kl=None) == -1
    assert run(B=0) == -1 and run(B=65536) == -1 and run(nb=0) == -1 and run(n_p=0) == -1 and run(n_q=0) == -1 and run(f=2) == -1
    assert run(p=ctypes.c_void_p(4098)) == -1 and run(p=ctypes.c_void_p(4100), f=1) == -1 and run(ws=ctypes.c_void_p(4104)) == -1
    assert run(hs=-1.0) == -1 and run(hs=float('nan')) == -1 and run(hs=float('inf')) == -1
    assert run(nb=16385) == -2 and run(n_p=1 << 32) == -2 and run(n_q=1 << 32) == -2 and run(n_p=1 << 32, f=1) == -2
    mm = lambda p=fake, q=fake, f=0, n_p=1024, n_q=1024, out=fake: lib.pnnp_minmax_f(p, q, f, i64(n_p), i64(n_q), out, None)
    assert mm(p=None) == -1 and mm(out=None) == -1 and mm(n_p=0) == -1 and mm(n_q=0) == -1 and mm(f=3) == -1
    assert mm(out=ctypes.c_void_p(4100)) == -1 and mm(n_p=1 << 32) == -2 and mm(n_q=1 << 32) == -2


def test_workspace_covers_the_histograms():
    lib = _lib.lib()
    lib.pnnp_hist_edges_ws_bytes.restype = ctypes.c_int64
    for B, nb in ((1, 1), (1, 1000), (16, 1000), (3, 16384), (65535, 16384)):
        assert lib.pnnp_hist_edges_ws_bytes(B, nb) >= B * 2 * nb * 4
    assert lib.pnnp_hist_edges_ws_bytes(0, 1000) == -1 and lib.pnnp_hist_edges_ws_bytes(1, 0) == -1
    assert lib.pnnp_hist_edges_ws_bytes(65536, 8) == -1 and lib.pnnp_hist_edges_ws_bytes(1, 16385) == -2

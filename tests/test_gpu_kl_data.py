"""The float-edge histogram KL on the device (csrc/hist_kl.hip; metrics.get_histogram, kl_div_3_data, kl_div_range, kl_div_3 and
NoiseFlowFitStep.kl3) against the reference's own outputs (tests/golden/kl_data.npz) and the numpy restatement tests/test_host_kl_data.py
pins to them.

Bounds: counts are integers and must be equal, and hist must be exactly counts / n.  A KL is a float64 sum of at most 16384 terms
y (log y - log y'), each with a few-ulp log: |error| <= 1e-10 * sum |terms| + 1e-300 (the bound of tests/test_gpu_kld.py; float64 leaves
it four decades of room).  Bin centres and kl_div_range's edges are host numpy, uploaded: bitwise the reference's."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import _kl_data_np as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, 'kl_data.npz'))


def _np(t):
    return t.detach().cpu().numpy()


def _counts(y, n):
    y = _np(y)
    c = np.rint(y * n).astype(np.int64)
    assert np.array_equal(c / float(n), y)                                   # y is exactly counts / n
    return c


def _check_kl(got, ref_kl, ref_abs, tag=''):
    got = [float(v) for v in got]
    print(f'{tag} kl device {got} reference {list(ref_kl)}')
    assert abs(got[0] - ref_kl[0]) <= 1e-10 * ref_abs[0] + 1e-300, (tag, got, ref_kl)
    assert abs(got[1] - ref_kl[1]) <= 1e-10 * ref_abs[1] + 1e-300, (tag, got, ref_kl)
    assert abs(got[2] - ref_kl[2]) <= 1e-10 * (ref_abs[0] + ref_abs[1]) / 2 + 1e-300, (tag, got, ref_kl)


def _bits(*tensors):
    return [_np(t).tobytes() for t in tensors]


@pytest.mark.parametrize('case', K.CASES)
def test_golden_cases(gold, case):
    from pnnp_amd import metrics
    pn, qn, e, from_arange = K.load_case(gold, case)
    p, q = torch.from_numpy(pn).cuda(), torch.from_numpy(qn).cuda()
    kw = {} if from_arange else {'bin_edges': e}
    fwd, inv, sym, (yp, yq) = metrics.kl_div_3_data(p, q, return_hist=True, **kw)
    nb = len(e) - 1
    for t in (fwd, inv, sym):
        assert t.dim() == 0 and t.dtype == torch.float64 and t.is_cuda
    assert yp.shape == (nb,) and yq.shape == (nb,) and yp.dtype == torch.float64 and yp.is_cuda
    assert np.array_equal(_counts(yp, pn.size), gold[case + '_cp']) and np.array_equal(_counts(yq, qn.size), gold[case + '_cq'])
    _, _, _, ab = K.counts_and_kl(pn, qn, e)
    _check_kl((fwd, inv, sym), gold[case + '_kl'], ab, case)
    if case in ('allout', 'halfout'):
        assert float(fwd) == 0.0 and float(inv) == 0.0 and float(sym) == 0.0
    hist, cen = metrics.get_histogram(p, **kw)
    assert torch.equal(hist, yp) and cen.dtype == torch.float64 and cen.is_cuda
    assert _np(cen).tobytes() == gold[case + '_cen'].tobytes()               # bitwise the reference's bin centres
    hq, _ = metrics.get_histogram(q, **kw)
    assert torch.equal(hq, yq)
    # the same edges as an array (no hint: the binary search), as a list and as a tensor; and a second run: all bitwise equal
    for edges in (e, list(e), torch.from_numpy(e).cuda()):
        again = metrics.kl_div_3_data(p, q, bin_edges=edges, return_hist=True)
        assert _bits(*again[:3], *again[3]) == _bits(fwd, inv, sym, yp, yq)
    again = metrics.kl_div_3_data(p, q, return_hist=True, **kw)
    assert _bits(*again[:3], *again[3]) == _bits(fwd, inv, sym, yp, yq)
    # the caller's arrays are not modified
    assert np.array_equal(_np(p), pn, equal_nan=True) and np.array_equal(_np(q), qn, equal_nan=True)


@pytest.mark.parametrize('case', K.RANGE_CASES)
def test_bl_none_cases(gold, case):
    from pnnp_amd import metrics
    pn, qn, wp = K.load_range_case(gold, case)
    p, q = torch.from_numpy(pn).cuda(), torch.from_numpy(qn).cuda()
    r = metrics.kl_div_range(p, q, wp=wp)
    x = gold[case + '_x']
    for k in ('hist_p', 'hist_q'):
        assert r[k][1].dtype == torch.float64 and r[k][1].is_cuda
        assert _np(r[k][1]).tobytes() == np.asarray(x, np.float64).tobytes()             # bitwise the reference's bin_edges * wp - 0
    assert len(x) - wp in (1, 2) and r['hist_p'][0].shape == (len(x) - 1,)
    assert np.array_equal(_counts(r['hist_p'][0], pn.size), gold[case + '_cp'])
    assert np.array_equal(_counts(r['hist_q'][0], qn.size), gold[case + '_cq'])
    e = K.range_edges(pn.reshape(-1), qn.reshape(-1), wp)
    _, _, _, ab = K.counts_and_kl(pn, qn, e)
    _check_kl((r['kl_fwd'], r['kl_inv'], r['kl_sym']), gold[case + '_kl'], ab, case)
    assert r['kl_fwd'].dim() == 0 and r['kl_fwd'].dtype == torch.float64 and r['kl_fwd'].is_cuda
    assert np.array_equal(_np(p), pn) and np.array_equal(_np(q), qn)


def test_kl_div_range_refuses_what_arange_refuses():
    from pnnp_amd import metrics
    g = torch.Generator().manual_seed(31)
    good = torch.randn(4, 33, 7, generator=g).cuda()
    for dtype in (torch.float32, torch.float64):
        for bad_value in (float('nan'), float('inf'), float('-inf')):
            bad = good.to(dtype).clone()
            bad[3, 32, 6] = bad_value                                        # the very last element
            with pytest.raises(ValueError, match='cannot compute length'):
                metrics.kl_div_range(good.to(dtype), bad)
            with pytest.raises(ValueError, match='cannot compute length'):
                metrics.kl_div_range(bad, good.to(dtype))
        const = torch.full((5, 7), 0.25, dtype=dtype, device='cuda')
        with pytest.raises(ValueError, match='cannot compute length'):
            metrics.kl_div_range(const, const.clone())
        r = metrics.kl_div_range(good.to(dtype), good.to(dtype) * 1.5, wp=64)            # and finite, varying data pass
        assert r['hist_p'][0].shape[0] in (64, 65)


def test_per_crop(gold):
    from pnnp_amd import metrics
    for pn, qn, kw in ((gold['data_a'], gold['data_b'], {}), (gold['data_nfp'], gold['data_nfq'], {'bin_edges': K.default_edges(-0.1, 0.1, 100)}),
                       (gold['data_dp'], gold['data_dq'], {'bin_edges': np.linspace(-6.0, 6.5, 778)})):
        p, q = torch.from_numpy(pn).cuda(), torch.from_numpy(qn).cuda()
        assert p.shape == (4, 64, 64)
        fwd, inv, sym, (yp, yq) = metrics.kl_div_3_data(p, q, per_crop=True, return_hist=True, **kw)
        hist, cen = metrics.get_histogram(p, per_crop=True, **kw)
        nb = cen.numel()
        assert fwd.shape == (4,) and yp.shape == (4, nb) and torch.equal(hist, yp)
        for b in range(4):
            one = metrics.kl_div_3_data(p[b], q[b], return_hist=True, **kw)
            assert _bits(*one[:3], *one[3]) == _bits(fwd[b], inv[b], sym[b], yp[b], yq[b]), b
        pooled = metrics.kl_div_3_data(p, q, return_hist=True, **kw)
        n = pn.size
        rows_p = sum(_counts(yp[b], n // 4) for b in range(4))
        rows_q = sum(_counts(yq[b], n // 4) for b in range(4))
        assert np.array_equal(_counts(pooled[3][0], n), rows_p) and np.array_equal(_counts(pooled[3][1], n), rows_q)
    from pnnp_amd import _lib
    with pytest.raises(_lib.PnnpError, match='leading size'):
        metrics.kl_div_3_data(p, q[:3], per_crop=True)
    with pytest.raises(_lib.PnnpError, match='one dtype'):
        metrics.kl_div_3_data(p, q.float())


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_lengths_and_offsets(dtype):
    """Lengths 1, 63, 64, 65 and 4097 from views that start 0 .. 3 elements into their storage (p and q at different offsets): the scalar
    head and tail of the 16-byte loads, for both element sizes."""
    from pnnp_amd import metrics
    g = torch.Generator().manual_seed(32)
    bp = (torch.randn(4200, generator=g, dtype=torch.float64) * 0.2 + 0.5).to(dtype).cuda()
    bq = (torch.randn(4200, generator=g, dtype=torch.float64) * 0.25 + 0.5).to(dtype).cuda()
    e = K.default_edges()
    for n in (1, 63, 64, 65, 4097):
        for off in range(4):
            p, q = bp[off:off + n], bq[(off + 1) % 4:(off + 1) % 4 + n]
            assert p.data_ptr() % 16 == (off * p.element_size()) % 16
            cp, cq, kl, ab = K.counts_and_kl(_np(p), _np(q), e, K.hint_of(e))
            fwd, inv, sym, (yp, yq) = metrics.kl_div_3_data(p, q, return_hist=True)
            assert np.array_equal(_counts(yp, n), cp) and np.array_equal(_counts(yq, n), cq), (n, off)
            _check_kl((fwd, inv, sym), kl, ab, f'{dtype} n {n} offset {off}')


def _arange_with(nb):
    """(left, right) whose arange has exactly nb bins (it has nb or nb + 1, depending on rounding)."""
    for right in (1.0, 1.5, 2.0, 1.25, 3.0, 0.75, 5.0):
        if len(K.default_edges(-0.25, right, nb)) == nb + 1:
            return -0.25, right
    raise AssertionError(nb)


# 10000: the last bin count whose edges fit in LDS beside the histograms; 10001 and 10240: the first that read them from global memory
@pytest.mark.parametrize('nb', [1, 2, 102, 1000, 10000, 10001, 10240, 16383, 16384])
def test_bin_counts(nb):
    from pnnp_amd import metrics
    left, right = _arange_with(nb)
    e = K.default_edges(left, right, nb)
    g = torch.Generator().manual_seed(33 + nb)
    mid, half = (left + right) / 2, (right - left) / 2
    p = (torch.rand(20011, generator=g, dtype=torch.float64) * 2.2 * half + (mid - 1.1 * half)).float()          # both ends overshoot
    q = torch.randn(30005, generator=g, dtype=torch.float64) * 0.4 * half + mid
    p[:e.size] = torch.from_numpy(e.astype(np.float32))[:p.numel()]          # float32(e[k]): on either side of the float64 edge
    for a, b in ((p, q.float()), (p.double(), q)):
        cp, cq, kl, ab = K.counts_and_kl(a.numpy(), b.numpy(), e, K.hint_of(e))
        ref, _ = np.histogram(a.numpy(), e)
        assert np.array_equal(cp, ref)
        ad, bd = a.cuda(), b.cuda()
        hinted = metrics.kl_div_3_data(ad, bd, left_edge=left, right_edge=right, n_bins=nb, return_hist=True)
        plain = metrics.kl_div_3_data(ad, bd, bin_edges=e, return_hist=True)
        for res, tag in ((hinted, 'hint'), (plain, 'search')):
            assert res[3][0].shape == (nb,)
            assert np.array_equal(_counts(res[3][0], a.numel()), cp) and np.array_equal(_counts(res[3][1], b.numel()), cq), (nb, tag)
            _check_kl(res[:3], kl, ab, f'nb {nb} {tag} {a.dtype}')
        assert _bits(*hinted[:3], *hinted[3]) == _bits(*plain[:3], *plain[3])
        hist, cen = metrics.get_histogram(ad, left_edge=left, right_edge=right, n_bins=nb)
        assert torch.equal(hist, hinted[3][0]) and np.array_equal(_np(cen), e[:-1] + ((right - left) / nb) / 2.0)


def test_many_blocks_and_identity_run_to_run():
    """4x4x128x128 as ONE crop (16 workgroups, several grid-stride trips) and per crop; narrow noise over the Noise Flow edges, where a
    wave's lanes crowd a few bins and the catch-all bins take the rest.  Two calls: bitwise-identical results."""
    from pnnp_amd import metrics
    g = torch.Generator().manual_seed(34)
    p = (torch.randn(4, 4, 128, 128, generator=g) * 0.03).cuda()
    q = (torch.randn(4, 4, 128, 128, generator=g) * 0.3).cuda()
    e = metrics.noise_flow_edges()
    cp, cq, kl, ab = K.counts_and_kl(_np(p), _np(q), e)
    a = metrics.kl_div_3_data(p, q, bin_edges=e, return_hist=True)
    assert np.array_equal(_counts(a[3][0], p.numel()), cp) and np.array_equal(_counts(a[3][1], q.numel()), cq)
    assert cq[0] > 1000 and cq[-1] > 1000 and cp.sum() == p.numel()
    _check_kl(a[:3], kl, ab, '256k')
    b = metrics.kl_div_3_data(p, q, bin_edges=e, return_hist=True)
    assert _bits(*a[:3], *a[3]) == _bits(*b[:3], *b[3])
    const = torch.full((1 << 20,), 0.5, device='cuda')                       # 2^20 samples in one bin: no lost update
    h, _ = metrics.get_histogram(const)
    c = _counts(h, 1 << 20)
    assert c[500] == 1 << 20 and c.sum() == 1 << 20


def test_refusals_leave_the_outputs_untouched():
    from pnnp_amd import _lib, metrics
    lib = metrics._hist_lib()
    p = torch.rand(2, 1024, device='cuda')
    edges = torch.linspace(0, 1, 11, dtype=torch.float64, device='cuda')
    ws = torch.full((4096,), 0x5a, dtype=torch.uint8, device='cuda')
    hist = torch.full((2, 2, 10), -7.0, dtype=torch.float64, device='cuda')
    kl = torch.full((2, 3), -7.0, dtype=torch.float64, device='cuda')
    out = torch.full((6,), -7.0, dtype=torch.float64, device='cuda')
    i64, f64, P = ctypes.c_int64, ctypes.c_double, _lib.ptr
    run = lambda B=2, n_p=1024, n_q=1024, nb=10, q=p, hs=0.0, e=edges: lib.pnnp_hist_edges_f64(
        P(p), P(q), 0, B, i64(n_p), i64(n_q), P(e), nb, f64(0.0), f64(hs), P(ws), P(hist), P(kl), _lib.stream())
    assert run(B=0) == -1 and run(nb=0) == -1 and run(n_p=0) == -1 and run(e=None) == -1 and run(hs=-2.0) == -1
    assert run(nb=16385) == -2 and run(n_p=1 << 32) == -2 and run(n_q=1 << 32) == -2
    assert lib.pnnp_minmax_f(P(p), P(p), 0, i64(1 << 32), i64(8), P(out), _lib.stream()) == -2
    assert lib.pnnp_minmax_f(P(p), P(p), 0, i64(0), i64(8), P(out), _lib.stream()) == -1
    torch.cuda.synchronize()
    assert bool((hist == -7.0).all()) and bool((kl == -7.0).all()) and bool((out == -7.0).all()) and bool((ws == 0x5a).all())
    for bad in ([0.0, 0.5, 0.4], [0.0, float('nan')], [0.0, float('inf')]):
        with pytest.raises(_lib.PnnpError, match='bin_edges'):
            metrics.kl_div_3_data(p, p, bin_edges=bad)
    with pytest.raises(_lib.PnnpError, match='float32 or float64'):
        metrics.get_histogram(p.half())
    assert run() == 0                                                        # and the same buffers do serve a good call
    torch.cuda.synchronize()
    assert bool((hist >= 0).all()) and bool((kl[:, 2] == (kl[:, 0] + kl[:, 1]) / 2).all())


def test_histogram_kl_functions(gold):
    from pnnp_amd import metrics
    hp, hq = torch.from_numpy(gold['k3_p']).cuda(), torch.from_numpy(gold['k3_q']).cuda()
    ref = gold['k3_vals']
    got = [metrics.kl_div_forward(hp, hq), metrics.kl_div_inverse(hp, hq), metrics.kl_div_sym(hp, hq), *metrics.kl_div_3(hp, hq)]
    for t, r in zip(got, ref):
        assert t.dim() == 0 and t.dtype == torch.float64 and t.is_cuda
        assert abs(float(t) - r) <= 1e-12 * abs(r), (float(t), r)
    assert np.array_equal(_np(hp), gold['k3_p'], equal_nan=True)
    z = torch.zeros(8, dtype=torch.float64, device='cuda')
    assert float(metrics.kl_div_forward(z, z)) == 0.0 and float(metrics.kl_div_3(z, z + 1)[2]) == 0.0


@pytest.mark.parametrize('training', [True, False])
def test_fit_step_kl3(training):
    from pnnp_amd import metrics
    from pnnp_amd.archs import NoiseFlow
    from pnnp_amd.trainer import NoiseFlowFitStep
    np.random.seed(3); torch.manual_seed(3)
    net = NoiseFlow({'x_shape': (4, 32, 32), 'arch': 'sdn|unc|unc|unc|unc|giso|unc|unc|unc|unc'}).cuda()
    net.train(training)
    fit = NoiseFlowFitStep(net, camera_type='SonyA7S2', noise_code='pgrq', clip=2)
    g = torch.Generator().manual_seed(35)
    hr = (torch.rand(2, 4, 32, 32, generator=g) * 0.3).cuda()
    hr[0, 0, 0, 0] = 1.5                                                     # clip: the score sees the clamped crop
    before = [p.detach().clone() for p in net.parameters()]
    np.random.seed(5)                                                        # (make_pair draws the camera parameters with numpy's generator)
    res, (noise, sampled) = fit.kl3(hr, iso=1600, per_crop=True, return_tensors=True)
    assert net.training is training and fit.step_count == 0
    assert all(torch.equal(a, b.detach()) for a, b in zip(before, net.parameters()))
    np.random.seed(5)
    real, _ = fit.make_pair(hr, 1600)                                        # the pair of the step's counters, again
    assert torch.equal(noise, real - hr.clamp(0, 1)) and sampled.shape == hr.shape
    by_hand = metrics.kl_div_3_data(noise, sampled, bin_edges=metrics.noise_flow_edges(), per_crop=True)
    assert len(res) == 3 and res[0].shape == (2,) and _bits(*res) == _bits(*by_hand)
    cp, cq, kl, ab = K.counts_and_kl(_np(noise[1]), _np(sampled[1]), metrics.noise_flow_edges())
    _check_kl([r[1] for r in res], kl, ab, 'kl3 crop 1')
    pooled = fit.kl3(hr, iso=1600, bin_edges=np.linspace(-0.2, 0.2, 41))
    assert pooled[0].dim() == 0 and net.training is training and fit.step_count == 0

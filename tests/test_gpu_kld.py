"""The noise-model score on the device (csrc/noise_score.hip; metrics.kl_div_norm, metrics.noise_model_score, NoiseFlowFitStep.score)
against the reference's own outputs (tests/golden/kld.npz) and the numpy restatement tests/test_host_kld.py pins to them.

Bounds: counts are integers and must be equal.  A KL is a float64 sum of at most 16383 terms y (log y - log y'), each with a few-ulp log:
|error| <= 1e-10 * sum |terms| (the issue's bound; float64 leaves it four decades of room).  Moments: 1e-9 relative to numpy's float64 std."""
import os

import numpy as np
import pytest
import torch

from tests import _kld_np

pytestmark = pytest.mark.gpu

CASES = ['narrow', 'wide', 'pos', 'posq', 'ties', 'inf', 'nan']
WP, BL = 16383, 512


def _tables():
    from pnnp_amd import metrics
    return metrics._kld_bin_lut(WP), len(metrics._kld_edges(WP)) - 1


def _counts(hist, n):
    y = hist[0].cpu().numpy()
    c = np.rint(y * n).astype(np.int64)
    assert np.array_equal(c / n, y)                                          # y is exactly counts / n
    return c


def _check_kl(res, names, ref_kl, ref_abs, tag=''):
    got = [float(res[k]) for k in names]
    print(f'{tag} kl device {got} reference {list(ref_kl)}')
    assert abs(got[0] - ref_kl[0]) <= 1e-10 * ref_abs[0] + 1e-300, (tag, got, ref_kl)
    assert abs(got[1] - ref_kl[1]) <= 1e-10 * ref_abs[1] + 1e-300, (tag, got, ref_kl)
    assert abs(got[2] - ref_kl[2]) <= 1e-10 * (ref_abs[0] + ref_abs[1]) / 2 + 1e-300, (tag, got, ref_kl)


def _check_dn(p, q, tag='', expect_flags=None):
    """kl_div_norm on one crop of device tensors against the restatement."""
    from pnnp_amd import metrics
    lut, nbins = _tables()
    pn, qn = p.cpu().numpy().reshape(-1), q.cpu().numpy().reshape(-1)
    cp, cq, flags, kl, ab = _kld_np.counts_and_kl(pn, qn, lut, nbins)
    if expect_flags is not None:
        assert flags == expect_flags, (tag, flags)
    res = metrics.kl_div_norm(p, q)
    n = pn.size
    assert np.array_equal(_counts(res['hist_p'], n), cp), tag
    assert np.array_equal(_counts(res['hist_q'], n), cq), tag
    _check_kl(res, ('kl_fwd', 'kl_inv', 'kl_sym'), kl, ab, tag)
    return res


@pytest.mark.parametrize('case', CASES)
def test_golden_cases(golden_dir, case):
    from pnnp_amd import metrics
    g = np.load(os.path.join(golden_dir, 'kld.npz'))
    p, q = torch.from_numpy(g[case + '_p']).cuda(), torch.from_numpy(g[case + '_q']).cuda()
    res = metrics.kl_div_norm(p, q)
    n = p.numel()
    assert res['kl_fwd'].dim() == 0 and res['kl_fwd'].dtype == torch.float64 and res['hist_p'][0].shape == (16383,)
    assert np.array_equal(_counts(res['hist_p'], n), g[case + '_cp'])
    assert np.array_equal(_counts(res['hist_q'], n), g[case + '_cq'])
    assert np.array_equal(res['hist_p'][1].cpu().numpy(), g['edges']) and np.array_equal(res['hist_q'][1].cpu().numpy(), g['edges'])
    lut, nbins = _tables()
    _, _, _, kl, ab = _kld_np.counts_and_kl(g[case + '_p'], g[case + '_q'], lut, nbins)
    _check_kl(res, ('kl_fwd', 'kl_inv', 'kl_sym'), g[case + '_kl'], ab, case)
    # the caller's arrays are not modified (the reference adds bl into them)
    assert np.array_equal(p.cpu().numpy(), g[case + '_p'], equal_nan=True) and np.array_equal(q.cpu().numpy(), g[case + '_q'], equal_nan=True)


def _sampler(y, seed, sig_gs=6.0, sig_r=1.0):
    from pnnp_amd import process
    prm = dict(K=1.5, sigGs=sig_gs, sigTL=3.0, lam=-0.02, sigR=sig_r, q=1 / 2 ** 14, ratio=1.0, wp=WP, bl=BL, bias=0)
    flags = process.noise_flags('pr', torch_mode=True)
    return process.noise_sample(y, process.pack_params([prm] * y.shape[0], y.device), flags, seed=seed, offset=3)


def _pair_reference(clean, real, noise, b):
    lut, nbins = _tables()
    p, q, output = _kld_np.pair_dn(clean[b].cpu().numpy(), real[b].cpu().numpy(), noise[b].cpu().numpy(), BL, WP)
    cp, cq, flags, kl, ab = _kld_np.counts_and_kl(p, q, lut, nbins)
    return cp, cq, kl, ab, real[b].cpu().numpy(), output


def _row(res, b):
    return {k: ((v[0][b], v[1]) if isinstance(v, tuple) else v[b]) for k, v in res.items()}


def _check_pair_row(row, b, clean, real, noise, tag):
    """One crop's result `row` against the restatement on crop b of the images."""
    cp, cq, kl, ab, tgt, output = _pair_reference(clean, real, noise, b)
    n = tgt.size
    assert np.array_equal(_counts(row['hist_p'], n), cp) and np.array_equal(_counts(row['hist_q'], n), cq), tag
    _check_kl(row, ('kl_int', 'kl_inv', 'kl_sym'), kl, ab, tag)
    gt64, out64 = tgt.astype(np.float64).std(), output.astype(np.float64).std()
    gt32, out32 = float(tgt.std()), float(output.std())
    print(f'{tag} std device {float(row["gt_std"])!r} {float(row["out_std"])!r} float64 {gt64!r} {out64!r}; '
          f'the reference\'s float32 .std() is off by {abs(gt32 - gt64) / gt64:.2e} / {abs(out32 - out64) / out64:.2e} relative')
    assert abs(float(row['gt_std']) - gt64) <= 1e-9 * gt64 and abs(float(row['out_std']) - out64) <= 1e-9 * out64, tag
    # diff_p = 100 (1 - out / gt): two stds within 1e-9 relative move the quotient by 2e-9 of itself
    assert abs(float(row['diff_p']) - 100 * (gt64 - out64) / gt64) <= 100 * 2.1e-9 * out64 / gt64, tag


def test_pair_mode_per_crop():
    """3 crops of 4x33x47 (6204 elements: crops start on 16-byte words, 1551 vectors each and no tail; the scalar head / tail is
    test_dn_mode_unaligned's) of sampler output, with clean values outside [0, 1].  Printed here (not a bar): the reference's own
    float32 .std() of these crops lies 1e-8 .. 1e-7 relative from the float64 value the device is held to within 1e-9."""
    from pnnp_amd import metrics
    g = torch.Generator().manual_seed(11)
    clean = (torch.rand(3, 4, 33, 47, generator=g) * 0.02).cuda()
    clean[0, 0, 0, :5] = 1.25; clean[1, 2, 7, 3] = -0.125; clean[2, 1, 4, 4] = 1.0
    real = _sampler(clean, seed=1)
    noise = _sampler(clean, seed=2) - clean
    res = metrics.noise_model_score(clean, real, noise, bl=BL, wp=WP, per_crop=True)
    assert res['kl_int'].shape == (3,) and res['gt_std'].dtype == torch.float64
    for b in range(3):
        _check_pair_row(_row(res, b), b, clean, real, noise, f'pair crop {b}')
        one = metrics.noise_model_score(clean[b:b + 1], real[b:b + 1], noise[b:b + 1], bl=BL, wp=WP)
        for k in ('kl_int', 'kl_inv', 'kl_sym', 'gt_std', 'out_std', 'diff_p'):
            assert one[k].dim() == 0 and one[k].cpu().numpy().tobytes() == res[k][b].cpu().numpy().tobytes(), (b, k)
        assert torch.equal(one['hist_p'][0], res['hist_p'][0][b]) and torch.equal(one['hist_q'][0], res['hist_q'][0][b])
    # run-to-run identity of the one-pass kernel: counts, KLs and the float64 moments (per-block partials, fixed-order sums)
    again = metrics.noise_model_score(clean, real, noise, bl=BL, wp=WP, per_crop=True)
    for k in ('kl_int', 'kl_inv', 'kl_sym', 'gt_std', 'out_std', 'diff_p'):
        assert again[k].cpu().numpy().tobytes() == res[k].cpu().numpy().tobytes(), k
    assert torch.equal(again['hist_p'][0], res['hist_p'][0]) and torch.equal(again['hist_q'][0], res['hist_q'][0])
    # crop 0 only without per_crop, like the reference
    first = metrics.noise_model_score(clean, real, noise, bl=BL, wp=WP)
    assert first['kl_int'].cpu().numpy().tobytes() == res['kl_int'][0].cpu().numpy().tobytes()
    line = metrics.score_log_line(first)
    assert line == f"kl_int:{float(first['kl_int']):.6f}, std:{float(first['out_std']):.3f} vs {float(first['gt_std']):.3f} ({float(first['diff_p']):.2f}%)"


def test_pair_mode_mismatched_alignment():
    """The three images at different offsets inside a 16-byte word: the scalar path."""
    from pnnp_amd import metrics
    g = torch.Generator().manual_seed(12)
    shape = (1, 4, 9, 11)
    n = 4 * 9 * 11
    clean0 = torch.rand(shape, generator=g) * 0.02
    vals = (clean0, clean0 + torch.randn(shape, generator=g) * 0.001, torch.randn(shape, generator=g) * 0.0011)
    views = []
    for v, o in zip(vals, (0, 1, 3)):
        t = torch.empty(n + 3, device='cuda')[o:o + n].view(shape)
        t.copy_(v)
        views.append(t)
    clean, real, noise = views
    assert len({t.data_ptr() % 16 for t in views}) == 3
    res = metrics.noise_model_score(clean, real, noise, bl=BL, wp=WP)
    _check_pair_row(res, 0, clean, real, noise, 'pair misaligned')


def test_dn_mode_unaligned():
    """Length 6203 from views that start one (p) and two (q) elements into their storage: vector head and tail, different for p and q."""
    g = torch.Generator().manual_seed(13)
    sp = torch.round(torch.randn(6204, generator=g) * 4).cuda()
    sq = torch.round(torch.randn(6205, generator=g) * 4.5).cuda()
    p, q = sp[1:], sq[2:]
    assert p.numel() == 6203 and p.data_ptr() % 16 == 4 and q.data_ptr() % 16 == 8
    _check_dn(p, q, 'unaligned', expect_flags=1)


def test_one_million_samples_and_identity_run_to_run():
    """16x4x128x128 narrow noise as ONE crop: many workgroups, several grid-stride trips.  Two calls: bitwise-identical results."""
    from pnnp_amd import metrics
    g = torch.Generator().manual_seed(14)
    p = torch.round(torch.randn(16, 4, 128, 128, generator=g) * 3.0).cuda()
    q = torch.round(torch.randn(16, 4, 128, 128, generator=g) * 3.2).cuda()
    a = _check_dn(p, q, '1M', expect_flags=1)
    b = metrics.kl_div_norm(p, q)
    for k in ('kl_fwd', 'kl_inv', 'kl_sym'):
        assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), k
    assert torch.equal(a['hist_p'][0], b['hist_p'][0]) and torch.equal(a['hist_q'][0], b['hist_q'][0])
    # per crop: 16 scores, each that of its crop alone
    pc = metrics.kl_div_norm(p, q, per_crop=True)
    assert pc['kl_sym'].shape == (16,) and pc['hist_p'][0].shape == (16, 16383)
    one = metrics.kl_div_norm(p[5], q[5])
    assert one['kl_sym'].cpu().numpy().tobytes() == pc['kl_sym'][5].cpu().numpy().tobytes()
    assert torch.equal(one['hist_q'][0], pc['hist_q'][0][5])


def test_every_sample_equal():
    """2^20 samples in one bin: the count is exact (no lost update, no 16-bit packing), with and without the shift."""
    from pnnp_amd import metrics
    lut, _ = _tables()
    n = 1 << 20
    p = torch.full((n,), 37.0, device='cuda'); q = torch.full((n,), 37.0, device='cuda')
    res = metrics.kl_div_norm(p, q)
    cp, cq = _counts(res['hist_p'], n), _counts(res['hist_q'], n)
    assert cp[lut[37]] == n and cp.sum() == n and cq[lut[37]] == n and cq.sum() == n
    assert float(res['kl_fwd']) == 0.0 and float(res['kl_sym']) == 0.0
    p = torch.full((n,), -3.0, device='cuda')
    res = metrics.kl_div_norm(p, q)
    cp, cq = _counts(res['hist_p'], n), _counts(res['hist_q'], n)
    assert cp[lut[509]] == n and cp.sum() == n and cq[lut[549]] == n and cq.sum() == n


def test_shift_flag_edges():
    g = torch.Generator().manual_seed(15)
    base = torch.round(torch.rand(3, 4, 16, 20, generator=g) * 30).cuda()            # >= 0
    q = torch.round(torch.rand(3, 4, 16, 20, generator=g) * 30 - 4).cuda()
    z = base.clone(); z[0, 0, 0, 0] = 0.0
    assert float(z.min()) == 0.0
    _check_dn(z[0], q[0], 'min exactly 0', expect_flags=0)
    m = base.clone(); m[0, 1, 2, 3] = -0.0
    _check_dn(m[0], q[0], '-0.0', expect_flags=0)
    last = base.clone(); last[2, 3, 15, 19] = -1.0                                   # the very last element of the last crop
    from pnnp_amd import metrics
    lut, nbins = _tables()
    pc = metrics.kl_div_norm(last, q, per_crop=True)
    for b in range(3):
        cp, cq, flags, kl, ab = _kld_np.counts_and_kl(last[b].cpu().numpy(), q[b].cpu().numpy(), lut, nbins)
        assert flags == (1 if b == 2 else 0)
        n = last[b].numel()
        assert np.array_equal(_counts((pc['hist_p'][0][b], None), n), cp) and np.array_equal(_counts((pc['hist_q'][0][b], None), n), cq), b
        _check_kl({k: pc[k][b] for k in ('kl_fwd', 'kl_inv', 'kl_sym')}, ('kl_fwd', 'kl_inv', 'kl_sym'), kl, ab, f'last-element crop {b}')
    _check_dn(last[2], q[2], 'negative last element', expect_flags=1)
    nn = base.clone(); nn[1, 0, 0, 1] = float('nan'); nn[1, 0, 0, 2] = -5.0; nn[1, 2, 0, 2] = -7.0
    res = _check_dn(nn[1], q[1], 'NaN with negatives', expect_flags=3)
    assert _counts(res['hist_p'], nn[1].numel()).sum() == nn[1].numel() - 1


def _fit(training):
    from pnnp_amd.archs import NoiseFlow
    from pnnp_amd.trainer import NoiseFlowFitStep
    np.random.seed(3); torch.manual_seed(3)
    net = NoiseFlow({'x_shape': (4, 64, 64), 'arch': 'sdn|unc|unc|unc|unc|giso|unc|unc|unc|unc'}).cuda()
    net.train(training)
    return net, NoiseFlowFitStep(net, camera_type='SonyA7S2', noise_code='pgrq', clip=2)


@pytest.mark.parametrize('training', [True, False])
def test_fit_step_score(training):
    net, fit = _fit(training)
    g = torch.Generator().manual_seed(16)
    hr = (torch.rand(2, 4, 64, 64, generator=g) * 0.3).cuda()
    hr[0, 0, 0, 0] = 1.5                                                             # clip: the score sees the clamped crop
    before = [p.detach().clone() for p in net.parameters()]
    res, (hr_used, real, noise) = fit.score(hr, iso=1600, per_crop=True, return_tensors=True)
    assert net.training is training and fit.step_count == 0
    assert all(torch.equal(a, b.detach()) for a, b in zip(before, net.parameters()))
    assert float(hr_used.max()) <= 1.0 and hr_used.shape == hr.shape and real.shape == hr.shape and noise.shape == hr.shape
    prm = fit._pair_params[0]
    assert (prm['bl'], prm['wp']) == (BL, WP)                                        # SonyA7S2
    for b in range(2):
        _check_pair_row(_row(res, b), b, hr_used, real, noise, f'fit.score crop {b}')
    res0 = fit.score(hr, iso=1600)
    assert res0['kl_int'].dim() == 0 and net.training is training


def test_a_worse_model_scores_worse():
    """Ordering only: two independent draws of one sampler are closer (kl_sym) than a draw against the sampler with its read-noise
    sigma x 1.5 (dark crops, where the read noise is the noise)."""
    from pnnp_amd import metrics
    g = torch.Generator().manual_seed(17)
    clean = (torch.rand(1, 4, 128, 128, generator=g) * 0.002).cuda()
    real = _sampler(clean, seed=21)
    same = _sampler(clean, seed=22) - clean
    worse = _sampler(clean, seed=22, sig_gs=9.0, sig_r=1.5) - clean
    a = metrics.noise_model_score(clean, real, same, bl=BL, wp=WP)
    b = metrics.noise_model_score(clean, real, worse, bl=BL, wp=WP)
    print('kl_sym same sampler', float(a['kl_sym']), 'sigma x 1.5', float(b['kl_sym']), 'diff_p', float(a['diff_p']), float(b['diff_p']))
    assert float(a['kl_sym']) < float(b['kl_sym'])
    assert abs(float(a['diff_p'])) < abs(float(b['diff_p']))

"""Dark-frame calibration on the device (csrc/calib.hip, pnnp_amd/calibrate.py) against the int64 / float64 numpy restatement
tests/_calib_ref.py: the integer statistics and the float32 residual bit for bit, the fit within the float64 reduction order, a round trip
through the shipped sampler, register_camera into the train step, and row_denoise."""
import numpy as np
import pytest
import torch

import _calib_ref as R

pytestmark = pytest.mark.gpu

# (N, H, W): one pixel pair; one 16-byte group; W % 8 != 0 (element accesses, a row tail); a second round of the row's 256 groups with a
# tail (258 = 256 + 2 groups, narrow: 2058 % 8 = 2); three rounds on the wide path (513 groups) and more than one wave per row slot
SHAPES = [(1, 2, 2), (3, 2, 8), (2, 4, 10), (5, 6, 2058), (4, 2, 4104)]


def _stack(N, H, W, kind, seed=0):
    if kind == 'random':
        return np.random.default_rng(seed).integers(0, 65536, size=(N, H, W), dtype=np.uint16)
    return np.full((N, H, W), 0 if kind == 'zeros' else 65535, np.uint16)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _check_stack(st, frames):
    s, ss, rs = R.accumulate(frames)
    assert st.n == frames.shape[0]
    assert st.sum.dtype == torch.int32 and st.sumsq.dtype == torch.int64 and st.rowsum.dtype == torch.int32
    assert torch.equal(st.sum.cpu().to(torch.int64), torch.from_numpy(s))
    assert torch.equal(st.sumsq.cpu(), torch.from_numpy(ss))
    assert torch.equal(st.rowsum.cpu().to(torch.int64), torch.from_numpy(rs))
    return s, ss, rs


@pytest.mark.parametrize('kind', ['random', 'zeros', 'ones'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_accumulate_is_exact(shape, kind):
    from pnnp_amd import calibrate
    N, H, W = shape
    fr = _stack(N, H, W, kind, seed=N * W)
    st = calibrate.DarkStack(H, W).add(_dev(fr))
    s, ss, _ = _check_stack(st, fr)
    assert np.array_equal(st.dark_shading().cpu().numpy().view(np.int32), R.dark_shading(s, N).view(np.int32))
    assert np.array_equal(st.black_level_error(512), R.black_level_error(s, N, 512))
    if N >= 2:
        assert np.array_equal(st.var_map().cpu().numpy(), R.var_map(s, ss, N))


def test_accumulate_past_32_and_16_bits():
    """40 frames of 65535: the squares pass 2^32, the sums 2^16, the row sums 2^19"""
    from pnnp_amd import calibrate
    fr = _stack(40, 2, 16, 'ones')
    st = calibrate.DarkStack(2, 16).add(_dev(fr))
    _check_stack(st, fr)
    assert int(st.sumsq[0, 0]) == 40 * 65535 * 65535 > 2 ** 32 and int(st.sum[1, 15]) == 40 * 65535
    assert (st.var_map() == 0).all()


def test_accumulate_in_chunks_equals_one_pass():
    from pnnp_amd import calibrate
    fr = _stack(5, 6, 2058, 'random', seed=9)
    d = _dev(fr)
    whole = calibrate.DarkStack(6, 2058).add(d)
    parts = calibrate.DarkStack(6, 2058)
    for lo, hi in ((0, 2), (2, 3), (3, 5)):                                              # chunks of 2, 1 and 2 frames
        parts.add(d[lo:hi])
    _check_stack(parts, fr)
    assert torch.equal(parts.sum, whole.sum) and torch.equal(parts.sumsq, whole.sumsq) and torch.equal(parts.rowsum, whole.rowsum)
    single = calibrate.DarkStack(6, 2058).add(d[1])                                      # a single [H,W] frame is a chunk of one
    _check_stack(single, fr[1:2])


def test_accumulate_more_frames_than_one_launch_takes():
    """1030 frames: the entry splits a chunk after 1024 frames (the kernel's row slots)"""
    from pnnp_amd import calibrate
    fr = _stack(1030, 2, 8, 'random', seed=3)
    _check_stack(calibrate.DarkStack(2, 8).add(_dev(fr)), fr)


@pytest.mark.parametrize('shape', SHAPES + [(40, 2, 16)], ids=lambda s: 'x'.join(map(str, s)))
def test_residual_is_the_float32_expression(shape):
    from pnnp_amd import calibrate
    N, H, W = shape
    rng = np.random.default_rng(W + N)
    fr = _stack(N, H, W, 'random', seed=W)
    ds = (rng.normal(0, 300, (H, W)) + rng.choice([0.0, 512.0, 65535.0], (H, W))).astype(np.float32)
    ro = rng.normal(0, 3, (N, H, 2)).astype(np.float32)
    assert (ds < 0).any() or H * W < 8
    got = calibrate.residuals(_dev(fr), _dev(ds), _dev(ro))
    assert got.dtype == torch.float32 and got.shape == (N, H, W)
    assert np.array_equal(got.cpu().numpy().view(np.int32), R.residual(fr, ds, ro).view(np.int32))


# ---------------------------------------------------------------------------- fit_dark against the restatement
WP, BL = 16383, 512
FLOAT_FIELDS = ('sigGs', 'sigGssig', 'sigTL', 'sigTLsig', 'sigR', 'sigRsig', 'biassig', 'sigGs_f', 'sigTL_f', 'sigR_f', 'm_f', 'v_res', 'v_row',
                'rowoff', 'lam_corr', 'black_level_error')


@pytest.fixture(scope='module')
def seeded():
    """bl + shading + per-(row, parity) offsets + a per-frame offset + Tukey-lambda read noise, rounded to uint16; fitted once by the restatement"""
    from scipy import stats
    rng = np.random.default_rng(20)
    N, H, W = 32, 64, 128
    shading = rng.normal(0, 2.0, (H, W)) + np.linspace(0, 6, W)[None]
    rows = np.repeat(rng.normal(0, 1.3, (N, H, 2))[:, :, None, :], W // 2, axis=2).reshape(N, H, W)
    read = stats.tukeylambda.rvs(-0.08, scale=2.5, size=(N, H, W), random_state=rng)
    frames = np.rint(BL + shading[None] + rows + rng.normal(0, 0.4, (N, 1, 1)) + read).clip(0, 65535).astype(np.uint16)
    given = (BL + shading + rng.normal(0, 0.05, (H, W))).astype(np.float32)               # a map measured elsewhere
    return dict(frames=frames, given=given, ref=R.fit_dark(frames, 1.7, WP, BL), ref_given=R.fit_dark(frames, 1.7, WP, BL, darkshading=given))


def _check_fit(got, ref, N):
    assert set(('Kmax', 'lam', 'sigGs', 'sigGssig', 'sigTL', 'sigTLsig', 'sigR', 'sigRsig', 'bias', 'biassig', 'q', 'wp', 'bl')) <= set(got)
    assert got['Kmax'] == 1.7 and got['bias'] == 0 and got['q'] == 1 / (WP + 1) and got['wp'] == WP and got['bl'] == BL
    assert got['n_frames'] == N and got['iso'] == 800
    assert np.array_equal(got['darkshading'].cpu().numpy().view(np.int32), ref['darkshading'].view(np.int32))
    # the order statistics: bit for bit CPU torch.quantile of the reference residual
    want_q = ref['quantiles32'].astype(np.float64)
    print(f"quantiles: {int((got['quantiles'] != want_q).sum())} of {want_q.size} differ, max |difference| {np.abs(got['quantiles'] - want_q).max():.3e}")
    assert np.array_equal(got['quantiles'], want_q)
    assert got['lam'] == ref['lam']
    for k in FLOAT_FIELDS:
        a, b = np.asarray(got[k], np.float64), np.asarray(ref[k], np.float64)
        assert a.shape == b.shape, k
        err, scale = np.abs(a - b).max(), np.abs(b).max()
        print(f'{k}: max error {err:.3e}, largest magnitude {scale:.3e}')
        assert err <= 1e-9 * scale, (k, err, scale)                                      # only v_res (the device's float64 sum) differs at all


def test_fit_dark_matches_the_restatement(seeded):
    from pnnp_amd import calibrate
    fr, ref = seeded['frames'], seeded['ref']
    d = _dev(fr)
    st = calibrate.DarkStack(64, 128).add(d)
    _check_stack(st, fr)
    got = calibrate.fit_dark(d, 800, 1.7, WP, BL)
    _check_fit(got, ref, 32)
    assert -0.3 < got['lam'] < 0.3 and 2.0 < got['sigTL'] < 3.0 and 1.0 < got['sigR'] < 1.6      # and it measures what was put in
    res = calibrate.residuals(d, got['darkshading'], torch.from_numpy(ref['rowoff'].astype(np.float32)).cuda())
    assert np.array_equal(res.cpu().numpy().view(np.int32), ref['residual'].view(np.int32))


def test_fit_dark_in_chunks_and_with_a_given_shading(seeded):
    from pnnp_amd import calibrate
    fr = seeded['frames']
    d = _dev(fr)
    _check_fit(calibrate.fit_dark([d[:7], d[7:8], d[8:]], 800, 1.7, WP, BL), seeded['ref'], 32)
    got = calibrate.fit_dark(d, 800, 1.7, WP, BL, darkshading=_dev(seeded['given']))
    _check_fit(got, seeded['ref_given'], 32)
    assert got['sigTL'] != seeded['ref']['sigTL']                                        # c = 1 and another map: another number
    one = calibrate.fit_dark(d[:1], 800, 1.7, WP, BL, darkshading=_dev(seeded['given']))  # a single frame works with a given map
    ref1 = R.fit_dark(fr[:1], 1.7, WP, BL, darkshading=seeded['given'])
    _check_fit(one, ref1, 1)
    assert one['sigTLsig'] == 0 and one['biassig'] == 0
    with pytest.raises(calibrate.PnnpError, match='at least 2'):
        calibrate.fit_dark(d[:1], 800, 1.7, WP, BL)


# ---------------------------------------------------------------------------- the round trip through the shipped sampler
TRUE = dict(K=1.0, sigGs=3.0, sigTL=3.2, lam=-0.05, sigR=1.0, q=1 / 16384, ratio=1.0, wp=WP, bl=BL, bias=0)
BARS = dict(sigTL=0.056113, lam=0.011216, sigR=0.039041, sigGs=0.036589)


def test_round_trip_through_the_sampler():
    """Dark frames drawn by the shipped sampler with known parameters, calibrated, give the parameters back.

    64 frames of [4,64,128] (mosaics 128 x 256), generate_noisy_torch(zeros, 'pgr', tukey=True, ori=True, clip=False), * (wp - bl) + bl,
    rounded to uint16, through rggb2bayer.  ``sigGs`` is compared with the normal-scale value of the Tukey-lambda law that was drawn
    (the slope of its quantiles on the normal quantiles, 6.282404).

    The bars are |mean error| + 5 std over 24 seeds of the REFERENCE alone: the C oracle sampler's stacks fitted by tests/_calib_ref.py
    (tools/calib_bars.py --seeds 24 --frames 64 --h 64 --w 128 --lam-points 1201; profiles/r7/calib.txt):
        parameter   true        mean        mean error  std         bar         bar / true
        sigTL       3.200000    3.231231   +0.031231    0.004976    0.056113    0.018
        lam        -0.050000   -0.042854   +0.007146    0.000814    0.011216    0.224
        sigR        1.000000    0.999100   -0.000900    0.007628    0.039041    0.039
        sigGs       6.282404    6.266345   -0.016059    0.004106    0.036589    0.006
    The biases are the estimators' (the mean-subtracted, rounded residual of a finite stack is more Gaussian than its source), part of the
    bar and not tuned away.  Two choices follow the same measurement at the smaller stack of 32 frames of [4,32,64], where the bar of lam
    was 0.0295, 59 % of the parameter: the stack was raised to this size, and lam is searched on a grid of 1201 points over the default
    range [-0.3, 0.3] -- on the default 121 points every seed returns the same grid point, the spread is 0 and the bar degenerates
    to the grid's rounding of the bias."""
    from pnnp_amd import calibrate, isp_ops, process
    process.manual_seed(7)
    z = process.generate_noisy_torch(torch.zeros(64, 4, 64, 128, device='cuda'), noise_code='pgr', tukey=True, ori=True, clip=False, param=TRUE)
    dn = (z * (WP - BL) + BL).round().clamp(0, 65535).to(torch.uint16)
    frames = torch.stack([isp_ops.rggb2bayer(f.permute(1, 2, 0).contiguous()) for f in dn])
    assert frames.shape == (64, 128, 256) and frames.dtype == torch.uint16
    assert np.array_equal(frames.cpu().numpy(), R.planes_to_mosaics(z.cpu().numpy(), WP, BL))
    fit = calibrate.fit_dark(frames, 1600, TRUE['K'], WP, BL, lam_grid=np.linspace(-0.3, 0.3, 1201))
    want = dict(sigTL=TRUE['sigTL'], lam=TRUE['lam'], sigR=TRUE['sigR'], sigGs=R.matching_sigGs(TRUE['sigTL'], TRUE['lam']))
    for k, bar in BARS.items():
        print(f'{k}: {fit[k]:.6f}, true {want[k]:.6f}, error {fit[k] - want[k]:+.6f}, bar {bar}')
    for k, bar in BARS.items():
        assert abs(fit[k] - want[k]) <= bar, (k, fit[k], want[k], bar)
    assert np.abs(fit['black_level_error']).max() < 0.1 and fit['biassig'] < 0.1


def test_registered_camera_reaches_the_train_step():
    from pnnp_amd import calibrate, process
    from pnnp_amd.archs import UNetSeeInDark
    from pnnp_amd.trainer import HipTrainStep
    table = process._SPEC['SonyA7S2']
    per_iso = {iso: dict(table[str(iso)], wp=4095, bl=240, q=1 / 4096) for iso in (100, 400, 1600)}
    try:
        process.register_camera('cam_gpu', per_iso=per_iso, regression=calibrate.fit_regression(per_iso))
        net = UNetSeeInDark(dict(nframes=1, res=False, nf=8, in_nc=4, out_nc=4)).cuda()
        ts = HipTrainStep(net, lr=1e-4, camera_type='cam_gpu', noise_code='prq')
        hr = torch.rand(1, 4, 32, 32, generator=torch.Generator().manual_seed(1)).cuda()
        np.random.seed(11)
        want = process.pack_params([process.sample_params_max(camera_type='cam_gpu', ratio=None)], hr.device)
        np.random.seed(11)
        _, rows = ts.make_noisy(hr)
        assert torch.equal(rows, want) and float(rows[0, 7]) == 4095 and float(rows[0, 8]) == 240
        out = ts.step(hr)
        assert out.shape == (2,) and bool(torch.isfinite(out).all())
        np.random.seed(12)
        p = process.sample_params_max(camera_type='cam_gpu', iso=400)
        assert p['wp'] == 4095 and p['lam'] == table['400']['lam']
    finally:
        process._SPEC.pop('cam_gpu', None)
        process._REG.pop('cam_gpu', None)


# ---------------------------------------------------------------------------- row_denoise
@pytest.mark.parametrize('iso', [100, 6400])
@pytest.mark.parametrize('hw', [(8, 16), (52, 40)], ids=['8x16', '52x40'])
def test_row_denoise(hw, iso):
    """a plane has H / 2 = 4 rows (the window of 25 reaches the replicated border from every row) or 26 (from most)"""
    from pnnp_amd import calibrate, isp_algos
    H, W = hw
    rng = np.random.default_rng(H + iso)
    data = (512 + rng.normal(0, 1.0, (H, W)) + rng.normal(0, 3.0, (H, 1))).astype(np.float32)
    data[H // 2] += 40                                                                   # a banding step several sigmaColor high
    want = R.row_denoise(data, iso)
    got = calibrate.row_denoise(torch.from_numpy(data).cuda(), iso)
    assert got.dtype == torch.float64 and got.shape == (H, W) and got.is_cuda
    err = np.abs(got.cpu().numpy() - want).max() / np.abs(want).max()
    print(f'row_denoise {H}x{W} iso {iso}: max error {err:.3e}')
    assert err <= 1e-12
    again = isp_algos.row_denoise(None, iso, data=data)                                  # numpy in, numpy out, the reference's signature
    assert isinstance(again, np.ndarray) and np.array_equal(again, got.cpu().numpy())
    assert np.abs(want - data).max() > 0.05                                              # and the filter does something

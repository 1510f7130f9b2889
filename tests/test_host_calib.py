"""Dark-frame calibration, the part that needs no GPU: the float64 restatement (tests/_calib_ref.py) against closed forms, fit_regression,
register_camera, the refusals (each before any launch or device call) and the exported entries."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import _calib_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ('pnnp_calib_accum_u16', 'pnnp_calib_residual_u16', 'pnnp_calib_rowmean_f32')


# ---------------------------------------------------------------------------- the restatement against closed forms
def test_ref_constant_stack():
    """every pixel 700 in 5 frames: sums 5 * 700, zero variance, zero row offsets and residuals, black-level error 700 - 512"""
    fr = np.full((5, 4, 6), 700, np.uint16)
    s, ss, rs = R.accumulate(fr)
    assert (s == 3500).all() and (ss == 5 * 490000).all() and rs.shape == (5, 4, 2) and (rs == 3 * 700).all()
    assert (R.dark_shading(s, 5) == np.float32(700)).all() and (R.var_map(s, ss, 5) == 0).all()
    assert np.array_equal(R.black_level_error(s, 5, 512), np.full(4, 188.0))
    with np.errstate(invalid='ignore'):                                                  # all quantiles equal: the correlation is 0 / 0
        fit = R.fit_dark(fr, K=1.0, wp=16383, bl=512, nq=10)
    assert (fit['residual'] == 0).all() and (fit['rowoff'] == 0).all() and (fit['v_res'] == 0).all() and fit['sigR'] == 0 and fit['biassig'] == 0
    assert fit['q'] == 1 / 16384 and fit['Kmax'] == 1.0 and fit['bias'] == 0 and fit['n_frames'] == 5


def test_ref_two_frames_by_hand():
    """H x W = 2 x 4, two frames that differ by a per-(row, parity) offset pattern: everything worked by hand"""
    a = np.array([[10, 20, 10, 20], [30, 40, 30, 40]], np.uint16)
    off = np.array([[2, 6, 2, 6], [4, 0, 4, 0]], np.uint16)                             # frame 1 = frame 0 + these
    fr = np.stack([a, a + off])
    s, ss, rs = R.accumulate(fr)
    assert np.array_equal(s, 2 * a.astype(np.int64) + off) and np.array_equal(ss, a.astype(np.int64) ** 2 + (a.astype(np.int64) + off) ** 2)
    assert np.array_equal(rs[0], [[20, 40], [60, 80]]) and np.array_equal(rs[1], [[24, 52], [68, 80]])
    assert np.array_equal(R.var_map(s, ss, 2), off.astype(np.float64) ** 2 / 2)          # two samples d apart: variance d^2 / 2
    assert np.array_equal(R.black_level_error(s, 2, 0), [11.0, 23.0, 40.0, 32.0])       # planes (0,0), (0,1), (1,1), (1,0)
    with np.errstate(invalid='ignore'):
        fit = R.fit_dark(fr, K=2.0, wp=1023, bl=64, nq=4)
    half = off[:, :2].astype(np.float64) / 2                                             # rowoff = -+ half the offset, per (row, parity)
    assert np.array_equal(fit['rowoff'][0], -half) and np.array_equal(fit['rowoff'][1], half)
    assert (fit['residual'] == 0).all()                                                  # the offsets explain the frames completely
    assert np.array_equal(fit['m_f'], [-1.5, 1.5]) and fit['biassig'] == pytest.approx(np.sqrt(4.5), rel=1e-15)
    v_row = np.var([1.0, 3.0, 2.0, 0.0], ddof=1)
    assert np.allclose(fit['v_row'], v_row, rtol=1e-15) and np.allclose(fit['sigR_f'], np.sqrt(2 * v_row), rtol=1e-15)   # c = N / (N - 1) = 2
    assert fit['q'] == 1 / 1024 and fit['sigRsig'] == 0


def test_ref_residual_is_two_float32_roundings():
    fr = np.array([[[65535, 3], [1, 0]]], np.uint16)
    ds = np.array([[0.1, -1e-3], [1.0000001, 3e-8]], np.float32)
    ro = np.array([[[1e-4, 0.3], [-7.0, 1e9]]], np.float32)
    want = np.empty((1, 2, 2), np.float32)
    for y in range(2):
        for x in range(2):
            want[0, y, x] = np.float32(np.float32(np.float32(fr[0, y, x]) - ds[y, x]) - ro[0, y, x])
    assert np.array_equal(R.residual(fr, ds, ro).view(np.int32), want.view(np.int32))


def test_ref_bilateral_filter():
    """a constant vector is a fixed point; far below sigmaColor it is the normalised Gaussian blur with a replicated border"""
    assert np.allclose(R.bilateral_1d(np.full(30, 3.25), 100), 3.25, rtol=1e-15)
    m = np.sin(np.arange(40) / 3.0) * 1e-6
    ss, k = 1 + 400 / 200, np.arange(-12, 13)
    w = np.exp(-k * k / (2 * ss * ss))
    want = np.array([(w * m[np.clip(i + k, 0, 39)]).sum() / w.sum() for i in range(40)])
    assert np.allclose(R.bilateral_1d(m, 400), want, rtol=1e-9, atol=1e-18)
    step = np.r_[np.zeros(20), np.full(20, 1000.0)]                                      # an edge 100 sigmaColor high survives
    assert np.allclose(R.bilateral_1d(step, 100), step, atol=1e-12)
    from pnnp_amd import calibrate
    x = np.random.default_rng(1).normal(500, 4, 77)
    for iso in (100, 6400):
        assert np.allclose(calibrate.bilateral_1d(x, iso), R.bilateral_1d(x, iso), rtol=1e-13)


def test_product_fit_statistics_match_the_restatement():
    from pnnp_amd import calibrate
    rng = np.random.default_rng(2)
    t, q = np.sort(rng.normal(size=50)), np.sort(rng.normal(size=(3, 50)) * 2.5 + 1)
    assert np.array_equal(calibrate.slope(t, q), R.slope(t, q)) and np.array_equal(calibrate.corr(t, q), R.corr(t, q))
    assert np.array_equal(calibrate.probabilities(1000), R.probabilities(1000)) and calibrate.probabilities(1000).dtype == np.float32
    assert R.slope(t, 3 * t + 7) == pytest.approx(3, rel=1e-14) and R.corr(t, 3 * t + 7) == pytest.approx(1, rel=1e-14)


# ---------------------------------------------------------------------------- fit_regression, register_camera
def test_fit_regression_reproduces_a_line():
    from pnnp_amd import calibrate, process
    table = process._SPEC['SonyA7S2']
    line = dict(TL=(0.74, 0.86), R=(0.79, -0.34), Gs=(0.83, 1.49))
    per_iso = {}
    for iso in ('100', '400', '1600', '6400'):
        row = dict(table[iso])
        for X, (k, b) in line.items():
            row['sig' + X] = float(np.exp(k * np.log(row['Kmax']) + b))
        per_iso[iso] = row
    reg = calibrate.fit_regression(per_iso)
    for X, (k, b) in line.items():
        assert reg[f'sig{X}k'] == pytest.approx(k, rel=1e-12) and reg[f'sig{X}b'] == pytest.approx(b, rel=1e-12) and reg[f'sig{X}sig'] < 1e-13
    assert reg['Kmin'] == np.log(table['100']['Kmax']) and reg['Kmax'] == np.log(table['6400']['Kmax'])
    assert reg['lam'] == pytest.approx(np.mean([table[i]['lam'] for i in per_iso]), rel=1e-15)
    assert (reg['q'], reg['wp'], reg['bl']) == (table['100']['q'], 16383, 512)
    assert set(reg) == set(process._REG['IMX686'])
    # the table's own values: the line through real measurements has a residual spread, and two ISOs leave none
    real = calibrate.fit_regression({i: table[i] for i in ('100', '400', '1600')})
    assert real['sigTLsig'] > 0 and 0 < real['sigGsk'] < 2
    assert calibrate.fit_regression({i: table[i] for i in ('100', '400')})['sigRsig'] < 1e-13
    with pytest.raises(calibrate.PnnpError, match='at least 2'):
        calibrate.fit_regression({'100': table['100']})
    with pytest.raises(calibrate.PnnpError, match='positive'):
        calibrate.fit_regression({'100': table['100'], '400': dict(table['400'], sigR=0.0)})
    with pytest.raises(calibrate.PnnpError, match='disagree'):
        calibrate.fit_regression({'100': table['100'], '400': dict(table['400'], wp=4095)})


def test_register_camera():
    from pnnp_amd import calibrate, process
    table = process._SPEC['SonyA7S2']
    for name in ('SonyA7S2', 'IMX686', 'NikonD850', 'SonyA7S2_lowISO', 'CRVD'):
        with pytest.raises(ValueError, match='built-in'):
            process.register_camera(name, per_iso={'100': table['100']})
    with pytest.raises(ValueError, match='lacks'):
        process.register_camera('cam_t', per_iso={'100': {'Kmax': 1.0}})
    with pytest.raises(ValueError, match='per_iso, regression or both'):
        process.register_camera('cam_t')
    with pytest.raises(ValueError, match='lacks'):
        process.register_camera('cam_t', regression={'Kmin': 0.0})
    assert process.get_specific_noise_params('cam_t', 100) is None
    try:
        extra = dict(table['400'], darkshading=object(), n_frames=7, Kmax=np.float64(0.5), wp=1023, bl=64, q=1 / 1024)
        per_iso = {100: dict(table['100'], wp=1023, bl=64, q=1 / 1024), '400': extra}
        process.register_camera('cam_t', per_iso=per_iso, regression=calibrate.fit_regression(per_iso))
        row = process.get_specific_noise_params('cam_t', iso=400)
        assert set(row) == set(table['400']) and row['Kmax'] == 0.5 and type(row['Kmax']) is float and row['wp'] == 1023
        assert process.get_specific_noise_params('cam_t', '100')['sigTL'] == table['100']['sigTL']
        with pytest.raises(KeyError):
            process.get_specific_noise_params('cam_t', 200)
        np.random.seed(4)
        p = process.sample_params_max(camera_type='cam_t', iso=400)
        np.random.seed(4)
        K = 0.5 * (1 + np.random.uniform(low=-0.01, high=+0.01))
        assert p['K'] == K and p['lam'] == table['400']['lam'] and p['wp'] == 1023 and p['bl'] == 64 and p['bias'] == 0
        reg = process.get_camera_noisy_params('cam_t')
        assert reg['wp'] == 1023 and reg['Kmax'] == np.log(0.5)
        np.random.seed(4)
        p = process.sample_params_max(camera_type='cam_t', ratio=None)                  # the regression row, not the NikonD850 fall-back
        assert p['wp'] == 1023 and abs(np.log(p['K']) - np.log(0.5)) <= 0.01 and 1 <= p['ratio'] <= np.exp(2.08)
        hbr = process.HighBitRecovery(camera_type='cam_t', noise_code='pgrq', perturb=False)
        hbr.get_lut([400])
        assert hbr.lut[400]['param']['wp'] == 1023 and hbr.lut[400]['kind'] == 1
        process.register_camera('cam_t', per_iso={'800': per_iso['400']})                # a registered name is replaced
        assert list(process._SPEC['cam_t']) == ['800'] and 'cam_t' in process._REG
    finally:
        process._SPEC.pop('cam_t', None)
        process._REG.pop('cam_t', None)


# ---------------------------------------------------------------------------- refusals and exports
@pytest.fixture(scope='module')
def lib():
    path = os.path.join(REPO, 'pnnp_amd', 'libpnnp_hip.so')
    if not os.path.exists(path):
        import __graft_entry__ as g
        g.build()
    return C.CDLL(path)


def test_library_exports_the_entries(lib):
    header = open(os.path.join(REPO, 'include', 'pnnp_hip.h')).read()
    for name in ENTRIES:
        assert getattr(lib, name) is not None and f'int {name}(' in header
    assert lib.pnnp_abi_version() == 9
    assert "'calib.hip': ['-ffp-contract=off']" in open(os.path.join(REPO, 'tools', 'build.py')).read()
    assert 'THE 1-D BILATERAL FILTER' in header


def test_c_entries_refuse_before_a_launch(lib):
    """PNNP_E_INVALID (-1) without touching a pointer: the addresses below are never dereferenced on the host and nothing is launched"""
    fake = C.c_void_p(0x1000)
    acc = lambda n, H, W, fr=fake, s=fake, ss=fake, rs=fake: lib.pnnp_calib_accum_u16(fr, n, H, W, s, ss, rs, None)
    res = lambda n, H, W, fr=fake, ds=fake, ro=fake, out=fake: lib.pnnp_calib_residual_u16(fr, n, H, W, ds, ro, out, None)
    for fn in (acc, res):
        assert fn(1, 3, 8) == -1 and fn(1, 8, 7) == -1 and fn(1, 0, 8) == -1 and fn(1, 8, 0) == -1 and fn(1, 1, 1) == -1      # odd or below 2
        assert fn(0, 8, 8) == -1 and fn(-1, 8, 8) == -1 and fn(32769, 8, 8) == -1                                             # the int32 sum
        assert fn(1, 8, 65538) == -1                                                                                          # the int32 row sum
        assert fn(1, 8, 8, fr=None) == -1 and fn(1, 8, 8, fr=C.c_void_p(0x1001)) == -1
    assert acc(1, 8, 8, s=None) == -1 and acc(1, 8, 8, ss=None) == -1 and acc(1, 8, 8, rs=None) == -1
    assert acc(1, 8, 8, s=C.c_void_p(0x1002)) == -1 and acc(1, 8, 8, ss=C.c_void_p(0x1004)) == -1 and acc(1, 8, 8, rs=C.c_void_p(0x1002)) == -1
    assert res(1, 8, 8, ds=None) == -1 and res(1, 8, 8, ro=None) == -1 and res(1, 8, 8, out=None) == -1 and res(1, 8, 8, out=C.c_void_p(0x1002)) == -1
    rm = lambda H, W, m=fake, o=fake: lib.pnnp_calib_rowmean_f32(m, H, W, o, None)
    assert rm(0, 8) == -1 and rm(8, 0) == -1 and rm(8, 8, m=None) == -1 and rm(8, 8, o=None) == -1 and rm(8, 8, o=C.c_void_p(0x1004)) == -1


def test_wrappers_refuse_before_any_device_call():
    """CPU tensors: a refusal that came after the first device call would be the 'got a CPU tensor' error instead"""
    from pnnp_amd import calibrate as K, isp_algos
    from pnnp_amd._lib import PnnpError
    for H, W in ((3, 8), (8, 7), (0, 8), (8, 1)):
        with pytest.raises(PnnpError, match='even sides'):
            K.DarkStack(H, W)
    with pytest.raises(PnnpError, match='at most 65536'):
        K.DarkStack(2, 65538)
    st = K.DarkStack(4, 8)                                                              # allocates nothing before the first chunk
    u16 = torch.zeros(2, 4, 8, dtype=torch.uint16)
    with pytest.raises(PnnpError, match='uint16'):
        st.add(u16.to(torch.int16))
    with pytest.raises(PnnpError, match='uint16'):
        st.add(np.zeros((2, 4, 8), np.uint16))
    with pytest.raises(PnnpError, match=r'expected \[n,H,W\]'):
        st.add(torch.zeros(2, 4, 10, dtype=torch.uint16))
    with pytest.raises(PnnpError, match='contiguous'):
        st.add(torch.zeros(2, 4, 16, dtype=torch.uint16)[:, :, ::2])
    st.n = 32767
    with pytest.raises(PnnpError, match='at most 32768'):
        st.add(u16)
    st.n = 0
    with pytest.raises(PnnpError, match='CPU tensor'):
        st.add(u16)                                                                      # the last check: everything else was in order
    assert st.n == 0 and st._sum is None
    with pytest.raises(PnnpError, match='at least 1'):
        st.dark_shading()
    ds, ro = torch.zeros(4, 8), torch.zeros(2, 4, 2)
    with pytest.raises(PnnpError, match='uint16'):
        K.residuals(u16.float(), ds, ro)
    with pytest.raises(PnnpError, match='even sides'):
        K.residuals(torch.zeros(2, 3, 8, dtype=torch.uint16), torch.zeros(3, 8), torch.zeros(2, 3, 2))
    with pytest.raises(PnnpError, match='ds must be'):
        K.residuals(u16, ds.double(), ro)
    with pytest.raises(PnnpError, match='rowoff must be'):
        K.residuals(u16, ds, torch.zeros(2, 4))
    with pytest.raises(PnnpError, match='CPU tensor'):
        K.residuals(u16, ds, ro)
    with pytest.raises(PnnpError, match='uint16'):
        K.fit_dark(u16.float(), 100, 1.0, 16383, 512)
    with pytest.raises(PnnpError, match='no frames'):
        K.fit_dark([], 100, 1.0, 16383, 512)
    with pytest.raises(PnnpError, match=r'expected \[n,H,W\]'):
        K.fit_dark([u16, torch.zeros(2, 4, 10, dtype=torch.uint16)], 100, 1.0, 16383, 512)
    with pytest.raises(PnnpError, match='nq'):
        K.fit_dark(u16, 100, 1.0, 16383, 512, nq=1)
    with pytest.raises(PnnpError, match='darkshading must be'):
        K.fit_dark(u16, 100, 1.0, 16383, 512, darkshading=torch.zeros(4, 8, dtype=torch.float64))
    with pytest.raises(PnnpError, match='data='):
        isp_algos.row_denoise('dark_iso100.npy', 100)
    with pytest.raises(PnnpError, match='data='):
        isp_algos.row_denoise('dark_iso100.npy', 100, data=None)

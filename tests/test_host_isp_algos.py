"""The classical raw filters (csrc/isp_algos.hip) as far as they can be checked without a GPU: tests/_isp_algos_ref.py, the restatement
the kernels are tested against, is pinned to frames worked out by hand and to the real functions' recorded outputs
(tests/golden/isp_algos*.npz); the built library exports every new entry; the C entries and the wrappers refuse bad arguments before
any device call."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests import _isp_algos_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
ENTRIES = ['pnnp_guided_ab_f32', 'pnnp_guided_apply_f32', 'pnnp_stdfilt_f32', 'pnnp_vst_f32', 'pnnp_bayer2gray_f32', 'pnnp_repair_bad_pixels']
META = json.load(open(os.path.join(HERE, 'golden', 'isp_algos.json')))
FILTERS = {c['tag']: c for c in META['filters']}


@pytest.fixture(scope='module')
def gold():
    g = dict(np.load(os.path.join(HERE, 'golden', 'isp_algos.npz')))
    g.update(np.load(os.path.join(HERE, 'golden', 'isp_algos_b.npz')))
    return g


# ---------------------------------------------------------------------------- the restatement against hand-computed frames
# 4 x 4, window 3.  REPLICATE pads to        REFLECT_101 pads to
#    1  1  2  3  4  4                          6  5  6  7  8  7
#    1  1  2  3  4  4                          2  1  2  3  4  3
#    5  5  6  7  8  8                          6  5  6  7  8  7
#    9  9 10 11 12 12                         10  9 10 11 12 11
#   13 13 14 15 16 16                         14 13 14 15 16 15
#   13 13 14 15 16 16                         10  9 10 11 12 11
# corner (0,0): REPLICATE 1+1+2 + 1+1+2 + 5+5+6 = 24; REFLECT_101 6+5+6 + 2+1+2 + 6+5+6 = 39.
# (0,1): REPLICATE 1+2+3 + 1+2+3 + 5+6+7 = 30; REFLECT_101 5+6+7 + 1+2+3 + 5+6+7 = 42.  Interior (1,1): 1+2+3+5+6+7+9+10+11 = 54 for both.
# (3,3): REPLICATE 11+12+12 + 15+16+16 + 15+16+16 = 129; REFLECT_101 11+12+11 + 15+16+15 + 11+12+11 = 114.
HAND4 = np.arange(1, 17, dtype=np.float32).reshape(4, 4)
SUMS_REPLICATE = {(0, 0): 24, (0, 1): 30, (1, 1): 54, (3, 3): 129}
SUMS_REFLECT = {(0, 0): 39, (0, 1): 42, (1, 1): 54, (3, 3): 114}


@pytest.mark.parametrize('separable', [False, True])
def test_box_mean_hand_values(separable):
    for border, sums in ((R.BORDER_REPLICATE, SUMS_REPLICATE), (R.BORDER_REFLECT_101, SUMS_REFLECT)):
        got = R.box_mean(HAND4, 3, border, separable=separable)
        assert got.dtype == np.float32
        for (y, x), s in sums.items():
            assert got[y, x] == np.float32(s * (1.0 / 9)), (border, y, x)
    assert np.array_equal(R.box_mean(HAND4, 1, R.BORDER_REPLICATE), HAND4)
    assert np.array_equal(R.boxFilter(HAND4, -1, (3, 3)), R.box_mean(HAND4, 3, R.BORDER_REFLECT_101))          # cv2's default border
    assert np.array_equal(R.blur(HAND4, (3, 3)), R.box_mean(HAND4, 3, R.BORDER_REFLECT_101))
    with pytest.raises(AssertionError):
        R.box_mean(HAND4, 9, R.BORDER_REFLECT_101)                                                              # 9 // 2 >= 4
    wide = R.box_mean(HAND4, 9, R.BORDER_REPLICATE)                                                             # REPLICATE takes any size
    # 9 x 9 around (0,0): rows -4..4 -> row 0 five times, rows 1..3 once, row 3 once more; the same for the columns
    wy = np.array([5, 1, 1, 2], np.float64)
    assert wide[0, 0] == np.float32((wy[:, None] * wy[None, :] * HAND4).sum() * (1.0 / 81))


def test_box_mean_sums_in_float64():
    # 2^24 + 1 + 1 + ... : a float32 sum would lose every 1 (the one row is replicated into all five of the window)
    x = np.ones((1, 5), np.float32)
    x[0, 0] = 2.0 ** 24
    got = R.box_mean(x, 5, R.BORDER_REPLICATE)
    assert got[0, 2] == np.float32(5 * (2.0 ** 24 + 4) * (1.0 / 25)) and got[0, 2] != np.float32(5 * 2.0 ** 24 * (1.0 / 25))
    assert got[0, 0] == np.float32(5 * (3 * 2.0 ** 24 + 2) * (1.0 / 25))


def test_resizes_hand_values():
    x = np.array([[1, 3, 5, 7], [9, 11, 13, 15], [2, 4, 6, 8], [10, 12, 14, 0]], np.float32)
    assert np.array_equal(R.resize_half(x), np.array([[6, 10], [7, 7]], np.float32))                            # (1+3+9+11)/4, ..., (6+8+14+0)/4
    lo = np.array([[0, 4], [8, 16]], np.float32)
    # a line [s0, s1] upsampled: s0, 0.75 s0 + 0.25 s1, 0.25 s0 + 0.75 s1, s1; rows first, then columns
    hz = np.array([[0, 1, 3, 4], [8, 10, 14, 16]], np.float32)
    want = np.stack([hz[0], 0.75 * hz[0] + 0.25 * hz[1], 0.25 * hz[0] + 0.75 * hz[1], hz[1]]).astype(np.float32)
    assert np.array_equal(R.resize_double(lo), want)
    assert np.array_equal(R.resize(lo, None, fx=2, fy=2, interpolation=R.INTER_LINEAR), want)
    one = np.array([[5.0]], np.float32)
    assert np.array_equal(R.resize_double(one), np.full((2, 2), 5, np.float32))
    five = np.arange(5, dtype=np.float32)[None, :].repeat(2, 0)                                                 # 5 wide: interior weights alternate
    assert np.array_equal(R.resize_double(five)[0], np.array([0, 0.25, 0.75, 1.25, 1.75, 2.25, 2.75, 3.25, 3.75, 4], np.float32))


def test_filter2d_and_median_hand_values():
    # 5 x 5 with one hot pixel; BORDER_REFLECT repeats the edge pixel
    x = np.zeros((5, 5), np.float32)
    x[0, 0], x[2, 2] = 16, 32
    g = R.bayer2gray(x)
    assert g[0, 0] == 9 and g[0, 1] == 3 and g[1, 1] == 1 + 2 and g[1, 0] == 3      # corner: weights 4 + 2 + 2 + 1 fall on the edge pixel
    assert g[2, 2] == 8 and g[2, 1] == 4 and g[1, 2] == 4 and g[3, 3] == 2 and g[4, 4] == 0
    m = np.array([[9, 1, 2, 3, 4], [5, 6, 7, 8, 0], [10, 11, 99, 13, 14], [15, 16, 17, 18, 19], [20, 21, 22, 23, 24]], np.uint16)
    med = R.medianBlur(m, 3)
    assert med.dtype == np.uint16
    assert med[2, 2] == 13            # 6 7 8 11 99 13 16 17 18 -> 13
    assert med[0, 0] == 6             # REPLICATE: 9 9 1 9 9 1 5 5 6 -> 1 1 5 5 6 9 9 9 9 -> 6
    assert med[0, 4] == 4             # 3 4 4 3 4 4 8 0 0 -> 0 0 3 3 4 4 4 4 8 -> 4
    # repair: colour planes at stride 2; two hot neighbours of one plane both read the unmodified frame
    raw = np.arange(64, dtype=np.uint16).reshape(8, 8)
    raw[2, 2], raw[2, 4] = 60000, 60001
    fixed = R.repair_bad_pixels(raw.copy(), [(2, 2), (2, 4), (2, 2)])
    plane = raw[0::2, 0::2]
    assert fixed[2, 2] == np.sort(plane[0:3, 0:3].reshape(-1))[4] and fixed[2, 4] == np.sort(plane[0:3, 1:4].reshape(-1))[4]
    assert fixed[2, 2] == 32          # 0 2 4 | 16 60000 60001 | 32 34 36 -> the fifth is 32
    assert fixed[2, 4] == 34          # 2 4 6 | 60000 60001 22 | 34 36 38 -> the fifth is 34: with (2,2) repaired to 32 first it would be 32
    changed = fixed != raw
    assert changed.sum() == 2


# ---------------------------------------------------------------------------- the goldens reproduce from the restatement
def _inputs(gold, c):
    return (gold[c['x']],) if c['fn'] == 'stdfilt' else (gold[c['p']], gold[c['I']])


@pytest.mark.parametrize('tag', sorted(FILTERS))
def test_filter_goldens_reproduce(gold, tag):
    c = FILTERS[tag]
    fn = getattr(R, c['fn'])
    args = [a.reshape(-1, *a.shape[-2:]) for a in _inputs(gold, c)]
    kw = dict(k=c['d']) if c['fn'] == 'stdfilt' else dict(d=c['d'], eps=c['eps'])
    ref32, d64 = gold[tag + '_ref32'], gold[tag + '_d64']
    ref64 = ref32.astype(np.float64) + d64
    got32 = np.stack([fn(*[a[i] for a in args], **kw) for i in range(args[0].shape[0])]).reshape(ref32.shape)
    got64 = np.stack([fn(*[a[i].astype(np.float64) for a in args], **kw) for i in range(args[0].shape[0])]).reshape(ref32.shape)
    assert got32.dtype == np.float32 and np.array_equal(got32.view(np.int32), ref32.view(np.int32))
    assert got64.dtype == np.float64 and np.array_equal(got64.view(np.int64), ref64.view(np.int64))
    e_ref = float(np.abs(ref32.astype(np.float64) - ref64).max())
    assert e_ref == c['e_ref'] and e_ref > 0 and c['sep_diff'] <= 1e-3 * ref32.size
    assert list(ref32.shape) == c['shape']


def test_other_goldens_reproduce(gold):
    x, y = gold['vst_x'], gold['ivst_x']
    assert x.size % 4 != 0 and (x < 0).any() and (x == 0).any()
    assert {(c['gain'], c['wp']) for c in META['vst']} == {(g, w) for g in (0.5, 1, 3.7) for w in (1, 16383)}
    assert any(c['sigma'] == 0 for c in META['vst']) and any(c['mu'] != 0 for c in META['vst'])
    for c in META['vst']:
        f, b = R.VST(x, c['sigma'], c['mu'], c['gain'], c['wp']), R.inverse_VST(y, c['sigma'], c['gain'], c['wp'])
        assert f.dtype == np.float32 and np.array_equal(f.view(np.int32), gold['vst_' + c['tag']].view(np.int32)), c
        assert np.array_equal(b.view(np.int32), gold['ivst_' + c['tag']].view(np.int32)), c
    assert np.array_equal(R.VST(x, 1.5).view(np.int32), gold['vst_default'].view(np.int32))
    for hw in ('6x10', '34x70'):
        assert np.array_equal(R.bayer2gray(gold[f'gray_{hw}_x']).view(np.int32), gold[f'gray_{hw}_out'].view(np.int32))
    for c in META['repair']:
        raw, pts = gold[f"repair_{c['tag']}_in"], gold[f"repair_{c['tag']}_pts"]
        assert pts.shape == (c['n'], 2) and raw.dtype == np.dtype(c['dtype'])
        assert np.array_equal(R.repair_bad_pixels(raw.copy(), [tuple(p) for p in pts]), gold[f"repair_{c['tag']}_out"])


def test_fixture_files_are_small():
    for name in ('isp_algos.npz', 'isp_algos_b.npz', 'isp_algos.json'):
        assert os.path.getsize(os.path.join(HERE, 'golden', name)) < (1 << 20), name


# ---------------------------------------------------------------------------- the library and the wrappers
@pytest.fixture(scope='module')
def lib():
    path = os.path.join(REPO, 'pnnp_amd', 'libpnnp_hip.so')
    if not os.path.exists(path):
        import __graft_entry__ as g
        g.build()
    return C.CDLL(path)


def test_library_exports_the_entries(lib):
    for name in ENTRIES:
        assert getattr(lib, name) is not None
    assert lib.pnnp_abi_version() == 9
    header = open(os.path.join(REPO, 'include', 'pnnp_hip.h')).read()
    for name in ENTRIES:
        assert f'int {name}(' in header
    flags = open(os.path.join(REPO, 'tools', 'build.py')).read()
    assert "'isp_algos.hip': ['-ffp-contract=off']" in flags


def test_c_entries_refuse_before_a_launch(lib):
    """PNNP_E_INVALID (-1) without touching a pointer: the addresses below are never dereferenced on the host and nothing is launched"""
    fake = C.c_void_p(0x1000)
    s = (C.c_int64 * 3)(64 * 64, 64, 1)
    ab = lambda N, H, W, d, flags, p=fake, st=s: lib.pnnp_guided_ab_f32(p, fake, N, H, W, st, d, C.c_float(1.0), flags, fake, fake, None)
    assert ab(1, 64, 64, 6, 0) == -1 and ab(1, 64, 64, 53, 0) == -1 and ab(1, 64, 64, 0, 0) == -1 and ab(1, 64, 64, -3, 0) == -1
    assert ab(1, 3, 64, 7, 1) == -1 and ab(1, 64, 3, 7, 1) == -1                   # REFLECT_101: 7 // 2 >= 3
    assert ab(1, 6, 64, 7, 2) == -1                                                # half: 7 // 2 >= 6 / 2
    assert ab(1, 63, 64, 7, 2) == -1 and ab(1, 64, 62 + 1, 7, 2) == -1             # half: odd sides
    assert ab(0, 64, 64, 7, 0) == -1 and ab(65536, 64, 64, 7, 0) == -1 and ab(1, 0, 64, 7, 0) == -1 and ab(1, 64, 64, 7, 4) == -1
    assert ab(1, 64, 64, 7, 0, p=None) == -1 and ab(1, 64, 64, 7, 0, p=C.c_void_p(0x1002)) == -1 and ab(1, 64, 64, 7, 0, st=None) == -1
    assert ab(1, 64, 64, 7, 0, st=(C.c_int64 * 3)(4096, 64, 0)) == -1
    assert lib.pnnp_guided_ab_f32(fake, fake, 1, 64, 64, s, 7, C.c_float(float('nan')), 0, fake, fake, None) == -1
    ap = lambda H, W, d, flags, ws=fake: lib.pnnp_guided_apply_f32(fake, fake, fake, 1, H, W, s, d, flags, ws, fake, s, None)
    assert ap(64, 64, 8, 0) == -1 and ap(64, 64, 53, 0) == -1 and ap(63, 64, 7, 2) == -1 and ap(64, 64, 7, 2, ws=None) == -1 and ap(4, 64, 7, 2) == -1
    sf = lambda H, W, k: lib.pnnp_stdfilt_f32(fake, 1, H, W, s, k, fake, s, None)
    assert sf(64, 64, 4) == -1 and sf(64, 64, 53) == -1 and sf(2, 64, 5) == -1 and sf(64, 2, 5) == -1
    vst = lambda n, inv, gain, wp, x=fake: lib.pnnp_vst_f32(x, C.c_int64(n), inv, C.c_double(1.0), C.c_double(0.0), C.c_double(gain), C.c_double(wp),
                                                            None, C.c_int64(1), fake, None)
    assert vst(0, 0, 1.0, 1.0) == -1 and vst(8, 2, 1.0, 1.0) == -1 and vst(8, 0, 0.0, 1.0) == -1 and vst(8, 1, 1.0, 0.0) == -1 and vst(8, 0, 1.0, 1.0, x=None) == -1
    assert lib.pnnp_bayer2gray_f32(fake, 1, 0, 8, C.c_void_p(0x2000), None) == -1 and lib.pnnp_bayer2gray_f32(fake, 1, 8, 8, fake, None) == -1
    rp = lambda es, H, W, n, pts=fake: lib.pnnp_repair_bad_pixels(fake, es, H, W, pts, n, fake, None)
    assert rp(1, 8, 8, 1) == -1 and rp(2, 7, 8, 1) == -1 and rp(2, 8, 9, 1) == -1 and rp(4, 8, 8, -1) == -1 and rp(2, 8, 8, 1, pts=None) == -1
    assert rp(2, 8, 8, 0) == 0 and rp(2, 8, 8, 0, pts=None) == 0                   # no points: nothing to do, nothing launched


def test_wrappers_refuse_before_any_device_call():
    """CPU tensors: a refusal that came after the first device call would be the 'got a CPU tensor' error instead"""
    from pnnp_amd import isp_algos as A, isp_ops
    from pnnp_amd._lib import PnnpError
    x = torch.zeros(8, 12)
    for fn in (A.GuidedFilter, A.FastGuidedFilter):
        with pytest.raises(PnnpError, match='odd'):
            fn(x, x, d=4)
        with pytest.raises(PnnpError, match='at most 51'):
            fn(x, x, d=53)
    with pytest.raises(PnnpError, match='odd'):
        A.stdfilt(x, k=6)
    with pytest.raises(PnnpError, match='at most 51'):
        A.stdfilt(x, k=53)
    with pytest.raises(PnnpError, match='even sides'):
        A.FastGuidedFilter(torch.zeros(7, 12), torch.zeros(7, 12))
    with pytest.raises(PnnpError, match='even sides'):
        A.FastGuidedFilter(torch.zeros(2, 8, 9), torch.zeros(2, 8, 9), layout='chw')
    with pytest.raises(PnnpError, match='REFLECT_101'):
        A.stdfilt(torch.zeros(3, 12), k=7)                                         # 7 // 2 >= 3
    with pytest.raises(PnnpError, match='REFLECT_101'):
        A.FastGuidedFilter(torch.zeros(6, 12), torch.zeros(6, 12), d=7)            # 7 // 2 >= 6 / 2
    with pytest.raises(PnnpError, match='agree'):
        A.GuidedFilter(x, torch.zeros(8, 10))
    with pytest.raises(PnnpError, match='float32'):
        A.GuidedFilter(x.to(torch.float16), x.to(torch.float16))
    with pytest.raises(PnnpError, match='layout'):
        A.stdfilt(x, layout='nchw')
    with pytest.raises(PnnpError, match='must not be 0'):
        A.VST(x, 1.0, gain=0)
    with pytest.raises(PnnpError, match='CPU tensor'):
        A.GuidedFilter(torch.zeros(3, 12), torch.zeros(3, 12), d=51)               # REPLICATE takes a window taller than the frame
    raw = torch.zeros(8, 12, dtype=torch.uint16)
    for pt in ((8, 0), (0, 12), (-1, 3), (3, -1)):
        with pytest.raises(PnnpError, match='outside'):
            isp_ops.repair_bad_pixels(raw, [(1, 1), pt])
    with pytest.raises(PnnpError, match='even sides'):
        isp_ops.repair_bad_pixels(torch.zeros(7, 12, dtype=torch.uint16), [(1, 1)])
    assert isp_ops.repair_bad_pixels(raw, []) is raw                               # an empty list: a no-op, also without a device
    with pytest.raises(PnnpError, match='float32 mosaic'):
        isp_ops.bayer2gray(raw)
    with pytest.raises(PnnpError, match='float32 mosaic'):
        isp_ops.bayer2gray(np.zeros((8, 12), np.uint16))


def test_evaluate_signature_keeps_its_defaults():
    import inspect
    from pnnp_amd import evaluate as E
    assert inspect.signature(E.evaluate).parameters['baseline'].default is None
    assert inspect.signature(E.EvalLoop.__init__).parameters['baseline'].default is None
    loop = E.EvalLoop(net=None)
    _, text = loop.finish(epoch=3)
    assert 'baseline' not in text and text.count('\n') == 2

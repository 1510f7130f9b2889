"""Op-level parity of the step-glue kernels of csrc/misc.hip (layout, 2x2 max-pool, channel_sum, clamp + L1 loss, Adam) and of
ops.amax, each against a plain CPU reference of the same operation: exact where the op is a copy, a select or one multiply-add,
float64 with a bar DERIVED from the kernel's summation order (never measured) where it sums.  The shapes are the smallest that
take every path of a kernel: fewer items than one block, ragged tails, and one shape past the launch cap of grid1d (2048 blocks
x 256 threads = 524 288 items; 256 blocks = 65 536 items for the layout kernel with an amax slot) so that the grid-stride loop
takes a second trip.  Every output buffer starts as NaN (or as a recognisable value where the op accumulates)."""
import functools
import itertools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = 'cuda'
U = 2.0 ** -24                      # float32 unit roundoff
NAN = float('nan')
INF = float('inf')
GRID_ITEMS = 2048 * 256             # grid1d's cap: items of one grid-stride trip
GRID_ITEMS_AMAX = 256 * 256         # ... of nchw_to_nhwc with an amax slot (below 2^22 items)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def _nan(*shape):
    return torch.full(shape, NAN, device=DEV)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _fbits(v):
    return int(torch.tensor([float(v)], dtype=torch.float32).view(torch.int32)[0])


def _slot(v=0.0):
    """An amax slot (csrc/h2.h) holding the bit pattern of the non-negative float ``v``."""
    return torch.tensor([float(v)], dtype=torch.float32).view(torch.int32).to(DEV)


def _slot_bits(s):
    return int(s.cpu()[0])


def _refused(fn, *untouched):
    """``fn`` raises PnnpError and none of the NaN-filled (255-filled for bytes) buffers was written."""
    from pnnp_amd._lib import PnnpError
    with pytest.raises(PnnpError):
        fn()
    torch.cuda.synchronize()
    for t in untouched:
        assert bool((t == 255).all() if t.dtype == torch.uint8 else torch.isnan(t).all())


# ------------------------------------------------------------------------------------------------------------------ ops.amax
@pytest.mark.parametrize('n', [1, 63, 64, 65, 300001])          # 300 001: 128 blocks x 256 threads x 4 floats = 131 072 per trip, three trips + a tail of 1
def test_amax_is_max_abs_as_bits_and_only_raises(n):
    from pnnp_amd import ops
    x = _rand(n, seed=n)
    x[-1] = -(float(x.abs().max()) + 1.25)                          # the maximum, negative, in the last element
    want = _fbits(x.abs().max())
    xd = x.to(DEV)
    s = _slot(0.0); ops.amax(xd, s)
    assert _slot_bits(s) == want
    s = _slot(1000.0); ops.amax(xd, s)
    assert _slot_bits(s) == _fbits(1000.0)                          # raise-only: a slot above stays
    s = _slot(1e-3); ops.amax(xd, s)
    assert _slot_bits(s) == want                                    # ... one below is raised
    s = _slot(0.0); ops.amax(torch.zeros(n, device=DEV), s)
    assert _slot_bits(s) == 0
    if n > 1:                                                       # a 4-byte aligned view: the kernel's scalar path
        s = _slot(0.0); ops.amax(xd[1:], s)
        assert _slot_bits(s) == want


# ------------------------------------------------------------------------------------------------------------------ 1. layout
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('C,more', [(c, m) for c in (1, 3, 4, 5, 8) for m in (0, 4)])
def test_nchw_to_nhwc_exact(B, C, more):
    from pnnp_amd import ops
    H, W, Cp = 7, 9, (C + 3) // 4 * 4 + more
    x = _rand(B, C, H, W, seed=C + more)
    dst = _nan(B, H, W, Cp)
    ops.nchw_to_nhwc(x.to(DEV), dst, Cp)
    got = dst.cpu()
    assert torch.equal(got[..., :C], nhwc(x))
    assert _same_bits(got[..., C:], torch.zeros(B, H, W, Cp - C))   # padding channels: exactly +0


@pytest.mark.parametrize('pad', [1, 16, 18])                        # 18 = min(H, W) - 1, the largest F.pad accepts
@pytest.mark.parametrize('Cp', [4, 8])
def test_nchw_to_nhwc_reflect_pad_equals_torch(pad, Cp):
    from pnnp_amd import ops
    B, C, H, W = 2, 3, 19, 23
    x = _rand(B, C, H, W, seed=pad)
    x[1, 2, H - 1, W - 1] = -7.5
    dst = _nan(B, H + 2 * pad, W + 2 * pad, Cp)
    s = _slot(0.0)
    ops.nchw_to_nhwc(x.to(DEV), dst, Cp, reflect_pad=pad, amax=s)
    got = dst.cpu()
    assert torch.equal(got[..., :C], nhwc(F.pad(x, (pad, pad, pad, pad), mode='reflect')))
    assert _same_bits(got[..., C:], torch.zeros_like(got[..., C:]))
    assert _slot_bits(s) == _fbits(7.5)                             # still max |x| of the source
    dst2 = _nan(B, H + 2 * pad, W + 2 * pad, Cp)
    ops.nchw_to_nhwc(x.to(DEV), dst2, Cp, reflect_pad=pad)          # the entry without a slot
    assert _same_bits(dst2, dst)


def test_nchw_to_nhwc_second_trip():
    from pnnp_amd import ops
    B, C, H, W, Cp = 3, 4, 300, 301, 8
    assert B * H * W * (Cp // 4) > GRID_ITEMS
    x = _rand(B, C, H, W, seed=1)
    dst = _nan(B, H, W, Cp)
    ops.nchw_to_nhwc(x.to(DEV), dst, Cp)
    assert torch.equal(dst[..., :C], nhwc(x).to(DEV))
    assert int(torch.count_nonzero(dst[..., C:])) == 0 and not bool(torch.isnan(dst).any())


def test_nchw_to_nhwc_amax_second_trip():
    from pnnp_amd import ops
    B, C, H, W, Cp = 2, 3, 130, 257, 8
    assert GRID_ITEMS_AMAX < B * H * W * (Cp // 4) < (1 << 22)
    x = _rand(B, C, H, W, seed=2)
    x[-1, -1, -1, -1] = -3.0                                        # the largest |value|: only the second trip reads it
    dst = _nan(B, H, W, Cp)
    s = _slot(0.0)
    ops.nchw_to_nhwc(x.to(DEV), dst, Cp, amax=s)
    assert torch.equal(dst[..., :C], nhwc(x).to(DEV))
    assert int(torch.count_nonzero(dst[..., C:])) == 0 and not bool(torch.isnan(dst).any())
    assert _slot_bits(s) == _fbits(3.0)


def test_nchw_to_nhwc_amax_slot():
    from pnnp_amd import ops
    B, C, H, W, Cp = 2, 3, 7, 9, 4
    x = _rand(B, C, H, W, seed=3)
    x[1, 0, 3, 4] = -float(x.abs().max()) * 1.5
    want = _fbits(x.abs().max())
    for preset, after in ((0.0, want), (1e-3, want), (64.0, _fbits(64.0))):
        s = _slot(preset)
        ops.nchw_to_nhwc(x.to(DEV), _nan(B, H, W, Cp), Cp, amax=s)
        assert _slot_bits(s) == after, preset
    s = _slot(0.0)
    ops.nchw_to_nhwc(torch.zeros(B, C, H, W, device=DEV), _nan(B, H, W, Cp), Cp, amax=s)
    assert _slot_bits(s) == 0                                       # an all-zero input leaves a zero slot at zero


@pytest.mark.parametrize('B,H,W,C', [(2, 7, 9, 3), (2, 7, 9, 4), (2, 300, 301, 3)])
@pytest.mark.parametrize('residual', [False, True])
def test_nhwc_to_nchw_exact(B, H, W, C, residual):
    from pnnp_amd import ops
    assert H < 100 or B * C * H * W > GRID_ITEMS                     # the last shape: a second grid-stride trip
    src = _rand(B, H, W, 8, seed=C)                                 # channels >= C hold values that must not leak
    res = _rand(B, C, H, W, seed=C + 1) if residual else None
    dst = _nan(B, C, H, W)
    ops.nhwc_to_nchw(src.to(DEV), dst, residual=res.to(DEV) if residual else None)
    ref = nchw(src[..., :C])
    assert torch.equal(dst.cpu(), ref + res if residual else ref)   # one float32 add


def test_layout_refusals():
    from pnnp_amd import ops
    x = _rand(2, 5, 7, 9, seed=4).to(DEV)
    big = _nan(2, 7 + 2 * 9, 9 + 2 * 9, 8)
    _refused(lambda: ops.nchw_to_nhwc(x, big, 4), big)                                # Cp < C
    _refused(lambda: ops.nchw_to_nhwc(x, big, 6), big)                                # Cp not a multiple of 4
    _refused(lambda: ops.nchw_to_nhwc(x, big, 8, reflect_pad=7), big)                 # pad >= H
    _refused(lambda: ops.nchw_to_nhwc(x.transpose(2, 3).contiguous(), big, 8, reflect_pad=7), big)   # pad >= W
    out = _nan(2, 5, 7, 9)
    _refused(lambda: ops.nhwc_to_nchw(_nan(2, 7, 9, 4), out), out)                    # Cp < C


# ------------------------------------------------------------------------------------------------------------------ 2. max-pool
def _place_windows(wins, C=4):
    """Windows (rows of 4 values in the order (0,0) (0,1) (1,0) (1,1)) -> NHWC [1, 4, 2 n, C]; every channel and window row sees
    the list in another rotation."""
    wins = np.asarray(wins, dtype=np.float32)
    n = len(wins)
    x = np.empty((1, 4, 2 * n, C), dtype=np.float32)
    for r in range(2):
        for c in range(C):
            w = np.roll(wins, 5 * c + 11 * r, axis=0)
            for k in range(4):
                x[0, 2 * r + k // 2, (k % 2)::2, c] = w[:, k]
    return torch.from_numpy(x)


@functools.lru_cache(None)
def _tie_input():
    """Every non-empty subset of the four positions sharing the window's maximum (positive and negative maxima), windows with
    +0.0 / -0.0, and negative-only windows."""
    wins = []
    for mx in (0.75, -0.5):
        for r in range(1, 5):
            for S in itertools.combinations(range(4), r):
                wins.append([mx if k in S else mx - 1.0 - 0.25 * k for k in range(4)])
    wins += [[0.0, -0.0, -1.0, -2.0], [-0.0, 0.0, -1.0, -1.0], [-0.0] * 4, [0.0] * 4, [-1.0, -0.0, 0.0, -3.0], [-3.0, -2.0, -1.0, -0.0],
             [0.0, 0.5, -0.0, 0.5], [-1.0, -2.0, -3.0, -4.0], [-4.0, -3.0, -2.0, -1.0], [-2.0, -1.0, -1.0, -3.0]]
    return _place_windows(wins)


@functools.lru_cache(None)
def _big_pool_input():
    B, H, W, C = 2, 258, 260, 64
    assert B * (H // 2) * (W // 2) * (C // 4) > GRID_ITEMS
    return _rand(B, H, W, C, seed=11)


def _pool_input(name):
    if name == 'tie':
        return _tie_input()
    if name == 'big':
        return _big_pool_input()
    return _rand(*name, seed=sum(name))


def _windows(x):
    """NHWC numpy -> [B, H/2, W/2, C, 4], the window in the order (0,0) (0,1) (1,0) (1,1)."""
    B, H, W, C = x.shape
    return x.reshape(B, H // 2, 2, W // 2, 2, C).transpose(0, 1, 3, 5, 2, 4).reshape(B, H // 2, W // 2, C, 4)


def _ref_codes(x):
    """bits 0-1: np.argmax (the first maximum); bits 2-5: x > 0 of the four window elements.  Finite windows only."""
    w = _windows(x.numpy())
    code = np.argmax(w, axis=-1).astype(np.uint8)
    for k in range(4):
        code |= (w[..., k] > 0).astype(np.uint8) << (2 + k)
    return torch.from_numpy(code)


def _code_errors(codes, x, only=None):
    """Decode the bytes the kernel wrote against the window contents, field by field."""
    w = _windows(x.numpy())
    c = codes.cpu().numpy()
    sel = np.ones(c.shape, dtype=bool) if only is None else only
    errs = []
    bad = ((c & 3) != np.argmax(w, axis=-1)) & sel
    if bad.any():
        errs.append(('argmax bits 0-1', int(bad.sum()), np.argwhere(bad)[:3].tolist()))
    for k in range(4):
        bad = (((c >> (2 + k)) & 1) != (w[..., k] > 0)) & sel
        if bad.any():
            errs.append((f'sign bit {2 + k}', int(bad.sum()), np.argwhere(bad)[:3].tolist()))
    bad = ((c >> 6) != 0) & sel
    if bad.any():
        errs.append(('bits 6-7 not zero', int(bad.sum())))
    return errs


@pytest.mark.parametrize('name', [(1, 2, 2, 4), (2, 6, 10, 12), 'tie', 'big'], ids=str)
def test_maxpool_fwd_and_codes(name):
    from pnnp_amd import ops
    x = _pool_input(name)
    B, H, W, C = x.shape
    xd = x.to(DEV)
    y = _nan(B, H // 2, W // 2, C)
    ops.maxpool_fwd(xd, y)
    assert torch.equal(nchw(y.cpu()), F.max_pool2d(nchw(x), 2))
    y2 = _nan(B, H // 2, W // 2, C)
    codes = torch.full((B, H // 2, W // 2, C), 255, dtype=torch.uint8, device=DEV)
    ops.maxpool_fwd(xd, y2, codes=codes)
    assert _same_bits(y2, y)                                        # the codes-writing forward: the same y bit for bit
    errs = _code_errors(codes, x)
    assert not errs, errs
    if name == 'tie':                                               # both zeros are "not positive"; argmax is non-trivial
        c = codes.cpu().numpy(); w = _windows(x.numpy())
        assert (((c[..., None] >> (2 + np.arange(4))) & 1)[w == 0] == 0).all()
        assert len(np.unique(c & 3)) == 4


def _act(t, mode):
    return F.leaky_relu(t, 0.2) if mode == 1 else (F.relu(t) if mode == 2 else t)


@pytest.mark.parametrize('mode', [0, 1, 2])
@pytest.mark.parametrize('name', ['tie', 'big'])
def test_maxpool_bwd_both_kernels_equal_autograd(name, mode):
    """gx (+)= route(gy) * act'(x) is one multiply and one add per element: the float32 reference (autograd of
    max_pool2d(act(pre)), whose tie rule -- the first maximum -- is the kernels', plus the base in the same order) must be met
    exactly.  The codes come from the numpy reference, not from the forward kernel."""
    from pnnp_amd import ops
    x = _pool_input(name)
    B, H, W, C = x.shape
    pre = nchw(x).requires_grad_(True)
    a = _act(pre, mode)
    gy = _rand(B, C, H // 2, W // 2, seed=20 + mode)
    F.max_pool2d(a, 2).backward(gy)
    route = nhwc(pre.grad)
    ad = nhwc(a.detach())
    codes = _ref_codes(ad).to(DEV)
    base = _rand(B, H, W, C, seed=30)
    base[-1, -1, -1, -1] = -1000.0                                  # the largest |stored value| when accumulating: the last item (second trip at 'big')
    ad, gyd = ad.to(DEV), nhwc(gy).to(DEV)
    for accumulate in (0, 1):
        want = (base + route if accumulate else route).to(DEV)
        start = base.to(DEV) if accumulate else _nan(B, H, W, C)
        gx = start.clone()
        ops.maxpool_bwd(ad, gyd, gx, mode, accumulate)
        assert torch.equal(gx, want), ('from x', accumulate, int((gx != want).sum()))
        gx = start.clone()
        s = _slot(0.0)
        ops.maxpool_bwd(ad, gyd, gx, mode, accumulate, codes=codes, amax_gx=s)
        assert torch.equal(gx, want), ('from codes', accumulate, int((gx != want).sum()))
        amax_bits = _fbits(want.abs().max())
        assert _slot_bits(s) == amax_bits, ('amax_gx', accumulate)  # max |stored gx|, the accumulated base included
        gx = start.clone()
        s = _slot(1e6)
        ops.maxpool_bwd(ad, gyd, gx, mode, accumulate, codes=codes, amax_gx=s)
        assert _slot_bits(s) == _fbits(1e6)                         # raise-only
        gx = start.clone()
        ops.maxpool_bwd(ad, gyd, gx, mode, accumulate, codes=codes)  # the entry without a slot
        assert torch.equal(gx, want)


def _nan_rule(x):
    """The pool's semantics on non-finite data (include/pnnp_hip.h): value = fmax over the window (NaN only if all four are),
    argmax = a scan from position 0 that moves on `x[k] > x[arg]` only (false against a NaN), sign bit = x > 0 (0 for a NaN)."""
    w = _windows(x.numpy())
    with np.errstate(invalid='ignore'):
        val = np.fmax(np.fmax(w[..., 0], w[..., 1]), np.fmax(w[..., 2], w[..., 3]))
        arg = np.zeros(w.shape[:-1], dtype=np.uint8); best = w[..., 0].copy()
        for k in range(1, 4):
            up = w[..., k] > best
            arg[up] = k; best[up] = w[..., k][up]
        code = arg.copy()
        for k in range(4):
            code |= (w[..., k] > 0).astype(np.uint8) << (2 + k)
    return torch.from_numpy(val), torch.from_numpy(code), torch.from_numpy(np.isnan(w).any(-1))


def _check_pool_of(x, pooled, codes):
    """Pooled values and codes of NHWC ``x`` (CPU) against the stated semantics; every window without a NaN against torch."""
    val, code, has_nan = _nan_rule(x)
    p = pooled.cpu(); c = codes.cpu()
    tref = nhwc(F.max_pool2d(nchw(x), 2))
    assert torch.equal(p[~has_nan], tref[~has_nan])
    errs = _code_errors(c, torch.nan_to_num(x, nan=0.0, posinf=INF, neginf=-INF), only=~has_nan.numpy())
    assert not errs, errs
    assert torch.equal(torch.isnan(p), torch.isnan(val)) and torch.equal(p[~torch.isnan(val)], val[~torch.isnan(val)])
    assert torch.equal(c, code)


def test_maxpool_non_finite_windows():
    from pnnp_amd import ops
    wins = [[NAN, 1.0, 2.0, 3.0], [1.0, 2.0, 3.0, NAN], [NAN] * 4, [INF, NAN, 1.0, 2.0], [NAN, INF, 1.0, 2.0], [-INF, NAN, -INF, -INF],
            [1.0, NAN, NAN, -2.0], [NAN, -1.0, -3.0, NAN], [INF, INF, 1.0, 2.0], [-INF] * 4, [-INF, -1.0, -INF, -2.0], [3.0, -INF, INF, 0.5],
            [0.25, 0.5, -0.5, 0.5], [-1.0, -2.0, -0.5, -0.5]]
    x = _place_windows(wins)
    B, H, W, C = x.shape
    xd = x.to(DEV)
    y = _nan(B, H // 2, W // 2, C); ops.maxpool_fwd(xd, y)
    y2 = torch.zeros_like(y); codes = torch.full(y.shape, 255, dtype=torch.uint8, device=DEV)
    ops.maxpool_fwd(xd, y2, codes=codes)
    assert _same_bits(y2, y)
    _check_pool_of(x, y, codes)


def _fused_pool_input():
    B, H, W, cin, cout = 2, 32, 64, 32, 32
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, H, W, cin, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) * 0.1
    b = torch.randn(cout, generator=g) * 0.1
    return x.to(DEV), w.to(DEV), b.to(DEV), cout


def _plant_non_finite(x):
    """One NaN per image (after any amax of the clean input was taken): the 3x3 patch of NaN outputs around an (even, even) pixel
    covers windows at positions {3}, {2,3}, {1,3} and all four; around an (odd, odd) pixel {0}, {0,1}, {0,2} and all four."""
    x[0, 6, 6, 3] = NAN
    x[1, 13, 21, 0] = NAN
    x[1, 24, 40, 5] = INF
    return x


@pytest.mark.parametrize('family', ['x3', 'h2'])
def test_fused_pool_epilogues_agree_with_the_pool_kernels_on_nan(family):
    """conv + LeakyReLU + MaxPool2d(2) in one kernel, with a NaN in the conv input: the pooled map and the codes it writes are
    bit-identical to what the two stand-alone pool kernels make of the full-resolution map the same launch stored."""
    from pnnp_amd import ops
    x, w, b, cout = _fused_pool_input()
    B, H, W, cin = x.shape
    y = _nan(B, H, W, cout); p = _nan(B, H // 2, W // 2, cout)
    c = torch.full(p.shape, 255, dtype=torch.uint8, device=DEV)
    jobs = ops.PackJobs()
    if family == 'x3':
        wx = torch.empty(ops.x3_weight_bytes(cin, cout), dtype=torch.uint8, device=DEV)
        jobs.add_x3(w, wx, None, cin_pad=cin); jobs.run()
        _plant_non_finite(x)
        ops.conv_x3_fwd_pool(x, None, wx, b, y, p, c, cout, 1)
    else:
        f = torch.zeros(ops.h2_weight_bytes(cin, cout), dtype=torch.uint8, device=DEV)
        sw = jobs.add_h2(w, f, None, cin_pad=cin); jobs.run()
        sx = ops.amax(x, _slot(0.0))                                # the scale of the clean input
        _plant_non_finite(x)
        bits = torch.zeros(ops.h2_bits_words(B, H, W, cout), dtype=torch.int32, device=DEV)
        ops.conv_h2_fwd_pool(x, None, f, sw, b, y, p, c, cout, 1, sx, amax_y=_slot(0.0), bits_y=bits)
    nan_per_window = torch.isnan(torch.from_numpy(_windows(y.cpu().numpy()))).sum(-1)
    assert int(((nan_per_window > 0) & (nan_per_window < 4)).sum()) > 0 and int((nan_per_window == 0).sum()) > 0
    pa = _nan(*p.shape); ops.maxpool_fwd(y, pa)
    pb = _nan(*p.shape); cb = torch.full(p.shape, 255, dtype=torch.uint8, device=DEV)
    ops.maxpool_fwd(y, pb, codes=cb)
    assert _same_bits(pa, p) and _same_bits(pb, p) and torch.equal(cb, c)
    _check_pool_of(y.cpu(), p, c)


# ------------------------------------------------------------------------------------------------------------------ 3. channel_sum
CS_BLOCKS = 1024                    # channel_sum_partial_kernel's grid: the workspace holds 1024 x C partials


@pytest.mark.parametrize('C', [4, 8, 32, 64, 512, 1024])
def test_channel_sum_vs_float64(C):
    """Bar per channel: L 2^-24 sum|x|, L the longest chain of float32 additions of the two kernels, read off their loops:
    a thread adds `trips` = ceil(npix / (1024 ppi)) pixels, thread q of a block adds the ppi = 256 / (C / 4) lanes' sums,
    a row-phase of rows_sum_kernel adds 1024 / 8 block partials and its first row the 8 phases."""
    from pnnp_amd import ops
    ppi = 256 // (C // 4)
    for npix in sorted({1, max(ppi - 1, 1), CS_BLOCKS * ppi + 3, 2 * CS_BLOCKS * ppi + 5}):
        x = _rand(npix, C, seed=C + npix) + 0.25
        xd = x.to(DEV)
        ws = _nan(CS_BLOCKS * C + 64); out = _nan(C)
        ops.channel_sum(xd, out, ws)
        assert not bool(torch.isnan(ws[:CS_BLOCKS * C]).any()), ('a partial was not written', C, npix)   # blocks past the end write zeros
        assert bool(torch.isnan(ws[CS_BLOCKS * C:]).all())
        L = -(-npix // (CS_BLOCKS * ppi)) + ppi + CS_BLOCKS // 8 + 8
        ref = x.double().sum(0); bar = L * U * x.double().abs().sum(0)
        err = (out.cpu().double() - ref).abs()
        assert bool((err <= bar).all()), (C, npix, float((err / bar).max()))
        out2 = _nan(C); ops.channel_sum(xd, out2, _nan(CS_BLOCKS * C))
        assert _same_bits(out2, out)                                # two runs: bit-identical
        out0 = _rand(C, seed=5) * 100
        acc = out0.clone().to(DEV); ops.channel_sum(xd, acc, ws, accumulate=1)
        assert _same_bits(acc, out0 + out.cpu()), (C, npix)         # accumulate: out0 + the sum, one float32 add


def test_channel_sum_refusals():
    from pnnp_amd import ops
    for C in (2, 12, 2048):
        out = _nan(C); ws = _nan(CS_BLOCKS * C)
        _refused(lambda: ops.channel_sum(torch.ones(16, C, device=DEV), out, ws), out, ws)
    out = _nan(8); ws = _nan(CS_BLOCKS * 8)
    _refused(lambda: ops.channel_sum(torch.ones(0, 8, device=DEV), out, ws), out, ws)


# ------------------------------------------------------------------------------------------------------------------ 4. clamp + L1 loss
L1_BPC = 64                         # blocks per crop of l1_clamp_kernel: a thread strides 64 x 256 = 16 384 pixels
BELOW_0 = float(np.nextafter(np.float32(0), np.float32(-1)))
ABOVE_1 = float(np.nextafter(np.float32(1), np.float32(2)))


def _loss_inputs(B, C, H, W, scaled, seed):
    """pred reaches outside [0, 1] (after scaling), hr too; planted on channel 0 of crop 0: the clamp's edges and their float32
    neighbours, pred == hr, and a value that is inside [0, 1] only after scaling."""
    pred = _rand(B, C, H, W, seed=seed) * 0.8 + 0.5
    hr = _rand(B, C, H, W, seed=seed + 1) * 0.7 + 0.5
    scale = None
    r0 = 1.0
    if scaled:
        g = torch.Generator().manual_seed(seed + 2)
        scale = torch.exp(torch.rand(B, generator=g) * math.log(600.0)) * 0.5          # log-uniform in [0.5, 300]
        scale[0] = 0.5; r0 = 0.5
        if B > 1:
            scale[1] = 300.0
        pred = pred / scale[:, None, None, None]
    p0, h0 = pred[0, 0].view(-1), hr[0, 0].view(-1)
    planted = [(0.0, 0.5), (-0.0, 0.5), (1.0 / r0, 0.5), (2 * BELOW_0 if scaled else BELOW_0, 0.5), (ABOVE_1 / r0, 0.5), (0.375 / r0, 0.375),
               (1.0 / r0, 1.0), (0.0, 0.0)]
    if scaled:
        planted.append((1.625, 0.25))                               # 1.625 x 0.5: inside [0, 1] only after scaling
    for i, (pv, hv) in enumerate(planted):
        p0[i] = pv; h0[i] = hv
    if scaled and B > 1:
        pred[1, 0, 0, 0] = 0.5; hr[1, 0, 0, 0] = 0.75                # x 300: inside before scaling, outside after
    if scaled:
        # The kernel forms pred * ratio in float32, the reference in float64.  Where the two products lie on different sides of a
        # clamp edge or of the target (about one element in 2^24) the op is discontinuous and the comparison meaningless: such
        # elements are set to 0 (an exact product).  Decided from the inputs alone.
        s4 = scale[:, None, None, None]
        for _ in range(2):
            p32, p64 = (pred * s4).double(), pred.double() * s4.double()
            amb = ((p32 >= 0) & (p32 <= 1)) != ((p64 >= 0) & (p64 <= 1))
            for t in (hr.double(), hr.double().clamp(0, 1)):
                amb |= torch.sign(p32.clamp(0, 1) - t) != torch.sign(p64.clamp(0, 1) - t)
            pred[amb] = 0.0
        assert not bool(amb.any())
    return pred, hr, scale


def _loss_reference(pred, hr, scale, clamp_target, grad_weight):
    """float64 autograd of F.l1_loss((pred * ratio).clamp(0, 1), target); the SSE always against the clamped target."""
    p = pred.double().requires_grad_(True)
    t = hr.double().clamp(0, 1) if clamp_target else hr.double()
    q = p * scale.double()[:, None, None, None] if scale is not None else p
    loss = F.l1_loss(q.clamp(0, 1), t)
    loss.backward()
    sse = ((q.detach().clamp(0, 1) - hr.double().clamp(0, 1)) ** 2).sum(dim=(1, 2, 3))
    return float(loss.detach()), sse, p.grad * float(np.float32(grad_weight))


def _run_loss(pred, hr, scale, Cp, clamp_target, grad_weight, want_grad=True):
    from pnnp_amd import ops
    B, C, H, W = pred.shape
    g = _nan(B, H, W, Cp) if want_grad else None
    lo = _nan(1 + B); ws = _nan(2 * B * L1_BPC)
    ops.l1_clamp_loss(pred.to(DEV), hr.to(DEV), g, lo, ws, scale=scale.to(DEV) if scale is not None else None,
                      clamp_target=clamp_target, grad_weight=grad_weight)
    return g, lo


LOSS_SHAPES = [(B, C, Cp, hw) for B in (1, 5) for C in (1, 3, 4, 8) for Cp in (4, 8) if Cp >= C for hw in ((3, 5), (16, 24), (130, 131))]


@pytest.mark.parametrize('B,C,Cp,hw', LOSS_SHAPES)
def test_l1_clamp_loss_vs_float64_autograd(B, C, Cp, hw):
    """Loss and per-crop SSE: relative bar L 2^-24, L the longest float32 addition chain of l1_clamp_kernel + l1_finish_kernel:
    a thread adds C terms for each of its ceil(hw / 16384) pixels (64 blocks x 256 threads per crop), the block's LDS tree has
    8 levels, a lane of the finish kernel adds 64 / 64 = 1 block partial, the shuffle tree has 6 levels; the loss then adds the
    B crops.  Gradient: exact sign, magnitude grad_weight ratio_b / (B C H W) within 4 x 2^-24 (the reciprocal and three
    float32 roundings), padding channels exactly 0, nothing left NaN."""
    H, W = hw
    N = B * C * H * W
    L = C * -(-H * W // (L1_BPC * 256)) + 8 + 1 + 6
    for scaled, clamp_target, gw in ((False, False, 1.0), (True, False, 1.0), (False, True, 0.6), (True, True, 0.6)):
        pred, hr, scale = _loss_inputs(B, C, H, W, scaled, seed=B + C + H)
        loss, sse, gref = _loss_reference(pred, hr, scale, clamp_target, gw)
        g, lo = _run_loss(pred, hr, scale, Cp, clamp_target, gw)
        what = (scaled, clamp_target, gw)
        g = g.cpu().double(); lo_c = lo.cpu().double()
        assert not bool(torch.isnan(g).any()), what
        assert _same_bits(g[..., C:].float(), torch.zeros_like(g[..., C:]).float()), what
        got, gref = g[..., :C], nhwc(gref)
        assert torch.equal(torch.sign(got), torch.sign(gref)), (what, int((torch.sign(got) != torch.sign(gref)).sum()))
        assert bool(((got - gref).abs() <= 4 * U * gref.abs()).all()), (what, float(((got - gref).abs() / gref.abs().clamp_min(1e-300)).max() / U))
        ratio = scale.double() if scaled else torch.ones(B, dtype=torch.float64)
        for b in range(B):                                          # every element is 0 or grad_weight ratio_b / N
            nz = torch.unique(gref[b].abs()); nz = nz[nz > 0]
            assert len(nz) >= 1 and bool(((nz - float(np.float32(gw)) * ratio[b] / N).abs() <= 1e-12 * nz).all()), what
        assert abs(float(lo_c[0]) - loss) <= (L + B) * U * loss, (what, 'loss', abs(float(lo_c[0]) - loss) / (U * loss), L + B)
        assert bool(((lo_c[1:] - sse).abs() <= L * U * sse).all()), (what, 'sse', float(((lo_c[1:] - sse).abs() / (U * sse)).max()), L)
        _, lo2 = _run_loss(pred, hr, scale, Cp, clamp_target, gw, want_grad=False)
        assert _same_bits(lo2, lo), what                            # grad_nhwc=None: the same loss and SSE
        if clamp_target:                                            # the SSE is against the clamped target whatever clamp_target says
            _, lo3 = _run_loss(pred, hr, scale, Cp, False, gw, want_grad=False)
            assert _same_bits(lo3[1:], lo[1:]), what
            _, lo4 = _run_loss(pred, hr, scale, Cp, clamp_target, 1.0, want_grad=False)
            assert _same_bits(lo4, lo), what                        # grad_weight touches neither the loss nor the SSE


def test_l1_clamp_loss_planted_edges():
    """What the planted elements of _loss_inputs must give, spelled out (channel 0 of crop 0, pixels 0 ..)."""
    B, C, H, W, Cp = 5, 3, 3, 5, 4
    N = B * C * H * W
    for scaled in (False, True):
        pred, hr, scale = _loss_inputs(B, C, H, W, scaled, seed=1)
        g, _ = _run_loss(pred, hr, scale, Cp, False, 1.0)
        g0 = g.cpu()[0].reshape(-1, Cp)[:, 0].double() * N / (0.5 if scaled else 1.0)
        want = [-1, -1, 1, 0, 0, 0, 0, 0] + ([1] if scaled else [])    # 0, -0, 1 pass; the neighbours outside do not; pred == hr gives 0
        assert torch.allclose(g0[:len(want)], torch.tensor(want, dtype=torch.float64), rtol=1e-6, atol=0), (scaled, g0[:len(want)].tolist())
        if scaled:
            assert float(g.cpu()[1, 0, 0, 0]) == 0.0


def test_l1_clamp_loss_nan_prediction():
    B, C, H, W, Cp = 5, 4, 16, 24, 8
    pred, hr, _ = _loss_inputs(B, C, H, W, False, seed=2)
    _, sse, _ = _loss_reference(pred, hr, None, False, 1.0)
    pred[2, 1, 7, 9] = NAN
    _, lo = _run_loss(pred, hr, None, Cp, False, 1.0)
    lo = lo.cpu().double()
    assert math.isnan(float(lo[0])) and math.isnan(float(lo[3]))
    L = C * 1 + 8 + 1 + 6
    for b in (0, 1, 3, 4):
        assert abs(float(lo[1 + b]) - float(sse[b])) <= L * U * float(sse[b]), b


def test_l1_clamp_loss_refusals():
    from pnnp_amd import ops

    def call(B, C, Cp):
        g = _nan(max(B, 1), 4, 4, Cp); lo = _nan(1 + max(B, 1)); ws = _nan(2 * max(B, 1) * L1_BPC)
        _refused(lambda: ops.l1_clamp_loss(torch.ones(B, C, 4, 4, device=DEV), torch.ones(B, C, 4, 4, device=DEV), g, lo, ws), g, lo, ws)
    call(2, 9, 8)
    call(2, 5, 4)
    call(2, 4, 12)
    call(0, 4, 8)


# ------------------------------------------------------------------------------------------------------------------ 5. Adam
def _f32(v):
    return float(np.float32(v))


def _adam_reference(dtype, p0, grads, m0, v0, step0, lr, b1, b2, eps):
    """torch.optim.Adam on the CPU in ``dtype``, from state (m0, v0, step0); also the float64 trajectory the m / v bars need."""
    p = p0.to(dtype).clone().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps)
    opt.state[p] = dict(step=torch.tensor(float(step0)), exp_avg=m0.to(dtype).clone(), exp_avg_sq=v0.to(dtype).clone())
    mtol = torch.zeros_like(p0, dtype=torch.float64); vtol = torch.zeros_like(mtol)
    for gk in grads:
        m_old = opt.state[p]['exp_avg'].double().clone()
        p.grad = gk.to(dtype)
        opt.step()
        # float32 roundings of one step, each at most 2^-24 of the quantity it rounds:
        #   m: fl(g - m), then fl(m + (1 - b1) (g - m));    v: fl((1 - b2) g), fl(. g), then fl(b2 v + .)
        mtol += U * ((1 - b1) * (gk.double() - m_old).abs() + opt.state[p]['exp_avg'].double().abs())
        vtol += U * (2 * (1 - b2) * gk.double() ** 2 + opt.state[p]['exp_avg_sq'].double())
    st = opt.state[p]
    return p.detach().double(), st['exp_avg'].double(), st['exp_avg_sq'].double(), mtol, vtol


def _adam_case(n, step0=0, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, grad_scale=1.0, steps=3):
    """Three kernel steps against torch.optim.Adam in float64 (the truth) and float32 (the yardstick).  The C ABI takes lr, the betas
    and eps as float32, so both references get those float32 values: 1 - 0.999f differs from 1 - 0.999 by 1.3e-5 relative, a different
    hyper-parameter and not an error of the arithmetic under test.  |p| is drawn from [0.25, 1): the bar's absolute term is one ulp of
    p, and it can tell the kernel from the yardstick only where the update's own float32 error (a few 2^-24 lr) is far below that."""
    from pnnp_amd import ops
    lr, b1, b2, eps = _f32(lr), _f32(b1), _f32(b2), _f32(eps)
    g = torch.Generator().manual_seed(n % 1000 + step0 % 7)
    p0 = (torch.rand(n, generator=g) * 0.75 + 0.25) * (torch.randint(0, 2, (n,), generator=g) * 2 - 1).float()
    grads = [(torch.rand(n, generator=g) * 2 - 1) * 0.1 for _ in range(steps)]
    zero_g = [i for i in (7, n - 2) if 0 <= i < n and n >= 1003]                    # g = 0 throughout (one of them in the tail of n = 2 100 003)
    tiny_g = [i for i in (11,) if n >= 1003]                                        # g = 1e-10: eps dominates the denominator
    for gk in grads:
        if zero_g:
            gk[zero_g] = 0.0
        if tiny_g:
            gk[tiny_g] = 1e-10
    fresh = step0 == 0
    m0 = torch.zeros(n) if fresh else (torch.rand(n, generator=g) * 2 - 1) * 0.05
    v0 = torch.zeros(n) if fresh else torch.rand(n, generator=g) * 0.01
    r64 = _adam_reference(torch.float64, p0, grads, m0, v0, step0, lr, b1, b2, eps)
    r32 = _adam_reference(torch.float32, p0, grads, m0, v0, step0, lr, b1, b2, eps)
    p, m, v = p0.to(DEV), m0.to(DEV), v0.to(DEV)
    assert p.numel() == n
    for i, gk in enumerate(grads):
        ops.adam_step(p, (gk / grad_scale).to(DEV), m, v, lr, step0 + i + 1, beta1=b1, beta2=b2, eps=eps, grad_scale=grad_scale)
    p, m, v = p.cpu(), m.cpu(), v.cpu()
    what = (n, step0, b1, b2, eps, grad_scale)
    ulp = torch.from_numpy(np.spacing(r64[0].abs().float().numpy())).double()
    for name, got, k, tol in (('p', p, 0, ulp), ('m', m, 1, r64[3]), ('v', v, 2, r64[4])):
        ek, e32 = (got.double() - r64[k]).abs(), (r32[k] - r64[k]).abs()
        worst = float((ek / (2 * e32 + tol).clamp_min(1e-300)).max())
        print('adam', what, name, 'worst |kernel - float64| / bar = %.3f' % worst)
        # worst ratio over all cases of this file, from a float32 emulation of adam_kernel's arithmetic on the CPU (with / without fused
        # multiply-adds): p 0.36 / 0.36, m 0.31 / 0.90, v 0.68 / 0.85; the line printed above gives the figure of the run at hand
        assert bool((ek <= 2 * e32 + tol).all()), (what, name, worst, int((ek > 2 * e32 + tol).sum()))
    if fresh and zero_g:
        assert torch.equal(p[zero_g], p0[zero_g]) and float(m[zero_g].abs().max()) == 0 and float(v[zero_g].abs().max()) == 0
    return p, m, v


@pytest.mark.parametrize('n', [1, 2, 3, 5, 1003, 2100003])         # 2 100 003: 525 000 float4s (a second trip) + a tail of 3; 1, 2, 3: the tail only
def test_adam_vs_torch(n):
    """Per element: |kernel - float64| <= 2 |float32 reference - float64| + one ulp of p (m, v: + the float32 roundings of their own
    update chain, summed along the float64 trajectory)."""
    assert n != 2100003 or n // 4 > GRID_ITEMS
    _adam_case(n)


@pytest.mark.parametrize('kw', [dict(grad_scale=0.25), dict(step0=99999), dict(b1=0.8, b2=0.99, eps=1e-6), dict(step0=1, lr=1e-4)], ids=str)
def test_adam_options(kw):
    """grad_scale (the gradient pre-multiplied by 4: the same bits as without), step 100 000 (bias corrections effectively 1, non-zero
    state), step 2 from a non-zero state, non-default betas and eps."""
    p, m, v = _adam_case(1003, **kw)
    if 'grad_scale' in kw:
        q = _adam_case(1003)
        assert _same_bits(p, q[0]) and _same_bits(m, q[1]) and _same_bits(v, q[2])


def test_adam_refusals():
    from pnnp_amd import ops

    def bufs(n):
        return [torch.full((n,), 1.0, device=DEV) for _ in range(4)]
    p, g, m, v = bufs(8)
    _unchanged = lambda: all(bool((t == 1.0).all()) for t in (p, g, m, v))
    _refused(lambda: ops.adam_step(p, g, m, v, 1e-3, 0))                                       # step = 0
    assert _unchanged()
    e = [torch.empty(0, device=DEV) for _ in range(4)]
    _refused(lambda: ops.adam_step(*e, 1e-3, 1))                                               # n = 0
    big = torch.full((9,), 1.0, device=DEV)
    for k in range(4):                                                                         # 4-byte but not 16-byte aligned
        args = [p, g, m, v]; args[k] = big[1:]
        _refused(lambda: ops.adam_step(*args, 1e-3, 1))
    assert _unchanged() and bool((big == 1.0).all())

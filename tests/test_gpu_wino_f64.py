"""The Winograd F(2x2,3x3) kernels (csrc/wino.hip, csrc/wino_wgrad.hip, wino_job of csrc/pack_jobs.hip) op by op against float64, element by element, at
shapes that reach every depth of wino_kernel's pipeline (1, 2, 3, 4, 5 chunks), the switch from src[0] to src[1] at chunk 1, 2, 3 and later with different
pixel strides, a split of the written columns inside a 64-column block, maps smaller than, equal to and one pixel past a 16 x 16 tile, and every class of
wino_wgrad_kernel's chunk loop (1, 2, 3, 4+ chunks per split, a shorter last split, a last split of one chunk, splits that cross an image boundary).
References, the derived bound  |got - ref64| <= (K + 10 + e) 2^-24 S_w 1.01  and the restated launch rules: tests/_wino_ref.py.  Every destination starts as
NaN (or a known base where the launch accumulates) with a guard band of 7.0 behind it; a case asserts the bound for every element, that no NaN is left and
that the guard is untouched, and prints the largest err / (2^-24 S_w) it saw (profiles/r7/wino_f64.txt keeps those of one run on 256 compute units).
tests/test_host_wino_ref.py checks, without a GPU, what the tables below reach and that the float32 emulation of the same inputs stays inside the bounds.

The refusal "a destination stride that is no multiple of 4" (wino_launch, PNNP_E_INVALID) cannot be asked for: every exported entry writes N = C1 + C2
columns with N % 64 == 0 and C1 % 32 == 0, which wino_launch checks first, so both strides are multiples of 32; it has no test here."""
import functools
import math

import pytest
import torch

import _wino_ref as W
from test_gpu_direct_f64 import ALL_ACTS, GUARD, _cus, _dst, _rand, nhwc

pytestmark = pytest.mark.gpu


def _check(what, got, guard, ref, act_map=True, depth=None, skip=None):
    """Every element within bound(ref) (and within the same bound with n = depth), no NaN, guard intact.  skip: a mask of elements judged elsewhere."""
    got = got.detach().cpu().double()
    if act_map:
        got = got.permute(0, 3, 1, 2)
    assert got.shape == ref.ref.shape, (what, got.shape, ref.ref.shape)
    keep = torch.ones_like(got, dtype=torch.bool) if skip is None else ~skip
    nans = int((~torch.isfinite(got) & keep).sum())
    err = (got - ref.ref).abs()
    ratio = float(torch.nan_to_num(err / (W.U * ref.S).clamp_min(1e-300), nan=float('inf'))[keep].max())
    print(f'wino_f64 | {what}: worst err / (2^-24 S_w) = {ratio:.3f}  (bound (n + e) 1.01 = {(ref.n + ref.e) * 1.01:.1f}'
          + (f', by depth {(depth + ref.e) * 1.01:.1f})' if depth else ')'))
    bad = ~(err <= W.bound(ref))
    if depth:
        bad |= ~(err <= W.bound(ref._replace(n=depth)))
    bad &= keep
    assert nans == 0, (what, 'NaN or inf left', nans)
    assert not bad.any(), (what, ratio, int(bad.sum()), got.numel(), bad.nonzero()[:5].tolist())
    assert bool((guard == 7.0).all()), (what, 'guard band written')


# ---------------------------------------------------------------- forward: ops.conv_wino_fwd
# (name, (B, H, W), C1, C2, Cout, variants); a variant is (act, bias, residual)
FWD_CASES = ([(f'depth K {k} on {m}', m, k, 0, 64, ALL_ACTS) for m in ((1, 5, 7), (1, 16, 16)) for k in (8, 16, 24, 32, 40)] +
             [(f'switch {c1} + {c2}', (2, 17, 31), c1, c2, 64, ALL_ACTS) for c1, c2 in ((8, 8), (8, 16), (16, 8), (24, 16), (32, 8), (8, 56))] +
             [(f'map {m}', m, 16, 0, 64, ALL_ACTS) for m in ((1, 1, 1), (1, 1, 40), (1, 33, 1), (1, 15, 17), (1, 16, 16), (1, 17, 15))] +
             [('map (3, 18, 34) Cout 128', (3, 18, 34), 16, 0, 128, ALL_ACTS), ('map (1, 9, 20) Cout 192', (1, 9, 20), 16, 0, 192, ALL_ACTS)])


@functools.lru_cache(maxsize=None)
def fwd_inputs(B, H, W_, C1, C2, Co):
    x1 = _rand(B, C1, H, W_, seed=1); x2 = _rand(B, C2, H, W_, seed=2) if C2 else None
    w = _rand(Co, C1 + C2, 3, 3, seed=3, scale=0.2); b = _rand(Co, seed=4); r = _rand(B, Co, H, W_, seed=9)
    return x1, x2, w, b, r


@pytest.mark.parametrize('case', FWD_CASES, ids=[c[0] for c in FWD_CASES])
def test_wino_fwd_vs_float64(case):
    from pnnp_amd import ops
    name, (B, H, W_), C1, C2, Co, variants = case
    assert W.wino_supported(C1 + C2, Co) and ops.wino_supported(C1 + C2, Co)
    x1, x2, w, b, r = fwd_inputs(B, H, W_, C1, C2, Co)
    xin = torch.cat([x1, x2], 1) if C2 else x1
    u = torch.full((16 * w.shape[0] * w.shape[1],), float('nan'), device='cuda')
    ops.pack_conv_weight_wino(w.cuda(), u, None)
    x1d, x2d, bd, rd = nhwc(x1).cuda(), nhwc(x2).cuda() if C2 else None, b.cuda(), nhwc(r).cuda()
    _, _, grid, nch = W.wino_grid(B, H, W_, C1 + C2, Co)
    for act, use_b, use_r in variants:
        ref = W.conv_fwd(xin, w, b if use_b else None, r if use_r else None, act)
        y, guard = _dst((B, H, W_, Co))
        ops.conv_wino_fwd(x1d, x2d, u, bd if use_b else None, y, Co, act, residual=rd if use_r else None)
        _check(f'conv_wino_fwd {name} grid {grid} chunks {nch} act {act} bias {use_b} residual {use_r}', y, guard, ref)


# ---------------------------------------------------------------- backward-data: ops.conv_wino_bwd_data
BWD_MAP = (2, 17, 31)
BWD_CASES = [(f'{co} -> {c1} + {c2}', co, c1, c2) for co in (8, 24, 40, 64) for c1, c2 in ((64, 0), (32, 32), (96, 32), (32, 96), (64, 64), (128, 64))]


@functools.lru_cache(maxsize=None)
def bwd_inputs(Co, C1, C2):
    B, H, W_ = BWD_MAP
    w = _rand(Co, C1 + C2, 3, 3, seed=3, scale=0.2); g = _rand(B, Co, H, W_, seed=5)
    m1 = _rand(B, C1, H, W_, seed=7); m2 = _rand(B, max(C2, 1), H, W_, seed=8)
    base1 = _rand(B, C1, H, W_, seed=11); base2 = _rand(B, max(C2, 1), H, W_, seed=10)
    return w, g, m1, m2, base1, base2


# (mode1, accumulate1, mode2, accumulate2) of the launches with two destinations: modes 1 and 2 on either side, accumulation on one side only, one side
# without a mask -- and each of them swapped
TWO_DST = ((1, 0, 2, 1), (2, 1, 1, 0), (0, 0, 1, 1), (1, 1, 0, 0))
ONE_DST = ((0, 0), (1, 0), (2, 1))


@pytest.mark.parametrize('case', BWD_CASES, ids=[c[0] for c in BWD_CASES])
def test_wino_bwd_data_vs_float64(case):
    from pnnp_amd import ops
    name, Co, C1, C2 = case
    B, H, W_ = BWD_MAP
    w, g, m1, m2, base1, base2 = bwd_inputs(Co, C1, C2)
    u = torch.full((16 * w.shape[0] * w.shape[1],), float('nan'), device='cuda')
    ops.pack_conv_weight_wino(w.cuda(), None, u)
    gd, m1d, m2d = nhwc(g).cuda(), nhwc(m1).cuda(), nhwc(m2).cuda()
    what = f'conv_wino_bwd_data {name} n_split {C1 if C2 else 0}'
    if C2:
        for mo1, ac1, mo2, ac2 in TWO_DST:
            d1, g1 = _dst((B, H, W_, C1), nhwc(base1) if ac1 else None); d2, g2 = _dst((B, H, W_, C2), nhwc(base2) if ac2 else None)
            ops.conv_wino_bwd_data(gd, u, d1, mask1=m1d if mo1 else None, mode1=mo1, accum1=ac1, dx2=d2, mask2=m2d if mo2 else None, mode2=mo2, accum2=ac2)
            _check(f'{what} dx1 mode {mo1} accumulate {ac1}', d1, g1, W.conv_bwd_data(g, w, 0, C1, m1 if mo1 else None, mo1, base1 if ac1 else None))
            _check(f'{what} dx2 mode {mo2} accumulate {ac2}', d2, g2, W.conv_bwd_data(g, w, C1, C1 + C2, m2 if mo2 else None, mo2, base2 if ac2 else None))
    else:
        for mo, ac in ONE_DST:
            d1, g1 = _dst((B, H, W_, C1), nhwc(base1) if ac else None)
            ops.conv_wino_bwd_data(gd, u, d1, mask1=m1d if mo else None, mode1=mo, accum1=ac)
            _check(f'{what} dx1 mode {mo} accumulate {ac}', d1, g1, W.conv_bwd_data(g, w, 0, C1, m1 if mo else None, mo, base1 if ac else None))


# ---------------------------------------------------------------- backward-data through a shortcut: ops.conv_wino_bwd_data_res
RES_CASES = [(f'{co} -> {c1} on {m} mode {mode}', m, co, c1, mode) for m in ((2, 17, 31), (1, 1, 1)) for co, c1 in ((24, 64), (64, 128)) for mode in (0, 1, 2)]


@functools.lru_cache(maxsize=None)
def res_inputs(B, H, W_, Co, C1):
    return (_rand(Co, C1, 3, 3, seed=3, scale=0.2), _rand(B, Co, H, W_, seed=5), _rand(B, C1, H, W_, seed=6), _rand(B, C1, H, W_, seed=7))


@pytest.mark.parametrize('case', RES_CASES, ids=[c[0] for c in RES_CASES])
def test_wino_bwd_data_res_vs_float64(case):
    from pnnp_amd import ops
    name, (B, H, W_), Co, C1, mode = case
    w, g, add, m = res_inputs(B, H, W_, Co, C1)
    u = torch.full((16 * Co * C1,), float('nan'), device='cuda')
    ops.pack_conv_weight_wino(w.cuda(), None, u)
    dx, guard = _dst((B, H, W_, C1))
    ops.conv_wino_bwd_data_res(nhwc(g).cuda(), u, dx, nhwc(add).cuda(), mask=nhwc(m).cuda() if mode else None, mode=mode)
    _check(f'conv_wino_bwd_data_res {name}', dx, guard, W.conv_bwd_data(g, w, mask=m if mode else None, mode=mode, addsrc=add))


# ---------------------------------------------------------------- the filter transform: ops.pack_conv_weight_wino
# (Cout, Cin) of the weight; the forward pack has K = Cin, N = Cout, the backward-data pack K = Cout, N = Cin, so the backward-data packs of the transposed
# shapes have the same K = 24 / 8 and N = 64 / 128 (a backward-data pack of Cin 24 or 8 is refused: N % 64)
PACK_CASES = [('forward Cout 64 Cin 24', 64, 24, False), ('forward Cout 128 Cin 8', 128, 8, False),
              ('backward-data Cout 24 Cin 64', 24, 64, True), ('backward-data Cout 8 Cin 128', 8, 128, True)]


@pytest.mark.parametrize('case', PACK_CASES, ids=[c[0] for c in PACK_CASES])
def test_wino_filter_transform_vs_float64(case):
    """Every U element within 4 x 2^-24 x (|G| |g| |G|^T) x 1.01 of G g G^T in float64; no element of the pack is left unwritten."""
    from pnnp_amd import ops
    name, Co, Ci, dgrad = case
    w = _rand(Co, Ci, 3, 3, seed=3, scale=0.2)
    K, N = (Co, Ci) if dgrad else (Ci, Co)
    buf = torch.full((16 * K * N + GUARD,), 7.0, device='cuda')
    u = buf[:16 * K * N]; u.fill_(float('nan'))
    ops.pack_conv_weight_wino(w.cuda(), None if dgrad else u, u if dgrad else None)
    got = W.unpack_u(u.cpu(), K, N).double()
    ref, S = W.filter_transform(w, dgrad)
    assert not torch.isnan(got).any() and bool((buf[16 * K * N:] == 7.0).all()), name
    err = (got - ref).abs()
    print(f'wino_f64 | pack_conv_weight_wino {name}: worst err / (2^-24 |G||g||G|^T) = {float((err / (W.U * S).clamp_min(1e-300)).max()):.3f}  (bound 4 x 1.01)')
    assert bool((err <= 4 * W.U * S * 1.01).all()), name


# ---------------------------------------------------------------- weight gradient: ops.conv_wino_bwd_weight
def _many_map(cus):
    """B = 3 images of 4s x 8s pixels, s the smallest odd number with s * s > cus: 3 s^2 chunks (odd, so the last split is short and, s^2 being odd, splits
    of four or more chunks cross the image boundaries).  256 CUs: s = 17, 3 x 68 x 136, 867 chunks, per = 4, 217 splits, the last of 3."""
    s = math.isqrt(cus) + 1
    s += 1 - s % 2
    return (3, 4 * s, 8 * s)


def wg_cases(cus):
    """(name, (B, H, W), Cout, C1, C2, channels of the g tensor, channels of the x1 tensor, class, crosses an image, chunks in the last split or None)"""
    m = lambda blocks, per, rem, cross=False: W.ww_map(cus, blocks, per, rem, cross)
    return [('one chunk, four edge masks', (1, 4, 8), 64, 64, 0, 64, 64, 'one', False, 1),
            ('one row of chunks', (1, 4, 40), 64, 64, 0, 64, 64, 'one', False, 1),
            ('one column of chunks', (1, 20, 8), 64, 64, 0, 64, 64, 'one', False, 1),
            ('two chunks per split, last of one', m(1, 2, 1), 64, 64, 0, 64, 64, 'two', False, 1),
            ('three chunks per split, last of two', m(1, 3, 2), 64, 64, 0, 64, 64, 'three', False, 2),
            ('many chunks per split across images', _many_map(cus), 64, 64, 0, 64, 64, 'many', True, None),
            ('four chunks per split, last of one', m(1, 4, 1), 64, 64, 0, 64, 64, 'many', False, 1),
            ('four blocks 128 x 128 across images', m(4, 4, 1, True), 128, 128, 0, 128, 128, 'many', True, 1),
            ('two inputs 64 + 64', m(2, 2, 1), 64, 64, 64, 64, 64, 'two', False, 1),
            ('two inputs 128 + 64', m(3, 3, 2), 64, 128, 64, 64, 128, 'three', False, 2),
            ('g a 128-channel tensor, 64 used', m(1, 3, 1), 64, 64, 0, 128, 64, 'three', False, 1),
            ('x1 a 128-channel tensor, 64 used', m(1, 2, 1), 64, 64, 0, 64, 128, 'two', False, 1)]


WG_NAMES = [c[0] for c in wg_cases(256)]


def wg_assert_class(case, cus):
    name, (B, H, W_), Co, C1, C2, gcs, xcs, cls, cross, last = case
    N = C1 + C2
    assert W.wino_wgrad_supported(H, W_, Co, C1, C2), name
    assert W.ww_class(B, H, W_, Co, N, cus) == cls, (name, W.ww_class(B, H, W_, Co, N, cus))
    assert W.ww_crosses_image(B, H, W_, Co, N, cus) or not cross, name
    nloc = W.ww_nloc(B, H, W_, Co, N, cus)
    assert last is None or nloc[-1] == last, (name, nloc[-1])
    if cls == 'many':
        assert W.ww_per(B, H, W_, Co, N, cus) >= 4 and nloc[-1] < nloc[0], name


@functools.lru_cache(maxsize=None)
def wg_inputs(B, H, W_, Co, C1, C2, gcs, xcs):
    g = _rand(B, gcs, H, W_, seed=5); x1 = _rand(B, xcs, H, W_, seed=1); x2 = _rand(B, C2, H, W_, seed=2) if C2 else None
    return g, x1, x2


@functools.lru_cache(maxsize=None)
def wg_refs(B, H, W_, Co, C1, C2, gcs, xcs, Z, per):
    g, x1, x2 = wg_inputs(B, H, W_, Co, C1, C2, gcs, xcs)
    return W.conv_bwd_weight(g[:, :Co], torch.cat([x1[:, :C1], x2], 1) if C2 else x1[:, :C1], Z, per)


def _ws(floats):
    buf = torch.full((floats + GUARD,), 7.0, device='cuda')
    ws = buf[:floats]; ws.fill_(float('nan'))
    return ws, buf[floats:]


@pytest.mark.parametrize('name', WG_NAMES)
def test_wino_bwd_weight_vs_float64(name):
    """dW and dbias into NaN, then accumulated onto a known base, each held to the bound by size and by depth.  The workspace is exactly the stated size in
    front of a guard; one float short is refused."""
    from pnnp_amd import _lib, ops
    cus = _cus()
    case = next(c for c in wg_cases(cus) if c[0] == name)
    _, (B, H, W_), Co, C1, C2, gcs, xcs, cls, cross, last = case
    wg_assert_class(case, cus)
    N = C1 + C2
    Z, per = W.ww_splits(B, H, W_, Co, N, cus), W.ww_per(B, H, W_, Co, N, cus)
    floats = ops.wino_wgrad_workspace_floats(B, H, W_, Co, N)
    assert floats == W.ww_workspace_floats(B, H, W_, Co, N, cus) == Z * (9 * Co * N + Co), name
    assert ops.wino_wgrad_supported(H, W_, Co, C1, C2)
    g, x1, x2 = wg_inputs(B, H, W_, Co, C1, C2, gcs, xcs)
    rW, dep_w, rb, dep_b = wg_refs(B, H, W_, Co, C1, C2, gcs, xcs, Z, per)
    gd, x1d, x2d = nhwc(g).cuda(), nhwc(x1).cuda(), nhwc(x2).cuda() if C2 else None
    what = f'conv_wino_bwd_weight {name} {(B, H, W_)} class {cls} Z {Z} per {per}'
    ws, wguard = _ws(floats)
    dW, gW = _dst((Co, N, 3, 3)); db, gb = _dst((Co,))
    with pytest.raises(_lib.PnnpError, match='code -4 '):
        ops.conv_wino_bwd_weight(gd, Co, x1d, C1, x2d, dW, db, ws[:floats - 1])
    torch.cuda.synchronize()
    assert bool(torch.isnan(dW).all()) and bool(torch.isnan(db).all()) and bool(torch.isnan(ws).all())
    ops.conv_wino_bwd_weight(gd, Co, x1d, C1, x2d, dW, db, ws)
    _check(what + ' dW', dW, gW, rW, act_map=False, depth=dep_w)
    _check(what + ' dbias', db, gb, rb, act_map=False, depth=dep_b)
    base_w, base_b = _rand(Co, N, 3, 3, seed=12, scale=10.0), _rand(Co, seed=13, scale=10.0)
    dW, gW = _dst((Co, N, 3, 3), base_w); db, gb = _dst((Co,), base_b)
    ops.conv_wino_bwd_weight(gd, Co, x1d, C1, x2d, dW, db, ws, accumulate=1)
    _check(what + ' dW accumulated', dW, gW, W.accumulated(rW, base_w), act_map=False, depth=dep_w)
    _check(what + ' dbias accumulated', db, gb, W.accumulated(rb, base_b), act_map=False, depth=dep_b)
    assert bool((wguard == 7.0).all()), (what, 'workspace guard written')


def test_wino_bwd_weight_without_dbias():
    from pnnp_amd import ops
    cus = _cus()
    case = next(c for c in wg_cases(cus) if c[0] == 'one row of chunks')
    _, (B, H, W_), Co, C1, C2, gcs, xcs, *_ = case
    Z, per = W.ww_splits(B, H, W_, Co, C1, cus), W.ww_per(B, H, W_, Co, C1, cus)
    g, x1, _ = wg_inputs(B, H, W_, Co, C1, C2, gcs, xcs)
    rW, dep_w, _, _ = wg_refs(B, H, W_, Co, C1, C2, gcs, xcs, Z, per)
    ws, wguard = _ws(ops.wino_wgrad_workspace_floats(B, H, W_, Co, C1))
    dW, gW = _dst((Co, C1, 3, 3))
    ops.conv_wino_bwd_weight(nhwc(g).cuda(), Co, nhwc(x1).cuda(), C1, None, dW, None, ws)
    _check('conv_wino_bwd_weight without dbias dW', dW, gW, rW, act_map=False, depth=dep_w)
    assert bool((wguard == 7.0).all())
    assert bool(torch.isnan(ws[Z * 9 * Co * C1:]).all()), 'the bias slabs were written without a dbias'


# ---------------------------------------------------------------- non-finite values (the contract stated in include/pnnp_hip.h)
NF_MAP = (1, 20, 36)
NF_PIXELS = {'tile corner': (4, 6), 'tile interior': (5, 7), 'image border': (19, 0)}


def _patch_tiles(H, W_, py, px):
    """The pixels of the 2x2 output tiles whose 4x4 patch (rows 2 ty - 1 .. 2 ty + 2) holds pixel (py, px)."""
    m = torch.zeros(H, W_, dtype=torch.bool)
    for ty in range((H + 1) // 2):
        for tx in range((W_ + 1) // 2):
            if 2 * ty - 1 <= py <= 2 * ty + 2 and 2 * tx - 1 <= px <= 2 * tx + 2:
                m[2 * ty:2 * ty + 2, 2 * tx:2 * tx + 2] = True
    return m


@pytest.mark.parametrize('where', list(NF_PIXELS))
@pytest.mark.parametrize('op', ['fwd', 'bwd_data'])
def test_wino_one_non_finite_input_stays_in_its_tiles(op, where):
    from pnnp_amd import ops
    B, H, W_ = NF_MAP
    py, px = NF_PIXELS[where]
    K, N = 16, 64
    src = _rand(B, K, H, W_, seed=1)
    w = _rand(N, K, 3, 3, seed=3, scale=0.2) if op == 'fwd' else _rand(K, N, 3, 3, seed=3, scale=0.2)
    u = torch.empty(16 * K * N, device='cuda')
    ops.pack_conv_weight_wino(w.cuda(), u if op == 'fwd' else None, None if op == 'fwd' else u)
    clean = W.conv_fwd(src, w) if op == 'fwd' else W.conv_bwd_data(src, w)
    allowed = _patch_tiles(H, W_, py, px)[None, None].expand(B, N, H, W_)
    for val in (float('nan'), float('inf'), float('-inf')):
        s = src.clone(); s[0, 5, py, px] = val
        ref64 = F_conv(op, s, w)
        y, guard = _dst((B, H, W_, N))
        if op == 'fwd':
            ops.conv_wino_fwd(nhwc(s).cuda(), None, u, None, y, N, 0)
        else:
            ops.conv_wino_bwd_data(nhwc(s).cuda(), u, y)
        bad = ~torch.isfinite(y.cpu().permute(0, 3, 1, 2))
        must = ~torch.isfinite(ref64)
        assert int(must.sum()) >= 4 * N, (op, where, val)
        assert bool((bad | ~must).all()), (op, where, val, 'an output that float64 makes non-finite is finite')
        assert bool((allowed | ~bad).all()), (op, where, val, 'a non-finite output outside the tiles whose patch holds the pixel', (bad & ~allowed).nonzero()[:5].tolist())
        _check(f'{op} {val} at {where} {(py, px)}: the other outputs', y, guard, clean, skip=allowed)


def F_conv(op, s, w):
    import torch.nn.functional as F
    return F.conv2d(s.double(), w.double(), padding=1) if op == 'fwd' else F.conv_transpose2d(s.double(), w.double(), padding=1)


@pytest.mark.parametrize('which', ['first chunk of a split', 'last chunk of a split'])
def test_wino_bwd_weight_one_inf_in_g(which):
    """One +inf in channel 5 of g: dbias[5] = +inf as the plain sum gives (it was NaN = inf + 0 x inf whenever the pixel lay in a split's last chunk, which the
    loop transforms a second time, parked, with weight 0); every other channel's dbias and dW row stays finite and within the bound; dW[5] is non-finite
    wherever float64 is."""
    from pnnp_amd import ops
    cus = _cus()
    case = next(c for c in wg_cases(cus) if c[0] == 'three chunks per split, last of two')
    _, (B, H, W_), Co, C1, C2, gcs, xcs, *_ = case
    Z, per = W.ww_splits(B, H, W_, Co, C1, cus), W.ww_per(B, H, W_, Co, C1, cus)
    assert per == 3
    chunk = per * (Z // 2) + (0 if which.startswith('first') else per - 1)          # of a split of three chunks
    cx, cy = chunk % (W_ // 8), chunk // (W_ // 8) % (H // 4)
    b, py, px = chunk // ((W_ // 8) * (H // 4)), 4 * cy + 1, 8 * cx + 3
    g, x1, _ = wg_inputs(B, H, W_, Co, C1, C2, gcs, xcs)
    rW, dep_w, rb, dep_b = wg_refs(B, H, W_, Co, C1, C2, gcs, xcs, Z, per)
    gi = g.clone(); gi[b, 5, py, px] = float('inf')
    import torch.nn.functional as F
    w64, b64 = W.R._wgrad(lambda x, w, b: F.conv2d(x, w, b, padding=1), (Co, C1, 3, 3), Co, x1.double(), gi.double())
    assert float(b64[5]) == float('inf')
    ws, wguard = _ws(ops.wino_wgrad_workspace_floats(B, H, W_, Co, C1))
    dW, gW = _dst((Co, C1, 3, 3)); db, gb = _dst((Co,))
    ops.conv_wino_bwd_weight(nhwc(gi).cuda(), Co, nhwc(x1).cuda(), C1, None, dW, db, ws)
    assert float(db[5]) == float('inf'), (which, float(db[5]))
    row = torch.zeros(Co, dtype=torch.bool); row[5] = True
    _check(f'one inf in g, {which}: dbias of the other channels', db, gb, rb, act_map=False, depth=dep_b, skip=row)
    _check(f'one inf in g, {which}: dW of the other channels', dW, gW, rW, act_map=False, depth=dep_w, skip=row[:, None, None, None].expand_as(rW.ref))
    assert bool((~torch.isfinite(dW[5].cpu()) | torch.isfinite(w64[5])).all()), (which, 'dW[5] finite where float64 is not')
    assert bool((wguard == 7.0).all())


# ---------------------------------------------------------------- refusals that launch nothing
def test_wino_refusals_leave_the_destination_untouched():
    """PNNP_E_UNSUPPORTED (-2): K % 8, N % 64, C1 % 8, n_split % 32 (C1 = 48 with C2 = 16); PNNP_E_INVALID (-1): a destination, bias, residual / addsrc or mask
    that is not 16-byte aligned.  B = 0 returns OK.  The destination keeps its contents."""
    from pnnp_amd import _lib, ops
    B, H, W_ = 1, 4, 8
    u = torch.zeros(16 * 64 * 64, device='cuda')
    t = lambda c, v=1.0: torch.full((B, H, W_, c), v, device='cuda')

    def off(c, k=1):                                # a [B][H][W][c] tensor k floats past a 16-byte boundary
        return torch.full((B * H * W_ * c + 4,), 3.0, device='cuda')[k:k + B * H * W_ * c].view(B, H, W_, c)

    def refused(code, fn, *dsts):
        with pytest.raises(_lib.PnnpError, match=f'code {code} '):
            fn()
        torch.cuda.synchronize()
        for dst in dsts:
            assert bool((dst == 3.0).all())

    y = t(64, 3.0)
    refused(-2, lambda: ops.conv_wino_fwd(t(12), None, u, None, y, 64, 0), y)                              # K % 8
    refused(-2, lambda: ops.conv_wino_fwd(t(12), t(4), u, None, y, 64, 0), y)                              # C1 % 8 with K = 16
    y32 = t(32, 3.0)
    refused(-2, lambda: ops.conv_wino_fwd(t(16), None, u, None, y32, 32, 0), y32)                          # N % 64
    d48, d16 = t(48, 3.0), t(16, 3.0)
    refused(-2, lambda: ops.conv_wino_bwd_data(t(16), u, d48, dx2=d16), d48, d16)                          # n_split % 32
    yo = off(64)
    refused(-1, lambda: ops.conv_wino_fwd(t(16), None, u, None, yo, 64, 0), yo)
    refused(-1, lambda: ops.conv_wino_fwd(t(16), None, u, torch.zeros(68, device='cuda')[1:65], y, 64, 0), y)          # bias
    refused(-1, lambda: ops.conv_wino_fwd(t(16), None, u, None, y, 64, 0, residual=off(64, 2)), y)
    refused(-1, lambda: ops.conv_wino_bwd_data(t(16), u, y, mask1=off(64, 3), mode1=1), y)
    d32a, d32b = t(32, 3.0), t(32, 3.0)
    refused(-1, lambda: ops.conv_wino_bwd_data(t(16), u, d32a, dx2=d32b, mask2=off(32), mode2=2), d32a, d32b)
    refused(-1, lambda: ops.conv_wino_bwd_data_res(t(16), u, y, off(64)), y)
    refused(-1, lambda: ops.conv_wino_bwd_data_res(t(16), u, yo, t(64)), yo)
    # B = 0: OK, nothing written
    L, p, st = ops._prep(), ops.ptr, ops.stream()
    x = t(16)
    assert L.pnnp_conv3x3_wino_fwd_f32(p(x), 16, None, 0, p(u), None, None, p(y), 0, H, W_, 64, 0, st) == 0
    assert L.pnnp_conv3x3_wino_bwd_data_f32(p(x), 16, p(u), p(y), 64, None, 0, 0, None, 0, None, 0, 0, 0, H, W_, st) == 0
    assert L.pnnp_conv3x3_wino_bwd_data_res_f32(p(x), 16, p(u), p(y), 64, p(t(64)), None, 0, 0, H, W_, st) == 0
    torch.cuda.synchronize()
    assert bool((y == 3.0).all())


def test_wino_bwd_weight_refusals_leave_the_destination_untouched():
    """H % 4, W % 8, channel counts that are no multiple of 64: PNNP_E_UNSUPPORTED, dW and dbias keep their contents."""
    from pnnp_amd import _lib, ops
    ws = torch.zeros(1 << 20, device='cuda')
    for (H, W_, Co, C1, C2) in ((6, 8, 64, 64, 0), (8, 12, 64, 64, 0), (8, 8, 32, 64, 0), (8, 8, 64, 32, 0), (8, 8, 64, 64, 32)):
        assert not W.wino_wgrad_supported(H, W_, Co, C1, C2) and not ops.wino_wgrad_supported(H, W_, Co, C1, C2)
        assert ops.wino_wgrad_workspace_floats(1, H, W_, Co, C1 + C2) == W.ww_workspace_floats(1, H, W_, Co, C1 + C2)
        t = lambda c: torch.ones((1, H, W_, c), device='cuda')
        dW = torch.full((Co, C1 + C2, 3, 3), 3.0, device='cuda'); db = torch.full((Co,), 3.0, device='cuda')
        with pytest.raises(_lib.PnnpError, match='code -2 '):
            ops.conv_wino_bwd_weight(t(Co), Co, t(C1), C1, t(C2) if C2 else None, dW, db, ws)
        torch.cuda.synchronize()
        assert bool((dW == 3.0).all()) and bool((db == 3.0).all())

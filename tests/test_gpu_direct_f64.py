"""The fp32 "direct" kernels (csrc/conv_igemm.hip, csrc/wgrad.hip) op by op against float64, element by element, at shapes that pick every reachable
instantiation of the launchers and give a workgroup one tile, or several with uneven shares (the persistent loop of igemm_kernel; the pixel-tile loop of
wgrad_kernel).  References, the derived bound  |got - ref64| <= (n + e) 2^-24 S 1.01  and the restated launch rules: tests/_direct_ref.py.  Every destination
starts as NaN (or a known base where the launch accumulates) with a guard band of 7.0 behind it; a case asserts the bound for every element, that no NaN is
left and that the guard is untouched, and prints the largest err / (2^-24 S) it saw (profiles/r7/direct_f64.txt keeps those of one run on 256 compute
units).  tests/test_host_direct_cases.py checks, without a GPU, what the tables below reach.

The refusal "addsrc together with accumulation" (pnnp_igemm_launch, PNNP_E_UNSUPPORTED) cannot be asked for: no exported entry passes both (the shortcut entry
has no accumulate argument, the forward's residual entry neither), so it has no test here."""
import math

import pytest
import torch

import _direct_ref as R

pytestmark = pytest.mark.gpu

GUARD = 1024
BIG = (264, 520)        # 17 x 33 tiles of 32 x 8 pixels (17 x 66 of 32 x 4): 2244 with the batches and N blocks below


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def _dst(shape, base=None):
    """A destination of `shape` on the device, NaN or `base`, with GUARD floats of 7.0 behind it -> (tensor, guard)."""
    n = math.prod(shape)
    buf = torch.full((n + GUARD,), 7.0, device='cuda')
    t = buf[:n].view(shape)
    if base is None:
        t.fill_(float('nan'))
    else:
        t.copy_(base)
    return t, buf[n:]


def _check(what, got, guard, ref, act_map=True, depth=None):
    """depth: a second, tighter n for the same bound (a weight gradient's summation depth, _direct_ref.wgrad_depth)."""
    got = got.detach().cpu().double()
    if act_map:
        got = got.permute(0, 3, 1, 2)
    assert got.shape == ref.ref.shape, (what, got.shape, ref.ref.shape)
    nans = int(torch.isnan(got).sum())
    err = (got - ref.ref).abs()
    ratio = float(torch.nan_to_num(err / (R.U * ref.S).clamp_min(1e-300), nan=float('inf')).max())
    n_max = float(torch.as_tensor(ref.n).max())
    print(f'direct_f64 | {what}: worst err / (2^-24 S) = {ratio:.3f}  (bound (n + e) 1.01 = {(n_max + ref.e) * 1.01:.1f}'
          + (f', by depth {(depth + ref.e) * 1.01:.1f})' if depth else ')'))
    bad = ~(err <= R.bound(ref))
    if depth:
        bad |= ~(err <= R.bound(ref._replace(n=depth)))
    assert nans == 0, (what, 'NaN left', nans)
    assert not bad.any(), (what, ratio, int(bad.sum()), got.numel(), bad.nonzero()[:5].tolist())
    assert bool((guard == 7.0).all()), (what, 'guard band written')


def _cus():
    from pnnp_amd import _lib
    return _lib.lib().pnnp_device_cus()


def _assert_class(what, tiles, cls):
    """The class a table row claims, on THIS device: 'one' -- a tile per workgroup; 'many' -- more tiles than 8 x CUs (8 = 32 wave slots / 4 waves: the most
    256-thread workgroups a CU holds, whatever the occupancy query returns) and no k x CUs, k = 1..4, divides them: some workgroup takes two, shares uneven."""
    cus = _cus()
    if cls == 'many':
        assert tiles > 8 * cus, (what, tiles, cus)
        for k in (1, 2, 3, 4):
            assert tiles % (k * cus) != 0, (what, tiles, k, cus)
    else:
        assert tiles <= cus, (what, tiles, cus)


# ---------------------------------------------------------------- forward: ops.conv_fwd
# (name, taps, (B, H, W), C1, C2, Cout, launch_taps instantiation (TAPS, KC, BN), class on 256 CUs, variants); a variant is (act, bias, residual)
ALL_ACTS = ((0, 1, 0), (1, 1, 0), (2, 1, 0), (1, 1, 1), (0, 0, 0))
FWD_CASES = [
    ('3x3 Cout 48: second N block half empty', 9, (1, 13, 70), 16, 0, 48, (9, 16, 32), 'one', ALL_ACTS),
    ('3x3 Cout 4', 9, (1, 9, 33), 8, 0, 4, (9, 8, 32), 'one', ALL_ACTS),
    ('3x3 Cout 8, two tensors, B 2', 9, (2, 11, 40), 8, 8, 8, (9, 8, 32), 'one', ALL_ACTS),
    ('3x3 Cout 16, 34 x 66', 9, (1, 34, 66), 24, 0, 16, (9, 8, 32), 'one', ALL_ACTS),
    ('3x3 Cout 96, Cin 32', 9, (1, 13, 70), 32, 0, 96, (9, 16, 64), 'one', ALL_ACTS),
    ('3x3 Cout 96, Cin 24', 9, (1, 9, 45), 24, 0, 96, (9, 8, 64), 'one', ALL_ACTS),
    ('3x3 Cout 160', 9, (1, 6, 70), 16, 0, 160, (9, 8, 128), 'one', ALL_ACTS),
    ('1x1 Cout 160, Cin 16', 1, (1, 6, 70), 16, 0, 160, (1, 16, 128), 'one', ALL_ACTS),
    ('1x1 Cout 160, Cin 8', 1, (1, 7, 33), 8, 0, 160, (1, 8, 128), 'one', ALL_ACTS),
    ('1x1 Cout 48', 1, (1, 13, 70), 32, 0, 48, (1, 16, 32), 'one', ALL_ACTS),
    ('1x1 Cout 4', 1, (1, 9, 33), 8, 0, 4, (1, 8, 32), 'one', ALL_ACTS),
    ('1x1 Cout 8', 1, (1, 9, 33), 8, 0, 8, (1, 8, 32), 'one', ALL_ACTS),
    ('1x1 Cout 16', 1, (1, 13, 70), 24, 0, 16, (1, 8, 32), 'one', ALL_ACTS),
    ('1x1 Cout 96, two tensors, B 2', 1, (2, 11, 40), 16, 16, 96, (1, 16, 64), 'one', ALL_ACTS),
    ('1x1 Cout 96, Cin 24', 1, (1, 13, 70), 24, 0, 96, (1, 8, 64), 'one', ALL_ACTS),
    # the persistent loop: 2244 tiles each
    ('persistent 3x3 Cout 48, act 1, bias', 9, (2,) + BIG, 8, 0, 48, (9, 8, 32), 'many', ((1, 1, 0),)),
    ('persistent 3x3 Cout 96', 9, (2,) + BIG, 8, 0, 96, (9, 8, 64), 'many', ((0, 0, 0),)),
    ('persistent 3x3 Cout 160', 9, (1,) + BIG, 8, 0, 160, (9, 8, 128), 'many', ((0, 0, 0),)),
    ('persistent 1x1 Cout 160, Cin 16', 1, (1,) + BIG, 16, 0, 160, (1, 16, 128), 'many', ((0, 0, 0),)),
    ('persistent 3x3 Cout 96, Cin 16, residual', 9, (2,) + BIG, 16, 0, 96, (9, 16, 64), 'many', ((2, 1, 1),)),
    ('persistent 1x1 Cout 48, Cin 16', 1, (2,) + BIG, 16, 0, 48, (1, 16, 32), 'many', ((1, 1, 0),)),
    ('persistent 1x1 Cout 96, Cin 8', 1, (2,) + BIG, 8, 0, 96, (1, 8, 64), 'many', ((0, 1, 0),)),
    ('persistent 1x1 Cout 160, Cin 8', 1, (1,) + BIG, 8, 0, 160, (1, 8, 128), 'many', ((2, 1, 0),)),
]


def fwd_launch(case):
    """(instantiation, tiles) of a FWD_CASES row: N = Cout, K chunks over the channels of ONE segment."""
    _, taps, (B, H, W), C1, C2, Co, *_ = case
    return R.igemm_inst(taps, Co, C1), R.igemm_tiles(B, H, W, Co)


@pytest.mark.parametrize('case', FWD_CASES, ids=[c[0] for c in FWD_CASES])
def test_conv_fwd_vs_float64(case):
    from pnnp_amd import ops
    name, taps, (B, H, W), C1, C2, Co, inst, cls, variants = case
    got_inst, tiles = fwd_launch(case)
    assert got_inst == inst, name
    _assert_class(name, tiles, cls)
    k = 3 if taps == 9 else 1
    x1 = _rand(B, C1, H, W, seed=1); x2 = _rand(B, C2, H, W, seed=2) if C2 else None
    w = _rand(Co, C1 + C2, k, k, seed=3, scale=0.2); b = _rand(Co, seed=4); r = _rand(B, Co, H, W, seed=9)
    xin = torch.cat([x1, x2], 1) if C2 else x1
    fwd = torch.empty(w.numel(), device='cuda')
    ops.pack_conv_weight(w.cuda(), fwd, None)
    x1d, x2d, bd, rd = nhwc(x1).cuda(), nhwc(x2).cuda() if C2 else None, b.cuda(), nhwc(r).cuda()
    for act, use_b, use_r in variants:
        ref = R.conv_fwd(xin, w, b if use_b else None, r if use_r else None, act)
        y, guard = _dst((B, H, W, Co))
        ops.conv_fwd(x1d, x2d, fwd, bd if use_b else None, y, Co, taps, act, residual=rd if use_r else None)
        _check(f'conv_fwd {name} <{inst}> tiles {tiles} act {act} bias {use_b} residual {use_r}', y, guard, ref)


# ---------------------------------------------------------------- backward-data: ops.conv_bwd_data
# (name, taps, (B, H, W), Cout (the K side), C1, C2, instantiation, class)
BWD_CASES = [
    ('3x3 16 -> 16 + 16: split inside a 32-column block', 9, (1, 13, 70), 16, 16, 16, (9, 16, 32), 'one'),
    ('3x3 8 -> 32 + 32', 9, (1, 13, 70), 8, 32, 32, (9, 8, 64), 'one'),
    ('3x3 32 -> 48, one destination', 9, (2, 11, 40), 32, 48, 0, (9, 16, 32), 'one'),
    ('1x1 32 -> 64 + 64, B 2', 1, (2, 11, 40), 32, 64, 64, (1, 16, 128), 'one'),
    ('1x1 8 -> 4 + 4', 1, (1, 9, 33), 8, 4, 4, (1, 8, 32), 'one'),
    ('persistent 3x3 8 -> 4 + 4', 9, (4,) + BIG, 8, 4, 4, (9, 8, 32), 'many'),       # the fewest channels the entry takes: K in eights, columns in fours
]


def bwd_launch(case):
    _, taps, (B, H, W), Co, C1, C2, *_ = case
    return R.igemm_inst(taps, C1 + C2, Co), R.igemm_tiles(B, H, W, C1 + C2)


@pytest.mark.parametrize('case', BWD_CASES, ids=[c[0] for c in BWD_CASES])
def test_conv_bwd_data_vs_float64(case):
    """Two destinations: plain into NaN, then LeakyReLU' on the first and ReLU' + accumulation on the second.  One destination: plain, then ReLU' + accumulation."""
    from pnnp_amd import ops
    name, taps, (B, H, W), Co, C1, C2, inst, cls = case
    got_inst, tiles = bwd_launch(case)
    assert got_inst == inst, name
    _assert_class(name, tiles, cls)
    k = 3 if taps == 9 else 1
    w = _rand(Co, C1 + C2, k, k, seed=3, scale=0.2); g = _rand(B, Co, H, W, seed=5)
    m1 = _rand(B, C1, H, W, seed=7); m2 = _rand(B, max(C2, 1), H, W, seed=8)
    base1 = _rand(B, C1, H, W, seed=11); base2 = _rand(B, max(C2, 1), H, W, seed=10)
    dg = torch.empty(w.numel(), device='cuda')
    ops.pack_conv_weight(w.cuda(), None, dg)
    gd = nhwc(g).cuda()
    what = f'conv_bwd_data {name} <{inst}> tiles {tiles}'
    big = cls == 'many'
    if not big:                                    # (the persistent case runs the masked, accumulating launch only)
        d1, g1 = _dst((B, H, W, C1)); d2, g2 = _dst((B, H, W, C2)) if C2 else (None, None)
        ops.conv_bwd_data(gd, dg, d1, dx2=d2, taps=taps)
        _check(what + ' dx1', d1, g1, R.conv_bwd_data(g, w, 0, C1))
        if C2:
            _check(what + ' dx2', d2, g2, R.conv_bwd_data(g, w, C1, C1 + C2))
    if C2:
        d1, g1 = _dst((B, H, W, C1)); d2, g2 = _dst((B, H, W, C2), nhwc(base2))
        ops.conv_bwd_data(gd, dg, d1, mask1=nhwc(m1).cuda(), mode1=1, dx2=d2, mask2=nhwc(m2).cuda(), mode2=2, accum2=1, taps=taps)
        _check(what + ' dx1 mode 1', d1, g1, R.conv_bwd_data(g, w, 0, C1, m1, 1))
        _check(what + ' dx2 mode 2 accumulated', d2, g2, R.conv_bwd_data(g, w, C1, C1 + C2, m2, 2, base2))
    else:
        d1, g1 = _dst((B, H, W, C1), nhwc(base1))
        ops.conv_bwd_data(gd, dg, d1, mask1=nhwc(m1).cuda(), mode1=2, accum1=1, taps=taps)
        _check(what + ' dx1 mode 2 accumulated', d1, g1, R.conv_bwd_data(g, w, 0, C1, m1, 2, base1))


# ---------------------------------------------------------------- backward-data through a shortcut: ops.conv_bwd_data_res
# (name, taps, (B, H, W), C, mode (0: no mask), instantiation, class)
RES_MAP = (1, 13, 70)
RES_CASES = [(f'{"3x3" if t == 9 else "1x1"} C {c} mode {m}', t, RES_MAP, c, m, (t, 16, 64 if c == 64 else 32), 'one')
             for t in (9, 1) for c in (32, 64) for m in (0, 1, 2)] + [
    ('persistent 3x3 C 32 mode 1', 9, (4,) + BIG, 32, 1, (9, 16, 32), 'many'),
    ('persistent 1x1 C 64 mode 2', 1, (4,) + BIG, 64, 2, (1, 16, 64), 'many'),
]


def res_launch(case):
    _, taps, (B, H, W), C, *_ = case
    return R.igemm_inst(taps, C, C), R.igemm_tiles(B, H, W, C)


def _res_inputs(taps, B, H, W, C):
    k = 3 if taps == 9 else 1
    w = _rand(C, C, k, k, seed=3, scale=0.2); g = _rand(B, C, H, W, seed=5)
    add = _rand(B, C, H, W, seed=6); m = _rand(B, C, H, W, seed=7)
    dg = torch.empty(w.numel(), device='cuda')
    from pnnp_amd import ops
    ops.pack_conv_weight(w.cuda(), None, dg)
    return w, g, add, m, dg


@pytest.mark.parametrize('case', RES_CASES, ids=[c[0] for c in RES_CASES])
def test_conv_bwd_data_res_vs_float64(case):
    from pnnp_amd import ops
    name, taps, (B, H, W), C, mode, inst, cls = case
    got_inst, tiles = res_launch(case)
    assert got_inst == inst, name
    _assert_class(name, tiles, cls)
    w, g, add, m, dg = _res_inputs(taps, B, H, W, C)
    dx, guard = _dst((B, H, W, C))
    ops.conv_bwd_data_res(nhwc(g).cuda(), dg, dx, nhwc(add).cuda(), mask=nhwc(m).cuda() if mode else None, mode=mode, taps=taps)
    _check(f'conv_bwd_data_res {name} <{inst}> tiles {tiles}', dx, guard, R.conv_bwd_data(g, w, mask=m if mode else None, mode=mode, addsrc=add))


@pytest.mark.parametrize('taps', [9, 1])
def test_conv_bwd_data_res_nan_reaches_its_own_element_or_window(taps):
    """A NaN in addsrc reaches exactly its own element of dx; a NaN in g exactly the pixels whose window holds it (3 x 3, or the pixel itself), every channel.
    Everything else keeps its bits.  The pixel (7, 31) is the last row and column of a 32 x 8 tile, so the window crosses both tile edges."""
    from pnnp_amd import ops
    B, H, W = RES_MAP
    C, py, px = 32, 7, 31
    w, g, add, m, dg = _res_inputs(taps, B, H, W, C)

    def out(g, add):
        dx, guard = _dst((B, H, W, C))
        ops.conv_bwd_data_res(nhwc(g).cuda(), dg, dx, nhwc(add).cuda(), mask=nhwc(m).cuda(), mode=1, taps=taps)
        assert bool((guard == 7.0).all())
        return dx.cpu()
    clean = out(g, add)
    assert not torch.isnan(clean).any()
    add_n = add.clone(); add_n[0, 5, py, px] = float('nan')
    got = out(g, add_n)
    want = torch.zeros_like(clean, dtype=torch.bool); want[0, py, px, 5] = True
    assert torch.equal(torch.isnan(got), want) and torch.equal(got[~want], clean[~want])
    g_n = g.clone(); g_n[0, 3, py, px] = float('nan')
    got = out(g_n, add)
    want = torch.zeros_like(clean, dtype=torch.bool)
    r = 1 if taps == 9 else 0
    want[0, py - r:py + r + 1, px - r:px + r + 1, :] = True
    assert torch.equal(torch.isnan(got), want) and torch.equal(got[~want], clean[~want])


def test_conv_bwd_data_res_refusals_leave_dx_untouched():
    """What the entry refuses before it launches: a destination, shortcut or mask that is not 16-byte aligned (PNNP_E_INVALID, -1), written channels that are
    no multiple of 4 (PNNP_E_UNSUPPORTED, -2), K channels that are no multiple of 8 (PNNP_E_INVALID).  dx keeps its contents."""
    from pnnp_amd import _lib, ops
    B, H, W, C = 1, 4, 8, 16
    n = B * H * W * C
    wpk = torch.zeros(9 * 16 * 16, device='cuda')
    g = torch.ones((B, H, W, C), device='cuda')

    def off(k=1):                                   # a [B][H][W][C] tensor k floats past a 16-byte boundary
        return torch.full((n + 4,), 3.0, device='cuda')[k:k + n].view(B, H, W, C)

    def refused(code, g, dx, add, mask=None, taps=9):
        with pytest.raises(_lib.PnnpError, match=f'code {code} '):
            ops.conv_bwd_data_res(g, wpk, dx, add, mask=mask, mode=1 if mask is not None else 0, taps=taps)
        torch.cuda.synchronize()
        assert bool((dx == 3.0).all())

    ok = lambda c=C: torch.full((B, H, W, c), 3.0, device='cuda')
    for taps in (9, 1):
        refused(-1, g, off(), ok(), taps=taps)
        refused(-1, g, ok(), off(2), taps=taps)
        refused(-1, g, ok(), ok(), mask=off(3), taps=taps)
        refused(-2, g, ok(6), ok(6), taps=taps)                                                      # C1 = 6
        refused(-1, torch.ones((B, H, W, 12), device='cuda'), ok(), ok(), taps=taps)                  # Cout = 12


# ---------------------------------------------------------------- ConvTranspose2d(2, stride 2): ops.convt_fwd / convt_bwd_data
# (name, (B, H, W) of the input, Cin, Cout, forward instantiation, backward-data instantiation, class of the backward-data launch)
CONVT_CASES = [
    ('16 -> 8: four sub-pixels in one 32-column block', (1, 5, 35), 16, 8, (1, 16, 32), (1, 8, 32), 'one'),
    ('8 -> 32', (1, 5, 35), 8, 32, (1, 8, 128), (1, 16, 32), 'one'),
    ('32 -> 16, B 2', (2, 3, 33), 32, 16, (1, 16, 64), (1, 16, 32), 'one'),
    ('persistent backward-data 8 -> 4', (4,) + BIG, 4, 8, None, (1, 8, 32), 'many'),
]


def convt_launches(case):
    """forward: N = 4 Cout columns over the input map, K = Cin; backward-data: N = Cin, four K segments of Cout channels."""
    _, (B, H, W), Ci, Co, fi, *_ = case
    f = (R.igemm_inst(1, 4 * Co, Ci), R.igemm_tiles(B, H, W, 4 * Co)) if fi else None
    return f, (R.igemm_inst(1, Ci, Co), R.igemm_tiles(B, H, W, Ci))


@pytest.mark.parametrize('case', CONVT_CASES, ids=[c[0] for c in CONVT_CASES])
def test_convt_vs_float64(case):
    from pnnp_amd import ops
    name, (B, H, W), Ci, Co, fi, bi, cls = case
    f, (got_bi, tiles) = convt_launches(case)
    assert got_bi == bi and (f is None or f[0] == fi), name
    _assert_class(name, tiles, cls)
    x = _rand(B, Ci, H, W, seed=1); w = _rand(Ci, Co, 2, 2, seed=2, scale=0.2); b = _rand(Co, seed=3)
    g = _rand(B, Co, 2 * H, 2 * W, seed=4); m = _rand(B, Ci, H, W, seed=5)
    fw = torch.empty(w.numel(), device='cuda'); dw = torch.empty(w.numel(), device='cuda')
    if fi:                                         # (the forward needs Cin in eights)
        ops.pack_convt_weight(w.cuda(), fw, dw)
        y, guard = _dst((B, 2 * H, 2 * W, Co))
        ops.convt_fwd(nhwc(x).cuda(), fw, b.cuda(), y, Co)
        _check(f'convt_fwd {name} <{fi}> tiles {f[1]}', y, guard, R.convt_fwd(x, w, b))
    else:
        ops.pack_convt_weight(w.cuda(), None, dw)
    dx, guard = _dst((B, H, W, Ci))
    ops.convt_bwd_data(nhwc(g).cuda(), dw, dx, mask=nhwc(m).cuda(), mode=1)
    _check(f'convt_bwd_data {name} <{bi}> tiles {tiles} mode 1', dx, guard, R.convt_bwd_data(g, w, m, 1))


# ---------------------------------------------------------------- Conv2d 3x3 stride 2: ops.conv_s2_fwd / conv_s2_bwd_data
# (name, (B, H, W) of the input, Cin, Cout, forward instantiation, backward-data instantiation, class of the backward-data launches)
S2_CASES = [
    ('8 -> 16', (1, 18, 70), 8, 16, (1, 8, 32), (1, 16, 32), 'one'),
    ('32 -> 64, B 2', (2, 10, 66), 32, 64, (1, 16, 64), (1, 16, 32), 'one'),
    ('16 -> 128', (1, 14, 34), 16, 128, (1, 16, 128), (1, 16, 32), 'one'),
    ('persistent backward-data 8 -> 4', (4, 2 * BIG[0], 2 * BIG[1]), 4, 8, None, (1, 8, 32), 'many'),
]


def s2_launches(case):
    """forward: nine K segments of Cin channels over the OUTPUT map; backward-data: one launch per input-pixel parity class, each over the output map, N = Cin."""
    _, (B, H, W), Ci, Co, fi, *_ = case
    f = (R.igemm_inst(1, Co, Ci), R.igemm_tiles(B, H // 2, W // 2, Co)) if fi else None
    return f, (R.igemm_inst(1, Ci, Co), R.igemm_tiles(B, H // 2, W // 2, Ci))


@pytest.mark.parametrize('case', S2_CASES, ids=[c[0] for c in S2_CASES])
def test_conv_s2_vs_float64(case):
    from pnnp_amd import ops
    name, (B, H, W), Ci, Co, fi, bi, cls = case
    f, (got_bi, tiles) = s2_launches(case)
    assert got_bi == bi and (f is None or f[0] == fi), name
    _assert_class(name, tiles, cls)
    x = _rand(B, Ci, H, W, seed=1); w = _rand(Co, Ci, 3, 3, seed=2, scale=0.2); b = _rand(Co, seed=3)
    g = _rand(B, Co, H // 2, W // 2, seed=4); m = _rand(B, Ci, H, W, seed=5); base = _rand(B, Ci, H, W, seed=6)
    dpk = torch.empty(w.numel(), device='cuda')
    ops.pack_conv_s2_dgrad(w.cuda(), dpk)
    gd = nhwc(g).cuda()
    if fi:
        fpk = torch.empty(w.numel(), device='cuda')
        ops.pack_conv_weight(w.cuda(), fpk, None)
        for act in (0, 1):
            y, guard = _dst((B, H // 2, W // 2, Co))
            ops.conv_s2_fwd(nhwc(x).cuda(), fpk, b.cuda(), y, Co, act)
            _check(f'conv_s2_fwd {name} <{fi}> tiles {f[1]} act {act}', y, guard, R.conv_fwd(x, w, b, None, act, stride=2))
        dx, guard = _dst((B, H, W, Ci))
        ops.conv_s2_bwd_data(gd, dpk, dx)
        _check(f'conv_s2_bwd_data {name} <{bi}> tiles 4 x {tiles}', dx, guard, R.conv_bwd_data(g, w, stride=2))
    dx, guard = _dst((B, H, W, Ci), nhwc(base))
    ops.conv_s2_bwd_data(gd, dpk, dx, mask=nhwc(m).cuda(), mode=2, accum=1)
    _check(f'conv_s2_bwd_data {name} <{bi}> tiles 4 x {tiles} mode 2 accumulated', dx, guard, R.conv_bwd_data(g, w, mask=m, mode=2, base=base, stride=2))


# ---------------------------------------------------------------- weight gradients: ops.conv_bwd_weight / convt_bwd_weight / conv_s2_bwd_weight
# (name, geometry taps (9, 1, 4: ConvTranspose2d, 18: stride 2), (B, H, W) of the U map (see wgrad_splits), M, N1, N2 (second input tensor, 3x3 / 1x1 only),
#  pick_shape, class).  3x3 / 1x1 / stride 2: M = Cout, N = Cin;  ConvTranspose2d: M = Cin, N = Cout.
def _wg_rows(taps, tag, two):
    small = (1, 7, 45)
    rows = [(f'{tag} 16 x 8', taps, small, 16, 8, 0, 0, 'one'),
            (f'{tag} 48 x 32', taps, small, 48, 32, 0, 1, 'one'),
            (f'{tag} 32 x 40', taps, small, 32, 40, 0, 2, 'one'),
            (f'{tag} 96 x 72' + (': 40 + 32, the boundary inside the first 64 columns' if two else ''), taps, (2, 7, 45), 96, 40 if two else 72, 32 if two else 0, 3, 'one')]
    m0 = (4, 66, 260) if taps != 4 else (2, 66, 260)          # 32 x 32: Z = 512 splits; 612 / 594 pixel tiles of 4 / 2 rows
    m3 = (2, 34, 130) if taps != 18 else (2, 17, 130)         # Z = 128; 170 pixel tiles of 2 / 1 rows
    rows += [(f'{tag} 32 x 32, uneven shares', taps, m0, 32, 32, 0, 0, 'many'),
             (f'{tag} 256 x 32, uneven shares', taps, (2, 34, 130), 256, 32, 0, 1, 'many'),
             (f'{tag} 32 x 256, uneven shares', taps, (2, 34, 130), 32, 128 if two else 256, 128 if two else 0, 2, 'many'),
             (f'{tag} 128 x 128, uneven shares', taps, m3, 128, 128, 0, 3, 'many')]
    return rows


WGRAD_CASES = _wg_rows(9, '3x3', True) + _wg_rows(1, '1x1', True) + _wg_rows(4, 'convT', False) + _wg_rows(18, 'stride 2', False)


@pytest.mark.parametrize('case', WGRAD_CASES, ids=[c[0] for c in WGRAD_CASES])
def test_bwd_weight_vs_float64(case):
    """dW and dbias into NaN, then accumulated onto a known base.  Two bounds: n = B*H*W + Z, the size of the sum, lets a 32 x 32 gradient over 612 pixel tiles
    be wrong by a whole tile's worth; n = the depth of the sum as the kernels build it (a few hundred at most) does not."""
    from pnnp_amd import _lib, ops
    name, taps, (B, H, W), M, N1, N2, shape, cls = case
    N = N1 + N2
    assert R.pick_shape(M, N) == shape and R.wgrad_class(B, H, W, M, N, taps) == cls, name
    Z = R.wgrad_splits(B, H, W, M, N, taps)
    assert _lib.lib().pnnp_wgrad_splits(B, H, W, M, N, taps) == Z, name
    ws = torch.full((ops.wgrad_workspace_floats(B, H, W, M, N, taps),), float('nan'), device='cuda')
    if taps == 4:                                  # U = the layer's input x [M], S = g [N] at twice the size
        x = _rand(B, M, H, W, seed=1); g = _rand(B, N, 2 * H, 2 * W, seed=5)
        rW, rb = R.convt_bwd_weight(x, g, Z)
        xd, gd = nhwc(x).cuda(), nhwc(g).cuda()
        run = lambda dW, db, acc: ops.convt_bwd_weight(xd, gd, dW, ws, accumulate=acc, dbias=db)
        wshape, nb = (M, N, 2, 2), N
    elif taps == 18:                               # U = g [M] on the output map, S = x [N] at twice the size
        x = _rand(B, N, 2 * H, 2 * W, seed=1); g = _rand(B, M, H, W, seed=5)
        rW, rb = R.conv_bwd_weight(g, x, 3, Z, stride=2)
        xd, gd = nhwc(x).cuda(), nhwc(g).cuda()
        run = lambda dW, db, acc: ops.conv_s2_bwd_weight(gd, xd, dW, db, ws, accumulate=acc)
        wshape, nb = (M, N, 3, 3), M
    else:
        k = 3 if taps == 9 else 1
        x1 = _rand(B, N1, H, W, seed=1); x2 = _rand(B, N2, H, W, seed=2) if N2 else None
        g = _rand(B, M, H, W, seed=5)
        rW, rb = R.conv_bwd_weight(g, torch.cat([x1, x2], 1) if N2 else x1, k, Z)
        x1d, x2d, gd = nhwc(x1).cuda(), nhwc(x2).cuda() if N2 else None, nhwc(g).cuda()
        run = lambda dW, db, acc: ops.conv_bwd_weight(gd, M, x1d, N1, x2d, dW, db, taps, ws, accumulate=acc)
        wshape, nb = (M, N, k, k), M
    what = f'bwd_weight {name} shape {shape} Z {Z} pixel tiles {R.wgrad_tiles(B, H, W, M, N, taps)}'
    dep_w, dep_b = R.wgrad_depth(B, H, W, M, N, taps), R.wgrad_depth(B, H, W, M, N, taps, bias=True)
    dW, gW = _dst(wshape); db, gb = _dst((nb,))
    run(dW, db, 0)
    _check(what + ' dW', dW, gW, rW, act_map=False, depth=dep_w)
    _check(what + ' dbias', db, gb, rb, act_map=False, depth=dep_b)
    base_w, base_b = _rand(*wshape, seed=12, scale=10.0), _rand(nb, seed=13, scale=10.0)
    dW, gW = _dst(wshape, base_w); db, gb = _dst((nb,), base_b)
    run(dW, db, 1)
    _check(what + ' dW accumulated', dW, gW, R.accumulated(rW, base_w), act_map=False, depth=dep_w)
    _check(what + ' dbias accumulated', db, gb, R.accumulated(rb, base_b), act_map=False, depth=dep_b)

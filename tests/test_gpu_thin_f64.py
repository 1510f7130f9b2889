"""The thin ends of the networks (csrc/thin.hip: the 1x1 head's forward and one-pass backward, the first 3x3 layer's forward and weight gradient,
thin_reduce_kernel) op by op against float64, element by element, at shapes that give a wave of the head kernels a second 64-pixel group (uncapped and with
the grid capped at 8 / 4 workgroups per compute unit), let a group straddle two images, and give a workgroup of the first-layer kernels a second tile and a
ragged last tile of 16 or 32 columns.  References, summation depths and the restated launch rules: tests/_thin_ref.py; the bound
|got - ref64| <= (n + e) 2^-24 S 1.01 and the destinations (NaN, or a known base where the launch accumulates, with a guard band of 7.0 behind them) are
those of tests/test_gpu_direct_f64.py.  A case asserts the bound for every element -- for a gradient twice, with n the size and with n the depth of the sum
-- that no NaN is left, that the guards are intact and that the channels past cout / cin of a strided destination are still NaN, and prints the largest
err / (2^-24 S) it saw (profiles/r7/thin_f64.txt keeps those of one run on 256 compute units).  tests/test_host_thin_cases.py checks, without a GPU, what
the tables below reach.  tests/test_gpu_thin.py stays beside this file: its `dW + dW` bit check of the accumulating launch is not repeated here."""
import ctypes as C

import pytest
import torch

import _thin_ref as R
from test_gpu_direct_f64 import _cus, _dst, _rand, nhwc

pytestmark = pytest.mark.gpu

NAN, INF = float('nan'), float('inf')


def resolve(shape, cus, per_cu=None, cout=None):
    """A table's shape: (B, H, W), or ('capped', straddle) / ('many', W): a function of the CU count (_thin_ref.head_capped_shape / first_many_shape)."""
    if shape[0] == 'capped':
        return R.head_capped_shape(cus, per_cu, shape[1])
    if shape[0] == 'many':
        return R.first_many_shape(cus, cout, shape[1])
    return shape


def _strided(t, cs, tail=NAN):
    """t [B,H,W,C] in a [B,H,W,cs] tensor whose channels past C hold `tail`; tail 'mixed': NaN, +inf, NaN, -inf, ..."""
    B, H, W, Cn = t.shape
    out = torch.full((B, H, W, cs), NAN if tail == 'mixed' else tail)
    out[..., :Cn] = t
    if tail == 'mixed':
        out[..., Cn + 1::4] = INF
        out[..., Cn + 3::4] = -INF
    return out


def _check(what, got, guard, ref, depth=None, expect_nan=None):
    """got: a CPU tensor in the layout of ref.ref.  depth: a second, tighter n for the same bound.  expect_nan: the elements that must be NaN (and no others)."""
    got = got.double()
    assert got.shape == ref.ref.shape, (what, got.shape, ref.ref.shape)
    want_nan = torch.zeros_like(got, dtype=torch.bool) if expect_nan is None else expect_nan.expand_as(got)
    S = ref.S.expand_as(got)
    err = (got - ref.ref).abs()
    ratio = float(torch.nan_to_num(err / (R.U * S).clamp_min(1e-300), nan=INF)[~want_nan].max())
    print(f'thin_f64 | {what}: worst err / (2^-24 S) = {ratio:.3f}  (bound (n + e) 1.01 = {(ref.n + ref.e) * 1.01:.1f}'
          + (f', by depth {(depth + ref.e) * 1.01:.1f})' if depth else ')'))
    assert torch.equal(torch.isnan(got), want_nan), (what, 'NaN', int(torch.isnan(got).sum()), int(want_nan.sum()))
    bad = ~(err <= R.bound(ref))
    if depth:
        bad |= ~(err <= R.bound(ref._replace(n=depth)))
    bad &= ~want_nan
    assert not bad.any(), (what, ratio, int(bad.sum()), got.numel(), bad.nonzero()[:5].tolist())
    assert bool((guard == 7.0).all()), (what, 'guard band written')


def _tail_is_nan(what, t, c):
    assert t.shape[-1] == c or bool(torch.isnan(t[..., c:]).all()), (what, 'channels past', c, 'written')


def _bits(v):
    return int(torch.as_tensor(v, dtype=torch.float32).reshape(1).view(torch.int32))


def _slot(value=0.0):
    """An amax slot (csrc/h2.h): the bits of a non-negative float32, raised with an integer atomic maximum."""
    return torch.tensor([value], dtype=torch.float32).view(torch.int32).cuda()


def _check_amax(what, slot, stored):
    assert int(slot.cpu()) == _bits(stored.abs().max()), (what, 'amax slot', int(slot.cpu()), _bits(stored.abs().max()))


ABOVE = 3.0e30               # an amax slot that already holds more than any case produces must keep its bits


# ---------------------------------------------------------------- head forward: ops.head_fwd
# (name, shape, cin, cout, class of the launch, residual variants, channels of x past cin -- NaN)
HEAD_FWD_CASES = [
    ('64 pixels: three idle waves', (1, 8, 8), 16, 1, 'one', (0, 1), 0),
    ('192 pixels: one idle wave', (1, 12, 16), 32, 3, 'one', (0, 1), 8),
    ('192 pixels in 4 images of 48', (4, 6, 8), 64, 2, 'one', (0, 1), 4),
    ('4 groups', (1, 16, 16), 64, 4, 'one', (0, 1), 0),
    ('8 groups', (2, 16, 16), 16, 4, 'one', (0, 1), 4),
    ('16 groups', (2, 16, 32), 32, 2, 'one', (0, 1), 8),
    ('12 groups, 3 images of 256', (3, 16, 16), 64, 1, 'one', (0, 1), 4),
    ('5 groups, 4 images of 80', (4, 4, 20), 16, 4, 'second', (0, 1), 0),
    ('9 groups, 12 images of 48', (12, 6, 8), 16, 3, 'second', (0, 1), 8),
    ('7 groups, 7 images of 64', (7, 8, 8), 32, 3, 'second', (0, 1), 8),
    ('7 groups, 14 images of 32', (14, 4, 8), 32, 1, 'second', (0, 1), 0),
    ('6 groups, 4 images of 96', (4, 8, 12), 32, 4, 'second', (0, 1), 4),
    ('9 groups, 6 images of 96', (6, 8, 12), 64, 2, 'second', (0, 1), 0),
    ('capped, 4 images of H x 80', ('capped', True), 16, 4, 'capped', (1,), 0),
    ('capped, 2 images of H x 64', ('capped', False), 32, 3, 'capped', (0,), 0),
    ('capped, 4 images of H x 80, Cin 64', ('capped', True), 64, 2, 'capped', (1,), 0),
]


@pytest.mark.parametrize('case', HEAD_FWD_CASES, ids=[f'{c[0]} Cin {c[2]}' for c in HEAD_FWD_CASES])
def test_head_fwd_vs_float64(case):
    from pnnp_amd import ops
    name, shape, cin, cout, cls, residuals, xtail = case
    B, H, W = resolve(shape, _cus(), R.HEAD_FWD_PER_CU)
    L = R.head_launch(B * H * W, R.HEAD_FWD_PER_CU, _cus())
    assert L['cls'] == cls, (name, L)
    x = _rand(B, cin, H, W, seed=1); w = _rand(cout, cin, 1, 1, seed=2, scale=0.3); b = _rand(cout, seed=3); r = _rand(B, cout, H, W, seed=4)
    xd, wd, bd, rd = _strided(nhwc(x), cin + xtail).cuda(), w.cuda(), b.cuda(), r.cuda()
    assert ops.head_supported(cin, cout, B * H * W)
    for res in residuals:
        out, guard = _dst((B, cout, H, W))
        ops.head_fwd(xd, wd, bd, out, residual=rd if res else None)
        _check(f'head_fwd {name} Cin {cin} Cout {cout} {B}x{H}x{W} groups {L["ngroups"]} blocks {L["blocks"]} trips {L["trips"]} residual {res}',
               out.cpu(), guard, R.head_fwd(x, w, b, r if res else None))


# ---------------------------------------------------------------- head backward: ops.head_bwd
# (name, shape, cin, cout, mode, class, channels of x past cin (NaN), channels of gx past cin (must stay NaN)); g always has 8 channels, NaN / inf past cout
HEAD_BWD_CASES = [
    ('64 pixels: three idle waves', (1, 8, 8), 16, 1, 1, 'one', 0, 0),
    ('192 pixels: one idle wave', (1, 12, 16), 32, 3, 2, 'one', 4, 4),
    ('192 pixels in 4 images of 48', (4, 6, 8), 64, 2, 0, 'one', 0, 8),
    ('4 groups', (1, 16, 16), 64, 4, 1, 'one', 0, 0),
    ('8 groups', (2, 16, 16), 16, 4, 2, 'one', 0, 4),
    ('16 groups', (2, 16, 32), 32, 2, 0, 'one', 8, 0),
    ('12 groups', (3, 16, 16), 32, 4, 1, 'one', 0, 4),
    ('5 groups', (4, 4, 20), 16, 4, 1, 'second', 0, 4),
    ('6 groups', (6, 8, 8), 16, 2, 0, 'second', 4, 0),
    ('7 groups, 14 images of 32', (14, 4, 8), 16, 3, 2, 'second', 4, 4),
    ('7 groups', (7, 8, 8), 32, 3, 0, 'second', 0, 0),
    ('15 groups', (5, 12, 16), 32, 1, 1, 'second', 0, 8),
    ('9 groups', (6, 8, 12), 64, 2, 2, 'second', 4, 0),
    ('13 groups', (13, 8, 8), 64, 4, 1, 'second', 0, 4),
    ('capped, 4 images of H x 80', ('capped', True), 16, 4, 1, 'capped', 0, 0),
    ('capped, 2 images of H x 64', ('capped', False), 32, 3, 2, 'capped', 0, 0),
    ('capped, 4 images of H x 80, Cin 64', ('capped', True), 64, 2, 0, 'capped', 0, 0),
]


def _head_bwd_inputs(B, H, W, cin, cout):
    return _rand(B, cin, H, W, seed=1), _rand(B, cout, H, W, seed=5), _rand(cout, cin, 1, 1, seed=2, scale=0.3)


@pytest.mark.parametrize('case', HEAD_BWD_CASES, ids=[f'{c[0]} Cin {c[2]} mode {c[4]}' for c in HEAD_BWD_CASES])
def test_head_bwd_vs_float64(case):
    """gx, dW, db and the amax slot into NaN / zero through a workspace of exactly the floats the launch needs; then accumulated onto a known base with the
    slot already above max |gx|."""
    from pnnp_amd import ops
    name, shape, cin, cout, mode, cls, xtail, gxtail = case
    cus = _cus()
    B, H, W = resolve(shape, cus, R.HEAD_BWD_PER_CU)
    npix = B * H * W
    L = R.head_launch(npix, R.HEAD_BWD_PER_CU, cus)
    assert L['cls'] == cls, (name, L)
    x, g, w = _head_bwd_inputs(B, H, W, cin, cout)
    xd, gd, wd = _strided(nhwc(x), cin + xtail).cuda(), _strided(nhwc(g), 8, 'mixed').cuda(), w.cuda()
    rgx, rW, rb = R.head_bwd(g, x, w, mode)
    dep_w, dep_b = R.head_bwd_depth(npix, cin, cus), R.head_bwd_depth(npix, cin, cus, bias=True)
    nws = R.head_bwd_workspace(npix, cin, cus)
    assert nws <= ops.head_bwd_workspace_floats(cin)
    what = f'head_bwd {name} Cin {cin} Cout {cout} mode {mode} {B}x{H}x{W} groups {L["ngroups"]} blocks {L["blocks"]} trips {L["trips"]}'
    base_w, base_b = _rand(cout, cin, 1, 1, seed=12, scale=10.0), _rand(cout, seed=13, scale=10.0)
    for acc in (0, 1):
        gx, ggx = _dst((B, H, W, cin + gxtail)); ws, gws = _dst((nws,))
        dW, gW = _dst((cout, cin, 1, 1), base_w if acc else None); db, gb = _dst((cout,), base_b if acc else None)
        slot = _slot(ABOVE if acc else 0.0)
        ops.head_bwd(gd, xd, wd, gx, dW, db, ws, mode=mode, accumulate=acc, amax_gx=slot)
        gxc = gx.cpu()
        tag = what + (' accumulated' if acc else '')
        _check(tag + ' gx', gxc[..., :cin].permute(0, 3, 1, 2), ggx, rgx)
        _tail_is_nan(tag + ' gx', gxc, cin)
        _check(tag + ' dW', dW.cpu(), gW, R.accumulated(rW, base_w) if acc else rW, depth=dep_w)
        _check(tag + ' db', db.cpu(), gb, R.accumulated(rb, base_b) if acc else rb, depth=dep_b)
        assert bool((gws == 7.0).all()), (tag, 'guard behind the workspace written')
        if acc:
            assert int(slot.cpu()) == _bits(ABOVE), (tag, 'amax slot lowered')
        else:
            _check_amax(tag, slot, gxc[..., :cin])


def test_head_bwd_nan_in_one_channel_of_g_stays_in_that_channel():
    """A NaN at one pixel of one real channel co of g: dW[co], db[co] and that pixel of gx are NaN, everything else is what it is without that term."""
    from pnnp_amd import ops
    B, H, W, cin, cout, mode, co = 4, 4, 20, 16, 3, 1, 1
    pb, ph, pw = 2, 1, 7
    x, g, w = _head_bwd_inputs(B, H, W, cin, cout)
    g0 = g.clone(); g0[pb, co, ph, pw] = 0.0
    gn = g.clone(); gn[pb, co, ph, pw] = NAN
    rgx, rW, rb = R.head_bwd(g0, x, w, mode)
    npix, cus = B * H * W, _cus()
    gx, ggx = _dst((B, H, W, cin)); dW, gW = _dst((cout, cin, 1, 1)); db, gb = _dst((cout,))
    ws = torch.empty(R.head_bwd_workspace(npix, cin, cus), device='cuda')
    ops.head_bwd(_strided(nhwc(gn), 8, 'mixed').cuda(), nhwc(x).cuda(), w.cuda(), gx, dW, db, ws, mode=mode)
    nan_x = torch.zeros(B, cin, H, W, dtype=torch.bool); nan_x[pb, :, ph, pw] = True
    nan_w = torch.zeros(cout, cin, 1, 1, dtype=torch.bool); nan_w[co] = True
    _check('head_bwd NaN in g: gx', gx.cpu().permute(0, 3, 1, 2), ggx, rgx, expect_nan=nan_x)
    _check('head_bwd NaN in g: dW', dW.cpu(), gW, rW, depth=R.head_bwd_depth(npix, cin, cus), expect_nan=nan_w)
    _check('head_bwd NaN in g: db', db.cpu(), gb, rb, depth=R.head_bwd_depth(npix, cin, cus, bias=True), expect_nan=nan_w[:, 0, 0, 0])


# ---------------------------------------------------------------- first layer: ops.first_fwd / first_bwd_weight
# (name, shape, cin, cout, act, bias, channels of y past cout (must stay NaN), class); x always has 8 channels: cin real, zeros up to 4, NaN in 4 .. 7
FIRST_FWD_CASES = [
    ('one tile of 16 columns', (1, 16, 16), 4, 32, 1, 1, 0, 'one'),
    ('one tile of 16 columns', (1, 8, 16), 3, 64, 2, 1, 4, 'one'),
    ('one column tile of 32', (2, 16, 32), 4, 32, 0, 1, 0, 'one'),
    ('48 + 32, two tile rows, B 2', (2, 32, 80), 3, 32, 0, 0, 4, 'one'),
    ('48 + 48 + 16', (1, 16, 112), 1, 32, 2, 1, 0, 'one'),
    ('48 + 48, two tile rows, B 2', (2, 32, 96), 4, 32, 1, 0, 8, 'one'),
    ('48 + 32, two tile rows, B 3', (3, 16, 80), 4, 64, 1, 1, 0, 'one'),
    ('48 + 48 + 16, three tile rows, B 2', (2, 24, 112), 1, 64, 0, 1, 4, 'one'),
    ('48 + 16, two tile rows', (1, 16, 64), 3, 64, 2, 0, 0, 'one'),
    ('48 + 32, two tile rows', (1, 16, 80), 1, 64, 1, 0, 8, 'one'),
    ('one column tile of 32, two tile rows, B 2', (2, 32, 32), 3, 32, 2, 0, 0, 'one'),
    ('many tiles, 48 + 16', ('many', 64), 4, 32, 1, 1, 0, 'many'),
    ('many tiles, 48 + 32', ('many', 80), 3, 64, 2, 1, 0, 'many'),
]
# (name, shape, cin, cout, channels of g past cout (NaN), class)
FIRST_WGRAD_CASES = [
    ('one tile of 16 columns', (1, 16, 16), 4, 32, 0, 'one'),
    ('one tile of 16 columns', (1, 8, 16), 3, 64, 4, 'one'),
    ('one column tile of 32', (2, 16, 32), 1, 32, 4, 'one'),
    ('48 + 32, two tile rows, B 2', (2, 32, 80), 3, 32, 8, 'one'),
    ('48 + 48 + 16', (1, 16, 112), 4, 32, 0, 'one'),
    ('48 + 32, two tile rows, B 3', (3, 16, 80), 1, 64, 0, 'one'),
    ('48 + 48 + 16, three tile rows, B 2', (2, 24, 112), 4, 64, 4, 'one'),
    ('48 + 16, two tile rows', (1, 16, 64), 3, 64, 0, 'one'),
    ('48 + 48, two tile rows, B 2', (2, 32, 96), 1, 32, 4, 'one'),
    ('one column tile of 32, B 2', (2, 8, 32), 4, 64, 8, 'one'),
    ('many tiles, 48 + 32', ('many', 80), 3, 32, 0, 'many'),
    ('many tiles, 48 + 16', ('many', 64), 4, 64, 0, 'many'),
]


def _x8(x):
    """The first layer's input as the kernels take it: [B,H,W,8], channels cin .. 3 zero; 4 .. 7 are never read and hold NaN."""
    B, cin, H, W = x.shape
    out = torch.full((B, H, W, 8), NAN)
    out[..., :4] = 0.0
    out[..., :cin] = nhwc(x)
    return out


def _first_what(kind, name, cin, cout, B, H, W, L):
    return (f'{kind} {name} Cin {cin} Cout {cout} {B}x{H}x{W} tiles {L["ntiles"]} blocks {L["blocks"]} per workgroup {L["per_wg"]} nw {sorted(L["nws"])}')


@pytest.mark.parametrize('case', FIRST_FWD_CASES, ids=[f'{c[0]} Cin {c[2]} Cout {c[3]} act {c[4]}' for c in FIRST_FWD_CASES])
def test_first_fwd_vs_float64(case):
    from pnnp_amd import ops
    name, shape, cin, cout, act, use_b, ytail, cls = case
    B, H, W = resolve(shape, _cus(), cout=cout)
    L = R.first_launch(B, H, W, cout, _cus())
    assert L['cls'] == cls, (name, L)
    x = _rand(B, cin, H, W, seed=1); w = _rand(cout, cin, 3, 3, seed=2, scale=0.3); b = _rand(cout, seed=3) if use_b else None
    assert ops.first_wgrad_supported(cin, cout, H, W)
    what = _first_what('first_fwd', name, cin, cout, B, H, W, L) + f' act {act} bias {use_b}'
    y, guard = _dst((B, H, W, cout + ytail))
    slot = _slot()
    xd, wd, bd = _x8(x).cuda(), w.cuda(), b.cuda() if use_b else None
    ops.first_fwd(xd, wd, bd, y, act, amax_y=slot)
    yc = y.cpu()
    _check(what, yc[..., :cout].permute(0, 3, 1, 2), guard, R.first_fwd(x, w, b, act))
    _tail_is_nan(what, yc, cout)
    _check_amax(what, slot, yc[..., :cout])
    slot = _slot(ABOVE)
    ops.first_fwd(xd, wd, bd, y, act, amax_y=slot)
    assert int(slot.cpu()) == _bits(ABOVE), (what, 'amax slot lowered')


@pytest.mark.parametrize('case', FIRST_WGRAD_CASES, ids=[f'{c[0]} Cin {c[2]} Cout {c[3]}' for c in FIRST_WGRAD_CASES])
def test_first_bwd_weight_vs_float64(case):
    """dW and db into NaN through a workspace of exactly the floats the launch needs, then accumulated onto a known base."""
    from pnnp_amd import ops
    name, shape, cin, cout, gtail, cls = case
    cus = _cus()
    B, H, W = resolve(shape, cus, cout=cout)
    L = R.first_launch(B, H, W, cout, cus)
    assert L['cls'] == cls, (name, L)
    x = _rand(B, cin, H, W, seed=1); g = _rand(B, cout, H, W, seed=5)
    xd, gd = _x8(x).cuda(), _strided(nhwc(g), cout + gtail).cuda()
    rW, rb = R.first_bwd_weight(g, x)
    dep_w, dep_b = R.first_wgrad_depth(B, H, W, cout, cus), R.first_wgrad_depth(B, H, W, cout, cus, bias=True)
    nws = R.first_wgrad_workspace(B, H, W, cout, cus)
    assert nws <= ops.first_wgrad_workspace_floats(cout)
    what = _first_what('first_bwd_weight', name, cin, cout, B, H, W, L)
    base_w, base_b = _rand(cout, cin, 3, 3, seed=12, scale=10.0), _rand(cout, seed=13, scale=10.0)
    for acc in (0, 1):
        ws, gws = _dst((nws,))
        dW, gW = _dst((cout, cin, 3, 3), base_w if acc else None); db, gb = _dst((cout,), base_b if acc else None)
        ops.first_bwd_weight(gd, cout, xd, cin, dW, db, ws, accumulate=acc)
        tag = what + (' accumulated' if acc else '')
        _check(tag + ' dW', dW.cpu(), gW, R.accumulated(rW, base_w) if acc else rW, depth=dep_w)
        _check(tag + ' db', db.cpu(), gb, R.accumulated(rb, base_b) if acc else rb, depth=dep_b)
        assert bool((gws == 7.0).all()), (tag, 'guard behind the workspace written')


def _first_wgrad_run(g, x, cin, cout):
    from pnnp_amd import ops
    B, _, H, W = g.shape
    dW, gW = _dst((cout, cin, 3, 3)); db, gb = _dst((cout,))
    ws = torch.empty(R.first_wgrad_workspace(B, H, W, cout, _cus()), device='cuda')
    ops.first_bwd_weight(nhwc(g).cuda(), cout, _x8(x).cuda(), cin, dW, db, ws)
    return dW.cpu(), gW, db.cpu(), gb


def test_first_bwd_weight_nan_in_one_channel_of_g_stays_in_that_channel():
    """A NaN at one interior pixel of channel co of g (in the ragged second column tile): dW[co] and db[co] are all NaN, every other channel within its bound."""
    B, H, W, cin, cout, co = 2, 32, 80, 3, 32, 5
    x = _rand(B, cin, H, W, seed=1); g = _rand(B, cout, H, W, seed=5)
    g[1, co, 17, 50] = NAN
    g0 = torch.nan_to_num(g, nan=0.0)
    rW, rb = R.first_bwd_weight(g0, x)
    dW, gW, db, gb = _first_wgrad_run(g, x, cin, cout)
    nan_w = torch.zeros(cout, cin, 3, 3, dtype=torch.bool); nan_w[co] = True
    cus = _cus()
    _check('first_bwd_weight NaN in g: dW', dW, gW, rW, depth=R.first_wgrad_depth(B, H, W, cout, cus), expect_nan=nan_w)
    _check('first_bwd_weight NaN in g: db', db, gb, rb, depth=R.first_wgrad_depth(B, H, W, cout, cus, bias=True), expect_nan=nan_w[:, 0, 0, 0])


def test_first_bwd_weight_inf_at_column_0_of_a_ragged_tile_stays_inf():
    """W = 64: the second column tile has 16 columns, and first_wgrad_kernel feeds its columns 16 .. 47 the g of the tile's column 0, made zero.  With
    +inf there (an interior pixel of image column 48) and x > 0 everywhere, float64 gives dW[co] = db[co] = +inf; a masking by multiplication gives
    inf * 0 = NaN.  Every other channel stays finite and within its bound."""
    B, H, W, cin, cout, co = 1, 16, 64, 4, 32, 3
    x = _rand(B, cin, H, W, seed=1) * 0.45 + 0.55                    # in (0.1, 1)
    g = _rand(B, cout, H, W, seed=5)
    g[0, co, 5, 48] = INF
    g0 = torch.nan_to_num(g, posinf=0.0)
    want_w, want_b = R.first_bwd_weight(g, x)
    assert bool(torch.isinf(want_w.ref[co]).all() and (want_w.ref[co] > 0).all() and want_b.ref[co] == INF) and int(torch.isinf(want_w.ref).sum()) == 9 * cin
    dW, gW, db, gb = _first_wgrad_run(g, x, cin, cout)
    for what, got, want in (('dW', dW, want_w.ref), ('db', db, want_b.ref)):
        print(f'thin_f64 | first_bwd_weight inf at tile column 0: {what}[{co}] = {got[co].flatten()[:4].tolist()}, float64 {want[co].flatten()[:4].tolist()}')
        assert torch.equal(torch.isnan(got), torch.isnan(want)), (what, 'NaN where float64 has none', torch.isnan(got).nonzero()[:5].tolist())
        assert torch.equal(torch.isinf(got), torch.isinf(want)) and torch.equal(got[torch.isinf(got)].double(), want[torch.isinf(want)]), what
    rW, rb = R.first_bwd_weight(g0, x)
    inf_w = torch.zeros(cout, cin, 3, 3, dtype=torch.bool); inf_w[co] = True
    cus = _cus()
    finite = lambda t: torch.where(torch.isinf(t), torch.full_like(t, NAN), t)
    _check('first_bwd_weight inf in g: dW', finite(dW), gW, rW, depth=R.first_wgrad_depth(B, H, W, cout, cus), expect_nan=inf_w)
    _check('first_bwd_weight inf in g: db', finite(db), gb, rb, depth=R.first_wgrad_depth(B, H, W, cout, cus, bias=True), expect_nan=inf_w[:, 0, 0, 0])


# ---------------------------------------------------------------- workspace and refusals

def _refused(code, fn, *untouched):
    from pnnp_amd import _lib
    with pytest.raises(_lib.PnnpError, match=f'code {code} '):
        fn()
    torch.cuda.synchronize()
    for t in untouched:
        assert bool(torch.isnan(t).all()), 'a refused call wrote to a destination'


def test_a_workspace_one_float_short_is_refused_and_nothing_is_written():
    from pnnp_amd import ops
    cus = _cus()
    nan = lambda *s: torch.full(s, NAN, device='cuda')
    B, H, W, cin, cout = 6, 8, 12, 64, 2                                    # 9 groups: 2 workgroups
    nws = R.head_bwd_workspace(B * H * W, cin, cus)
    assert nws == 2 * (4 * cin + 4)
    g, x, w = torch.ones(B, H, W, 8, device='cuda'), torch.ones(B, H, W, cin, device='cuda'), torch.ones(cout, cin, 1, 1, device='cuda')
    gx, dW, db, ws = nan(B, H, W, cin), nan(cout, cin, 1, 1), nan(cout), nan(nws - 1)
    _refused(-4, lambda: ops.head_bwd(g, x, w, gx, dW, db, ws, mode=1), gx, dW, db, ws)
    B, H, W, cin, cout = 2, 32, 80, 3, 32                                   # 8 tiles: 8 workgroups
    nws = R.first_wgrad_workspace(B, H, W, cout, cus)
    assert nws == 8 * 37 * cout
    g, x = torch.ones(B, H, W, cout, device='cuda'), torch.zeros(B, H, W, 8, device='cuda')
    dW, db, ws = nan(cout, cin, 3, 3), nan(cout), nan(nws - 1)
    _refused(-4, lambda: ops.first_bwd_weight(g, cout, x, cin, dW, db, ws), dW, db, ws)


def test_refusals_leave_the_destinations_untouched():
    """PNNP_E_INVALID (-1): mode / act outside 0 .. 2, a channel stride that is no multiple of 4, gcs < 4.  PNNP_E_UNSUPPORTED (-2): W % 16 != 0, H % TR != 0.
    B = 0 with real pointers: PNNP_OK and nothing written."""
    from pnnp_amd import ops
    from pnnp_amd._lib import ptr, stream
    L = ops._prep()
    nan = lambda *s: torch.full(s, NAN, device='cuda')
    one = lambda *s: torch.ones(s, device='cuda')
    B, H, W, cin, cout = 1, 8, 8, 16, 4
    w, bias = one(cout, cin, 1, 1), one(cout)
    ws = nan(ops.head_bwd_workspace_floats(cin))
    gx, dW, db, out = nan(B, H, W, cin), nan(cout, cin, 1, 1), nan(cout), nan(B, cout, H, W)
    for mode in (-1, 3):
        _refused(-1, lambda: ops.head_bwd(one(B, H, W, 8), one(B, H, W, cin), w, gx, dW, db, ws, mode=mode), gx, dW, db, ws)
    _refused(-1, lambda: ops.head_fwd(one(B, H, W, cin + 2), w, bias, out), out)                                        # xcs = 18
    _refused(-1, lambda: ops.head_bwd(one(B, H, W, 8), one(B, H, W, cin + 2), w, gx, dW, db, ws), gx, dW, db, ws)      # xcs = 18
    _refused(-1, lambda: ops.head_bwd(one(B, H, W, 6), one(B, H, W, cin), w, gx, dW, db, ws), gx, dW, db, ws)          # gcs = 6
    gx18 = nan(B, H, W, cin + 2)
    _refused(-1, lambda: ops.head_bwd(one(B, H, W, 8), one(B, H, W, cin), w, gx18, dW, db, ws), gx18, dW, db, ws)      # gxcs = 18
    g8, x16 = one(B, H, W, 8), one(B, H, W, cin)

    def raw_head_bwd(gcs, b):
        return L.pnnp_head_bwd_amax_f32(ptr(g8), gcs, ptr(x16), cin, cin, ptr(w), ptr(gx), cin, 1, ptr(dW), ptr(db), b, H, W, cout, 0,
                                        ptr(ws), C.c_int64(ws.numel()), ptr(None), stream())
    assert raw_head_bwd(0, B) == -1                                                                                     # gcs = 0 < 4, a multiple of 4
    assert raw_head_bwd(8, 0) == 0                                                                                      # B = 0
    assert L.pnnp_head_fwd_f32(ptr(x16), cin, cin, ptr(w), ptr(bias), ptr(None), ptr(out), 0, H, W, cout, stream()) == 0
    torch.cuda.synchronize()
    for t in (gx, dW, db, ws, out):
        assert bool(torch.isnan(t).all())

    cin, cout = 4, 32
    w3, b3 = one(cout, cin, 3, 3), one(cout)
    ws = nan(ops.first_wgrad_workspace_floats(64))

    def first(Hh, Ww, co, act=1, xcs=8):
        y, dW, db = nan(1, Hh, Ww, co), nan(co, cin, 3, 3), nan(co)
        return (lambda: ops.first_fwd(one(1, Hh, Ww, xcs), one(co, cin, 3, 3), one(co), y, act), y,
                lambda: ops.first_bwd_weight(one(1, Hh, Ww, co), co, one(1, Hh, Ww, xcs), cin, dW, db, ws), dW, db)
    for act in (-1, 3):
        fwd, y, _, _, _ = first(16, 16, 32, act=act)
        _refused(-1, fwd, y)
    for code, args in ((-1, dict(Hh=16, Ww=16, co=32, xcs=6)), (-2, dict(Hh=16, Ww=24, co=32)), (-2, dict(Hh=12, Ww=16, co=64))):
        fwd, y, bwd, dW, db = first(**args)
        _refused(code, fwd, y)
        _refused(code, bwd, dW, db, ws)
    assert not ops.first_wgrad_supported(cin, 32, 16, 24) and not ops.first_wgrad_supported(cin, 64, 12, 16) and ops.first_wgrad_supported(cin, 32, 16, 16)
    x8, y, dW, db, g = one(1, 16, 16, 8), nan(1, 16, 16, cout), nan(cout, cin, 3, 3), nan(cout), one(1, 16, 16, cout)
    assert L.pnnp_first_fwd_amax_f32(ptr(x8), 8, cin, ptr(w3), ptr(b3), ptr(y), cout, 0, 16, 16, cout, 1, ptr(None), stream()) == 0
    assert L.pnnp_first_bwd_weight_f32(ptr(g), cout, cout, ptr(x8), 8, cin, ptr(dW), ptr(db), 0, 16, 16, 0, ptr(ws), C.c_int64(ws.numel()), stream()) == 0
    torch.cuda.synchronize()
    for t in (y, dW, db, ws):
        assert bool(torch.isnan(t).all())

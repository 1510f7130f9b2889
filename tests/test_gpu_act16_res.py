"""GPU checks of the layers fp16 activation storage needs for ResUnet (ConvPolicy.h1_act16_res): the 3x3 residual epilogue with fp16 on all three sides
(pnnp_conv3x3_h1_fwd_res_et), the stride-2 and 1x1 layers with fp16 activations (pnnp_conv_s2_h1_fwd_et, pnnp_conv1x1_h1_fwd_et) and the two streaming kernels
at the network's ends (pnnp_first_fwd_amax_et, pnnp_head_fwd_et).  As in tests/test_gpu_act16.py two exact facts carry everything: an fp16 source is taken
as it is (the float32-source launch fed x16.float() computes the same sums whenever max |x16| < 2^15), and an fp16 store is ONE rounding of the float32 value
the float32-storage launch stores.  So every comparison is torch.equal on bit patterns against kernels that existed before; nothing is a tolerance."""
import pytest
import torch

from test_gpu_act16 import NAN, _operands, _same, _x16, _zslot
from test_gpu_conv import _rand, nhwc
from test_gpu_h1 import CASES, _pack, _slot
from test_gpu_h1_pointwise import SHAPES as PW_SHAPES, _pack as _pw_pack, _weights as _pw_weights

pytestmark = pytest.mark.gpu

RES_CASES = [c for c in CASES if c[4] == 0 or c[4] == c[3]]
# every stride-2 and 1x1 shape of the pointwise tests (one item, a wrapping ring, 72 items; 64- and 128-column tiles) + the smallest stride-2 map on 32-column
# tiles (N = 96), ragged both ways.  With pad 1, stride 2 and the even sizes the layer takes, the FIRST output row and column of every case take taps outside
# the map (row / column -1); the last ones never do (2 (H/2 - 1) + 1 = H - 1), so there is no such case to add.
PW_CASES = {c: s for c, s in PW_SHAPES.items() if c[0] in ('s2', '1x1')}
PW_CASES[('s2', 32, 96)] = (1, 6, 10)


def _code(fn, *a, **k):
    from pnnp_amd._lib import PnnpError
    with pytest.raises(PnnpError) as e:
        fn(*a, **k)
    s = str(e.value)
    return int(s.split('code ')[1].split(' ')[0]) if 'code ' in s else None


# ------------------------------------------------------------------ 1. the residual epilogue
@pytest.mark.parametrize('amax', [3.0, 2.0 ** -9])
@pytest.mark.parametrize('case', RES_CASES)
def test_act16_res_3x3_equals_the_rounded_float32_residual_launch(case, amax):
    """y16 = float16((acc 2^dexp + bias) + float(r16)): the float32 launch's value, rounded once; the slot holds the float32 sum.  Both tile widths, ragged maps."""
    from pnnp_amd import ops
    B, H, W, C1, C2, Co = case
    L = _operands(case)
    x1 = _x16((B, C1, H, W), 5, amax); x2 = _x16((B, C2, H, W), 6, amax) if C2 else None
    r16 = _x16((B, Co, H, W), 7, amax)
    if amax < 1e-2:
        sub = (r16.float().abs() < 2.0 ** -14) & (r16 != 0)
        assert 0.01 < float(sub.float().mean()) < 0.2, 'part of the residual is fp16-subnormal'
    x1f = x1.float(); x2f = x2.float() if C2 else None
    y32 = torch.full((B, H, W, Co), NAN, device='cuda'); a32 = _zslot()
    ops.conv_h1_fwd(x1f, x2f, L['f'], L['sw'], L['b'], y32, Co, 0, _slot(x1f), _slot(x2f) if C2 else None, amax_y=a32, residual=r16.float())
    y16 = torch.full((B, H, W, Co), NAN, dtype=torch.float16, device='cuda'); a16 = _zslot()
    ops.conv_h1a_fwd(x1, x2, L['f'], L['sw'], L['b'], y16, Co, 0, amax_y=a16, residual=r16)
    assert not torch.isnan(y16).any(), 'the sentinel-filled output is fully overwritten'
    assert not torch.isnan(y32).any() and float(y32.abs().max()) > 0
    assert _same(y16, y32.half())
    assert torch.equal(a16, a32), 'the slot records the float32 sum before the rounding'
    assert not _same(y16.float(), y32)                               # (not vacuous: the rounding happened)
    # ... and the residual is in it: without one the result differs
    y0 = torch.full_like(y16, NAN)
    ops.conv_h1a_fwd(x1, x2, L['f'], L['sw'], L['b'], y0, Co, 0)
    assert not _same(y0, y16)


def test_act16_res_nan_in_the_residual_reaches_exactly_its_element():
    from pnnp_amd import ops
    for case in ((2, 8, 32, 32, 32, 32), (3, 120, 250, 64, 0, 64)):  # 32- and 64-column tiles
        assert case in RES_CASES
        B, H, W, C1, C2, Co = case
        L = _operands(case)
        x1 = _x16((B, C1, H, W), 5, 3.0); x2 = _x16((B, C2, H, W), 6, 3.0) if C2 else None
        r = _x16((B, Co, H, W), 7, 3.0)
        y_ok = torch.full((B, H, W, Co), NAN, dtype=torch.float16, device='cuda')
        ops.conv_h1a_fwd(x1, x2, L['f'], L['sw'], L['b'], y_ok, Co, 0, residual=r)
        assert torch.isfinite(y_ok).all()
        for at in ((0, 0, 0, 0), (B - 1, H - 1, W - 1, Co - 1), (B - 1, H // 2, W // 3, 21)):
            rb = r.clone(); rb[at] = NAN
            y = torch.full_like(y_ok, NAN)
            ops.conv_h1a_fwd(x1, x2, L['f'], L['sw'], L['b'], y, Co, 0, residual=rb)
            hit = torch.zeros_like(y, dtype=torch.bool); hit[at] = True
            assert bool(torch.isnan(y[at])) and _same(y[~hit], y_ok[~hit]), (case, at)


# ------------------------------------------------------------------ 2. stride-2 and 1x1
_PW = {}


def _pw_operands(case):
    if case not in _PW:
        kind, K, N = case
        w = _pw_weights(kind, K, N).cuda(); b = _rand(N, seed=4).cuda()
        f, sw = _pw_pack(kind, w)[:2]
        wpos = (_pw_weights(kind, K, N).abs() + 0.01).cuda()           # (no zero weight: every output a value reaches sees it)
        fp, swp = _pw_pack(kind, wpos)[:2]
        _PW[case] = dict(b=b, f=f, sw=sw, fp=fp, swp=swp)
    return _PW[case]


def _pw_run(kind, x1, x2, f, sw, b, y, N, act, amax_y=None):
    """the fp16 launch for fp16 tensors, the float32 twin (with the sources' slots) for float32 ones"""
    from pnnp_amd import ops
    if x1.dtype == torch.float16:
        if kind == 's2':
            return ops.conv_s2_h1a_fwd(x1, f, sw, b, y, N, act, amax_y=amax_y)
        return ops.conv1x1_h1a_fwd(x1, x2, f, sw, b, y, N, act, amax_y=amax_y)
    if kind == 's2':
        return ops.conv_s2_h1_fwd(x1, _slot(x1), f, sw, b, y, N, act, amax_y=amax_y)
    return ops.conv1x1_h1_fwd(x1, _slot(x1), x2, _slot(x2), f, sw, b, y, N, act, amax_y=amax_y)


@pytest.mark.parametrize('case', sorted(PW_CASES))
def test_act16_res_pointwise_equals_the_rounded_float32_twin(case):
    """x16 -> y16 against the _f32 twin fed x16.float(): through the nine strided tap segments (taps outside the map read zero) / the two segments of
    cat([u, skip]); the three tile widths between the cases; equal slots."""
    from pnnp_amd import ops
    kind, K, N = case
    B, H, W = PW_CASES[case]
    assert {(c[2] % 128 == 0, c[2] % 64 == 0) for c in PW_CASES} == {(True, True), (False, True), (False, False)}, 'the three tile widths'
    L = _pw_operands(case)
    OH, OW = (H // 2, W // 2) if kind == 's2' else (H, W)
    for amax, act in ((3.0, 0), (2.0 ** -9, 0), (3.0, 2)):
        x1 = _x16((B, K, H, W), 3, amax); x2 = _x16((B, K, H, W), 8, amax) if kind == '1x1' else None
        y32 = torch.full((B, OH, OW, N), NAN, device='cuda'); a32 = _zslot()
        _pw_run(kind, x1.float(), x2.float() if x2 is not None else None, L['f'], L['sw'], L['b'], y32, N, act, amax_y=a32)
        y16 = torch.full((B, OH, OW, N), NAN, dtype=torch.float16, device='cuda'); a16 = _zslot()
        _pw_run(kind, x1, x2, L['f'], L['sw'], L['b'], y16, N, act, amax_y=a16)
        assert not torch.isnan(y16).any() and not torch.isnan(y32).any() and float(y32.abs().max()) > 0
        assert _same(y16, y32.half()) and torch.equal(a16, a32), (amax, act)
        assert not _same(y16.float(), y32)


@pytest.mark.parametrize('case', sorted(PW_CASES))
def test_act16_res_pointwise_nan_reaches_exactly_its_windows(case):
    """stride 2: input (iy, ix) is read by the outputs oy with 2 oy - 1 <= iy <= 2 oy + 1 (likewise ox); 1x1: by its own pixel, from either segment"""
    kind, K, N = case
    B, H, W = PW_CASES[case]
    L = _pw_operands(case)
    OH, OW = (H // 2, W // 2) if kind == 's2' else (H, W)
    x1 = _x16((B, K, H, W), 3, 3.0); x2 = _x16((B, K, H, W), 8, 3.0) if kind == '1x1' else None
    y_ok = torch.full((B, OH, OW, N), NAN, dtype=torch.float16, device='cuda')
    _pw_run(kind, x1, x2, L['fp'], L['swp'], None, y_ok, N, 0)
    assert torch.isfinite(y_ok).all()
    for seg, (iy, ix) in ((0, (1, 1)), (0, (H - 1, W - 1)), (1, (H // 2, W - 2))):
        if seg == 1 and kind != '1x1':
            seg = 0
        xs = [x1.clone(), x2.clone() if x2 is not None else None]
        xs[seg][B - 1, iy, ix, K - 5] = NAN
        y = torch.full_like(y_ok, NAN)
        _pw_run(kind, xs[0], xs[1], L['fp'], L['swp'], None, y, N, 0)
        hit = torch.zeros((OH, OW), dtype=torch.bool, device='cuda')
        if kind == 's2':
            hit[iy // 2:(iy + 1) // 2 + 1, ix // 2:(ix + 1) // 2 + 1] = True       # (slices clip at the map's edge)
        else:
            hit[iy, ix] = True
        assert torch.isnan(y[B - 1][hit]).all() and int(hit.sum()) in (1, 2, 4), (iy, ix)
        assert _same(y[B - 1][~hit], y_ok[B - 1][~hit]) and _same(y[:B - 1], y_ok[:B - 1]), (iy, ix)


# ------------------------------------------------------------------ 3. the streaming kernels at the ends
@pytest.mark.parametrize('cout,shape', [(32, (2, 32, 80)), (64, (1, 24, 16)), (32, (1, 16, 112))])      # ragged last tile column (W % 48); one narrow tile; B = 2
def test_act16_res_first_layer_stores_one_rounding_of_the_float32_layer(cout, shape):
    from pnnp_amd import ops
    B, H, W = shape
    x = torch.zeros(B, H, W, 8, device='cuda'); x[..., :4] = nhwc(_rand(B, 4, H, W, seed=1)).cuda()
    w = _rand(cout, 4, 3, 3, seed=2, scale=0.5).cuda(); b = _rand(cout, seed=3).cuda()
    for act in (2, 0, 1):
        y32 = torch.full((B, H, W, cout), NAN, device='cuda'); a32 = _zslot()
        ops.first_fwd(x, w, b, y32, act, amax_y=a32)
        y16 = torch.full((B, H, W, cout), NAN, dtype=torch.float16, device='cuda'); a16 = _zslot()
        ops.first_fwd_et(x, w, b, y16, act, amax_y=a16)
        assert not torch.isnan(y16).any() and _same(y16, y32.half()) and torch.equal(a16, a32) and not _same(y16.float(), y32)
        yb = torch.full_like(y32, NAN)                               # float32 through the new entry: the twin itself
        ops.first_fwd_et(x, w, b, yb, act)
        assert _same(yb, y32)


@pytest.mark.parametrize('res', [False, True])
@pytest.mark.parametrize('cin,shape', [(32, (1, 8, 40)), (32, (2, 16, 48)), (64, (1, 8, 24)), (16, (1, 8, 8))])
def test_act16_res_head_reads_fp16_exactly(cin, shape, res):
    """(1, 8, 40): 320 pixels = 5 wave groups of 64, not a multiple of the 4 waves of a workgroup; (1, 8, 8): a single group"""
    from pnnp_amd import ops
    B, H, W = shape
    for amax in (3.0, 2.0 ** -9):
        x = _x16((B, cin, H, W), 9, amax)
        w = _rand(4, cin, 1, 1, seed=2, scale=0.3).cuda(); b = _rand(4, seed=3, scale=0.1).cuda()
        r = _rand(B, 4, H, W, seed=4).cuda() if res else None
        o32 = torch.full((B, 4, H, W), NAN, device='cuda')
        ops.head_fwd(x.float(), w, b, o32, residual=r)
        o16 = torch.full_like(o32, NAN)
        ops.head_fwd_et(x, w, b, o16, residual=r)
        assert not torch.isnan(o16).any() and _same(o16, o32) and float(o32.abs().max()) > 0
        ob = torch.full_like(o32, NAN)
        ops.head_fwd_et(x.float(), w, b, ob, residual=r)
        assert _same(ob, o32)


# ------------------------------------------------------------------ 4. refusals
def test_act16_res_refusals_leave_the_outputs_untouched():
    """PNNP_E_INVALID (-1) / PNNP_E_UNSUPPORTED (-2) from the C entries, PnnpError without a code from the wrappers' dtype checks; nothing is launched."""
    from pnnp_amd import ops
    B, H, W, C, Co = 1, 16, 32, 32, 32
    x = _x16((B, C, H, W), 1, 3.0); xf = x.float(); sx = _slot(xf)
    r = _x16((B, Co, H, W), 2, 3.0)
    f, sw = _pack(_rand(Co, C, 3, 3, seed=2, scale=0.1).cuda())
    n = B * H * W * Co
    big = torch.full((n + 16,), 7.0, dtype=torch.float16, device='cuda')
    y = big[:n].view(B, H, W, Co); y_off = big[4:4 + n].view(B, H, W, Co)
    y32 = torch.full((B, H, W, Co), 7.0, device='cuda')
    rbig = torch.cat([r.view(-1), r.view(-1)[:16]])
    # -- 3x3 residual
    assert _code(ops.conv_h1a_fwd, x, None, f, sw, None, y, Co, 1, residual=r) == -2                        # a residual together with an activation
    assert _code(ops.conv_h1a_fwd, x, None, f, sw, None, y, Co, 2, residual=r) == -2
    assert _code(ops.conv_h1a_fwd, x, None, f, sw, None, y, Co, 0, residual=r.float()) is None              # the wrapper: a float32 residual beside an fp16 y
    assert _code(ops.conv_h1a_fwd, x, None, f, sw, None, y32, Co, 0, residual=r) is None                    # ... and the reverse
    assert _code(ops.conv_h1a_fwd, x, None, f, sw, None, y, Co, 0, residual=r[:, :H - 1]) is None           # another geometry
    L, P, S = ops._prep(), ops.ptr, ops.stream
    raw = lambda xx, ax, res, yy, s16, r16, d16, act=0: L.pnnp_conv3x3_h1_fwd_res_et(P(xx), C, P(ax), None, 0, None, P(f), P(sw), None, P(res), P(yy), None,
                                                                                     s16, r16, d16, B, H, W, Co, act, S())
    assert raw(x, None, r.float(), y, 1, 0, 1) == -2                                                         # the entry: a float32 residual, fp16 destination
    assert raw(x, None, r, y32, 1, 1, 0) == -2                                                               # an fp16 residual, float32 destination
    assert raw(xf, sx, r, y, 0, 1, 1) == -2                                                                  # a float32 source
    assert raw(x, None, None, y, 1, 1, 1) == -1                                                              # no residual
    assert raw(x, None, r, y, 1, 1, 1, act=1) == -2
    assert _code(ops.conv_h1a_fwd, x, None, f, sw, None, y_off, Co, 0, residual=r) == -1                    # y not 16-byte aligned
    assert _code(ops.conv_h1a_fwd, x, None, f, sw, None, y, Co, 0, residual=rbig[4:4 + n].view(B, H, W, Co)) == -1      # the residual not 16-byte aligned
    xw = torch.full((B, H, W, C + 8), 1.0, dtype=torch.float16, device='cuda')
    assert _code(ops.conv_h1a_fwd, xw[..., :C + 4], None, f, sw, None, y, Co, 0, residual=r) == -1          # channel stride not a multiple of 8
    # -- stride 2 and 1x1
    w1 = _pw_weights('1x1', C, Co).cuda(); f1, sw1 = _pw_pack('1x1', w1)[:2]
    w3 = _pw_weights('s2', C, Co).cuda(); f3, sw3 = _pw_pack('s2', w3)[:2]
    ns = B * (H // 2) * (W // 2) * Co
    bigs = torch.full((ns + 16,), 7.0, dtype=torch.float16, device='cuda')
    ys = bigs[:ns].view(B, H // 2, W // 2, Co); ys32 = torch.full((B, H // 2, W // 2, Co), 7.0, device='cuda')
    assert _code(ops.conv_s2_h1a_fwd, x, f3, sw3, None, ys32, Co, 0) == -2                                   # fp16 -> float32: no such kernel
    assert _code(ops.conv_s2_h1a_fwd, xf, f3, sw3, None, ys, Co, 0, amax_x=sx) == -2                         # float32 -> fp16
    assert _code(ops.conv_s2_h1a_fwd, xf, f3, sw3, None, ys32, Co, 0) == -1                                  # the twin without the source's slot
    assert _code(ops.conv_s2_h1a_fwd, x.double(), f3, sw3, None, ys, Co, 0) is None
    assert _code(ops.conv_s2_h1a_fwd, x[:, :15], f3, sw3, None, ys, Co, 0) == -1                             # odd height
    assert _code(ops.conv_s2_h1a_fwd, x, f3, sw3, None, bigs[4:4 + ns].view(B, H // 2, W // 2, Co), Co, 0) == -1      # y misaligned
    assert _code(ops.conv_s2_h1a_fwd, xw[..., :C + 4], f3, sw3, None, ys, Co, 0) == -1                       # K % 32 (and a channel stride % 8)
    assert _code(ops.conv1x1_h1a_fwd, x, xf, f1, sw1, None, y, Co, 0) is None                                # a float32 segment beside an fp16 one
    assert _code(ops.conv1x1_h1a_fwd, x, x, f1, sw1, None, y32, Co, 0) == -2                                 # fp16 -> float32
    assert _code(ops.conv1x1_h1a_fwd, xf, xf, f1, sw1, None, y, Co, 0, sx, sx) == -2                         # float32 -> fp16
    assert _code(ops.conv1x1_h1a_fwd, x, x, f1, sw1, None, y_off, Co, 0) == -1
    assert _code(ops.conv1x1_h1a_fwd, x, x[..., :16].contiguous(), f1, sw1, None, y, Co, 0) == -1            # C2 != C1
    raw1 = L.pnnp_conv1x1_h1_fwd_et(P(x), C, None, P(x), C, None, P(f1), P(sw1), None, P(y32), P(y), None, 1, 1, B, H, W, Co, 0, S())
    assert raw1 == -2                                                                                        # the fp16 1x1 layer takes no residual
    # -- the streaming kernels
    x8 = torch.zeros(B, H, W, 8, device='cuda'); wf = _rand(32, 4, 3, 3, seed=2).cuda()
    assert _code(ops.first_fwd_et, x8.half(), wf, None, y, 0) is None                                        # an fp16 input
    assert _code(ops.first_fwd_et, x8, wf, None, y.double(), 0) is None
    assert _code(ops.first_fwd_et, x8, wf, None, y[..., :16], 0) == -1                                       # fewer channels than the layer writes
    assert _code(ops.first_fwd_et, x8[:, :8], wf, None, y[:, :8], 0) == -2                                   # H % 16 at 32 channels
    out = torch.full((B, 4, H, W), 7.0, device='cuda'); hw = _rand(4, C, 1, 1, seed=3).cuda(); hb = torch.zeros(4, device='cuda')
    assert _code(ops.head_fwd_et, x.double(), hw, hb, out) is None
    assert _code(ops.head_fwd_et, x, hw.half(), hb, out) is None
    assert _code(ops.head_fwd_et, x, hw, None, out) == -1                                                    # the head has a bias
    assert _code(ops.head_fwd_et, x.view(-1)[2:2 + B * H * (W - 2) * C].view(B, H, W - 2, C), hw, hb, out[..., :W - 2]) == -1      # x not 8-byte aligned
    assert _code(ops.head_fwd_et, x[:, :, :31], hw, hb, out[..., :31]) == -2                                 # pixels % 64
    torch.cuda.synchronize()
    for k, t in dict(y=big, y32=y32, ys=bigs, ys32=ys32, out=out).items():
        assert bool((t == 7).all()), k
    ops.conv_h1a_fwd(x, None, f, sw, None, y, Co, 0, residual=r)                                             # and the plain requests go through
    ops.conv_s2_h1a_fwd(x, f3, sw3, None, ys, Co, 0)
    torch.cuda.synchronize()
    assert not bool((y == 7.0).any()) and bool((big[n:] == 7.0).all()) and not bool((ys == 7.0).any()) and bool((bigs[ns:] == 7.0).all())

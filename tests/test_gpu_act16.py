"""GPU checks of the fp16x1 3x3 layers with fp16 ACTIVATIONS (csrc/conv_h1s.hip H1a, the pnnp_conv3x3_h1_*_et entries, ops.conv_h1a_*).  Two facts carry
every test, and both are exact:

  1. the store is a pure rounding: a launch with an fp16 destination writes float16(y32), y32 what the float32-storage launch (ops.conv_h1_*) writes for the
     same operands -- one round to nearest even, subnormals kept, no saturation;
  2. an fp16 source is exact: fed x16, a launch gives bit for bit what the float32-source launch gives for x16.float() whenever max |x16| < 2^15 (that launch
     computes f16(x 2^se), se >= 0, which is exact for every fp16 value; all products and partial sums then differ by the same power of two).

So every comparison here is torch.equal on bit patterns against the EXISTING kernels; nothing is a tolerance."""
import pytest
import torch

from test_gpu_conv import _rand, nchw, nhwc
from test_gpu_h1 import CASES, _pack, _slot, _slot_value

pytestmark = pytest.mark.gpu

NAN = float('nan')


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.float16 else t.view(torch.int32)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _zslot():
    return torch.zeros(1, dtype=torch.int32, device='cuda')


def _x16(shape, seed, amax):
    """an NHWC fp16 tensor whose largest magnitude is exactly ``amax`` (a power of two or 3.0: fp16 values)"""
    x = (nhwc(_rand(*shape, seed=seed)) * amax).half()
    x.view(-1)[seed] = amax
    assert float(x.abs().max()) == amax
    return x.cuda()


_OPS = {}


def _operands(case):
    """weights, pack and float32 inputs of one case: built once, shared, never modified"""
    if case not in _OPS:
        B, H, W, C1, C2, Co = case
        x1 = nhwc(_rand(B, C1, H, W, seed=1)).cuda(); x2 = nhwc(_rand(B, C2, H, W, seed=2)).cuda() if C2 else None
        w = _rand(Co, C1 + C2, 3, 3, seed=3, scale=0.2).cuda(); b = _rand(Co, seed=4).cuda()
        f, sw = _pack(w)
        _OPS[case] = dict(x1=x1, x2=x2, w=w, b=b, f=f, sw=sw, s1=_slot(x1), s2=_slot(x2) if C2 else None)
    return _OPS[case]


# ------------------------------------------------------------------ 1. the store is a pure rounding
@pytest.mark.parametrize('case', CASES)
def test_act16_store_is_one_rounding_of_the_float32_store(case):
    from pnnp_amd import ops
    B, H, W, C1, C2, Co = case
    L = _operands(case)
    for act in (0, 1, 2):
        y32 = torch.full((B, H, W, Co), NAN, device='cuda'); a32 = _zslot()
        ops.conv_h1_fwd(L['x1'], L['x2'], L['f'], L['sw'], L['b'], y32, Co, act, L['s1'], L['s2'], amax_y=a32)
        y16 = torch.full((B, H, W, Co), NAN, dtype=torch.float16, device='cuda'); a16 = _zslot()
        ops.conv_h1a_fwd(L['x1'], L['x2'], L['f'], L['sw'], L['b'], y16, Co, act, L['s1'], L['s2'], amax_y=a16)
        assert not torch.isnan(y16).any(), 'the sentinel-filled output is fully overwritten'
        assert _same(y16, y32.half())
        assert torch.equal(a16, a32), 'the slot records the float32 value before the rounding'
        assert not _same(y16.float(), y32)                       # (the comparison is not vacuous: the rounding happened)


# ------------------------------------------------------------------ 2. an fp16 source is exact
@pytest.mark.parametrize('amax', [3.0, 2.0 ** -9])
@pytest.mark.parametrize('case', CASES)
def test_act16_fp16_source_equals_the_float32_source_launch(case, amax):
    from pnnp_amd import ops
    B, H, W, C1, C2, Co = case
    L = _operands(case)
    x1 = _x16((B, C1, H, W), 5, amax); x2 = _x16((B, C2, H, W), 6, amax) if C2 else None
    if amax < 1e-2:
        sub = (x1.float().abs() < 2.0 ** -14) & (x1 != 0)
        assert 0.01 < float(sub.float().mean()) < 0.2, 'part of the tensor is fp16-subnormal'
    x1f = x1.float(); x2f = x2.float() if C2 else None
    s1 = _slot(x1f); s2 = _slot(x2f) if C2 else None
    for act in (0, 1):
        y32 = torch.full((B, H, W, Co), NAN, device='cuda'); a32 = _zslot()
        ops.conv_h1_fwd(x1f, x2f, L['f'], L['sw'], L['b'], y32, Co, act, s1, s2, amax_y=a32)
        ya = torch.full_like(y32, NAN); aa = _zslot()
        ops.conv_h1a_fwd(x1, x2, L['f'], L['sw'], L['b'], ya, Co, act, amax_y=aa)                  # fp16 -> float32: no slots for the sources
        assert _same(ya, y32) and torch.equal(aa, a32)
        yb = torch.full((B, H, W, Co), NAN, dtype=torch.float16, device='cuda'); ab = _zslot()
        ops.conv_h1a_fwd(x1, x2, L['f'], L['sw'], L['b'], yb, Co, act, amax_y=ab)                  # fp16 -> fp16
        assert _same(yb, y32.half()) and torch.equal(ab, a32)
    assert float(y32.abs().max()) > 0


# ------------------------------------------------------------------ 3. fused pool
@pytest.mark.parametrize('cin,cout,shape', [(32, 32, (2, 32, 64)), (32, 64, (1, 48, 96)), (64, 64, (2, 16, 32))])
def test_act16_fused_maxpool(cin, cout, shape):
    from pnnp_amd import ops
    B, H, W = shape
    x = _x16((B, cin, H, W), 7, 3.0)
    x[0, :4, :8] = 0.0
    g = torch.Generator(device='cuda').manual_seed(cin + cout)
    w = torch.randn(cout, cin, 3, 3, device='cuda', generator=g) * 0.1
    b = torch.randn(cout, device='cuda', generator=g) * 0.1
    b[: cout // 2] = 0.0
    f, sw = _pack(w)
    xf = x.float(); sx = _slot(xf)
    y0 = torch.empty(B, H, W, cout, device='cuda'); p0 = torch.empty(B, H // 2, W // 2, cout, device='cuda')
    c0 = torch.empty(B, H // 2, W // 2, cout, dtype=torch.uint8, device='cuda'); a0 = _zslot()
    ops.conv_h1_fwd_pool(xf, None, f, sw, b, y0, p0, c0, cout, 1, sx, amax_y=a0)
    y1 = torch.full((B, H, W, cout), NAN, dtype=torch.float16, device='cuda'); p1 = torch.full((B, H // 2, W // 2, cout), NAN, dtype=torch.float16, device='cuda')
    c1 = torch.full_like(c0, 255); a1 = _zslot()
    ops.conv_h1a_fwd_pool(x, None, f, sw, b, y1, p1, c1, cout, 1, amax_y=a1)
    assert _same(y1, y0.half()) and _same(p1, p0.half()) and torch.equal(c1, c0) and torch.equal(a1, a0)
    assert int((c1 & 3 != 0).sum()) > 0 and int((c1 >> 2 == 0).sum()) > 0


# ------------------------------------------------------------------ 4. split-K
@pytest.mark.parametrize('case', [(1, 32, 32, 512, 0, 512), (1, 64, 64, 128, 128, 256)])
def test_act16_splitk(case):
    from pnnp_amd import ops
    B, H, W, C1, C2, Co = case
    x1 = _x16((B, C1, H, W), 1, 3.0); x2 = _x16((B, C2, H, W), 2, 3.0) if C2 else None
    w = _rand(Co, C1 + C2, 3, 3, seed=3, scale=0.05).cuda(); bias = _rand(Co, seed=4).cuda()
    f, sw = _pack(w)
    x1f = x1.float(); x2f = x2.float() if C2 else None
    s1, s2 = _slot(x1f), (_slot(x2f) if C2 else None)
    chunks = (2 if C2 else 1) * ((C1 + 15) // 16)
    ks = ops.h2_splitk(B, H, W, chunks, Co)
    assert ks > 1 and chunks % ks == 0, (ks, chunks)
    y32 = torch.full((B, H, W, Co), NAN, device='cuda'); a32 = _zslot(); ws = torch.empty(ks * y32.numel(), device='cuda')
    ops.conv_h1_fwd_splitk(x1f, x2f, f, sw, bias, y32, Co, 1, s1, ks, ws, amax_x2=s2, amax_y=a32)
    for dt in (torch.float16, torch.float32):
        y = torch.full((B, H, W, Co), NAN, dtype=dt, device='cuda'); am = _zslot(); ws2 = torch.full_like(ws, NAN)
        ops.conv_h1a_fwd_splitk(x1, x2, f, sw, bias, y, Co, 1, ks, ws2, amax_y=am)
        assert _same(y, y32.to(dt)) and torch.equal(am, a32)
        assert torch.equal(ws2, ws), 'the slabs stay float32 and hold the same partial sums'


# ------------------------------------------------------------------ 5. head
@pytest.mark.parametrize('res', [False, True])
def test_act16_fused_head(res):
    from pnnp_amd import ops
    B, H, W = 2, 48, 32
    x = _x16((B, 32, H, W), 9, 3.0)
    g = torch.Generator(device='cuda').manual_seed(36)
    w = torch.randn(32, 32, 3, 3, device='cuda', generator=g) * 0.1; b = torch.randn(32, device='cuda', generator=g) * 0.1
    hw = torch.randn(4, 32, 1, 1, device='cuda', generator=g) * 0.2; hb = torch.rand(4, device='cuda', generator=g) * 0.2 - 0.1
    r = torch.rand(B, 4, H, W, device='cuda', generator=g) if res else None
    f, sw = _pack(w)
    xf = x.float()
    o0 = torch.full((B, 4, H, W), NAN, device='cuda')
    ops.conv_h1_fwd_head(xf, None, f, sw, b, None, 32, 1, _slot(xf), hw, hb, o0, residual=r)
    o1 = torch.full_like(o0, NAN)
    ops.conv_h1a_fwd_head(x, None, f, sw, b, 32, 1, hw, hb, o1, residual=r)
    assert not torch.isnan(o1).any() and _same(o1, o0)


# ------------------------------------------------------------------ 6. NaN / inf stay local
def test_act16_nan_and_inf_in_an_fp16_source_reach_exactly_their_3x3_outputs():
    from pnnp_amd import ops
    B, H, W, Ci, Co = 1, 16, 32, 32, 32
    x = _x16((B, Ci, H, W), 1, 3.0)
    w = (_rand(Co, Ci, 3, 3, seed=2, scale=0.2).abs() + 0.01).cuda()      # (no zero weight: every output of the 3x3 window sees the planted value)
    f, sw = _pack(w)
    y_ok = torch.full((B, H, W, Co), NAN, dtype=torch.float16, device='cuda')
    ops.conv_h1a_fwd(x, None, f, sw, None, y_ok, Co, 0)
    assert torch.isfinite(y_ok).all()
    for bad in (NAN, float('inf')):
        xb = x.clone(); xb[0, 5, 7, 3] = bad
        y = torch.full_like(y_ok, NAN)
        ops.conv_h1a_fwd(xb, None, f, sw, None, y, Co, 0)
        assert not torch.isfinite(y[0, 4:7, 6:9]).any()
        far = torch.ones((H, W), dtype=torch.bool, device='cuda'); far[4:7, 6:9] = False
        assert _same(y[0][far], y_ok[0][far]), 'every other output is bit for bit what it was'


# ------------------------------------------------------------------ 7. refusals
def test_act16_refusals_leave_the_outputs_untouched():
    """PNNP_E_INVALID (-1) / PNNP_E_UNSUPPORTED (-2) from the C entries, PnnpError without a code from the wrappers' dtype checks; nothing is launched.
    (Masks, accumulation, a residual and a second destination are not arguments of any _et entry: the launcher refuses them, and no caller can ask.)"""
    from pnnp_amd import ops
    from pnnp_amd._lib import PnnpError
    B, H, W, C, Co = 1, 16, 32, 32, 32
    x = _x16((B, C, H, W), 1, 3.0); xf = x.float(); sx = _slot(xf)
    w = _rand(Co, C, 3, 3, seed=2, scale=0.1).cuda()
    f, sw = _pack(w)
    n = B * H * W * Co
    big = torch.full((n + 16,), 7.0, dtype=torch.float16, device='cuda')
    y = big[:n].view(B, H, W, Co); y_off = big[4:4 + n].view(B, H, W, Co)                                  # + 8 bytes: not a 16-byte word
    pooled = torch.full((B, H // 2, W // 2, Co), 7.0, dtype=torch.float16, device='cuda'); pooled32 = torch.full((B, H // 2, W // 2, Co), 7.0, device='cuda')
    codes = torch.full((B, H // 2, W // 2, Co), 7, dtype=torch.uint8, device='cuda')
    out = torch.full((B, 4, H, W), 7.0, device='cuda'); hw = torch.randn(4, 32, 1, 1, device='cuda')
    ws = torch.full((2 * n,), 7.0, device='cuda')
    slot_bytes = torch.zeros(8, dtype=torch.uint8, device='cuda')
    xwide = torch.full((B, H, W, C + 8), 1.0, dtype=torch.float16, device='cuda')
    w64 = _rand(64, C, 3, 3, seed=3, scale=0.1).cuda(); f64, sw64 = _pack(w64)

    def code(fn, *a, **k):
        with pytest.raises(PnnpError) as e:
            fn(*a, **k)
        s = str(e.value)
        return int(s.split('code ')[1].split(' ')[0]) if 'code ' in s else None
    assert code(ops.conv_h1a_fwd, x, xf, f, sw, None, y, Co, 0) is None                                    # a float32 segment beside an fp16 one
    assert code(ops.conv_h1a_fwd, xf, x, f, sw, None, y, Co, 0, sx, sx) is None
    assert code(ops.conv_h1a_fwd, x.double(), None, f, sw, None, y, Co, 0) is None                         # a third dtype
    assert code(ops.conv_h1a_fwd_pool, x, None, f, sw, None, y, pooled32, codes, Co, 1) is None            # pooled unlike y
    assert code(ops.conv_h1a_fwd_splitk, x, None, f, sw, None, y, Co, 0, 2, ws.half()) is None             # fp16 slabs
    assert code(ops.conv_h1a_fwd, x, None, f, sw, None, y_off, Co, 0) == -1                                # y not 16-byte aligned
    assert code(ops.conv_h1a_fwd, x.view(-1)[4:4 + B * H * (W - 1) * C].view(B, H, W - 1, C), None, f, sw, None, y[:, :, :W - 1], Co, 0) == -2      # x misaligned
    assert code(ops.conv_h1a_fwd, x, None, f, sw, None, y, Co, 0, amax_y=slot_bytes[1:5]) == -1               # a misaligned slot
    assert code(ops.conv_h1a_fwd, xf, None, f, sw, None, y, Co, 0) == -1                                   # float32 source without its slot
    assert code(ops.conv_h1a_fwd, xwide[..., :C + 4], None, f, sw, None, y, Co, 0) == -1                   # K % 8
    assert code(ops.conv_h1a_fwd, x, None, f, sw, None, y.view(B, H, W * 2, 16), 16, 0) == -2              # Cout % 32
    assert code(ops.conv_h1a_fwd_head, x, None, f64, sw64, None, 64, 1, hw, None, out) == -2               # head: Cout != 32
    assert code(ops.conv_h1a_fwd_pool, xf, None, f, sw, None, y, pooled, codes, Co, 1, sx) == -2           # pool: fp16 on both sides only
    assert code(ops.conv_h1a_fwd_pool, x[:, :15], None, f, sw, None, y[:, :15], pooled, codes, Co, 1) == -1      # pool: odd height
    assert code(ops.conv_h1a_fwd_pool, x, None, f, sw, None, y, pooled.view(-1)[4:], codes, Co, 1) == -2   # pool: the pooled map misaligned
    assert code(ops.conv_h1a_fwd_splitk, x, None, f, sw, None, y_off, Co, 0, 2, ws) == -1                  # split-K: y misaligned
    assert code(ops.conv_h1a_fwd_splitk, x, None, f, sw, None, y, Co, 0, 2, ws[:n]) == -4                  # ... the workspace too small
    torch.cuda.synchronize()
    for k, t in dict(y=big, pooled=pooled, pooled32=pooled32, codes=codes, out=out, ws=ws).items():
        assert bool((t == 7).all()), k
    assert not bool(slot_bytes.any())
    ops.conv_h1a_fwd(x, None, f, sw, None, y, Co, 0)                                                       # and the plain request goes through
    torch.cuda.synchronize()
    assert not bool((y == 7.0).any()) and bool((big[n:] == 7.0).all())
    assert ops.image_fits(1424, 2128, 32, 2) and ops.image_fits(1424, 2128, 32, 4)
    assert ops.image_fits(4096, 8000, 32, 2) and not ops.image_fits(4096, 8000, 32, 4) and not ops.image_fits(4096, 8000, 32, 3)


# ------------------------------------------------------------------ 8. ConvTranspose2d(k2, s2)
from test_gpu_h1_pointwise import SHAPES as PW_SHAPES, _pack as _pw_pack, _weights as _pw_weights      # noqa: E402

CONVT_CASES = sorted(c for c in PW_SHAPES if c[0] == 'convt')


@pytest.mark.parametrize('case', CONVT_CASES)
def test_act16_convt_equals_the_rounded_float32_twin(case):
    """x16 -> y16 against convt_h1_fwd fed x16.float(): an exact source and one rounding at the store, through the sub-pixel scatter; at B = 2 and on the
    ragged map too.  The slot is the twin's."""
    from pnnp_amd import ops
    _, K, N = case
    B, H, W = PW_SHAPES[case]
    Co = N // 4
    w = _pw_weights('convt', K, N).cuda(); b = _rand(Co, seed=4).cuda()
    f, sw = _pw_pack('convt', w)[:2]
    for amax in (3.0, 2.0 ** -9):
        x = _x16((B, K, H, W), 3, amax); xf = x.float()
        y32 = torch.full((B, 2 * H, 2 * W, Co), NAN, device='cuda'); a32 = _zslot()
        ops.convt_h1_fwd(xf, _slot(xf), f, sw, b, y32, Co, amax_y=a32)
        y16 = torch.full((B, 2 * H, 2 * W, Co), NAN, dtype=torch.float16, device='cuda'); a16 = _zslot()
        ops.convt_h1a_fwd(x, f, sw, b, y16, Co, amax_y=a16)
        assert not torch.isnan(y16).any() and _same(y16, y32.half()) and torch.equal(a16, a32)


def test_act16_convt_locality_and_refusals():
    from pnnp_amd import ops
    from pnnp_amd._lib import PnnpError
    K, N, B, H, W = 64, 128, 1, 8, 16
    Co = N // 4
    w = (_pw_weights('convt', K, N).abs() + 0.01).cuda()
    f, sw = _pw_pack('convt', w)[:2]
    x = _x16((B, K, H, W), 3, 3.0)
    y_ok = torch.full((B, 2 * H, 2 * W, Co), NAN, dtype=torch.float16, device='cuda')
    ops.convt_h1a_fwd(x, f, sw, None, y_ok, Co)
    assert torch.isfinite(y_ok).all()
    for bad in (NAN, float('inf')):
        xb = x.clone(); xb[0, 3, 5, 7] = bad
        y = torch.full_like(y_ok, NAN)
        ops.convt_h1a_fwd(xb, f, sw, None, y, Co)
        hit = torch.zeros((2 * H, 2 * W), dtype=torch.bool, device='cuda'); hit[6:8, 10:12] = True
        assert not torch.isfinite(y[0][hit]).any() and _same(y[0][~hit], y_ok[0][~hit])

    def code(fn, *a, **k):
        with pytest.raises(PnnpError) as e:
            fn(*a, **k)
        s = str(e.value)
        return int(s.split('code ')[1].split(' ')[0]) if 'code ' in s else None
    n = B * 4 * H * W * Co
    big = torch.full((n + 16,), 7.0, dtype=torch.float16, device='cuda')
    y = big[:n].view(B, 2 * H, 2 * W, Co); y32 = torch.full((B, 2 * H, 2 * W, Co), 7.0, device='cuda')
    assert code(ops.convt_h1a_fwd, x, f, sw, None, y32, Co) == -2                                          # fp16 -> float32: no such kernel
    assert code(ops.convt_h1a_fwd, x.float(), f, sw, None, y, Co, _slot(x.float())) == -2                  # float32 -> fp16
    assert code(ops.convt_h1a_fwd, x.double(), f, sw, None, y, Co) is None
    assert code(ops.convt_h1a_fwd, x, f, sw, None, big[4:4 + n].view(B, 2 * H, 2 * W, Co), Co) == -1       # y misaligned
    assert code(ops.convt_h1a_fwd, x, f[8:], sw, None, y, Co) == -1                                        # the pack misaligned
    torch.cuda.synchronize()
    assert bool((big == 7).all()) and bool((y32 == 7).all())


# ------------------------------------------------------------------ 9. MaxPool2d(2) of an fp16 map (a pooled layer that ran split-K)
@pytest.mark.parametrize('shape', [(2, 8, 16, 64), (1, 6, 10, 24), (3, 34, 18, 8)])      # C / 8 even, odd (3) and 1; more than one block
def test_act16_maxpool_equals_the_float32_pass(shape):
    """bit for bit ops.maxpool_fwd on x16.float(), rounded (the maximum of fp16 values is one of them); a NaN and an inf behave as there; refusals"""
    from pnnp_amd import ops
    from pnnp_amd._lib import PnnpError
    B, H, W, C = shape
    x = _x16((B, C, H, W), 3, 3.0)
    x[0, 1, 2, 3] = NAN; x[0, 3, 5, 1] = float('inf'); x[B - 1, H - 1, W - 1, C - 1] = -float('inf')
    want = ops.maxpool_fwd(x.float(), torch.full((B, H // 2, W // 2, C), NAN, device='cuda'))
    got = ops.maxpool_fwd_f16(x, torch.full((B, H // 2, W // 2, C), NAN, dtype=torch.float16, device='cuda'))
    assert _same(got, want.half()) and torch.isinf(got).any()
    y = torch.full((B, H // 2, W // 2, C), 7.0, dtype=torch.float16, device='cuda')
    with pytest.raises(PnnpError):
        ops.maxpool_fwd_f16(x.float(), y)                           # a float32 map
    with pytest.raises(PnnpError):
        ops.maxpool_fwd_f16(x[:, :H - 1], y)                        # odd height
    with pytest.raises(PnnpError):
        ops.maxpool_fwd_f16(x[..., :C - 4].contiguous(), y)         # C % 8
    torch.cuda.synchronize()
    assert bool((y == 7).all())

"""GPU checks of the opt-in fp16x1 ("h1") eval forward (csrc/conv_h1s.hip): ONE fp16 rounding per operand, products exact, float32
accumulation.  The yardstick is tests/_h1_ref.py, the float64 convolution of the operands rounded as the kernel rounds them (pinned on
the host by tests/test_host_h1_ref.py): against it the kernel must be as accurate as the fp32-MFMA kernel fed the same rounded operands
(the bar of test_h2_is_as_accurate_as_the_fp32_mfma_kernel), and against the UNROUNDED float64 result it must show exactly the documented
error -- one rounding, not zero and nothing worse.  Then the fused variants, the refusals, whole networks and the public interface."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _h1_ref import act64, conv64, h1_conv, h1_resunet_forward, h1_round, h1_scale_exp, h1_unet_forward
from test_gpu_conv import _rand, nchw, nhwc
from test_gpu_wide_tiles import WIDE_CASES

pytestmark = pytest.mark.gpu

CASES32 = [(1, 8, 32, 8, 0, 32),          # padded K
           (2, 8, 32, 32, 32, 32),        # concat
           (1, 9, 33, 24, 0, 96),         # ragged map, K not a multiple of 16
           (3, 19, 50, 48, 48, 32),       # ragged concat
           (1, 4, 4, 256, 0, 256)]        # map smaller than a tile, 16 chunks
CASES = CASES32 + list(WIDE_CASES[:2])     # + 64-column tiles, full and ragged


def _slot(*tensors):
    from pnnp_amd import ops
    s = torch.zeros(1, dtype=torch.int32, device='cuda')
    for t in tensors:
        ops.amax(t, s)
    return s


def _slot_value(s):
    return float(s.cpu().view(torch.float32)[0])


def _pack(w, cin_pad=None):
    from pnnp_amd import ops
    co, ci = w.shape[:2]
    jobs = ops.PackJobs()
    f = torch.full((ops.h1_weight_bytes(cin_pad or ci, co),), 0xAB, dtype=torch.uint8, device='cuda')
    sw = jobs.add_h1(w, f, cin_pad=cin_pad)
    jobs.run()
    return f, sw


def _rel(a, b):
    return float((a - b).norm() / b.norm())


_LAYER = {}


def _layer(case):
    """Operands, float64 references and the three activations' h1 outputs of one case, computed once and shared (never modified)."""
    if case in _LAYER:
        return _LAYER[case]
    from pnnp_amd import ops
    B, H, W, C1, C2, Co = case
    x1 = _rand(B, C1, H, W, seed=1).cuda(); x2 = _rand(B, C2, H, W, seed=2).cuda() if C2 else None
    w = _rand(Co, C1 + C2, 3, 3, seed=3, scale=0.2).cuda(); b = _rand(Co, seed=4).cuda()
    xin = torch.cat([x1, x2], 1) if C2 else x1
    f, sw = _pack(w)
    x1c = nhwc(x1); x2c = nhwc(x2) if C2 else None
    s1 = _slot(x1c); s2 = _slot(x2c) if C2 else None
    emu_pre = conv64(h1_round(xin), h1_round(w), b)                 # (one scale for both segments: the larger slot = max |cat|)
    exact_pre = conv64(xin, w, b)
    # the fp32-MFMA kernel on the already-rounded operands (exact in float32)
    xr, wr = h1_round(xin).float(), h1_round(w).float()
    f32 = torch.empty(wr.numel(), device='cuda'); ops.pack_conv_weight(wr, f32, None)
    x1r = nhwc(xr[:, :C1]); x2r = nhwc(xr[:, C1:]) if C2 else None
    ys, y32s, amax = {}, {}, {}
    for act in (0, 1, 2):
        y = torch.full((B, H, W, Co), float('nan'), device='cuda')
        sy = torch.zeros(1, dtype=torch.int32, device='cuda')
        ops.conv_h1_fwd(x1c, x2c, f, sw, b, y, Co, act, s1, s2, amax_y=sy)
        y32 = torch.empty_like(y)
        ops.conv_fwd(x1r, x2r, f32, b, y32, Co, 9, act)
        ys[act], y32s[act], amax[act] = nchw(y), nchw(y32).double(), _slot_value(sy)
    terms = conv64(xin.abs(), w.abs())
    _LAYER[case] = dict(x1=x1c, x2=x2c, s1=s1, s2=s2, w=w, b=b, f=f, sw=sw, xin=xin, emu=emu_pre, exact=exact_pre, y=ys, y32=y32s, amax=amax, terms=terms)
    return _LAYER[case]


# ------------------------------------------------------------------ 1. pack
def test_h1_pack_is_the_rounded_scaled_weights_bit_for_bit():
    """[N/32][K16][tap 10][octet 2][32][8] fp16: taps 0-8 = float16(w 2^se) bit for bit, tap 9 and the padded K rows zero, max in [2^14, 2^15)."""
    w = (_rand(64, 24, 3, 3, seed=3) * torch.logspace(-3, 1, 64 * 24 * 9).reshape(64, 24, 3, 3)).cuda()
    f, sw = _pack(w)
    amax = _slot_value(sw)
    assert amax == float(w.abs().max())
    se = h1_scale_exp(amax)
    assert se == 14 - int(np.floor(np.log2(amax)))
    a = f.view(torch.float16).cpu().numpy().reshape(2, 2, 10, 2, 32, 8)                    # [nb][chunk][tap][octet][nn][e]
    assert not a[:, :, 9].view(np.uint16).any()                                            # the zero tap
    got = a[:, :, :9].transpose(1, 3, 5, 0, 4, 2).reshape(32, 64, 9)                       # [k][n][tap]
    assert not got[24:].view(np.uint16).any()                                              # K rows 24-31: padding
    want = (w.cpu().numpy().astype(np.float64) * 2.0 ** se).astype(np.float16).reshape(64, 24, 9).transpose(1, 0, 2)
    assert np.array_equal(got[:24].view(np.uint16), want.view(np.uint16))
    assert np.array_equal(got[:24].astype(np.float64) * 2.0 ** -se, h1_round(w).cpu().numpy().reshape(64, 24, 9).transpose(1, 0, 2))
    assert 2.0 ** 14 <= np.abs(got.astype(np.float64)).max() < 2.0 ** 15


# ------------------------------------------------------------------ 2. a layer against the emulation
@pytest.mark.parametrize('case', CASES)
def test_h1_layer_equals_the_emulation_to_fp32_mfma_accuracy(case):
    from pnnp_amd import ops
    B, H, W, C1, C2, Co = case
    assert ops.h2_tile_columns(B, H, W, Co) == (64 if case in WIDE_CASES else 32)
    L = _layer(case)
    for act in (0, 1, 2):
        ref = act64(L['emu'], act)
        y = L['y'][act]
        assert not torch.isnan(y).any(), 'the sentinel-filled output is fully overwritten'
        e1, e32 = _rel(y.double(), ref), _rel(L['y32'][act], ref)
        print(f'h1 {case} act {act}: relative L2 vs the emulation {e1:.2e}, fp32-MFMA on the rounded operands {e32:.2e}')
        assert e1 < 2.0 * e32 + 1e-8 and e1 < 5e-7
        assert L['amax'][act] == float(y.abs().max()), 'amax of the stored output'


# ------------------------------------------------------------------ 3. the error is the one documented
@pytest.mark.parametrize('case', CASES)
def test_h1_error_is_one_fp16_rounding_per_operand(case):
    """|y - exact64| <= (2^-10 + 2^-20) conv(|x|, |w|) + tiny per element ((1 + 2^-11)^2 - 1 on every product, the rest for the float32 sums), tiny = half
    an fp16 subnormal step per operand; and the relative L2 of y - exact64 is the emulation's own to within [0.5, 2]: one rounding happened."""
    L = _layer(case)
    sx, sw = 2.0 ** -h1_scale_exp(float(L['xin'].abs().max())), 2.0 ** -h1_scale_exp(float(L['w'].abs().max()))
    ones_x, ones_w = torch.ones_like(L['xin']), torch.ones_like(L['w'])
    tiny = 2.0 ** -25 * (sx * conv64(ones_x, L['w'].abs()) + sw * conv64(L['xin'].abs(), ones_w) + 2.0 ** -25 * sx * sw * conv64(ones_x, ones_w))
    bound = (2.0 ** -10 + 2.0 ** -20) * L['terms'] + tiny
    for act in (0, 1, 2):                                          # (the activations are 1-Lipschitz: the bound carries over)
        exact = act64(L['exact'], act)
        err = (L['y'][act].double() - exact).abs()
        worst = float((err / bound).max())
        e_y, e_emu = _rel(L['y'][act].double(), exact), _rel(act64(L['emu'], act), exact)
        print(f'h1 {case} act {act}: max |err| / bound {worst:.3f}; relative L2 vs exact float64: kernel {e_y:.3e}, emulation {e_emu:.3e}')
        assert worst <= 1.0
        assert 0.5 * e_emu <= e_y <= 2.0 * e_emu
        assert e_emu > 1e-5                                        # (the rounding is really there: fp16x2 sits at 1e-7)


# ------------------------------------------------------------------ 4. fused pool
@pytest.mark.parametrize('cin,cout,shape', [(32, 32, (2, 32, 64)), (32, 64, (1, 48, 96)), (64, 64, (2, 16, 32))])
def test_h1_fused_maxpool(cin, cout, shape):
    from pnnp_amd import ops
    B, H, W = shape
    g = torch.Generator(device='cuda').manual_seed(cin + cout)
    x = torch.randn(B, H, W, cin, device='cuda', generator=g)
    x[0, :4, :8] = 0.0
    w = torch.randn(cout, cin, 3, 3, device='cuda', generator=g) * 0.1
    b = torch.randn(cout, device='cuda', generator=g) * 0.1
    b[: cout // 2] = 0.0
    f, sw = _pack(w)
    sx = _slot(x)
    y0 = torch.empty(B, H, W, cout, device='cuda'); p0 = torch.empty(B, H // 2, W // 2, cout, device='cuda')
    c0 = torch.empty(B, H // 2, W // 2, cout, dtype=torch.uint8, device='cuda'); a0 = torch.zeros(1, dtype=torch.int32, device='cuda')
    ops.conv_h1_fwd(x, None, f, sw, b, y0, cout, 1, sx, amax_y=a0)
    ops.maxpool_fwd(y0, p0, codes=c0)
    y1 = torch.full_like(y0, float('nan')); p1 = torch.full_like(p0, float('nan')); c1 = torch.full_like(c0, 255)
    a1 = torch.zeros(1, dtype=torch.int32, device='cuda')
    ops.conv_h1_fwd_pool(x, None, f, sw, b, y1, p1, c1, cout, 1, sx, amax_y=a1)
    # y as in test 2: against the emulation, next to the fp32-MFMA kernel on the rounded operands
    xn = nchw(x)
    ref = act64(conv64(h1_round(xn), h1_round(w), b), 1)
    xr, wr = nhwc(h1_round(xn).float()), h1_round(w).float()
    f32 = torch.empty(wr.numel(), device='cuda'); ops.pack_conv_weight(wr, f32, None)
    y32 = torch.empty_like(y1); ops.conv_fwd(xr, None, f32, b, y32, cout, 9, 1)
    e1, e32 = _rel(nchw(y1).double(), ref), _rel(nchw(y32).double(), ref)
    print(f'h1 + pool {cin}->{cout} {shape}: relative L2 vs the emulation {e1:.2e}, fp32-MFMA {e32:.2e}')
    assert e1 < 2.0 * e32 + 1e-8 and e1 < 5e-7
    assert _slot_value(a1) == float(y1.abs().max())
    # the pooled map and the codes are exact functions of the stored y: torch's evaluation, and bit for bit the un-fused pair of kernels
    win = y1.reshape(B, H // 2, 2, W // 2, 2, cout).permute(0, 1, 3, 5, 2, 4).reshape(B, H // 2, W // 2, cout, 4)
    assert torch.equal(p1, nhwc(F.max_pool2d(nchw(y1), 2)))
    codes = (win.argmax(-1) + ((win > 0).long() * torch.tensor([4, 8, 16, 32], device='cuda')).sum(-1)).to(torch.uint8)
    ties = (win == win.amax(-1, keepdim=True)).sum(-1) > 1         # (argmax of a tie: torch's choice is not pinned; the kernel's is the first)
    assert torch.equal(c1[~ties], codes[~ties])
    assert torch.equal(y1, y0) and torch.equal(p1, p0) and torch.equal(c1, c0) and torch.equal(a1, a0)
    assert int((c1 & 3 != 0).sum()) > 0 and int((c1 >> 2 == 0).sum()) > 0


# ------------------------------------------------------------------ 5. split-K
@pytest.mark.parametrize('case', [(1, 32, 32, 512, 0, 512), (1, 64, 64, 128, 128, 256)])
def test_h1_splitk_forward_equals_the_unsplit_launch(case):
    from pnnp_amd import ops
    B, H, W, C1, C2, Co = case
    x1 = _rand(B, C1, H, W, seed=1).cuda(); x2 = _rand(B, C2, H, W, seed=2).cuda() if C2 else None
    w = _rand(Co, C1 + C2, 3, 3, seed=3, scale=0.05).cuda(); bias = _rand(Co, seed=4).cuda()
    f, sw = _pack(w)
    x1c = nhwc(x1); x2c = nhwc(x2) if C2 else None
    s1, s2 = _slot(x1c), (_slot(x2c) if C2 else None)
    chunks = (2 if C2 else 1) * ((C1 + 15) // 16)
    ks = ops.h2_splitk(B, H, W, chunks, Co)
    assert ks > 1 and chunks % ks == 0, (ks, chunks)
    y0 = torch.empty(B, H, W, Co, device='cuda')
    ops.conv_h1_fwd(x1c, x2c, f, sw, bias, y0, Co, 1, s1, s2)

    def split():
        y = torch.full((B, H, W, Co), float('nan'), device='cuda'); am = torch.zeros(1, dtype=torch.int32, device='cuda')
        ws = torch.empty(ks * y.numel(), device='cuda')
        ops.conv_h1_fwd_splitk(x1c, x2c, f, sw, bias, y, Co, 1, s1, ks, ws, amax_x2=s2, amax_y=am)
        return y, am
    y, am = split()
    y_b, am_b = split()
    assert torch.equal(y, y_b) and torch.equal(am, am_b)          # a fixed-order reduce: deterministic
    d = float((y - y0).abs().max() / y0.abs().max())
    print(f'h1 split-K x {ks} {case}: max |diff| / max |y| vs the unsplit launch {d:.2e}')
    assert d < 1e-5
    assert _slot_value(am) == float(y.abs().max())
    xin = torch.cat([x1, x2], 1) if C2 else x1
    ref = act64(conv64(h1_round(xin), h1_round(w), bias), 1)
    xr, wr = h1_round(xin).float(), h1_round(w).float()
    f32 = torch.empty(wr.numel(), device='cuda'); ops.pack_conv_weight(wr, f32, None)
    y32 = torch.empty_like(y); ops.conv_fwd(nhwc(xr[:, :C1]), nhwc(xr[:, C1:]) if C2 else None, f32, bias, y32, Co, 9, 1)
    e1, e32 = _rel(nchw(y).double(), ref), _rel(nchw(y32).double(), ref)
    print(f'h1 split-K {case}: relative L2 vs the emulation {e1:.2e}, fp32-MFMA {e32:.2e}')
    assert e1 < 2.0 * e32 + 1e-8 and e1 < 5e-7


# ------------------------------------------------------------------ 6. head
@pytest.mark.parametrize('width', [32, 50])
@pytest.mark.parametrize('res', [False, True])
def test_h1_fused_head_equals_conv_then_head_kernel(width, res):
    """conv9_2 + LeakyReLU + conv10_1 in one launch against conv_h1_fwd followed by the head kernel: the head's 32-term sums in another order, 1e-6 of
    the largest output (the bar of test_fused_head_equals_conv_then_head_kernel); the 32-channel map is not stored, or stored bit-equal when asked for."""
    from pnnp_amd import ops
    B, H, W = 2, 48, width
    g = torch.Generator(device='cuda').manual_seed(4 + width)
    x = torch.randn(B, H, W, 32, device='cuda', generator=g)
    w = torch.randn(32, 32, 3, 3, device='cuda', generator=g) * 0.1; b = torch.randn(32, device='cuda', generator=g) * 0.1
    hw = torch.randn(4, 32, 1, 1, device='cuda', generator=g) * 0.2; hb = torch.rand(4, device='cuda', generator=g) * 0.2 - 0.1
    r = torch.rand(B, 4, H, W, device='cuda', generator=g) if res else None
    f, sw = _pack(w)
    sx = _slot(x)
    y0 = torch.empty(B, H, W, 32, device='cuda'); o0 = torch.empty(B, 4, H, W, device='cuda')
    ops.conv_h1_fwd(x, None, f, sw, b, y0, 32, 1, sx)
    ops.head_fwd(y0, hw, hb, o0, residual=r)
    o1 = torch.full_like(o0, float('nan'))
    ops.conv_h1_fwd_head(x, None, f, sw, b, None, 32, 1, sx, hw, hb, o1, residual=r)
    scale = float(o0.abs().max())
    d = float((o1 - o0).abs().max())
    print(f'h1 fused head, width {width} res {res}: max |diff| / max |out| {d / scale:.2e}')
    assert d <= 1e-6 * scale
    y2 = torch.full_like(y0, float('nan')); o2 = torch.full_like(o0, float('nan')); a2 = torch.zeros(1, dtype=torch.int32, device='cuda')
    ops.conv_h1_fwd_head(x, None, f, sw, b, y2, 32, 1, sx, hw, hb, o2, amax_y=a2, residual=r)
    assert torch.equal(y2, y0) and torch.equal(o2, o1) and _slot_value(a2) == float(y0.abs().max())


# ------------------------------------------------------------------ 7. NaN / inf
def test_h1_nan_and_inf_propagate_and_stay_local():
    from pnnp_amd import ops
    B, H, W, Ci, Co = 1, 16, 32, 32, 32
    x = nhwc(_rand(B, Ci, H, W, seed=1)).cuda(); w = _rand(Co, Ci, 3, 3, seed=2, scale=0.2).cuda()
    f, sw = _pack(w)
    y_ok = torch.zeros((B, H, W, Co), device='cuda')
    ops.conv_h1_fwd(x, None, f, sw, None, y_ok, Co, 0, _slot(x))
    for bad in (float('nan'), float('inf')):
        xb = x.clone(); xb[0, 5, 7, 3] = bad
        y = torch.zeros((B, H, W, Co), device='cuda')
        ops.conv_h1_fwd(xb, None, f, sw, None, y, Co, 0, _slot(xb))                        # (a diverged tensor takes scale 1)
        assert not torch.isfinite(y[0, 4:7, 6:9]).any()
        far = torch.ones((H, W), dtype=torch.bool, device='cuda'); far[3:8, 5:10] = False
        assert torch.isfinite(y[0][far]).all()
        # outside the neighbourhood the same operands at scale 1 instead of 2^14: the emulation at that scale
        ref = nhwc(conv64(h1_round(nchw(x), float('inf')), h1_round(w), None))
        assert float((y[0][far].double() - ref[0][far]).norm() / ref[0][far].norm()) < 5e-7


# ------------------------------------------------------------------ 8. refusals
def test_h1_refusals_leave_the_outputs_untouched():
    """What the C entries can be asked for and do not do: PNNP_E_INVALID (-1) for misaligned or missing pointers, PNNP_E_UNSUPPORTED (-2) for shapes and
    epilogues without a kernel, PNNP_E_WORKSPACE (-4); nothing is launched.  (Masks, accumulation and a second destination are not arguments of any h1
    entry: the launcher refuses them, and no caller can ask.)"""
    from pnnp_amd import ops
    from pnnp_amd._lib import PnnpError
    B, H, W, C, Co = 1, 16, 32, 32, 32
    x = torch.randn(B, H, W, C, device='cuda'); w = torch.randn(Co, C, 3, 3, device='cuda') * 0.1
    f, sw = _pack(w)
    sx = _slot(x)
    big = torch.full((B * H * W * Co + 8,), 7.0, device='cuda')
    y = big[:B * H * W * Co].view(B, H, W, Co); y_off = big[1:1 + B * H * W * Co].view(B, H, W, Co)
    bias = torch.full((Co + 4,), 7.0, device='cuda')
    pooled = torch.full((B, H // 2, W // 2, Co), 7.0, device='cuda'); codes = torch.full((B, H // 2, W // 2, Co), 7, dtype=torch.uint8, device='cuda')
    out = torch.full((B, 4, H, W), 7.0, device='cuda'); hw = torch.randn(4, 32, 1, 1, device='cuda')
    ws = torch.full((2 * B * H * W * Co + 4,), 7.0, device='cuda')
    res = torch.randn(B, H, W, Co, device='cuda')
    w64 = torch.randn(64, C, 3, 3, device='cuda') * 0.1; f64, sw64 = _pack(w64)
    x12 = torch.randn(B, H, W, 12, device='cuda')

    def code(fn, *a, **k):
        with pytest.raises(PnnpError) as e:
            fn(*a, **k)
        return int(str(e.value).split('code ')[1].split(' ')[0])
    assert code(ops.conv_h1_fwd, x, None, f, sw, None, y_off, Co, 0, sx) == -1                               # y not 16-byte aligned
    assert code(ops.conv_h1_fwd, x, None, f, sw, bias[1:1 + Co], y, Co, 0, sx) == -1                         # bias not 16-byte aligned
    assert code(ops.conv_h1_fwd, x, None, f, sw, None, y, Co, 0, None) == -1                                 # no amax slot for x
    assert code(ops.conv_h1_fwd, x, None, f, sw, None, y, Co, 1, sx, residual=res) == -2                     # residual + activation: no such epilogue
    assert code(ops.conv_h1_fwd, x12, None, f, sw, None, y, Co, 0, _slot(x12)) == -1                         # K % 8
    assert code(ops.conv_h1_fwd, x, None, f, sw, None, y.view(B, H, W * 2, 16), 16, 0, sx) == -2             # Cout % 32
    assert code(ops.conv_h1_fwd_splitk, x, None, f, sw, None, y_off, Co, 0, sx, 2, ws) == -1                 # split-K: y misaligned
    assert code(ops.conv_h1_fwd_splitk, x, None, f, sw, bias[1:1 + Co], y, Co, 0, sx, 2, ws) == -1           # ... bias
    assert code(ops.conv_h1_fwd_splitk, x, None, f, sw, None, y, Co, 0, sx, 2, ws[1:]) == -1                 # ... the workspace
    assert code(ops.conv_h1_fwd_splitk, x, None, f, sw, None, y, Co, 0, sx, 2, ws[:B * H * W * Co]) == -4    # ... too small
    assert code(ops.conv_h1_fwd_head, x, None, f64, sw64, None, None, 64, 1, sx, hw, None, out) == -2        # head: Cout != 32
    assert code(ops.conv_h1_fwd_pool, x[:, :15], None, f, sw, None, y[:, :15], pooled, codes, Co, 1, sx) == -1      # pool: odd height
    assert code(ops.conv_h1_fwd_pool, x, None, f, sw, None, y, pooled.view(-1)[1:], codes, Co, 1, sx) == -2  # pool: the pooled map misaligned
    torch.cuda.synchronize()
    for k, t in dict(y=big, bias=bias, pooled=pooled, codes=codes, out=out, ws=ws).items():
        assert bool((t == 7).all()), k
    ops.conv_h1_fwd(x, None, f, sw, None, y, Co, 0, sx)                                                      # and the plain request goes through
    torch.cuda.synchronize()
    assert not bool((y == 7.0).any()) and bool((big[B * H * W * Co:] == 7.0).all())


# ------------------------------------------------------------------ 9. networks
def _net(arch, scale, res=False):
    from oracle import net_torch as O
    from pnnp_amd.archs import ResUnet, UNetSeeInDark
    shapes = O.unet_param_shapes(nf=32) if arch == 'unet' else O.resunet_param_shapes(nf=32)
    sd = {k: v * scale for k, v in O.init_state(shapes, seed=5).items()}
    net = (UNetSeeInDark if arch == 'unet' else ResUnet)(dict(nframes=1, res=res, nf=32, in_nc=4, out_nc=4))
    net.load_state_dict({k: v.clone() for k, v in sd.items()})
    return net.cuda().eval(), sd


def _input(shape):
    g = torch.Generator().manual_seed(11)
    x = torch.rand(*shape, generator=g)
    if shape[0] > 1:
        x[0] *= 100.0                                               # one crop x 100 brighter than its batch-mate
    else:
        x[0, :, 8:40, 16:48] *= 100.0                               # ... than the rest of the frame
    return x.cuda()


@pytest.mark.parametrize('wscale', [1.0, 6.0])                      # init_state as it is (N(0, 0.02): a nearly dead network), and x 6: every layer matters
@pytest.mark.parametrize('arch,shape', [('unet', (2, 4, 64, 64)), ('unet', (1, 4, 80, 112)), ('resunet', (1, 4, 64, 64))])
def test_h1_network_forward_vs_float64(arch, shape, wscale):
    """With h1_eval on, the output's relative L2 against the EXACT float64 forward is at most 2 e_emu + the eval-forward bar, e_emu the emulation's own
    relative L2 (tests/_h1_ref.py: float64, rounding exactly at the plan's 'h1*' layers).  The factor 2 is derived, not measured: a last-bit difference in a
    float32 activation can flip an fp16 rounding, the engine and the emulation then make independent errors of equal size on those elements, which add to
    at most 2 x (typically sqrt 2).  The bar of an eval forward is rtol 1e-4 / atol 2e-6 per element (tests/test_gpu_unet.py), here as its L2 norm."""
    net, sd = _net(arch, wscale)
    e = net.engine
    x = _input(shape)
    sd64 = {k: v.double().cuda() for k, v in sd.items()}
    fwd = h1_unet_forward if arch == 'unet' else h1_resunet_forward
    with torch.no_grad():
        y_h2 = net(x).clone()
        e.set_policy(h1_eval=True)
        y_h1 = net(x).clone()
        plan = e._plan
        e.set_policy(h1_eval=False)
        y_off = net(x).clone()
    h1_layers = [n for n, s in plan.steps.items() if s.fwd.startswith('h1')]
    assert len(h1_layers) >= 18 and plan.h2 and not plan.train
    if arch == 'unet':
        assert any(s.fwd == 'h1+splitk' for s in plan.steps.values()) and plan['conv9_2'].fwd == 'h1+head' and plan['conv1_2'].fwd in ('h1+pool', 'h1+splitk')
    exact = fwd(sd64, x)
    emu = fwd(sd64, x, h1_layers)
    e_emu, e_h1, e_h2 = _rel(emu, exact), _rel(y_h1.double(), exact), _rel(y_h2.double(), exact)
    bar = float((2e-6 + 1e-4 * exact.abs()).norm() / exact.norm())
    print(f'{arch} {shape} weights x {wscale}: relative L2 vs exact float64: h1 {e_h1:.3e}, emulation {e_emu:.3e}, fp16x2 {e_h2:.3e}; bar term {bar:.2e}')
    assert torch.isfinite(y_h1).all()
    assert e_h1 <= 2.0 * e_emu + bar
    if wscale > 1.0:
        assert e_emu > 10 * e_h2                                    # (the emulation does round: the comparison is not vacuous)
    # the switch off again: bit-equal to before, and to a fresh engine
    fresh, _ = _net(arch, wscale)
    with torch.no_grad():
        assert torch.equal(y_off, y_h2) and torch.equal(fresh(x), y_h2)


def test_h1_eval_forward_leaves_training_bit_identical():
    from pnnp_amd.trainer import HipTrainStep
    x = _input((2, 4, 64, 64)); t = torch.rand(2, 4, 64, 64, device='cuda', generator=torch.Generator(device='cuda').manual_seed(2))

    def run(h1):
        net, _ = _net('unet', 6.0)
        net.train()
        ts = HipTrainStep(net, lr=1e-4, clip=0)
        if h1:
            net.engine.set_policy(h1_eval=True)
            with torch.no_grad():
                net(x)                                              # an h1 eval forward on the training shape, then the step WITH the switch still on
        losses = [ts.step(t, noisy=x)[0].clone() for _ in range(2)]
        return torch.stack(losses), [p.detach().clone() for p in net.parameters()], net.engine._plan.table()
    l0, p0, t0 = run(False)
    l1, p1, t1 = run(True)
    assert t1 == t0 and not any(str(f).startswith('h1') for fam in t1.values() for f in fam)
    assert torch.equal(l1, l0) and all(torch.equal(a, b) for a, b in zip(p1, p0))


# ------------------------------------------------------------------ 10. the public path
def test_h1_public_precision_argument():
    from pnnp_amd import isp_ops, tiles
    from pnnp_amd._lib import PnnpError
    from pnnp_amd.evaluate import EvalLoop, evaluate, forward_tiled, predict
    net, _ = _net('unet', 6.0, res=True)
    e = net.engine
    g = torch.Generator().manual_seed(3)
    Hh, Ww, P, BASE = 150, 170, 64, 16
    x = torch.rand(1, 4, Hh, Ww, generator=g).cuda()
    with torch.no_grad():
        e.set_policy(h1_eval=True)
        comp = tiles.eval_merge(net(tiles.eval_crop(x, P, BASE)), Hh, Ww, BASE)
        assert any(s.fwd.startswith('h1') for s in e._plan.steps.values())
        e.set_policy(h1_eval=False)
        comp32 = tiles.eval_merge(net(tiles.eval_crop(x, P, BASE)), Hh, Ww, BASE)
    e._h2_sub.pop('h1_eval')
    got = forward_tiled(net, x, P, base=BASE, precision='fp16')
    assert torch.equal(got, comp) and not torch.equal(comp, comp32)
    assert not e.policy.h1_eval and 'h1_eval' not in e._h2_sub      # restored
    assert torch.equal(forward_tiled(net, x, P, base=BASE, precision='fp32'), comp32) and torch.equal(forward_tiled(net, x, P, base=BASE), comp32)
    e.set_policy(h1_eval=True)                                      # None leaves the engine's policy alone; 'fp32' overrides it for the call
    assert torch.equal(forward_tiled(net, x, P, base=BASE), comp) and torch.equal(forward_tiled(net, x, P, base=BASE, precision='fp32'), comp32)
    assert e.policy.h1_eval
    e.set_policy(h1_eval=False)
    raw = torch.from_numpy(np.random.default_rng(3).integers(400, 16383, size=(2 * Hh, 2 * Ww), dtype=np.uint16))
    packed = isp_ops.raw2bayer(raw.cuda(), wp=16383, bl=512)[None]
    with torch.no_grad():
        e.set_policy(h1_eval=True)
        want = tiles.eval_merge(net(tiles.eval_crop(packed, P, BASE)), Hh, Ww, BASE)[0]
        e.set_policy(h1_eval=False)
    assert torch.equal(predict(net, raw, 16383, 512, P, base=BASE, precision='fp16'), want)
    # evaluate: the 64 x 64 case; the switch comes back also when the call raises
    hr = torch.rand(1, 4, 64, 64, generator=g).cuda() * 0.5
    lr = (hr + 0.02 * torch.randn(1, 4, 64, 64, generator=g).cuda()).clamp(0, 1)
    m16 = evaluate(net, lr, hr, precision='fp16')['metrics'].cpu()
    assert not e.policy.h1_eval
    m32 = evaluate(net, lr, hr, precision='fp32')['metrics'].cpu()
    print(f'evaluate 64 x 64: [PSNR, SSIM] fp16 {m16[:2].tolist()} fp32 {m32[:2].tolist()}')
    assert abs(float(m16[0] - m32[0])) < 0.05 and torch.equal(m16[2:], m32[2:])
    with pytest.raises(PnnpError):
        evaluate(net, lr[0], hr, precision='fp16')                  # not [1,C,H,W]: raises inside the call
    assert not e.policy.h1_eval
    with pytest.raises(PnnpError):
        evaluate(net, lr, hr, precision='bf16')
    loop = EvalLoop(net, brightness_correct=True, precision='fp16')
    out = loop.step('a', lr, hr)
    assert torch.equal(out['metrics'].cpu(), m16) and not e.policy.h1_eval

"""GPU checks of the opt-in fp16x1 POINTWISE layers of an eval forward (csrc/gemm_h1s.hip: ConvTranspose2d, the 1x1 shortcut, the stride-2 3x3 convolution
with ONE fp16 piece per operand; ConvPolicy.h1_pointwise, precision='fp16_all').  The yardstick is tests/_h1pw_ref.py (pinned on the host by
tests/test_host_h1pw_ref.py).  The layer cases are every distinct (kind, K, N) the plans of UNet (nf = 32) and ResUnet turn to pointwise 'h1', at the smallest
maps that still reach each path of the kernel: one K item (K = 32) and more items than the weight ring has stages (K = 512: the ring wraps; 72 items for the
deepest stride-2 layer), the 128-, 64- and 32-column tiles, ragged tiles (W no multiple of 32, H no multiple of 8), B = 2, two K segments, nine tap segments.

Bars: against the emulation the kernel must be as accurate as the fp32 direct kernel fed the same rounded operands (e1 < 2 e32 + 1e-8 and e1 < 5e-7: the bar of
test_h1_layer_equals_the_emulation_to_fp32_mfma_accuracy); against the UNROUNDED float64 layer every element stays within (2^-10 + 2^-20) sum |x||w| + tiny and
the relative L2 is the emulation's own to within [0.5, 2].  Whole networks: e <= 2 e_emu + the eval-forward bar (the factor 2 as derived in
tests/test_gpu_h1.py: a last-bit difference in a float32 activation can flip an fp16 rounding, and the two then err independently).

Not reachable from here: the launcher's refusal of masks, bit images, accumulating and second destinations (PNNP_E_UNSUPPORTED in pnnp_gemm_h1s_launch).  They
are not arguments of any h1 entry of the C ABI, so no caller outside the library can ask; the refusals that CAN be asked for are checked below."""
import numpy as np
import pytest
import torch

from _h1_ref import act64, h1_resunet_forward, h1_round, h1_scale_exp, h1_unet_forward
from _h1pw_ref import h1_conv1x1, h1_conv_s2, h1_convt, h1pw_resunet_forward, h1pw_unet_forward
from test_gpu_conv import _rand, nchw, nhwc

pytestmark = pytest.mark.gpu

CH = [32, 64, 128, 256, 512]
# (kind, K per segment, N of the forward GEMM) -> (B, H, W) of the INPUT map
SHAPES = {('convt', 512, 1024): (1, 8, 8),        # 16 items: the ring of 4 stages wraps; 128-column tiles; a map smaller than a tile
          ('convt', 256, 512): (2, 8, 16),
          ('convt', 128, 256): (1, 16, 24),
          ('convt', 64, 128): (1, 24, 40),        # ragged: two tile columns, three tile rows
          ('1x1', 256, 256): (1, 8, 8),           # two K segments of 8 items
          ('1x1', 128, 128): (2, 8, 16),
          ('1x1', 64, 64): (1, 24, 40),           # 64-column tiles
          ('1x1', 32, 32): (2, 24, 40),           # 32-column tiles, ONE item per segment
          ('s2', 32, 64): (2, 32, 48),            # nine tap segments of one item, 64-column tiles, output 16 x 24
          ('s2', 64, 128): (1, 16, 16),
          ('s2', 128, 256): (1, 24, 40),          # output 12 x 20: ragged both ways
          ('s2', 256, 512): (1, 16, 16)}          # 72 items
CASES = sorted(SHAPES)


def _plan_cases():
    """every distinct (kind, K, N) that the eval plans turn to pointwise 'h1' (host functions only)"""
    from pnnp_amd.archs import plan as P
    pol = P.ConvPolicy()
    pol.h1_eval = pol.h1_pointwise = True
    got = set()
    pu = P.resolve_unet(CH, 4, 4, pol, False, 1, 64, 64)
    pr = P.resolve_resunet(CH, 4, 4, pol, False, 1, 64, 64)
    for i in range(6, 10):
        for p in (pu, pr):
            assert p[f'upv{i}'].fwd == 'h1'
        got.add(('convt', CH[10 - i], 4 * CH[9 - i]))
        assert pr[f'sc{i}'].fwd == 'h1'
        got.add(('1x1', CH[9 - i], CH[9 - i]))
    for i in range(1, 5):
        assert pr[f'pool{i}'].fwd == 'h1'
        got.add(('s2', CH[i - 1], CH[i]))
    return got


def test_the_cases_are_the_plans():
    assert _plan_cases() == set(SHAPES)


def _slot(*tensors):
    from pnnp_amd import ops
    s = torch.zeros(1, dtype=torch.int32, device='cuda')
    for t in tensors:
        ops.amax(t, s)
    return s


def _slot_value(s):
    return float(s.cpu().view(torch.float32)[0])


def _rel(a, b):
    return float((a - b).norm() / b.norm())


def _pack(kind, w, fill=0):
    """the kind-8 pack of ``w`` and the weight tensor's slot; K, N of the forward GEMM"""
    from pnnp_amd import ops
    if kind == 'convt':
        K, N = w.shape[0], 4 * w.shape[1]
    elif kind == '1x1':
        K, N = w.shape[1], w.shape[0]
    else:
        K, N = 9 * w.shape[1], w.shape[0]
    jobs = ops.PackJobs()
    f = torch.full((ops.h1_pointwise_weight_bytes(K, N),), fill, dtype=torch.uint8, device='cuda')
    sw = getattr(jobs, f'add_h1_{kind}')(w, f)
    jobs.run()
    return f, sw, K, N


def _matrix(kind, w):
    """the [K][N] matrix of the forward GEMM in the documented order"""
    if kind == 'convt':                                            # column s Cout + co, s = 2 a + c
        return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)
    if kind == '1x1':
        return w[:, :, 0, 0].t()
    return w.reshape(w.shape[0], w.shape[1], 9).permute(2, 1, 0).reshape(9 * w.shape[1], w.shape[0])      # row t Cin + ci


def _weights(kind, K, N, seed=3):
    if kind == 'convt':
        return _rand(K, N // 4, 2, 2, seed=seed, scale=0.2)
    if kind == '1x1':
        return _rand(N, 2 * K, 1, 1, seed=seed, scale=0.2)
    return _rand(N, K, 3, 3, seed=seed, scale=0.2)


# ------------------------------------------------------------------ 1. pack
@pytest.mark.parametrize('kind,K,N', [('convt', 64, 128), ('1x1', 32, 96), ('s2', 32, 64)])
def test_h1_pointwise_pack_is_the_rounded_scaled_weights_bit_for_bit(kind, K, N):
    """[N/32][K/32][octet 4][32][8] fp16: element (k, n) at block n / 32, item k / 32, octet (k / 8) % 4, column n % 32, lane k % 8 = float16(w 2^se) bit for
    bit, every byte of the buffer written, the maximum in [2^14, 2^15)."""
    w = _weights(kind, K, N)
    w = (w * torch.logspace(-3, 1, w.numel()).reshape(w.shape)).cuda()
    f, sw, Kt, Nt = _pack(kind, w, fill=0xAB)
    amax = _slot_value(sw)
    assert amax == float(w.abs().max())
    se = h1_scale_exp(amax)
    a = f.view(torch.float16).cpu().numpy().reshape(Nt // 32, Kt // 32, 4, 32, 8)          # [nb][item][octet][nn][e]
    got = a.transpose(1, 2, 4, 0, 3).reshape(Kt, Nt)
    m = _matrix(kind, w.cpu()).numpy().astype(np.float64)
    assert m.shape == (Kt, Nt)
    want = (m * 2.0 ** se).astype(np.float16)
    assert np.array_equal(got.view(np.uint16), want.view(np.uint16))
    assert np.array_equal(got.astype(np.float64) * 2.0 ** -se, _matrix(kind, h1_round(w).cpu()).numpy())
    assert 2.0 ** 14 <= np.abs(got.astype(np.float64)).max() < 2.0 ** 15


# ------------------------------------------------------------------ 2. layers
_LAYER = {}


def _lin(kind, x, w):
    """the layer's linear map in float64, unrounded, without bias"""
    if kind == 'convt':
        return h1_convt(x, w, None, rounded=False)
    if kind == '1x1':
        return h1_conv1x1(x, None, w, None, 0, rounded=False)
    return h1_conv_s2(x, w, None, 0, rounded=False)


def _layer(case):
    """Operands, float64 references and the kernel's outputs of one case, computed once and shared (never modified).  Variants: the activations the entry takes
    (ConvTranspose2d: none) and, for the 1x1 layer, 'res' = bias + residual without activation (the general epilogue)."""
    if case in _LAYER:
        return _LAYER[case]
    from pnnp_amd import ops
    kind, K, N = case
    B, H, W = SHAPES[case]
    w = _weights(kind, K, N).cuda()
    Co = N // 4 if kind == 'convt' else N
    b = _rand(Co, seed=4).cuda()
    x = _rand(B, K, H, W, seed=1).cuda()
    x2 = (_rand(B, K, H, W, seed=2) * 8.0).cuda() if kind == '1x1' else None               # the second segment sets the scale of both
    xin = torch.cat([x, x2], 1) if x2 is not None else x
    OH, OW = (2 * H, 2 * W) if kind == 'convt' else (H // 2, W // 2) if kind == 's2' else (H, W)
    res = _rand(B, Co, OH, OW, seed=5).cuda() if kind == '1x1' else None
    f, sw, _, _ = _pack(kind, w)
    xc, x2c = nhwc(x), (nhwc(x2) if x2 is not None else None)
    s1, s2 = _slot(xc), (_slot(x2c) if x2 is not None else None)
    resc = nhwc(res) if res is not None else None
    # the fp32 direct kernels on the already-rounded operands (exact in float32)
    xr, wr = h1_round(xin).float(), h1_round(w).float()
    f32 = torch.empty(wr.numel(), device='cuda')
    if kind == 'convt':
        ops.pack_convt_weight(wr, f32, None)
    else:
        ops.pack_conv_weight(wr, f32, None)
    xrc, xr2c = nhwc(xr[:, :K]), (nhwc(xr[:, K:]) if x2 is not None else None)
    variants = [0] if kind == 'convt' else [0, 1, 2] + (['res'] if kind == '1x1' else [])
    emu_pre, exact_pre = _lin(kind, h1_round(xin), h1_round(w)), _lin(kind, xin, w)
    bb = b.double().reshape(1, -1, 1, 1)
    ys, y32s, amax, emu, exact = {}, {}, {}, {}, {}
    for v in variants:
        act = 0 if v == 'res' else v
        r = resc if v == 'res' else None
        y = torch.full((B, OH, OW, Co), float('nan'), device='cuda')
        sy = torch.zeros(1, dtype=torch.int32, device='cuda')
        y32 = torch.empty_like(y)
        if kind == 'convt':
            ops.convt_h1_fwd(xc, s1, f, sw, b, y, Co, amax_y=sy)
            ops.convt_fwd(xrc, f32, b, y32, Co)
        elif kind == '1x1':
            ops.conv1x1_h1_fwd(xc, s1, x2c, s2, f, sw, b, y, Co, act, residual=r, amax_y=sy)
            ops.conv_fwd(xrc, xr2c, f32, b, y32, Co, 1, act, residual=r)
        else:
            ops.conv_s2_h1_fwd(xc, s1, f, sw, b, y, Co, act, amax_y=sy)
            ops.conv_s2_fwd(xrc, f32, b, y32, Co, act)
        add = res.double() if v == 'res' else 0.0
        ys[v], y32s[v], amax[v] = nchw(y), nchw(y32).double(), _slot_value(sy)
        emu[v], exact[v] = act64(emu_pre + bb + add, act), act64(exact_pre + bb + add, act)
    _LAYER[case] = dict(kind=kind, xin=xin, w=w, variants=variants, y=ys, y32=y32s, amax=amax, emu=emu, exact=exact, terms=_lin(kind, xin.abs(), w.abs()))
    return _LAYER[case]


@pytest.mark.parametrize('case', CASES)
def test_h1_pointwise_layer_equals_the_emulation_to_fp32_accuracy(case):
    L = _layer(case)
    for v in L['variants']:
        y, ref = L['y'][v], L['emu'][v]
        assert not torch.isnan(y).any(), 'the sentinel-filled output is fully overwritten'
        e1, e32 = _rel(y.double(), ref), _rel(L['y32'][v], ref)
        print(f'h1 pointwise {case} {SHAPES[case]} variant {v}: relative L2 vs the emulation {e1:.2e}, fp32 direct kernel on the rounded operands {e32:.2e}')
        assert e1 < 2.0 * e32 + 1e-8 and e1 < 5e-7
        assert L['amax'][v] == float(y.abs().max()), 'amax of the stored output'


@pytest.mark.parametrize('case', CASES)
def test_h1_pointwise_error_is_one_fp16_rounding_per_operand(case):
    """|y - exact64| <= (2^-10 + 2^-20) sum |x||w| + tiny per element ((1 + 2^-11)^2 - 1 on every product, the rest for the float32 sums), tiny = half an fp16
    subnormal step per operand, as in test_h1_error_is_one_fp16_rounding_per_operand; and the relative L2 of y - exact64 is the emulation's own to within
    [0.5, 2]: one rounding happened.  (Bias, residual and the 1-Lipschitz activations carry the bound over.)"""
    L = _layer(case)
    kind = L['kind']
    sx, sw = 2.0 ** -h1_scale_exp(float(L['xin'].abs().max())), 2.0 ** -h1_scale_exp(float(L['w'].abs().max()))
    ones_x, ones_w = torch.ones_like(L['xin']), torch.ones_like(L['w'])
    tiny = 2.0 ** -25 * (sx * _lin(kind, ones_x, L['w'].abs()) + sw * _lin(kind, L['xin'].abs(), ones_w) + 2.0 ** -25 * sx * sw * _lin(kind, ones_x, ones_w))
    bound = (2.0 ** -10 + 2.0 ** -20) * L['terms'] + tiny
    for v in L['variants']:
        exact = L['exact'][v]
        err = (L['y'][v].double() - exact).abs()
        worst = float((err / bound).max())
        e_y, e_emu = _rel(L['y'][v].double(), exact), _rel(L['emu'][v], exact)
        print(f'h1 pointwise {case} variant {v}: max |err| / bound {worst:.3f}; relative L2 vs exact float64: kernel {e_y:.3e}, emulation {e_emu:.3e}')
        assert worst <= 1.0
        assert 0.5 * e_emu <= e_y <= 2.0 * e_emu
        assert e_emu > 1e-5                                        # (the rounding is really there: fp16x2 sits at 1e-7)


# ------------------------------------------------------------------ 3. NaN / inf
@pytest.mark.parametrize('kind', ['convt', '1x1', 's2'])
def test_h1_pointwise_nan_reaches_exactly_the_outputs_it_feeds(kind):
    """One NaN (one inf) input element: the 2 x 2 block of ConvTranspose2d, the one pixel of the 1x1 layer, the covering windows of the stride-2 layer -- every
    channel of those pixels, and nothing else (no padding word and no neighbouring pixel is multiplied with it)."""
    from pnnp_amd import ops
    B, H, W, K, Co = 1, 16, 40, 32, 32
    iy, ix = 5, 8
    x = _rand(B, K, H, W, seed=1).cuda()
    x2 = _rand(B, K, H, W, seed=2).cuda() if kind == '1x1' else None
    w = _weights(kind, K, 4 * Co if kind == 'convt' else Co).cuda()
    f, sw, _, _ = _pack(kind, w)
    OH, OW = (2 * H, 2 * W) if kind == 'convt' else (H // 2, W // 2) if kind == 's2' else (H, W)
    hit = torch.zeros((OH, OW), dtype=torch.bool, device='cuda')
    if kind == 'convt':
        hit[2 * iy:2 * iy + 2, 2 * ix:2 * ix + 2] = True
    elif kind == '1x1':
        hit[iy, ix] = True
    else:                                                           # output (oy, ox) reads input rows 2 oy - 1 .. 2 oy + 1
        for oy in range(OH):
            for ox in range(OW):
                hit[oy, ox] = abs(iy - 2 * oy) <= 1 and abs(ix - 2 * ox) <= 1
        assert int(hit.sum()) == 2
    for bad in (float('nan'), float('inf')):
        xb = x.clone()
        xb[0, 3, iy, ix] = bad
        xc, x2c = nhwc(xb), (nhwc(x2) if x2 is not None else None)
        y = torch.zeros((B, OH, OW, Co), device='cuda')
        if kind == 'convt':
            ops.convt_h1_fwd(xc, _slot(xc), f, sw, None, y, Co)
        elif kind == '1x1':
            ops.conv1x1_h1_fwd(xc, _slot(xc), x2c, _slot(x2c), f, sw, None, y, Co, 0)
        else:
            ops.conv_s2_h1_fwd(xc, _slot(xc), f, sw, None, y, Co, 0)
        assert not torch.isfinite(y[0][hit]).any()
        assert torch.isfinite(y[0][~hit]).all()
        # elsewhere: the same operands at scale 1 (a diverged tensor's slot), i.e. the emulation at that scale
        xin = torch.cat([x, x2], 1) if x2 is not None else x
        ref = nhwc(_lin(kind, h1_round(xin, float('inf')), h1_round(w)))
        assert float((y[0][~hit].double() - ref[0][~hit]).norm() / ref[0][~hit].norm()) < 5e-7


# ------------------------------------------------------------------ 4. refusals
def test_h1_pointwise_refusals_leave_the_outputs_untouched():
    """What the C entries can be asked for and do not do: PNNP_E_INVALID (-1) for misaligned or missing pointers and slots and channel counts off the 32 grid of
    K, PNNP_E_UNSUPPORTED (-2) for N % 32; nothing is launched.  (Masks, bit images, accumulation and a second destination: see the module docstring.)"""
    from pnnp_amd import ops
    from pnnp_amd._lib import PnnpError
    B, H, W, C, Co = 1, 16, 32, 32, 32
    x = torch.randn(B, H, W, C, device='cuda'); x2 = torch.randn(B, H, W, C, device='cuda')
    sx, sx2 = _slot(x), _slot(x2)
    w1 = torch.randn(Co, 2 * C, 1, 1, device='cuda') * 0.1; f1, sw1, _, _ = _pack('1x1', w1)
    wt = torch.randn(C, Co, 2, 2, device='cuda') * 0.1; ft, swt, _, _ = _pack('convt', wt)
    w3 = torch.randn(Co, C, 3, 3, device='cuda') * 0.1; f3, sw3, _, _ = _pack('s2', w3)
    big = torch.full((4 * B * H * W * Co + 8,), 7.0, device='cuda')
    n1 = B * H * W * Co
    y = big[:n1].view(B, H, W, Co); y_off = big[1:1 + n1].view(B, H, W, Co)
    yt = big[:4 * n1].view(B, 2 * H, 2 * W, Co); ys = big[:n1 // 4].view(B, H // 2, W // 2, Co)
    bias = torch.full((Co + 4,), 7.0, device='cuda')
    raw = torch.zeros(16, dtype=torch.uint8, device='cuda')
    odd_slot = raw[1:5]                                              # a slot off the 4-byte grid
    x16 = torch.randn(B, H, W, 16, device='cuda')
    res = torch.full((n1 + 4,), 7.0, device='cuda')

    def code(fn, *a, **k):
        with pytest.raises(PnnpError) as e:
            fn(*a, **k)
        return int(str(e.value).split('code ')[1].split(' ')[0])
    assert code(ops.conv1x1_h1_fwd, x, sx, x2, sx2, f1, sw1, None, y_off, Co, 0) == -1                       # y not 16-byte aligned
    assert code(ops.conv1x1_h1_fwd, x, sx, x2, sx2, f1, sw1, bias[1:1 + Co], y, Co, 0) == -1                 # bias not 16-byte aligned
    assert code(ops.conv1x1_h1_fwd, x, sx, x2, sx2, f1, sw1, None, y, Co, 0, residual=res[1:1 + n1].view(B, H, W, Co)) == -1      # residual misaligned
    assert code(ops.conv1x1_h1_fwd, x, odd_slot, x2, sx2, f1, sw1, None, y, Co, 0) == -1                     # a misaligned slot: the input's
    assert code(ops.conv1x1_h1_fwd, x, sx, x2, odd_slot, f1, sw1, None, y, Co, 0) == -1                      # ... the second segment's
    assert code(ops.conv1x1_h1_fwd, x, sx, x2, sx2, f1, odd_slot, None, y, Co, 0) == -1                      # ... the weights'
    assert code(ops.conv1x1_h1_fwd, x, sx, x2, sx2, f1, sw1, None, y, Co, 0, amax_y=odd_slot) == -1          # ... the output's
    assert code(ops.conv1x1_h1_fwd, x, sx, x2, None, f1, sw1, None, y, Co, 0) == -1                          # no slot for the second segment
    assert code(ops.conv1x1_h1_fwd, x, None, None, None, f1, sw1, None, y, Co, 0) == -1                      # no slot for x
    assert code(ops.conv1x1_h1_fwd, x, sx, x16, _slot(x16), f1, sw1, None, y, Co, 0) == -1                   # C2 != C1
    assert code(ops.conv1x1_h1_fwd, x16, _slot(x16), None, None, f1, sw1, None, y, Co, 0) == -1              # K % 32
    assert code(ops.conv1x1_h1_fwd, x, sx, None, None, f1, sw1, None, y.view(B, H, W * 2, 16), 16, 0) == -2  # N % 32
    assert code(ops.convt_h1_fwd, x, odd_slot, ft, swt, None, yt, Co) == -1
    assert code(ops.convt_h1_fwd, x, sx, ft, swt, None, yt, Co, amax_y=odd_slot) == -1
    assert code(ops.convt_h1_fwd, x, sx, ft[8:], swt, None, yt, Co) == -1                                    # the pack misaligned
    assert code(ops.convt_h1_fwd, x16, _slot(x16), ft, swt, None, yt, Co) == -1
    assert code(ops.conv_s2_h1_fwd, x, odd_slot, f3, sw3, None, ys, Co, 0) == -1
    assert code(ops.conv_s2_h1_fwd, x[:, :15], sx, f3, sw3, None, ys, Co, 0) == -1                           # odd height
    assert code(ops.conv_s2_h1_fwd, x, sx, f3, sw3, bias[1:1 + Co], ys, Co, 0) == -1
    torch.cuda.synchronize()
    for k, t in dict(y=big, bias=bias, res=res).items():
        assert bool((t == 7).all()), k
    assert not bool(raw.any())
    ops.conv1x1_h1_fwd(x, sx, x2, sx2, f1, sw1, None, y, Co, 0)                                              # and the plain request goes through
    torch.cuda.synchronize()
    assert not bool((y == 7.0).any()) and bool((big[n1:] == 7.0).all())


# ------------------------------------------------------------------ 5. networks
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


POINTWISE = {'unet': [f'upv{i}' for i in range(6, 10)],
             'resunet': [f'upv{i}' for i in range(6, 10)] + [f'sc{i}' for i in range(6, 10)] + [f'pool{i}' for i in range(1, 5)]}


@pytest.mark.parametrize('wscale', [1.0, 6.0])                      # init_state as it is (N(0, 0.02): a nearly dead network), and x 6: every layer matters
@pytest.mark.parametrize('arch,shape', [('unet', (2, 4, 64, 64)), ('unet', (1, 4, 80, 112)), ('resunet', (1, 4, 64, 64))])
def test_h1_pointwise_network_forward_vs_float64(arch, shape, wscale):
    """With h1_eval AND h1_pointwise on, the output's relative L2 against the EXACT float64 forward is at most 2 e_emu + the eval-forward bar, e_emu the
    emulation's own (tests/_h1pw_ref.py: float64, rounding exactly at the plan's 'h1*' steps, 3x3 and pointwise).  The factor 2 is the derived one of
    test_h1_network_forward_vs_float64; the bar of an eval forward is rtol 1e-4 / atol 2e-6 per element (tests/test_gpu_unet.py), here as its L2 norm."""
    net, sd = _net(arch, wscale)
    e = net.engine
    x = _input(shape)
    sd64 = {k: v.double().cuda() for k, v in sd.items()}
    fwd = h1pw_unet_forward if arch == 'unet' else h1pw_resunet_forward
    with torch.no_grad():
        y_h2 = net(x).clone()
        e.set_policy(h1_pointwise=True)                             # alone, without h1_eval: nothing changes
        y_alone = net(x).clone()
        assert not any(str(s.fwd).startswith('h1') for s in e._plan.steps.values())
        e.set_policy(h1_eval=True, h1_pointwise=False)
        y_h1 = net(x).clone()
        plan_h1 = e._plan
        e.set_policy(h1_pointwise=True)
        y_all = net(x).clone()
        plan = e._plan
        e.set_policy(h1_eval=False, h1_pointwise=False)
        y_off = net(x).clone()
    assert torch.equal(y_alone, y_h2)
    assert all(plan_h1[n].fwd == 'h2' for n in POINTWISE[arch])
    assert all(plan[n].fwd == 'h1' and plan[n].pack == ('h1', None) for n in POINTWISE[arch])
    assert not any(plan[n].fwd == 'h2' for n in plan.steps if n.startswith(('upv', 'sc', 'pool')))
    assert plan.h2 and not plan.train
    h1_layers = [n for n, s in plan.steps.items() if s.fwd.startswith('h1')]
    assert len(h1_layers) >= 18 + len(POINTWISE[arch])
    exact = fwd(sd64, x)
    emu = fwd(sd64, x, h1_layers)
    e_emu, e_all, e_h1, e_h2 = _rel(emu, exact), _rel(y_all.double(), exact), _rel(y_h1.double(), exact), _rel(y_h2.double(), exact)
    bar = float((2e-6 + 1e-4 * exact.abs()).norm() / exact.norm())
    print(f'{arch} {shape} weights x {wscale}: relative L2 vs exact float64: fp16_all {e_all:.3e}, emulation {e_emu:.3e}, h1_eval only {e_h1:.3e}, '
          f'fp16x2 {e_h2:.3e}; bar term {bar:.2e}')
    assert torch.isfinite(y_all).all()
    assert e_all <= 2.0 * e_emu + bar
    assert not torch.equal(y_all, y_h1)                             # (the pointwise layers did change kernels)
    if wscale > 1.0:
        assert e_emu > 10 * e_h2                                    # (the emulation does round: the comparison is not vacuous)
    # both switches off again: bit-equal to before, and to a fresh engine
    fresh, _ = _net(arch, wscale)
    with torch.no_grad():
        assert torch.equal(y_off, y_h2) and torch.equal(fresh(x), y_h2)


def test_h1_pointwise_leaves_training_bit_identical():
    from pnnp_amd.trainer import HipTrainStep
    x = _input((2, 4, 64, 64)); t = torch.rand(2, 4, 64, 64, device='cuda', generator=torch.Generator(device='cuda').manual_seed(2))

    def run(arch, on):
        net, _ = _net(arch, 6.0)
        net.train()
        ts = HipTrainStep(net, lr=1e-4, clip=0)
        if on:
            net.engine.set_policy(h1_eval=True, h1_pointwise=True)
            with torch.no_grad():
                net.eval()
                net(x)                                              # an fp16_all eval forward on the training shape, then the step WITH both switches still on
                assert any(s.fwd == 'h1' for n, s in net.engine._plan.steps.items() if n.startswith('upv'))
                net.train()
        losses = [ts.step(t, noisy=x)[0].clone() for _ in range(2)]
        return torch.stack(losses), [p.detach().clone() for p in net.parameters()], net.engine._plan.table()
    for arch in ('unet', 'resunet'):
        l0, p0, t0 = run(arch, False)
        l1, p1, t1 = run(arch, True)
        assert t1 == t0 and not any(str(f).startswith('h1') for fam in t1.values() for f in fam)
        assert torch.equal(l1, l0) and all(torch.equal(a, b) for a, b in zip(p1, p0))


# ------------------------------------------------------------------ 6. the public path
def test_h1_pointwise_public_precision_argument():
    from pnnp_amd import isp_ops, tiles
    from pnnp_amd._lib import PnnpError
    from pnnp_amd.evaluate import EvalLoop, evaluate, forward_tiled, predict
    net, _ = _net('unet', 6.0, res=True)
    e = net.engine
    g = torch.Generator().manual_seed(3)
    Hh, Ww, P, BASE = 150, 170, 64, 16
    x = torch.rand(1, 4, Hh, Ww, generator=g).cuda()
    with torch.no_grad():
        comp32 = tiles.eval_merge(net(tiles.eval_crop(x, P, BASE)), Hh, Ww, BASE)
        e.set_policy(h1_eval=True)
        comp16 = tiles.eval_merge(net(tiles.eval_crop(x, P, BASE)), Hh, Ww, BASE)
        e.set_policy(h1_pointwise=True)
        comp_all = tiles.eval_merge(net(tiles.eval_crop(x, P, BASE)), Hh, Ww, BASE)
        assert all(e._plan[f'upv{i}'].fwd == 'h1' for i in range(6, 10))
        e.set_policy(h1_eval=False, h1_pointwise=False)
    e._h2_sub.pop('h1_eval'); e._h2_sub.pop('h1_pointwise')
    assert not torch.equal(comp_all, comp16) and not torch.equal(comp16, comp32)
    # 'fp16' is h1_eval alone, exactly as before; 'fp32' and None likewise
    assert torch.equal(forward_tiled(net, x, P, base=BASE, precision='fp16'), comp16)
    assert torch.equal(forward_tiled(net, x, P, base=BASE, precision='fp32'), comp32) and torch.equal(forward_tiled(net, x, P, base=BASE), comp32)
    assert torch.equal(forward_tiled(net, x, P, base=BASE, precision='fp16_all'), comp_all)
    assert not e.policy.h1_eval and not e.policy.h1_pointwise and not ({'h1_eval', 'h1_pointwise'} & set(e._h2_sub))      # restored
    e.set_policy(h1_eval=True)                                      # an engine serving 'fp16': 'fp16_all' borrows the second switch only
    assert torch.equal(forward_tiled(net, x, P, base=BASE, precision='fp16_all'), comp_all)
    assert e.policy.h1_eval and not e.policy.h1_pointwise
    assert torch.equal(forward_tiled(net, x, P, base=BASE), comp16)
    e.set_policy(h1_eval=False)
    raw = torch.from_numpy(np.random.default_rng(3).integers(400, 16383, size=(2 * Hh, 2 * Ww), dtype=np.uint16))
    packed = isp_ops.raw2bayer(raw.cuda(), wp=16383, bl=512)[None]
    with torch.no_grad():
        e.set_policy(h1_eval=True, h1_pointwise=True)
        want = tiles.eval_merge(net(tiles.eval_crop(packed, P, BASE)), Hh, Ww, BASE)[0]
        e.set_policy(h1_eval=False, h1_pointwise=False)
    assert torch.equal(predict(net, raw, 16383, 512, P, base=BASE, precision='fp16_all'), want)
    # evaluate: the switches come back also when the call raises
    hr = torch.rand(1, 4, 64, 64, generator=g).cuda() * 0.5
    lr = (hr + 0.02 * torch.randn(1, 4, 64, 64, generator=g).cuda()).clamp(0, 1)
    m_all = evaluate(net, lr, hr, precision='fp16_all')['metrics'].cpu()
    assert not e.policy.h1_eval and not e.policy.h1_pointwise
    m32 = evaluate(net, lr, hr, precision='fp32')['metrics'].cpu()
    print(f'evaluate 64 x 64: [PSNR, SSIM] fp16_all {m_all[:2].tolist()} fp32 {m32[:2].tolist()}')
    assert abs(float(m_all[0] - m32[0])) < 0.05 and torch.equal(m_all[2:], m32[2:])
    with pytest.raises(PnnpError):
        evaluate(net, lr[0], hr, precision='fp16_all')              # not [1,C,H,W]: raises inside the call
    assert not e.policy.h1_eval and not e.policy.h1_pointwise
    with pytest.raises(PnnpError):
        evaluate(net, lr, hr, precision='fp16_some')
    loop = EvalLoop(net, brightness_correct=True, precision='fp16_all')
    out = loop.step('a', lr, hr)
    assert torch.equal(out['metrics'].cpu(), m_all) and not e.policy.h1_eval and not e.policy.h1_pointwise

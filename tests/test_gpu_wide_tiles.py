"""The 64-column tile instantiations of the fp16x2 ("h2") and bf16x3 ("x3") 3x3 kernels (csrc/conv_h2s.hip, csrc/conv_x3s.hip) against references that
are not kernels of this library -- torch float32 on the CPU at the bars of tests/test_gpu_conv.py, float64 on the CPU next to the fp32-MFMA kernel at the
bars of tests/test_gpu_h2.py / test_gpu_x3.py -- at shapes the width rule (pnnp_h2_tile_columns; one helper for both families, csrc/igemm.h) resolves to
64 columns.  The benchmark step (UNet nf = 32, B = 16, 512 x 512) runs 14 of its 18 conv layers on these instantiations; the shared shape list of
tests/test_gpu_x3.py resolves to 32 columns everywhere (tests/test_host_wide_cases.py records both facts without a GPU).

Every case ASSERTS the width of every launch it makes (as tests/test_gpu_unpool.py does): a case that falls back to 32 columns is the gap this file closes.
No bar here is new; a wide case that needs a looser bar than its narrow twin is a finding.

Which epilogue of launch_h2s<64, .> each test reaches (csrc/conv_h2s.hip, the dispatch at the end of pnnp_igemm_h2s_launch):
  EK_FWD   test_wide_h2_fwd (bias, activations, sign bits, amax), test_wide_h2_bwd_data (the unmasked launches)
  EK_POOL  test_wide_h2_fwd_pool
  EK_BWD   test_wide_h2_bwd_data (float32 masks)
  EK_BWDB  test_wide_h2_bwd_data (the unmasked column ranges), test_wide_h2_bwd_data_bit_masks, test_wide_h2_unpool_against_float64 (the launch without gp)
  EK_BWDU  test_wide_h2_unpool_against_float64
  EK_RES   test_wide_h2_bwd_data (conv_h2_bwd_data_res without a mask)
  EK_GEN   test_wide_h2_fwd (residual + ReLU), test_wide_h2_bwd_data (accumulate; the residual launch with a mask), test_wide_h2_splitk
(EK_HEAD exists for 32 columns only.)"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_gpu_conv import close, nchw, nhwc, _rand
from test_gpu_h2 import _both, _decode_bits, _packs, _slot, _slot_value
from test_gpu_x3 import _packs as _packs_x3

pytestmark = pytest.mark.gpu
LRELU, RELU = 1, 2

# B, H, W, C1, C2 (0 = one segment), Cout.  Tiles = ceil(W / 32) ceil(H / 16) B ceil(N / 64); 64 columns from 192 tiles on (256 compute units).
# Forward: N = Cout; backward-data: N = C1 + C2 (one launch, two destinations) -- both in the comment.  H and W even: the pooled forward runs on every case.
WIDE_CASES = [
    (3, 128, 256, 64, 0, 64),            # 64 -> 64 (conv2_2), 192 / 192 tiles: exactly at the threshold
    (3, 120, 250, 64, 0, 64),            # ... on a map that fills neither its last tile row nor its last tile column: 8 x 8 x 3 = 192 / 192
    (8, 120, 250, 64, 0, 64),            # ... well above the threshold (512 / 512: two tiles per workgroup of the persistent grid), ragged edges
    (2, 128, 192, 128, 0, 128),          # 128 -> 128 (conv3_2), 192 / 192
    (2, 96, 128, 256, 0, 256),           # 256 -> 256 (conv4_2), 192 / 192
    (2, 48, 128, 512, 0, 512),           # 512 -> 512 (conv5_2), 192 / 192
    (3, 128, 256, 64, 64, 64),           # cat([up, skip]) 64 + 64 -> 64 (conv8_1), 192 / 384
    (2, 128, 192, 128, 128, 128),        # 128 + 128 -> 128 (conv7_1), 192 / 384
    (2, 96, 128, 256, 256, 256),         # 256 + 256 -> 256 (conv6_1), 192 / 384
    (3, 128, 256, 32, 32, 64),           # two 32-channel segments; backward-data splits N = 64 into 32 + 32 (conv9_1's two destinations), 192 / 192
]
IDS = ['x'.join(map(str, c)) for c in WIDE_CASES]
# (B, H, W, channels of g, channels of each half of cat([up, skip])) for the skip-gradient launch, N = the half's channels: 192 tiles each
UNPOOL_CASES = [(3, 120, 250, 64, 64), (2, 96, 256, 128, 128), (2, 96, 128, 256, 256)]


def _wide(B, H, W, N, pool=False):
    from pnnp_amd import ops
    return ops.h2_tile_columns(B, H, W, N, pool) == 64


@functools.lru_cache(maxsize=None)
def _fwd_data(case):
    """Inputs of a forward case and conv2d(cat(x1, x2), w, b) in float32 on the CPU.  A patch of batch 0 is zero and half the channels have no bias, so the
    output holds a region of exact zeros: windows whose four elements tie (the pooled forward's first-maximum rule) and elements that are not > 0."""
    B, H, W, C1, C2, Co = case
    x1 = _rand(B, C1, H, W, seed=1); x2 = _rand(B, C2, H, W, seed=2) if C2 else None
    x1[0, :, :8, :16] = 0.0
    if C2:
        x2[0, :, :8, :16] = 0.0
    w = _rand(Co, C1 + C2, 3, 3, seed=3, scale=0.2); b = _rand(Co, seed=4)
    b[: Co // 2] = 0.0
    pre = F.conv2d(torch.cat([x1, x2], 1) if C2 else x1, w, b, padding=1)
    return x1, x2, w, b, pre


@functools.lru_cache(maxsize=None)
def _bwd_data(case):
    """w, g and autograd's d/d(input) of conv2d(., w, padding=1) in float32 on the CPU."""
    B, H, W, C1, C2, Co = case
    w = _rand(Co, C1 + C2, 3, 3, seed=3, scale=0.2)
    g = _rand(B, Co, H, W, seed=5)
    xin = _rand(B, C1 + C2, H, W, seed=6).requires_grad_(True)
    F.conv2d(xin, w, None, padding=1).backward(g)
    return w, g, xin.grad


def _act(t, act):
    return F.leaky_relu(t, 0.2) if act == 1 else (F.relu(t) if act == 2 else t)


def _pool_reference(y):
    """(pooled map, one-byte codes) of MaxPool2d(2) on an NHWC CPU tensor, in torch: the argmax (window order (0,0), (0,1), (1,0), (1,1), first maximum wins
    -- F.max_pool2d's return_indices) in bits 0-1, the four `> 0` flags in bits 2-5 (csrc/misc.hip, maxpool2_fwd_codes_kernel); and the number of tied windows."""
    B, H, W, Cc = y.shape
    pooled, idx = F.max_pool2d(nchw(y), 2, return_indices=True)          # idx: flat position in the [H, W] plane
    arg = ((idx // W) % 2) * 2 + (idx % W) % 2
    win = torch.stack([y[:, dy::2, dx::2] for dy in (0, 1) for dx in (0, 1)])      # [4][B][H/2][W/2][C]
    code = nhwc(arg).to(torch.int32)
    for k in range(4):
        code |= (win[k] > 0).to(torch.int32) << (2 + k)
    tied = int(((win == nhwc(pooled)[None]).sum(0) > 1).sum())
    return nhwc(pooled), code.to(torch.uint8), tied


# --------------------------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize('case', WIDE_CASES, ids=IDS)
def test_wide_h2_fwd(case):
    from pnnp_amd import ops
    B, H, W, C1, C2, Co = case
    assert _wide(B, H, W, Co)
    x1, x2, w, b, pre = _fwd_data(case)
    f, _, sw = _packs(w.cuda(), dgrad=False)
    x1c = nhwc(x1).cuda(); x2c = nhwc(x2).cuda() if C2 else None
    s1 = _slot(x1c); s2 = _slot(x2c) if C2 else None
    for act in (0, 1, 2):
        y = torch.full((B, H, W, Co), float('nan'), device='cuda')
        sy = torch.zeros(1, dtype=torch.int32, device='cuda')
        bits = torch.full((ops.h2_bits_words(B, H, W, Co),), -1, dtype=torch.int32, device='cuda')
        ops.conv_h2_fwd(x1c, x2c, f, sw, b.cuda(), y, Co, act, s1, s2, amax_y=sy, bits_y=bits)
        close(nchw(y), _act(pre, act), what=f'h2 fwd {case} act{act}')
        assert _slot_value(sy) == float(y.abs().max()), 'amax of the stored output'
        assert np.array_equal(_decode_bits(bits, B, H, W, Co), (y > 0).cpu().numpy()), 'sign bits of the stored output'
    r = _rand(B, Co, H, W, seed=9)
    y = torch.full((B, H, W, Co), float('nan'), device='cuda')
    sy = torch.zeros(1, dtype=torch.int32, device='cuda')
    ops.conv_h2_fwd(x1c, x2c, f, sw, b.cuda(), y, Co, 2, s1, s2, amax_y=sy, residual=nhwc(r).cuda())
    close(nchw(y), F.relu(pre + r), what='h2 residual')
    assert _slot_value(sy) == float(y.abs().max())


@pytest.mark.parametrize('case', WIDE_CASES, ids=IDS)
def test_wide_h2_fwd_pool(case):
    """conv3x3 + LeakyReLU + MaxPool2d(2) in one kernel: y against torch float32; the pooled map, the codes, the amax slot and the sign bits are exact
    functions of the y the kernel stored, and are compared exactly with torch's evaluation of them."""
    from pnnp_amd import ops
    B, H, W, C1, C2, Co = case
    assert _wide(B, H, W, Co, pool=True) and _wide(B, H, W, Co)
    x1, x2, w, b, pre = _fwd_data(case)
    f, _, sw = _packs(w.cuda(), dgrad=False)
    x1c = nhwc(x1).cuda(); x2c = nhwc(x2).cuda() if C2 else None
    y = torch.full((B, H, W, Co), float('nan'), device='cuda'); pooled = torch.full((B, H // 2, W // 2, Co), float('nan'), device='cuda')
    codes = torch.full((B, H // 2, W // 2, Co), 255, dtype=torch.uint8, device='cuda')
    sy = torch.zeros(1, dtype=torch.int32, device='cuda')
    bits = torch.full((ops.h2_bits_words(B, H, W, Co),), -1, dtype=torch.int32, device='cuda')
    ops.conv_h2_fwd_pool(x1c, x2c, f, sw, b.cuda(), y, pooled, codes, Co, LRELU, _slot(x1c), _slot(x2c) if C2 else None, amax_y=sy, bits_y=bits)
    close(nchw(y), _act(pre, 1), what=f'h2 fwd+pool {case}')
    ys = y.cpu()
    p_ref, c_ref, tied = _pool_reference(ys)
    assert tied > 0, 'the case holds windows whose maximum is not unique'
    assert torch.equal(pooled.cpu(), p_ref), 'pooled map'
    assert torch.equal(codes.cpu(), c_ref), 'argmax / sign codes'
    assert int((c_ref & 3 != 0).sum()) > 0 and int((c_ref >> 2 == 0).sum()) > 0
    assert _slot_value(sy) == float(ys.abs().max())
    assert np.array_equal(_decode_bits(bits, B, H, W, Co), (ys > 0).numpy())


# --------------------------------------------------------------------------------------------------------------------- backward-data
@pytest.mark.parametrize('case', WIDE_CASES, ids=IDS)
def test_wide_h2_bwd_data(case):
    from pnnp_amd import ops
    B, H, W, C1, C2, Co = case
    assert _wide(B, H, W, C1 + C2)
    w, g, ref = _bwd_data(case)
    _, dg, sw = _packs(w.cuda(), fwd=False)
    gc = nhwc(g).cuda(); sg = _slot(gc)
    new = lambda: torch.zeros(1, dtype=torch.int32, device='cuda')
    nan = lambda c: torch.full((B, H, W, c), float('nan'), device='cuda')
    m1 = _rand(B, C1, H, W, seed=7); m2 = _rand(B, max(C2, 1), H, W, seed=8)
    m1c = nhwc(m1).cuda(); m2c = nhwc(m2).cuda() if C2 else None
    # no masks: one launch, one or two destinations
    d1 = nan(C1); d2 = nan(C2) if C2 else None
    a1, a2 = new(), new()
    ops.conv_h2_bwd_data(gc, sg, dg, sw, d1, amax_dx1=a1, dx2=d2, amax_dx2=a2)
    close(nchw(d1), ref[:, :C1], what=f'h2 dgrad {case}')
    assert _slot_value(a1) == float(d1.abs().max())
    if C2:
        close(nchw(d2), ref[:, C1:], what=f'h2 dgrad2 {case}')
        assert _slot_value(a2) == float(d2.abs().max())
    # float32 masks: LeakyReLU' on destination 1 and ReLU' on destination 2 (one destination: either mode)
    for mode in ((1,) if C2 else (1, 2)):
        d1 = nan(C1); d2 = nan(C2) if C2 else None
        a1, a2 = new(), new()
        ops.conv_h2_bwd_data(gc, sg, dg, sw, d1, mask1=m1c, mode1=mode, amax_dx1=a1, dx2=d2, mask2=m2c, mode2=2 if C2 else 0, amax_dx2=a2)
        close(nchw(d1), ref[:, :C1] * torch.where(m1 > 0, 1.0, 0.2 if mode == 1 else 0.0), what=f'h2 mask1 mode {mode}')
        assert _slot_value(a1) == float(d1.abs().max())
        if C2:
            close(nchw(d2), ref[:, C1:] * (m2 > 0).float(), what='h2 mask2')
            assert _slot_value(a2) == float(d2.abs().max())
    # ... accumulating into the last destination
    base = _rand(B, C2 or C1, H, W, seed=10)
    acc = nhwc(base).cuda().clone(); aa = new()
    if C2:
        ops.conv_h2_bwd_data(gc, sg, dg, sw, nan(C1), mask1=m1c, mode1=1, dx2=acc, mask2=m2c, mode2=2, accum2=1, amax_dx2=aa)
        close(nchw(acc), base + ref[:, C1:] * (m2 > 0).float(), what='h2 mask2+accum')
    else:
        ops.conv_h2_bwd_data(gc, sg, dg, sw, acc, mask1=m1c, mode1=2, accum1=1, amax_dx1=aa)
        close(nchw(acc), base + ref * (m1 > 0).float(), what='h2 mask1+accum')
    assert _slot_value(aa) == float(acc.abs().max()), 'an accumulating destination reports the SUM it stored'
    # a column range of the pack into one destination (what the decoder's split backward-data launches), no pooled gradient
    for col0, c in ((0, C1), (C1, C2)) if C2 else ((0, C1),):
        if not _wide(B, H, W, c):
            continue                                                     # (32 + 32 out of N = 64: a 32-column range is a narrow launch, tests/test_gpu_unpool.py)
        dx = nan(c); ad = new()
        ops.conv_h2_bwd_data_unpool(gc, sg, dg, sw, col0, C1 + C2, dx, amax_dx=ad)
        close(nchw(dx), ref[:, col0:col0 + c], what=f'h2 dgrad columns [{col0}, {col0 + c})')
        assert _slot_value(ad) == float(dx.abs().max())
    # + the identity shortcut's gradient in the epilogue (ResUnet's b{l}_0), without and with the ReLU' mask
    if not C2:
        add = _rand(B, C1, H, W, seed=11)
        for mode in (0, 2):
            dx = nan(C1); ad = new()
            ops.conv_h2_bwd_data_res(gc, sg, dg, sw, dx, addsrc=nhwc(add).cuda(), mask=m1c if mode else None, mode=mode, amax_dx=ad)
            close(nchw(dx), (ref + add) * ((m1 > 0).float() if mode else 1.0), what=f'h2 dgrad res mode {mode}')
            assert _slot_value(ad) == float(dx.abs().max())


def _masking_layer(B, H, W, Cm, pool=False):
    """The output of a forward h2 layer 32 -> Cm with LeakyReLU and the sign bits the kernel wrote for it."""
    from pnnp_amd import ops
    wm = _rand(Cm, 32, 3, 3, seed=12, scale=0.2).cuda(); bm = _rand(Cm, seed=13).cuda()
    fm, _, swm = _packs(wm, dgrad=False)
    xm = nhwc(_rand(B, 32, H, W, seed=14)).cuda()
    ym = torch.empty((B, H, W, Cm), device='cuda')
    bits = torch.full((ops.h2_bits_words(B, H, W, Cm),), -1, dtype=torch.int32, device='cuda')
    if pool:
        pooled = torch.empty((B, H // 2, W // 2, Cm), device='cuda'); codes = torch.empty((B, H // 2, W // 2, Cm), dtype=torch.uint8, device='cuda')
        ops.conv_h2_fwd_pool(xm, None, fm, swm, bm, ym, pooled, codes, Cm, LRELU, _slot(xm), bits_y=bits)
    else:
        ops.conv_h2_fwd(xm, None, fm, swm, bm, ym, Cm, LRELU, _slot(xm), bits_y=bits)
    assert 0.2 < float((ym > 0).float().mean()) < 0.8
    return ym, bits


def _run_bit_masks(case, pool=False):
    """Backward-data with the act' mask as the sign bits a forward h2 layer (the pooled one for ``pool``) wrote, against the same launch with the float32
    activation: bit-identical, and equal to autograd's gradient times the derivative of the STORED activation.  One destination: modes 1 and 2; two: the
    mask on the second only (the decoder's cat([up, skip])).  Returns the channels of the masking tensor."""
    from pnnp_amd import ops
    B, H, W, C1, C2, Co = case
    w, g, ref = _bwd_data(case)
    _, dg, sw = _packs(w.cuda(), fwd=False)
    gc = nhwc(g).cuda(); sg = _slot(gc)
    new = lambda: torch.zeros(1, dtype=torch.int32, device='cuda')
    Cm = C2 if C2 else C1
    ym, bits = _masking_layer(B, H, W, Cm, pool=pool)
    ymc = nchw(ym).cpu()
    if C2:
        ra = torch.empty((B, H, W, C1), device='cuda'); rb = torch.empty((B, H, W, C2), device='cuda')
        ops.conv_h2_bwd_data(gc, sg, dg, sw, ra, dx2=rb, mask2=ym, mode2=1)
        qa = torch.full_like(ra, float('nan')); qb = torch.full_like(rb, float('nan')); sa, sb = new(), new()
        ops.conv_h2_bwd_data(gc, sg, dg, sw, qa, amax_dx1=sa, dx2=qb, bits2=bits, mode2=1, amax_dx2=sb)
        assert torch.equal(ra, qa) and torch.equal(rb, qb)
        assert _slot_value(sa) == float(qa.abs().max()) and _slot_value(sb) == float(qb.abs().max())
        close(nchw(qa), ref[:, :C1], what='bit masks: destination 1 (no mask)')
        close(nchw(qb), ref[:, C1:] * torch.where(ymc > 0, 1.0, 0.2), what='bit masks: destination 2')
    else:
        for mode in (1, 2):
            ra = torch.empty((B, H, W, C1), device='cuda'); qa = torch.full_like(ra, float('nan')); sa = new()
            ops.conv_h2_bwd_data(gc, sg, dg, sw, ra, mask1=ym, mode1=mode)
            ops.conv_h2_bwd_data(gc, sg, dg, sw, qa, bits1=bits, mode1=mode, amax_dx1=sa)
            assert torch.equal(ra, qa), mode
            assert _slot_value(sa) == float(qa.abs().max())
            close(nchw(qa), ref * torch.where(ymc > 0, 1.0, 0.2 if mode == 1 else 0.0), what=f'bit masks mode {mode}')
    return Cm


@pytest.mark.parametrize('case', WIDE_CASES, ids=IDS)
def test_wide_h2_bwd_data_bit_masks(case):
    """The act' mask as the sign bits a forward h2 layer wrote, read by a 64-column backward-data launch: bit-identical to the float32-mask launch, and
    (hence both) equal to autograd's gradient times the activation's derivative -- the mask taken from the tensor the forward kernel stored."""
    B, H, W, C1, C2, Co = case
    assert _wide(B, H, W, C1 + C2)
    _run_bit_masks(case)


def test_sign_bit_image_written_narrow_read_wide():
    """conv9_1 at the benchmark: the skip tensor's bits come from a 32-column forward (N = 32), the two-destination backward-data launch that reads them
    writes N = 64 on 64-column tiles.  The image layout does not depend on either width."""
    case = (3, 128, 256, 32, 32, 64)
    B, H, W, C1, C2, Co = case
    assert not _wide(B, H, W, C2) and _wide(B, H, W, C1 + C2)
    assert _run_bit_masks(case) == 32


def test_sign_bit_image_written_wide_read_narrow():
    """One crop: the pooled forward keeps 64 columns on any grid, the backward-data launch that reads its bits runs on 32-column tiles below the threshold."""
    case = (1, 64, 64, 64, 0, 64)
    B, H, W, C1, C2, Co = case
    assert _wide(B, H, W, C1, pool=True) and not _wide(B, H, W, C1)
    assert _run_bit_masks(case, pool=True) == 64
    case = (1, 64, 96, 32, 64, 64)                # ... and as the second destination of a narrow two-destination launch
    B, H, W, C1, C2, Co = case
    assert _wide(B, H, W, C2, pool=True) and not _wide(B, H, W, C1 + C2)
    assert _run_bit_masks(case, pool=True) == 64


# --------------------------------------------------------------------------------------------------------------------- EK_BWDU against float64
@pytest.mark.parametrize('case', UNPOOL_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_wide_h2_unpool_against_float64(case):
    """The skip-gradient launch with MaxPool2d's backward in its epilogue against
        dx_ref = lrelu'(skip) convT_f64(g, w)[columns of the skip half] + lrelu'(skip) unpool(gp, argmax of skip's windows)
    in float64 on the CPU, the mask and the argmax taken from the skip tensor the forward kernel STORED (so no element is excluded: there is no element whose
    mask or argmax the reference could see differently).  A = the kernel's error, B = the error of the same composition on the fp32-MFMA kernels
    (ops.conv_bwd_data with the float32 mask, then ops.maxpool_bwd); A <= 2 B + 1e-8 as relative L2 and as max-element / max |ref| -- the bar of
    test_h2_dgrad_is_as_accurate_as_the_fp32_mfma_kernel.  The same for the launch without the pooled gradient (bit masks alone)."""
    from pnnp_amd import ops
    from test_gpu_unpool import _setup
    B, H, W, Cg, C = case
    assert _wide(B, H, W, C)
    g, sg, dg, sw, skip, codes, bits, gp = _setup(B, H, W, Cg, C)
    w = _rand(Cg, 2 * C, 3, 3, seed=3, scale=0.2)                      # (_setup's weights: seed + 3)
    new = lambda: torch.zeros(1, dtype=torch.int32, device='cuda')
    q = torch.full((B, H, W, C), float('nan'), device='cuda'); qa = new()
    ops.conv_h2_bwd_data_unpool(g, sg, dg, sw, C, 2 * C, q, bits=bits, mode=LRELU, amax_dx=qa, gp=gp, codes=codes)
    p = torch.full((B, H, W, C), float('nan'), device='cuda'); pa = new()
    ops.conv_h2_bwd_data_unpool(g, sg, dg, sw, C, 2 * C, p, bits=bits, mode=LRELU, amax_dx=pa)
    d32 = torch.empty(w.numel(), device='cuda'); ops.pack_conv_weight(w.cuda(), None, d32)
    r_u = torch.empty((B, H, W, C), device='cuda'); r = torch.full((B, H, W, C), float('nan'), device='cuda')
    ops.conv_bwd_data(g, d32, r_u, dx2=r, mask2=skip, mode2=LRELU)
    r_plain = r.clone()
    ops.maxpool_bwd(skip, gp, r, LRELU, 1)
    torch.cuda.synchronize()
    assert _slot_value(qa) == float(q.abs().max()) and _slot_value(pa) == float(p.abs().max())
    # the reference
    sk = skip.cpu()
    slope = torch.where(sk > 0, 1.0, 0.2).double()
    conv = nhwc(F.conv_transpose2d(nchw(g.cpu()).double(), w[:, C:].double(), None, padding=1))
    _, idx = F.max_pool2d(nchw(sk), 2, return_indices=True)
    arg = nhwc(((idx // W) % 2) * 2 + (idx % W) % 2)
    up = torch.zeros(B, H, W, C, dtype=torch.float64)
    for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        up[:, dy::2, dx::2] = torch.where(arg == k, gp.cpu().double(), 0.0)
    for what, got, base, ref in (('+ un-pooled gradient', q, r, slope * (conv + up)), ('bit masks alone', p, r_plain, slope * conv)):
        ea, eb = float((got.cpu().double() - ref).norm() / ref.norm()), float((base.cpu().double() - ref).norm() / ref.norm())
        ma, mb = float((got.cpu().double() - ref).abs().max() / ref.abs().max()), float((base.cpu().double() - ref).abs().max() / ref.abs().max())
        print(f'skip gradient {case} {what} vs float64: rel L2 h2 {ea:.2e} fp32-MFMA {eb:.2e}; max-element / max|ref| h2 {ma:.2e} fp32-MFMA {mb:.2e}')
        assert ea <= 2.0 * eb + 1e-8, (what, ea, eb)
        assert ma <= 2.0 * mb + 1e-8, (what, ma, mb)


# --------------------------------------------------------------------------------------------------------------------- the float64 yardsticks on a wide grid
# tests/test_gpu_h2.py's recipes and bars; only the map (3 x 120 x 250: 192 ragged tiles at N = 64) and, where the narrow test writes 32 channels, N = 64 differ.
YB, YH, YW = 3, 120, 250


def test_wide_h2_is_as_accurate_as_the_fp32_mfma_kernel():
    Ci, Co = 512, 64
    assert _wide(YB, YH, YW, Co)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(YB, Ci, YH, YW, generator=g) * torch.logspace(-4, 4, Ci, base=10.0).reshape(1, Ci, 1, 1).roll(1, 1)
    w = torch.randn(Co, Ci, 3, 3, generator=g) * 0.05
    ref = F.conv2d(x.double(), w.double(), None, padding=1)
    y2, y32 = _both(x, w)
    e2, e32 = float((y2 - ref).norm() / ref.norm()), float((y32 - ref).norm() / ref.norm())
    print(f'wide: relative L2 error vs float64: h2 {e2:.2e}, fp32 MFMA {e32:.2e}')
    assert e2 < 2.0 * e32 + 1e-8 and e2 < 5e-7


def test_wide_h2_dgrad_is_as_accurate_as_the_fp32_mfma_kernel():
    Ci, Co = 64, 512
    assert _wide(YB, YH, YW, Ci)
    gen = torch.Generator().manual_seed(1)
    g = torch.randn(YB, Co, YH, YW, generator=gen) * torch.logspace(-4, 4, Co, base=10.0).reshape(1, Co, 1, 1).roll(3, 1)
    w = torch.randn(Co, Ci, 3, 3, generator=gen) * 0.05
    ref = F.conv_transpose2d(g.double(), w.double(), None, padding=1)
    y2, y32 = _both(g, w, dgrad=True)
    e2, e32 = float((y2 - ref).norm() / ref.norm()), float((y32 - ref).norm() / ref.norm())
    m2, m32 = float((y2 - ref).abs().max() / ref.abs().max()), float((y32 - ref).abs().max() / ref.abs().max())
    print(f'wide: dgrad vs float64: rel L2 h2 {e2:.2e} fp32-MFMA {e32:.2e}; max-element / max|ref| h2 {m2:.2e} fp32-MFMA {m32:.2e}')
    assert e2 < 2.0 * e32 + 1e-8 and e2 < 5e-7
    assert m2 < 2.0 * m32 + 1e-8


def test_wide_h2_max_element_error_under_cancellation():
    Ci, Co = 256, 64
    assert _wide(YB, YH, YW, Co)
    gen = torch.Generator().manual_seed(4)
    xa = torch.randn(YB, Ci // 2, YH, YW, generator=gen)
    xb = xa * (1 + 2.0 ** -12 * torch.randn(YB, Ci // 2, YH, YW, generator=gen))
    x = torch.stack([xa, xb], 2).reshape(YB, Ci, YH, YW)
    wa = torch.randn(Co, Ci // 2, 3, 3, generator=gen) * 0.1
    w = torch.stack([wa, -wa], 2).reshape(Co, Ci, 3, 3)
    ref = F.conv2d(x.double(), w.double(), None, padding=1)
    terms = F.conv2d(x.double().abs(), w.double().abs(), None, padding=1)
    assert float(ref.abs().mean() / terms.mean()) < 1e-3
    y2, y32 = _both(x, w)
    r2, r32 = float(((y2 - ref).abs() / terms).max()), float(((y32 - ref).abs() / terms).max())
    print(f'wide: cancellation: max |err| / sum|terms|: h2 {r2:.2e}, fp32-MFMA {r32:.2e} (2^-24 = {2.0 ** -24:.2e})')
    assert r2 < 2.0 * r32 + 2.0 ** -26 and r2 < 8 * 2.0 ** -24


def test_wide_h2_dynamic_range():
    xs, wsc = 1e-30, 1.0
    Ci, Co = 128, 64
    assert _wide(YB, YH, YW, Co)
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(YB, Ci, YH, YW, generator=gen) * xs
    w = torch.randn(Co, Ci, 3, 3, generator=gen) * 0.05 * wsc
    ref = F.conv2d(x.double(), w.double(), None, padding=1)
    y2, y32 = _both(x, w)
    e2, e32 = float((y2 - ref).norm() / ref.norm()), float((y32 - ref).norm() / ref.norm())
    print(f'wide: scale x {xs:g} w {wsc:g}: rel L2 vs float64 h2 {e2:.2e}, fp32-MFMA {e32:.2e}')
    assert torch.isfinite(y2).all()
    assert e2 < 2.0 * e32 + 1e-8 and e2 < 1e-6


@pytest.mark.parametrize('direction', ['fwd', 'dgrad'])
def test_wide_h2_wide_range_inside_one_tensor(direction):
    """One channel at 1e+6 x the others: outputs whose filters ignore it keep 1e-5 relative, those that see it are at float32 level
    (test_h2_wide_range_inside_one_tensor_degrades_gracefully / _backward_data)."""
    Ca, Cb = 64, 64                                 # channels of the split tensor / channels written, half of them blind to channel 0
    assert _wide(YB, YH, YW, Cb)
    gen = torch.Generator().manual_seed(7 if direction == 'fwd' else 8)
    a = torch.randn(YB, Ca, YH, YW, generator=gen); a[:, 0] *= 1e6
    if direction == 'fwd':
        w = torch.randn(Cb, Ca, 3, 3, generator=gen) * 0.1; w[:32, 0] = 0.0
        ref = F.conv2d(a.double(), w.double(), None, padding=1)
    else:
        w = torch.randn(Ca, Cb, 3, 3, generator=gen) * 0.1; w[0, :32] = 0.0
        ref = F.conv_transpose2d(a.double(), w.double(), None, padding=1)
    y2, _ = _both(a, w, dgrad=direction == 'dgrad')
    e_blind = float((y2[:, :32] - ref[:, :32]).norm() / ref[:, :32].norm())
    e_see = float((y2[:, 32:] - ref[:, 32:]).norm() / ref[:, 32:].norm())
    print(f'wide: {direction}, one channel 1e6 x the others: rel L2 of outputs that ignore it {e_blind:.2e}, that see it {e_see:.2e}')
    assert torch.isfinite(y2).all() and e_blind < 1e-5 and e_see < 5e-7


@pytest.mark.parametrize('direction', ['fwd', 'dgrad'])
def test_wide_h2_single_outlier_bounds_the_damage(direction):
    """ONE element at 1e+8 x the rest of its tensor: everything it does not touch within 2^-40 x 1e8, the pixels it reaches at float32 level."""
    Ca, Cb = 64, 64
    assert _wide(YB, YH, YW, Cb)
    gen = torch.Generator().manual_seed(10)
    bound = 2.0 ** -40 * 1e8
    a = torch.randn(YB, Ca, YH, YW, generator=gen); a[0, 3, 8, 16] = 1e8
    w = torch.randn(Cb, Ca, 3, 3, generator=gen) * 0.1 if direction == 'fwd' else torch.randn(Ca, Cb, 3, 3, generator=gen) * 0.1
    ref = F.conv2d(a.double(), w.double(), None, padding=1) if direction == 'fwd' else F.conv_transpose2d(a.double(), w.double(), None, padding=1)
    y2, y32 = _both(a, w, dgrad=direction == 'dgrad')
    near = torch.zeros(YB, YH, YW, dtype=torch.bool); near[0, 7:10, 15:18] = True          # the 3 x 3 pixels the outlier reaches
    far = ~near
    sel = lambda t, m: t.permute(0, 2, 3, 1)[m]
    e_far = float((sel(y2, far) - sel(ref, far)).norm() / sel(ref, far).norm())
    e32_far = float((sel(y32, far) - sel(ref, far)).norm() / sel(ref, far).norm())
    e_near = float((sel(y2, near) - sel(ref, near)).norm() / sel(ref, near).norm())
    print(f'wide: {direction}, one element 1e8: rel L2 away from it {e_far:.2e} (fp32-MFMA {e32_far:.2e}; bound {bound:.1e}), at the pixels it reaches {e_near:.2e}')
    assert torch.isfinite(y2).all() and e_far < bound and e_near < 5e-7


# --------------------------------------------------------------------------------------------------------------------- split-K
def test_wide_h2_splitk():
    """K cut into slices on a grid whose slices x tiles clear the threshold: the partial-sum launch (no epilogue work) runs on 64-column tiles.  160 channels =
    10 chunks of K, 80 tiles of 32 columns: 2 slices do not fill the chip, the next divisor (5) gives 40 x 5 = 200 tiles of 64 columns."""
    from pnnp_amd import ops
    case = (1, 80, 256, 160, 0, 64)
    B, H, W, C1, C2, Co = case
    chunks = (C1 + 15) // 16
    ks = ops.h2_splitk(B, H, W, chunks, Co)
    assert ks > 1 and chunks % ks == 0, (ks, chunks)
    assert _wide(B * ks, H, W, Co) and not _wide(B, H, W, Co)
    x1 = _rand(B, C1, H, W, seed=1)
    w = _rand(Co, C1, 3, 3, seed=3, scale=0.05); bias = _rand(Co, seed=4)
    ref = F.leaky_relu(F.conv2d(x1, w, bias, padding=1), 0.2)
    x1c = nhwc(x1).cuda()
    f, _, sw = _packs(w.cuda(), dgrad=False)
    s1 = _slot(x1c)
    y0 = torch.empty(B, H, W, Co, device='cuda')
    ops.conv_h2_fwd(x1c, None, f, sw, bias.cuda(), y0, Co, 1, s1)
    y = torch.full((B, H, W, Co), float('nan'), device='cuda'); am = torch.zeros(1, dtype=torch.int32, device='cuda')
    bits = torch.full((ops.h2_bits_words(B, H, W, Co),), -1, dtype=torch.int32, device='cuda')
    ws = torch.full((ks * y.numel(),), float('nan'), device='cuda')
    ops.conv_h2_fwd_splitk(x1c, None, f, sw, bias.cuda(), y, Co, 1, s1, ks, ws, amax_y=am, bits_y=bits)
    close(nchw(y), ref, what=f'split-K x {ks} {case}')
    d = float((y - y0).abs().max() / y0.abs().max())
    print(f'wide: split-K x {ks} {case}: max |diff| / max |y| vs the unsplit launch {d:.2e}')
    assert d < 4e-6
    assert _slot_value(am) == float(y.abs().max())
    assert np.array_equal(_decode_bits(bits, B, H, W, Co), (y > 0).cpu().numpy())


# --------------------------------------------------------------------------------------------------------------------- the bf16x3 family (the range tripwire's fallback)
# conv_x3s.hip asks the same width rule (pnnp_conv3_tile_columns, csrc/igemm.h), so ops.h2_tile_columns answers for these launches too.
@pytest.mark.parametrize('case', WIDE_CASES, ids=IDS)
def test_wide_x3_fwd(case):
    from pnnp_amd import ops
    B, H, W, C1, C2, Co = case
    assert _wide(B, H, W, Co)
    x1, x2, w, b, pre = _fwd_data(case)
    f, _ = _packs_x3(w.cuda(), dgrad=False)
    x1c = nhwc(x1).cuda(); x2c = nhwc(x2).cuda() if C2 else None
    for act in (0, 1, 2):
        y = torch.full((B, H, W, Co), float('nan'), device='cuda')
        ops.conv_x3_fwd(x1c, x2c, f, b.cuda(), y, Co, act)
        close(nchw(y), _act(pre, act), what=f'x3 fwd {case} act{act}')
    r = _rand(B, Co, H, W, seed=9)
    y = torch.full((B, H, W, Co), float('nan'), device='cuda')
    ops.conv_x3_fwd(x1c, x2c, f, b.cuda(), y, Co, 2, residual=nhwc(r).cuda())
    close(nchw(y), F.relu(pre + r), what='x3 residual')


@pytest.mark.parametrize('case', WIDE_CASES, ids=IDS)
def test_wide_x3_fwd_pool(case):
    from pnnp_amd import ops
    B, H, W, C1, C2, Co = case
    assert _wide(B, H, W, Co, pool=True)
    x1, x2, w, b, pre = _fwd_data(case)
    f, _ = _packs_x3(w.cuda(), dgrad=False)
    y = torch.full((B, H, W, Co), float('nan'), device='cuda'); pooled = torch.full((B, H // 2, W // 2, Co), float('nan'), device='cuda')
    codes = torch.full((B, H // 2, W // 2, Co), 255, dtype=torch.uint8, device='cuda')
    ops.conv_x3_fwd_pool(nhwc(x1).cuda(), nhwc(x2).cuda() if C2 else None, f, b.cuda(), y, pooled, codes, Co, LRELU)
    close(nchw(y), _act(pre, 1), what=f'x3 fwd+pool {case}')
    p_ref, c_ref, tied = _pool_reference(y.cpu())
    assert tied > 0
    assert torch.equal(pooled.cpu(), p_ref), 'pooled map'
    assert torch.equal(codes.cpu(), c_ref), 'argmax / sign codes'


@pytest.mark.parametrize('case', WIDE_CASES, ids=IDS)
def test_wide_x3_bwd_data(case):
    from pnnp_amd import ops
    B, H, W, C1, C2, Co = case
    assert _wide(B, H, W, C1 + C2)
    w, g, ref = _bwd_data(case)
    _, dg = _packs_x3(w.cuda(), fwd=False)
    gc = nhwc(g).cuda()
    nan = lambda c: torch.full((B, H, W, c), float('nan'), device='cuda')
    m1 = _rand(B, C1, H, W, seed=7); m2 = _rand(B, max(C2, 1), H, W, seed=8)
    m1c = nhwc(m1).cuda(); m2c = nhwc(m2).cuda() if C2 else None
    d1 = nan(C1); d2 = nan(C2) if C2 else None
    ops.conv_x3_bwd_data(gc, dg, d1, dx2=d2)
    close(nchw(d1), ref[:, :C1], what=f'x3 dgrad {case}')
    if C2:
        close(nchw(d2), ref[:, C1:], what=f'x3 dgrad2 {case}')
    d1 = nan(C1); d2 = nan(C2) if C2 else None
    ops.conv_x3_bwd_data(gc, dg, d1, mask1=m1c, mode1=1, dx2=d2, mask2=m2c, mode2=2 if C2 else 0)
    close(nchw(d1), ref[:, :C1] * torch.where(m1 > 0, 1.0, 0.2), what='x3 mask1')
    if C2:
        close(nchw(d2), ref[:, C1:] * (m2 > 0).float(), what='x3 mask2')
        d1 = nan(C1); d2 = nan(C2)
        ops.conv_x3_bwd_data(gc, dg, d1, dx2=d2, mask2=m2c, mode2=1)                 # the decoder's launch: a mask on the second destination only
        close(nchw(d1), ref[:, :C1], what='x3 dst1 (no mask)')
        close(nchw(d2), ref[:, C1:] * torch.where(m2 > 0, 1.0, 0.2), what='x3 dst2 (LeakyReLU mask)')
    base = _rand(B, C2 or C1, H, W, seed=10)
    acc = nhwc(base).cuda().clone()
    if C2:
        ops.conv_x3_bwd_data(gc, dg, nan(C1), mask1=m1c, mode1=1, dx2=acc, mask2=m2c, mode2=2, accum2=1)
        close(nchw(acc), base + ref[:, C1:] * (m2 > 0).float(), what='x3 mask2+accum')
    else:
        ops.conv_x3_bwd_data(gc, dg, acc, mask1=m1c, mode1=2, accum1=1)
        close(nchw(acc), base + ref * (m1 > 0).float(), what='x3 mask1+accum')
        add = _rand(B, C1, H, W, seed=11)
        for mode in (0, 2):
            dx = nan(C1)
            ops.conv_x3_bwd_data_res(gc, dg, dx, addsrc=nhwc(add).cuda(), mask=m1c if mode else None, mode=mode)
            close(nchw(dx), (ref + add) * ((m1 > 0).float() if mode else 1.0), what=f'x3 dgrad res mode {mode}')


def test_wide_x3_is_as_accurate_as_the_fp32_mfma_kernel():
    """test_x3_is_as_accurate_as_the_fp32_mfma_kernel (K = 9 x 512, operands spanning 8 decades) on 192 ragged 64-column tiles."""
    from pnnp_amd import ops
    Ci, Co = 512, 64
    assert _wide(YB, YH, YW, Co)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(YB, Ci, YH, YW, generator=g) * torch.logspace(-4, 4, Ci, base=10.0).reshape(1, Ci, 1, 1).roll(1, 1)
    w = torch.randn(Co, Ci, 3, 3, generator=g) * 0.05
    ref = F.conv2d(x.double(), w.double(), None, padding=1)
    f3, _ = _packs_x3(w.cuda(), dgrad=False)
    f32 = torch.empty(w.numel(), device='cuda'); ops.pack_conv_weight(w.cuda(), f32, None)
    xc = nhwc(x).cuda()
    y3 = torch.empty((YB, YH, YW, Co), device='cuda'); y32 = torch.empty_like(y3)
    ops.conv_x3_fwd(xc, None, f3, None, y3, Co, 0)
    ops.conv_fwd(xc, None, f32, None, y32, Co, 9, 0)
    e3 = float((nchw(y3).cpu().double() - ref).norm() / ref.norm())
    e32 = float((nchw(y32).cpu().double() - ref).norm() / ref.norm())
    print(f'wide: relative L2 error vs float64: bf16x3 {e3:.2e}, fp32 MFMA {e32:.2e}')
    assert e3 < 2.0 * e32 + 1e-8 and e3 < 5e-7

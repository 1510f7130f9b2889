"""MaxPool2d backward folded into the epilogue of the decoder's skip-gradient launch (csrc/conv_h2s.hip EK_BWDU, ops.conv_h2_bwd_data_unpool)
against the composition it replaces: the two-destination backward-data launch + the max-pool backward pass with codes.  Both paths do the same
float32 operations in the same order, so every comparison is bit-exact (torch.equal), the amax slots included."""
import pytest
import torch

from test_gpu_conv import _rand, nhwc
from test_gpu_h2 import _packs, _slot

pytestmark = pytest.mark.gpu
LRELU = 1

# (B, H, W, channels of g, channels of each half, tile columns the single-destination launches must resolve to)
CASES = [(2, 64, 64, 32, 32, 32),          # 32 -> 32 + 32: the shape of conv9_1
         (2, 48, 80, 32, 32, 32),          # a map that does not fill its 16 x 32 pixel tiles
         (2, 48, 80, 64, 64, 32),          # ... with two 32-column tiles per pixel tile
         (2, 128, 384, 64, 64, 64),        # 64 -> 64 + 64 on 64-column tiles
         (2, 96, 256, 128, 128, 64)]       # 128 -> 128 + 128 on 64-column tiles


def _setup(B, H, W, Cg, C, seed=0):
    """g, the backward-data pack of Conv2d(2 C -> Cg), and a skip tensor with its pooled map's codes and its sign bits, written by the pooled
    forward kernel as in a training forward; the pooled map's gradient with exact zeros and negative zeros among the selected elements."""
    from pnnp_amd import ops
    w = _rand(Cg, 2 * C, 3, 3, seed=seed + 3, scale=0.2)
    _, dg, sw = _packs(w.cuda(), fwd=False)
    g = nhwc(_rand(B, Cg, H, W, seed=seed + 5)).cuda()
    wm = _rand(C, 32, 3, 3, seed=seed + 12, scale=0.2).cuda(); bm = _rand(C, seed=seed + 13).cuda()
    fm, _, swm = _packs(wm, dgrad=False)
    xm = nhwc(_rand(B, 32, H, W, seed=seed + 14)).cuda()
    skip = torch.empty((B, H, W, C), device='cuda')
    pooled = torch.empty((B, H // 2, W // 2, C), device='cuda')
    codes = torch.empty((B, H // 2, W // 2, C), dtype=torch.uint8, device='cuda')
    bits = torch.zeros(ops.h2_bits_words(B, H, W, C), dtype=torch.int32, device='cuda')
    ops.conv_h2_fwd_pool(xm, None, fm, swm, bm, skip, pooled, codes, C, LRELU, _slot(xm), bits_y=bits)
    assert 0.2 < float((skip > 0).float().mean()) < 0.8
    gp = nhwc(_rand(B, C, H // 2, W // 2, seed=seed + 21)).cuda()
    r = torch.rand(gp.shape, generator=torch.Generator().manual_seed(seed + 22)).cuda()
    gp[r < 0.1] = 0.0                       # the code selects an element whose pooled gradient is exactly zero ...
    gp[(r >= 0.1) & (r < 0.2)] = -0.0       # ... or a negative zero
    return g, _slot(g), dg, sw, skip, codes, bits, gp


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_unpool_equals_two_destination_launch_plus_pool_pass(case):
    from pnnp_amd import ops
    B, H, W, Cg, C, bn = case
    assert ops.h2_tile_columns(B, H, W, C) == bn
    g, sg, dg, sw, skip, codes, bits, gp = _setup(B, H, W, Cg, C)
    new = lambda: torch.zeros(1, dtype=torch.int32, device='cuda')
    # what it replaces: g_u and the masked skip gradient in one launch, then the pass adds the un-pooled gradient in place
    r_u = torch.full((B, H, W, C), float('nan'), device='cuda'); r_s = torch.full((B, H, W, C), float('nan'), device='cuda')
    ra_u, ra_d2, ra_pool = new(), new(), new()
    ops.conv_h2_bwd_data(g, sg, dg, sw, r_u, amax_dx1=ra_u, dx2=r_s, bits2=bits, mode2=LRELU, amax_dx2=ra_d2)
    ops.maxpool_bwd(skip, gp, r_s, LRELU, 1, codes=codes, amax_gx=ra_pool)
    # the split: columns [0, C) early, columns [C, 2 C) with the pool's backward in the epilogue
    q_u = torch.full((B, H, W, C), float('nan'), device='cuda'); q_s = torch.full((B, H, W, C), float('nan'), device='cuda')
    qa_u, qa_pool = new(), new()
    ops.conv_h2_bwd_data_unpool(g, sg, dg, sw, 0, 2 * C, q_u, amax_dx=qa_u)
    ops.conv_h2_bwd_data_unpool(g, sg, dg, sw, C, 2 * C, q_s, bits=bits, mode=LRELU, amax_dx=qa_pool, gp=gp, codes=codes)
    torch.cuda.synchronize()
    assert not torch.isnan(q_u).any() and not torch.isnan(q_s).any()
    assert torch.equal(r_u, q_u), 'g_u'
    assert torch.equal(r_s, q_s), 'skip gradient + un-pooled gradient'
    # bit patterns as well: the sign of a zero is part of "the same operations in the same order"
    assert torch.equal(r_s.view(torch.int32), q_s.view(torch.int32)), 'skip gradient, bit patterns'
    assert int(ra_u) == int(qa_u), 'amax slot of g_u'
    assert int(ra_pool) == int(qa_pool), 'amax slot of the summed gradient'
    assert float(qa_pool.view(torch.float32)) == float(q_s.abs().max()), 'the slot holds max |stored value|'
    # the plain column range alone (no pool) is the two-destination launch's second destination
    p_s = torch.full((B, H, W, C), float('nan'), device='cuda')
    r2_u = torch.empty_like(r_u); r2_s = torch.empty_like(r_s)
    ops.conv_h2_bwd_data(g, sg, dg, sw, r2_u, dx2=r2_s, bits2=bits, mode2=LRELU)
    ops.conv_h2_bwd_data_unpool(g, sg, dg, sw, C, 2 * C, p_s, bits=bits, mode=LRELU)
    assert torch.equal(r2_s, p_s)


def test_unpool_engine_step_is_bit_identical():
    """UNet nf = 32, B = 2, 128 x 128: one training step with the switch off and on from the same seed."""
    from pnnp_amd.archs import UNetSeeInDark, initialize_weights
    from pnnp_amd.trainer import HipTrainStep
    gen = torch.Generator().manual_seed(5)
    x = torch.rand(2, 4, 128, 128, generator=gen).cuda(); t = torch.rand(2, 4, 128, 128, generator=gen).cuda()
    out = {}
    for on in (False, True):
        torch.manual_seed(1997)
        net = UNetSeeInDark(dict(nframes=1, res=False, nf=32, in_nc=4, out_nc=4))
        initialize_weights(net)
        net = net.cuda()
        net.engine.set_policy(unpool_fused=on)
        ts = HipTrainStep(net, lr=1e-4, clip=0)
        loss = ts.step(t, noisy=x)
        torch.cuda.synchronize()
        plan = net.engine._plan
        assert [plan[f'conv{i}_1'].unpool for i in range(6, 10)] == [on] * 4
        out[on] = (loss.clone(), net.engine.params.grad.clone(), net.engine.params.flat.clone())
    assert torch.isfinite(out[True][1]).all() and float(out[True][1].abs().max()) > 0
    assert torch.equal(out[False][0], out[True][0]), 'loss vector'
    assert torch.equal(out[False][1], out[True][1]), 'flat gradient buffer'
    assert torch.equal(out[False][2], out[True][2]), 'parameters after the Adam step'


def test_unpool_single_level_switch():
    """set_policy(unpool_levels=...) keeps the other levels on the stand-alone pass."""
    from pnnp_amd.archs import UNetSeeInDark
    net = UNetSeeInDark(dict(nframes=1, res=False, nf=32, in_nc=4, out_nc=4))
    net.engine.set_policy(unpool_levels=(2, 4))
    plan = net.engine._plan_for(2, 128, 128, True)
    assert [plan[f'conv{i}_1'].unpool for i in range(6, 10)] == [True, False, True, False]       # conv6_1: level 4 ... conv9_1: level 1


@pytest.mark.parametrize('what', ['odd height', 'odd width', 'no bits', 'accumulate', 'column offset', 'columns past the pack'])
def test_unpool_refusals_launch_nothing(what):
    from pnnp_amd import ops
    from pnnp_amd._lib import PnnpError
    B, H, W, Cg, C = 1, 32, 32, 32, 32
    g, sg, dg, sw, skip, codes, bits, gp = _setup(B, H, W, Cg, C)
    dx = torch.full((B, H, W, C), float('nan'), device='cuda')
    kw = dict(bits=bits, mode=LRELU, gp=gp, codes=codes)
    col0, code = C, -2
    if what == 'odd height':
        g, dx = g[:, :31].contiguous(), dx[:, :31].contiguous()
    elif what == 'odd width':
        g, dx = g[:, :, :31].contiguous(), dx[:, :, :31].contiguous()
    elif what == 'no bits':
        kw['bits'] = None
    elif what == 'accumulate':
        kw['accum'] = 1
    elif what == 'column offset':
        col0, code = 16, -1
    else:
        col0, code = 2 * C, -1
    with pytest.raises(PnnpError, match=f'code {code} '):
        ops.conv_h2_bwd_data_unpool(g, _slot(g), dg, sw, col0, 2 * C, dx, **kw)
    torch.cuda.synchronize()
    assert torch.isnan(dx).all(), 'nothing was launched'

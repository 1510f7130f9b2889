"""GPU checks of fp16 activation storage for ResUnet (precision='fp16_act_res': ConvPolicy.h1_act16_res, Plan.act16) at the level of the network.  As in
tests/test_gpu_act16_net.py the yardstick runs no new code: the layer-by-layer composition of the EXISTING float32-storage ops (ops.conv_h1_fwd with its
residual, ops.conv_s2_h1_fwd, ops.conv1x1_h1_fwd, ops.convt_h1_fwd, ops.first_fwd, ops.head_fwd; the engine's own packs and plan) with ``.half().float()``
after every stored map -- to which the engine's output must be BIT-equal -- and tests/_act16_resunet_ref.py in float64 for the accuracy bar.  The weights'
scale comes from tests/test_host_act16_res.py, where it is chosen on the CPU so that all 31 maps stay inside fp16."""
import pytest
import torch

from _act16_resunet_ref import STORED, act16_resunet_forward, identity
from test_gpu_h1 import _net, _rel, _slot
from test_host_act16_res import ALL4, NET_SHAPES, WSCALE

pytestmark = pytest.mark.gpu
RELU = 2


def _input(shape, seed=11):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed)).cuda()


def _compose(net, x):
    """ResUnet on the float32-storage ops with every stored map rounded to fp16 and back; plan and packs: the engine's, of its last forward (on x's shape)"""
    from pnnp_amd import ops
    e = net.engine
    plan, wp, P = e._plan, e._wp, dict(net.named_parameters())
    B, _, H, W = x.shape
    ch = e.ch
    r = lambda t: t.half().float()
    new = lambda h, w, c: torch.empty(B, h, w, c, device='cuda')
    x8 = torch.empty(B, H, W, e.cin_pad, device='cuda')
    ops.nchw_to_nhwc(x, x8, e.cin_pad)

    def c3(name, x1, x2, h, w, cout, act, bias=None, residual=None):
        assert plan[name].fwd == 'h1' and plan[name].ks == 1
        f, _, ws = wp[name]
        return r(ops.conv_h1_fwd(x1, x2, f, ws, bias, new(h, w, cout), cout, act, _slot(x1), _slot(x2) if x2 is not None else None, residual=residual))
    if plan['conv_in'].fwd == 'thin':
        xin = r(ops.first_fwd(x8, P['conv_in.weight'], P['conv_in.bias'], new(H, W, ch[0]), RELU))
    else:
        xin = c3('conv_in', x8, None, H, W, ch[0], RELU, bias=P['conv_in.bias'])
    skips = []
    for l in range(1, 6):
        h, w, c = H >> (l - 1), W >> (l - 1), ch[l - 1]
        t = c3(f'b{l}_0', xin, None, h, w, c, RELU)
        cur = c3(f'b{l}_1', t, None, h, w, c, 0, residual=xin)
        if l < 5:
            skips.append(cur)
            f, _, ws = wp[f'pool{l}']
            xin = r(ops.conv_s2_h1_fwd(cur, _slot(cur), f, ws, P[f'pool{l}.conv.bias'], new(h // 2, w // 2, ch[l]), ch[l], 0))
    for i in range(6, 10):
        lv = 9 - i
        h, w, c = H >> lv, W >> lv, ch[lv]
        f, _, ws = wp[f'upv{i}']
        u = r(ops.convt_h1_fwd(cur, _slot(cur), f, ws, P[f'upv{i}.bias'], new(h, w, c), c))
        skip = skips[lv]
        t = c3(f'b{i}_0', u, skip, h, w, c, RELU)
        f, _, ws = wp[f'sc{i}']
        sc = r(ops.conv1x1_h1_fwd(u, _slot(u), skip, _slot(skip), f, ws, None, new(h, w, c), c, 0))
        cur = c3(f'b{i}_1', t, None, h, w, c, 0, residual=sc)
    assert plan['conv10'].fwd == 'thin'
    out = torch.empty(B, 4, H, W, device='cuda')
    ops.head_fwd(cur, P['conv10.weight'], P['conv10.bias'], out, residual=x if net.res else None)
    return out


def _on(e, on):
    e.set_policy(h1_eval=on, h1_pointwise=on, h1_act16=on, h1_act16_res=on)


def _switches(e):
    return [bool(getattr(e.policy, k)) for k in ALL4]


@pytest.mark.parametrize('res', [False, True])
@pytest.mark.parametrize('shape', NET_SHAPES)
def test_act16_res_network_equals_the_composition_and_meets_the_float64_bar(shape, res):
    net, sd = _net('resunet', WSCALE, res=res)
    e = net.engine
    x = _input(shape)
    with torch.no_grad():
        _on(e, True)
        y = net(x).clone()
        plan = e._plan
        assert plan.act16 and not plan.train
        bufs = e.bufs[(shape[0], shape[2], shape[3], x.device)].t
        assert sorted(k[:-8] for k in bufs if k.endswith(':float16')) == sorted(STORED) and bufs['x8'].dtype == torch.float32
        comp = _compose(net, x)
        assert torch.isfinite(y).all() and torch.equal(y, comp)
        rng = e.act16_range()
        assert len(rng) == 31 and not any(r['overflow'] or r['inherited'] for r in rng) and all(0 < r['amax'] < 65504 for r in rng)
        e.set_policy(h1_act16_res=False)                            # three switches: the fp16_all plan, float32 storage
        y_all = net(x).clone()
        p_all = e._plan
        assert not p_all.act16 and p_all.table() == plan.table() and p_all.packs == plan.packs
        assert [s.ks for s in p_all.steps.values()] == [s.ks for s in plan.steps.values()]
        assert not torch.equal(y_all, y)                            # (the stores do round)
        e.set_policy(h1_act16=False)
        assert torch.equal(net(x), y_all)                           # 'fp16_all' itself
        _on(e, False)
        y_off = net(x).clone()
    # against float64: 2 x the emulation's own error + the eval-forward bar; `exact` is the fp16_all emulation (unrounded stores) of the plan that ran
    sd64 = {k: v.double().cuda() for k, v in sd.items()}
    h1_first = plan['conv_in'].fwd == 'h1'
    exact = act16_resunet_forward(sd64, x, res=res, store=identity, h1_first=h1_first)
    emu = act16_resunet_forward(sd64, x, res=res, h1_first=h1_first)
    e_emu, e_act, e_all = _rel(emu, exact), _rel(y.double(), exact), _rel(y_all.double(), exact)
    bar = float((2e-6 + 1e-4 * exact.abs()).norm() / exact.norm())
    print(f'resunet {shape} res {res} weights x {WSCALE}: relative L2 vs the unrounded-store float64 emulation: fp16_act_res {e_act:.3e}, its emulation {e_emu:.3e}, '
          f'fp16_all {e_all:.3e}; bar term {bar:.2e}')
    assert e_act <= 2.0 * e_emu + bar
    assert e_emu > 1e-5                                             # (the emulation does round: the comparison is not vacuous)
    fresh, _ = _net('resunet', WSCALE, res=res)                     # the switches off again: bit-equal to a fresh engine
    with torch.no_grad():
        assert torch.equal(fresh(x), y_off)


@pytest.mark.parametrize('tile_batch', [None, 1])
def test_act16_res_forward_tiled_equals_the_composition_per_tile(tile_batch):
    from pnnp_amd import tiles
    from pnnp_amd.evaluate import forward_tiled
    net, _ = _net('resunet', WSCALE, res=True)
    e = net.engine
    Hh, Ww, P, BASE = 100, 132, 64, 16
    x = _input((1, 4, Hh, Ww), seed=3)
    got = forward_tiled(net, x, P, base=BASE, tile_batch=tile_batch, precision='fp16_act_res')
    assert e._plan.act16
    assert _switches(e) == [False] * 4 and not any(k in e._h2_sub for k in ALL4)      # all four restored
    crops = tiles.eval_crop(x, P, BASE)
    with torch.no_grad():
        _on(e, True)
        outs = []
        for c in ([crops] if tile_batch is None else crops.split(tile_batch)):
            c = c.contiguous()
            net(c)                                                  # (the plan of this batch size)
            assert e._plan.act16
            outs.append(_compose(net, c))
        _on(e, False)
    want = tiles.eval_merge(torch.cat(outs), Hh, Ww, BASE)
    assert torch.equal(got, want)


def test_act16_res_leaves_everything_else_where_it_was():
    from pnnp_amd._lib import PnnpError
    from pnnp_amd.evaluate import evaluate, forward_tiled
    from pnnp_amd.trainer import HipTrainStep
    x = _input((1, 4, 64, 64))
    # ResUnet: 'fp16_act' is still 'fp16_all', bit for bit; the new name is not
    rnet, _ = _net('resunet', WSCALE)
    a = forward_tiled(rnet, x, 64, base=16, precision='fp16_all')
    b = forward_tiled(rnet, x, 64, base=16, precision='fp16_act')
    assert torch.equal(a, b) and not rnet.engine._plan.act16
    c = forward_tiled(rnet, x, 64, base=16, precision='fp16_act_res')
    assert rnet.engine._plan.act16 and not torch.equal(c, a) and _rel(c, a) < 1e-2
    # UNet: 'fp16_act_res' is 'fp16_act', bit for bit (the fourth switch touches only resolve_resunet)
    unet, _ = _net('unet', 3.0, res=True)
    ua = forward_tiled(unet, x, 64, base=16, precision='fp16_act')
    pa = unet.engine._plan
    ub = forward_tiled(unet, x, 64, base=16, precision='fp16_act_res')
    assert pa.act16 and unet.engine._plan.act16 and unet.engine._plan.table() == pa.table() and torch.equal(ua, ub)
    # a training step with all four switches on: bit-identical to one with them off
    xt = _input((2, 4, 64, 64)); t = _input((2, 4, 64, 64), seed=2)

    def run(on):
        net, _ = _net('resunet', WSCALE)
        net.train()
        ts = HipTrainStep(net, lr=1e-4, clip=0)
        if on:
            _on(net.engine, True)
            with torch.no_grad():
                net.eval(); net(xt); net.train()                    # an eval forward with fp16 storage on the training shape first, then the steps WITH the switches on
            assert net.engine._plan.act16
        losses = [ts.step(t, noisy=xt)[0].clone() for _ in range(2)]
        return torch.stack(losses), [p.detach().clone() for p in net.parameters()], net.engine._plan.table(), net.engine._plan.act16
    l0, p0, t0, a0 = run(False)
    l1, p1, t1, a1 = run(True)
    assert t1 == t0 and not a0 and not a1
    assert torch.equal(l1, l0) and all(torch.equal(u, v) for u, v in zip(p1, p0))
    # the switches come back when the call raises; an unknown precision still raises
    hr = _input((1, 4, 64, 64), seed=5) * 0.5
    with pytest.raises(PnnpError):
        evaluate(rnet, hr[0], hr, precision='fp16_act_res')          # not [1,C,H,W]: raises inside the call
    assert _switches(rnet.engine) == [False] * 4
    lr = (hr + 0.02 * _input((1, 4, 64, 64), seed=6) - 0.01).clamp(0, 1)
    m = evaluate(rnet, lr, hr, precision='fp16_act_res')['metrics']
    assert torch.isfinite(m).all() and rnet.engine._plan.act16 and _switches(rnet.engine) == [False] * 4
    with pytest.raises(PnnpError):
        evaluate(rnet, hr, hr, precision='fp16_act_everything')


@pytest.mark.parametrize('precision', [None, 'fp32', 'fp16', 'fp16_all'])
def test_act16_res_leaves_the_other_precisions_bit_identical(precision):
    """An engine that has served 'fp16_act_res' (its plans, fp16 buffers and overrides came and went) gives under every other precision exactly what an engine
    that never saw the switch gives with the policy set by hand."""
    from pnnp_amd.evaluate import _PRECISION, forward_tiled
    x = _input((1, 4, 100, 132), seed=3)
    used, _ = _net('resunet', WSCALE, res=True)
    forward_tiled(used, x, 64, base=16, precision='fp16_act_res')
    assert used.engine._plan.act16
    got = forward_tiled(used, x, 64, base=16, precision=precision)
    assert not used.engine._plan.act16 and not any(k in used.engine._h2_sub for k in ('h1_act16', 'h1_act16_res'))
    fresh, _ = _net('resunet', WSCALE, res=True)
    if precision is not None:
        fresh.engine.set_policy(**_PRECISION[precision])
    want = forward_tiled(fresh, x, 64, base=16)
    assert torch.equal(got, want)
    # ... and the switch left ON beside the others is inert unless all four are on
    fresh.engine.set_policy(h1_act16_res=True)
    again = forward_tiled(fresh, x, 64, base=16)
    assert not fresh.engine._plan.act16 and torch.equal(again, want)


def test_act16_res_runs_a_frame_past_the_float32_bound():
    """6144 x 4096 at nf = 32: (H + 4) W 32 channels x 4 bytes is past 2^31, x 2 bytes is not.  Refused with three switches (ResUnet then has float32 maps),
    whole with four.  The frame repeats a 1024 x 1024 pattern -- a multiple of every tile and of the four 2x grids -- so blocks one period apart and 256 px from
    the borders see the same halo at the same place in their tiles: their outputs are bit-equal unless an address is wrong -- the residual read and the stride-2
    taps are new 2-byte address arithmetic.  The last block lies past the 2^31-byte offset of a float32 map.

    ResUnet's receptive field, one-sided, in full-resolution pixels: the 3x3 taps add 1 (conv_in) + 2 (block 1) + 1 (pool1) + 4 + 2 + 8 + 4 + 16 + 8 (blocks 2-4 and
    their stride-2 layers, each at its level's pixel size) + 32 (block 5, 16-px pixels) + 16 + 8 + 4 + 2 (blocks 6-9) = 108; the 1x1 shortcuts, the head and the
    ConvTranspose2d taps add none, the alignment of the four 2x grids at most 1 + 2 + 4 + 8 = 15: at most 123 px, below the 256 the blocks keep from the border."""
    from pnnp_amd import ops
    from pnnp_amd._lib import PnnpError
    H, W, T = 6144, 4096, 1024
    assert 108 + 15 < 256
    assert not ops.image_fits(H, W, 32, 4) and ops.image_fits(H, W, 32, 2) and (H - T + 256) * W * 32 * 4 >= 2 ** 31
    net, _ = _net('resunet', WSCALE)
    e = net.engine
    x = torch.rand(1, 4, T, T, device='cuda', generator=torch.Generator(device='cuda').manual_seed(4)).repeat(1, 1, H // T, W // T)
    with torch.no_grad():
        with pytest.raises(PnnpError):
            net(x)                                                  # the default path: float32 maps
        e.set_policy(h1_eval=True, h1_pointwise=True, h1_act16=True)
        with pytest.raises(PnnpError, match='h1_act16_res'):
            net(x)                                                  # three switches: ResUnet's fp16_all plan, float32 maps; the refusal names the fourth
        _on(e, True)
        y = net(x)
        assert e._plan.act16 and tuple(y.shape) == (1, 4, H, W)
    assert torch.isfinite(y).all()
    near = y[:, :, 256:768, 256:768]
    far = y[:, :, H - T + 256:H - T + 768, W - T + 256:W - T + 768]
    assert float(near.abs().max()) > 0 and torch.equal(far, near)
    mid = y[:, :, 2 * T + 256:2 * T + 768, T + 256:T + 768]
    assert torch.equal(mid, near)
    rng = e.act16_range()
    assert len(rng) == 31 and not any(r['overflow'] or r['inherited'] for r in rng)
    net.train()
    try:
        with pytest.raises(PnnpError):
            net(x)                                                  # a training forward has no fp16 storage: refused before anything is launched
    finally:
        net.eval(); _on(e, False)

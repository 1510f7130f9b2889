"""GPU checks of the fp16-STORAGE eval forward (precision='fp16_act': ConvPolicy.h1_act16, Plan.act16) at the level of the network.  The yardstick runs no
new code: the layer-by-layer composition of the EXISTING float32-storage h1 ops (ops.conv_h1_fwd & co., the engine's own packs and the plan's own
variants and K slices) with ``.half().float()`` between the layers -- to which the engine's output must be BIT-equal (an fp16 source is exact, an fp16
store is one rounding: tests/test_gpu_act16.py) -- and tests/_act16_ref.py in float64 for the accuracy bar.  Weights are init_state x 3: x 6, the other
fp16 tests' scale, takes the decoder's maps past 65504 -- the range caveat of unscaled storage, which test_act16_range_report provokes on purpose."""
import pytest
import torch

from _act16_ref import act16_unet_forward
from _h1_ref import h1_unet_forward
from test_gpu_h1 import _net, _rel, _slot

pytestmark = pytest.mark.gpu
WSCALE = 3.0


def _input(shape, seed=11):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed)).cuda()


def _compose(net, x):
    """UNetSeeInDark on the float32-storage h1 ops with every stored map rounded to fp16 and back; plan and packs: the engine's, of its last forward (on x's shape)"""
    from pnnp_amd import ops
    e = net.engine
    plan, wp, P = e._plan, e._wp, dict(net.named_parameters())
    B, _, H, W = x.shape
    ch = e.ch
    r = lambda t: t.half().float()
    x8 = torch.empty(B, H, W, e.cin_pad, device='cuda')
    ops.nchw_to_nhwc(x, x8, e.cin_pad)

    def conv(name, x1, x2, h, w, cout):
        f, _, ws = wp[name]
        y = torch.empty(B, h, w, cout, device='cuda')
        s = plan[name]
        if s.fwd == 'h1+splitk':
            ops.conv_h1_fwd_splitk(x1, x2, f, ws, P[name + '.bias'], y, cout, 1, _slot(x1), s.ks, torch.empty(s.ks * y.numel(), device='cuda'),
                                   amax_x2=_slot(x2) if x2 is not None else None)
        else:
            ops.conv_h1_fwd(x1, x2, f, ws, P[name + '.bias'], y, cout, 1, _slot(x1), _slot(x2) if x2 is not None else None)
        return r(y)
    cur, skips = x8, []
    for i in range(1, 6):
        h, w, c = H >> (i - 1), W >> (i - 1), ch[i - 1]
        cur = conv(f'conv{i}_2', conv(f'conv{i}_1', cur, None, h, w, c), None, h, w, c)
        if i < 5:
            skips.append(cur)
            cur = ops.maxpool_fwd(cur, torch.empty(B, h // 2, w // 2, c, device='cuda'))
    for i in range(6, 10):
        lvl = 9 - i
        h, w, c = H >> lvl, W >> lvl, ch[lvl]
        f, _, ws = wp[f'upv{i}']
        u = r(ops.convt_h1_fwd(cur, _slot(cur), f, ws, P[f'upv{i}.bias'], torch.empty(B, h, w, c, device='cuda'), c))
        cur = conv(f'conv{i}_1', u, skips[lvl], h, w, c)
        if i < 9:
            cur = conv(f'conv{i}_2', cur, None, h, w, c)
    f, _, ws = wp['conv9_2']
    out = torch.empty(B, 4, H, W, device='cuda')
    ops.conv_h1_fwd_head(cur, None, f, ws, P['conv9_2.bias'], None, ch[0], 1, _slot(cur), P['conv10_1.weight'], P['conv10_1.bias'], out, residual=x if net.res else None)
    return out


def _on(e, on):
    e.set_policy(h1_eval=on, h1_pointwise=on, h1_act16=on)


@pytest.mark.parametrize('res', [False, True])
@pytest.mark.parametrize('shape', [(2, 4, 64, 64), (1, 4, 80, 112)])
def test_act16_network_equals_the_composition_and_meets_the_float64_bar(shape, res):
    net, sd = _net('unet', WSCALE, res=res)
    e = net.engine
    x = _input(shape)
    with torch.no_grad():
        _on(e, True)
        y = net(x).clone()
        plan = e._plan
        assert plan.act16 and not plan.train
        assert any(s.fwd == 'h1+splitk' for s in plan.steps.values()) and plan['conv9_2'].fwd == 'h1+head'
        assert any(k.endswith(':float16') for k in e.bufs[(shape[0], shape[2], shape[3], x.device)].t)
        comp = _compose(net, x)
        assert torch.isfinite(y).all() and torch.equal(y, comp)
        rng = e.act16_range()
        assert len(rng) == 21 and not any(r['overflow'] or r['inherited'] for r in rng) and all(0 < r['amax'] < 65504 for r in rng)
        e.set_policy(h1_act16=False)
        y_all = net(x).clone()
        assert not e._plan.act16 and not torch.equal(y_all, y)     # (the stores do round)
        _on(e, False)
        y_off = net(x).clone()
    # against float64: 2 x the emulation's own error + the eval-forward bar (tests/test_gpu_h1.py::test_h1_network_forward_vs_float64)
    sd64 = {k: v.double().cuda() for k, v in sd.items()}
    exact = h1_unet_forward(sd64, x, res=res)
    emu = act16_unet_forward(sd64, x, res=res)
    e_emu, e_act, e_all = _rel(emu, exact), _rel(y.double(), exact), _rel(y_all.double(), exact)
    bar = float((2e-6 + 1e-4 * exact.abs()).norm() / exact.norm())
    print(f'unet {shape} res {res} weights x {WSCALE}: relative L2 vs exact float64: fp16_act {e_act:.3e}, its emulation {e_emu:.3e}, fp16_all {e_all:.3e}; bar term {bar:.2e}')
    assert e_act <= 2.0 * e_emu + bar
    assert e_emu > 1e-5                                             # (the emulation does round: the comparison is not vacuous)
    # the switches off again: bit-equal to a fresh engine
    fresh, _ = _net('unet', WSCALE, res=res)
    with torch.no_grad():
        assert torch.equal(fresh(x), y_off)


@pytest.mark.parametrize('tile_batch', [None, 1])
def test_act16_forward_tiled_equals_the_composition_per_tile(tile_batch):
    from pnnp_amd import tiles
    from pnnp_amd.evaluate import forward_tiled
    net, _ = _net('unet', WSCALE, res=True)
    e = net.engine
    Hh, Ww, P, BASE = 100, 132, 64, 16
    x = _input((1, 4, Hh, Ww), seed=3)
    got = forward_tiled(net, x, P, base=BASE, tile_batch=tile_batch, precision='fp16_act')
    assert not e.policy.h1_act16 and not e.policy.h1_eval and not e.policy.h1_pointwise and 'h1_act16' not in e._h2_sub      # restored
    crops = tiles.eval_crop(x, P, BASE)
    with torch.no_grad():
        _on(e, True)
        outs = []
        for c in ([crops] if tile_batch is None else crops.split(tile_batch)):
            c = c.contiguous()
            net(c)                                                  # (the plan of this batch size: the composition follows its variants and K slices)
            assert e._plan.act16
            outs.append(_compose(net, c))
        _on(e, False)
    want = tiles.eval_merge(torch.cat(outs), Hh, Ww, BASE)
    assert torch.equal(got, want)


def test_act16_leaves_everything_else_where_it_was():
    from pnnp_amd._lib import PnnpError
    from pnnp_amd.evaluate import evaluate, forward_tiled
    from pnnp_amd.trainer import HipTrainStep
    # ResUnet: 'fp16_act' is 'fp16_all', bit for bit (its residual adds read float32 shortcuts: no fp16 storage)
    rnet, _ = _net('resunet', WSCALE)
    x = _input((1, 4, 64, 64))
    a = forward_tiled(rnet, x, 64, base=16, precision='fp16_all')
    b = forward_tiled(rnet, x, 64, base=16, precision='fp16_act')
    assert torch.equal(a, b) and not rnet.engine._plan.act16
    # a training step with all three switches on: bit-identical to one with them off
    xt = _input((2, 4, 64, 64)); t = _input((2, 4, 64, 64), seed=2)

    def run(on):
        net, _ = _net('unet', WSCALE)
        net.train()
        ts = HipTrainStep(net, lr=1e-4, clip=0)
        if on:
            _on(net.engine, True)
            with torch.no_grad():
                net(xt)                                             # an eval-mode forward on the training shape first, then the steps WITH the switches still on
        losses = [ts.step(t, noisy=xt)[0].clone() for _ in range(2)]
        return torch.stack(losses), [p.detach().clone() for p in net.parameters()], net.engine._plan.table(), net.engine._plan.act16
    l0, p0, t0, a0 = run(False)
    l1, p1, t1, a1 = run(True)
    assert t1 == t0 and not a0 and not a1
    assert torch.equal(l1, l0) and all(torch.equal(u, v) for u, v in zip(p1, p0))
    # the switches come back when the call raises
    net, _ = _net('unet', WSCALE, res=True)
    hr = _input((1, 4, 64, 64), seed=5) * 0.5
    with pytest.raises(PnnpError):
        evaluate(net, hr[0], hr, precision='fp16_act')               # not [1,C,H,W]: raises inside the call
    assert not net.engine.policy.h1_act16 and not net.engine.policy.h1_eval and not net.engine.policy.h1_pointwise
    lr = (hr + 0.02 * _input((1, 4, 64, 64), seed=6) - 0.01).clamp(0, 1)
    m = evaluate(net, lr, hr, precision='fp16_act')['metrics']
    assert torch.isfinite(m).all() and net.engine._plan.act16 and not net.engine.policy.h1_act16
    with pytest.raises(PnnpError):
        evaluate(net, hr, hr, precision='fp16_everything')


def test_act16_range_report():
    """conv1_1's weights x S, conv1_2's / S: conv1_1's float32 values pass 65504 while everything downstream keeps its size.  The output holds inf / NaN, the
    report names conv1_1 as the layer that overflowed and no other (maps behind it inherit the inf: amax inf), nothing faults."""
    net, _ = _net('unet', WSCALE)
    e = net.engine
    x = _input((1, 4, 64, 64))
    with torch.no_grad():
        _on(e, True)
        net(x)
        a11 = next(r['amax'] for r in e.act16_range() if r['name'] == 'conv1_1')
        S = 2.0 ** 18 / a11
        P = dict(net.named_parameters())
        P['conv1_1.weight'].mul_(S); P['conv1_1.bias'].mul_(S); P['conv1_2.weight'].div_(S)
        y = net(x)
        torch.cuda.synchronize()
        rng = {r['name']: r for r in e.act16_range()}
        _on(e, False)
    assert not torch.isfinite(y).all()
    assert rng['conv1_1']['overflow'] and 65504 < rng['conv1_1']['amax'] < float('inf')
    assert [n for n, r in rng.items() if r['overflow']] == ['conv1_1']


@pytest.mark.parametrize('precision', [None, 'fp32', 'fp16', 'fp16_all'])
def test_act16_leaves_the_other_precisions_bit_identical(precision):
    """An engine that has served 'fp16_act' (its plans, fp16 buffers and the h1_act16 override came and went) gives under every other precision exactly what
    an engine that never saw the switch gives with the policy set by hand -- the outputs of the parent commit's code path."""
    from pnnp_amd.evaluate import _PRECISION, forward_tiled
    x = _input((1, 4, 100, 132), seed=3)
    used, _ = _net('unet', WSCALE, res=True)
    forward_tiled(used, x, 64, base=16, precision='fp16_act')
    assert used.engine._plan.act16
    got = forward_tiled(used, x, 64, base=16, precision=precision)
    assert not used.engine._plan.act16 and 'h1_act16' not in used.engine._h2_sub
    fresh, _ = _net('unet', WSCALE, res=True)
    if precision is not None:
        fresh.engine.set_policy(**_PRECISION[precision])
    assert not hasattr(fresh.engine.policy, 'h1_act16') or not fresh.engine.policy.h1_act16
    want = forward_tiled(fresh, x, 64, base=16)
    assert torch.equal(got, want)
    # ... and the switch left ON beside the others is inert unless all three are on (that IS fp16 storage)
    fresh.engine.set_policy(h1_act16=True)
    again = forward_tiled(fresh, x, 64, base=16)
    assert fresh.engine._plan.act16 == (precision == 'fp16_all')
    if precision != 'fp16_all':
        assert torch.equal(again, want)


def test_act16_runs_a_frame_past_the_float32_bound():
    """6144 x 4096 at nf = 32: (H + 4) W 32 channels x 4 bytes is past 2^31 (from row 4096 on every byte offset of a float32 map would be), x 2 bytes is not.
    Refused without fp16 storage, before anything runs; whole under 'fp16_act'.  The check is exact: the frame repeats a 1024 x 1024 pattern -- a multiple of every
    tile and of the pooling -- so two blocks one period apart and away from the borders (256 px, more than the network's receptive field of ~110) see the same
    halo at the same place in their tiles in the same launches: their outputs are bit-equal unless an address is wrong.  One block lies in the first period,
    the other in the last, past the float32 bound."""
    from pnnp_amd import ops
    from pnnp_amd._lib import PnnpError
    H, W, T = 6144, 4096, 1024
    assert not ops.image_fits(H, W, 32, 4) and ops.image_fits(H, W, 32, 2) and (H - T + 256) * W * 32 * 4 >= 2 ** 31
    net, _ = _net('unet', WSCALE)
    e = net.engine
    x = torch.rand(1, 4, T, T, device='cuda', generator=torch.Generator(device='cuda').manual_seed(4)).repeat(1, 1, H // T, W // T)
    with torch.no_grad():
        with pytest.raises(PnnpError):
            net(x)                                                  # the default path: float32 maps
        e.set_policy(h1_eval=True, h1_pointwise=True)
        with pytest.raises(PnnpError):
            net(x)                                                  # fp16_all: float32 maps too
        _on(e, True)
        y = net(x)
        assert e._plan.act16 and tuple(y.shape) == (1, 4, H, W)
    assert torch.isfinite(y).all()
    near = y[:, :, 256:768, 256:768]
    far = y[:, :, H - T + 256:H - T + 768, W - T + 256:W - T + 768]
    assert float(near.abs().max()) > 0 and torch.equal(far, near)
    mid = y[:, :, 2 * T + 256:2 * T + 768, T + 256:T + 768]
    assert torch.equal(mid, near)
    net.train()
    try:
        with pytest.raises(PnnpError):
            net(x)                                                  # a training forward has no fp16 storage: refused before anything is launched
    finally:
        net.eval(); _on(e, False)

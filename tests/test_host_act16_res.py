"""Host checks of fp16 activation storage for ResUnet (ConvPolicy.h1_act16_res, precision='fp16_act_res'): the plan, the precision tables, the exports and
tests/_act16_resunet_ref.py against tests/_h1pw_ref.py.  No GPU.

WSCALE is chosen HERE, on the CPU, for the GPU tests that import it.  ResUnet's residual sums carry no activation, so its maps grow with the weights' scale
much faster than UNet's: with init_state x 3 (the UNet tests' scale) c7 reaches 6.1e4 on a 1x4x80x112 input -- at the edge of fp16; x 2.5 gives 2.2e3 (c7),
with the smallest map's maximum (t1) at 0.31; x 2 gives 60.  2.5 leaves a factor 29 to 65504 and 14 to 2^15 (below which the layer emulations' scaled input
rounding is exact for fp16 values, as the kernels' unscaled read is), while the maps still span four decades."""
import torch

from _act16_ref import r16
from _act16_resunet_ref import STORED, act16_resunet_forward, identity
from _h1pw_ref import h1pw_resunet_forward

CH = [32, 64, 128, 256, 512]
WSCALE = 2.5
NET_SHAPES = [(2, 4, 64, 64), (1, 4, 80, 112)]                      # the GPU network test's inputs (seed 11)
ALL3 = dict(h1_eval=True, h1_pointwise=True, h1_act16=True)
ALL4 = dict(ALL3, h1_act16_res=True)
LAYERS = ['conv_in'] + [f'b{i}_{j}' for i in range(1, 10) for j in (0, 1)] + [f'pool{i}' for i in range(1, 5)] + [f'upv{i}' for i in range(6, 10)] + \
         [f'sc{i}' for i in range(6, 10)]


def net_input(shape, seed=11):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed))


def _sd(scale=WSCALE):
    from oracle import net_torch as O
    return {k: v.double() * scale for k, v in O.init_state(O.resunet_param_shapes(nf=32), seed=5).items()}


def _pol(**kw):
    from pnnp_amd.archs import plan as P
    pol = P.ConvPolicy()
    for k, v in kw.items():
        setattr(pol, k, v)
    return pol


def _ks(plan):
    return [s.ks for s in plan.steps.values()]


def test_act16_res_plan():
    from pnnp_amd.archs import plan as P
    base = P.ConvPolicy()
    assert base.h1_act16_res is False and len(base.plan_key()) == len(base.key()) + 6
    R = lambda pol, train, *shape: P.resolve_resunet(CH, 4, 4, pol, train, *shape)
    # alone, or with any proper subset of the other three, the switch is inert
    for sub in (dict(), dict(h1_eval=True), dict(h1_eval=True, h1_pointwise=True), dict(h1_eval=True, h1_act16=True), dict(h1_pointwise=True, h1_act16=True)):
        p0, p1 = R(_pol(**sub), False, 1, 256, 256), R(_pol(h1_act16_res=True, **sub), False, 1, 256, 256)
        assert not p1.act16 and p1.table() == p0.table() and p1.packs == p0.packs and _ks(p1) == _ks(p0), sub
    for shape in ((1, 256, 256), (2, 64, 64), (1, 80, 112), (16, 512, 512)):
        all16 = R(_pol(h1_eval=True, h1_pointwise=True), False, *shape)
        three = R(_pol(**ALL3), False, *shape)
        four = R(_pol(**ALL4), False, *shape)
        assert not all16.act16 and not three.act16 and four.act16                              # three switches: today's plan
        for p in (three, four):
            assert p.table() == all16.table() and p.packs == all16.packs and _ks(p) == _ks(all16)
        assert four['conv_in'].fwd in ('thin', 'h1') and four['conv10'].fwd == 'thin'
        assert all(four[n].fwd == 'h1' for n in LAYERS[1:])
        tr = R(_pol(**ALL4), True, *shape)                                                     # training plans are unchanged
        tr0 = R(_pol(), True, *shape)
        assert not tr.act16 and tr.table() == tr0.table() and tr.packs == tr0.packs
    # a layer on another family, or a head outside the streaming kernel, keeps float32 storage: the fp16_all plan of that policy
    for off in (dict(h2_pointwise=False), dict(thin=False)):
        held = R(_pol(**ALL4, **off), False, 1, 256, 256)
        want = R(_pol(h1_eval=True, h1_pointwise=True, **off), False, 1, 256, 256)
        assert not held.act16 and held.table() == want.table() and held.packs == want.packs, off
    assert R(_pol(**ALL4, thin=False), False, 1, 256, 256)['conv10'].fwd == 'direct'
    # the plan key differs from the three-switch policy's, the pack key does not
    a, b = _pol(**ALL3), _pol(**ALL4)
    assert a.plan_key() != b.plan_key() and a.key() == b.key()
    # UNet never reads the fourth switch
    for sub in (dict(), dict(h1_eval=True, h1_pointwise=True), ALL3):
        for train in (False, True):
            u0 = P.resolve_unet(CH, 4, 4, _pol(**sub), train, 1, 512, 512)
            u1 = P.resolve_unet(CH, 4, 4, _pol(h1_act16_res=True, **sub), train, 1, 512, 512)
            assert u1.act16 == u0.act16 and u1.table() == u0.table() and u1.packs == u0.packs and _ks(u1) == _ks(u0)


def test_act16_res_switch_comes_from_the_environment_and_set_policy(monkeypatch):
    from pnnp_amd.archs import plan as P
    monkeypatch.setenv('PNNP_H1_ACT16_RES', '1')
    assert P.ConvPolicy().h1_act16_res is True and P.ConvPolicy(h2=False).h1_act16_res is False
    monkeypatch.setenv('PNNP_H1_ACT16_RES', '0')
    assert P.ConvPolicy().h1_act16_res is False


def test_act16_res_precision_tables():
    from pnnp_amd import evaluate
    from pnnp_amd._lib import PnnpError
    # the two pinned tables are what they were; the new name lives beside them
    assert evaluate._PRECISION == {'fp32': dict(h1_eval=False), 'fp16': dict(h1_eval=True), 'fp16_all': dict(h1_eval=True, h1_pointwise=True)}
    assert evaluate._PRECISION_STORAGE == {'fp16_act': ALL3}
    assert evaluate._PRECISION_STORAGE_RES == {'fp16_act_res': ALL4}

    class Eng:                                                       # what _precision touches of an engine
        def __init__(self):
            from pnnp_amd.archs import plan as P
            self.policy, self._h2_sub, self.calls = P.ConvPolicy(), {}, []

        def set_policy(self, **kw):
            self.calls.append(dict(kw))
            for k, v in kw.items():
                setattr(self.policy, k, v); self._h2_sub[k] = v

    class Net:
        engine = Eng()
    net = Net()
    with evaluate._precision(net, 'fp16_act_res'):
        assert all(getattr(net.engine.policy, k) for k in ALL4) and net.engine.calls == [ALL4]
    assert not any(getattr(net.engine.policy, k) for k in ALL4) and net.engine._h2_sub == {}
    try:
        with evaluate._precision(net, 'fp16_act_res'):
            raise KeyError('inside the call')
    except KeyError:
        pass
    assert not any(getattr(net.engine.policy, k) for k in ALL4) and net.engine._h2_sub == {}      # restored on an exception too
    net.engine.set_policy(h1_eval=True)                              # a switch the caller had set by hand stays set, and stays an override
    with evaluate._precision(net, 'fp16_act_res'):
        pass
    assert net.engine.policy.h1_eval and not net.engine.policy.h1_act16_res and set(net.engine._h2_sub) == {'h1_eval'}
    for bad in ('fp16_act_all', 'fp16_res', ''):
        try:
            with evaluate._precision(net, bad):
                pass
            raise AssertionError(bad)
        except PnnpError as e:
            assert 'fp16_act_res' in str(e)


def test_act16_res_exports_and_the_abi_version():
    import os
    from pnnp_amd import _lib, ops
    L = _lib.lib()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'pnnp_hip.h')).read()
    for name in ('pnnp_conv3x3_h1_fwd_res_et', 'pnnp_conv_s2_h1_fwd_et', 'pnnp_conv1x1_h1_fwd_et', 'pnnp_first_fwd_amax_et', 'pnnp_head_fwd_et'):
        assert hasattr(L, name) and name + '(' in hdr, name
    for name in ('conv_s2_h1a_fwd', 'conv1x1_h1a_fwd', 'first_fwd_et', 'head_fwd_et'):
        assert callable(getattr(ops, name)), name
    assert L.pnnp_abi_version() == ops.ABI_VERSION == 9               # entries only: the version stays


def test_act16_resunet_ref_without_the_stores_is_the_fp16_all_emulation():
    sd = _sd()
    x = net_input((1, 4, 32, 32))
    for res in (False, True):
        want = h1pw_resunet_forward(sd, x, LAYERS, res=res)
        got = act16_resunet_forward(sd, x, res=res, store=identity)
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    # with them the result moves, by about 2^-11 per stored map
    got16 = act16_resunet_forward(sd, x)
    e = float((got16 - want + x.double()).norm() / (want - x.double()).norm())
    assert 1e-5 < e < 1e-2, e


def test_act16_resunet_stored_maps_stay_inside_fp16_at_the_gpu_tests_scale():
    """Every one of the 31 stored maps, at WSCALE and on the GPU network test's inputs, for conv_in on either kernel: 0 < max |map| < 2^15 (< 65504 is what the
    store needs; < 2^15 is what makes the emulation's scaled input rounding exact), a factor 4 inside on both sides of fp16's normal range."""
    sd = _sd()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    for shape in NET_SHAPES:
        for h1_first in (True, False):
            maps = {}
            out = act16_resunet_forward(sd, net_input(shape), maps=maps, h1_first=h1_first)
            assert sorted(maps) == sorted(STORED) and len(maps) == 31
            for name, t in maps.items():
                a = float(t.abs().max())
                assert 0.0 < a < 65504.0 and 4.0 * 2.0 ** -14 < a < 2.0 ** 15 / 4.0, (shape, name, a)
                assert torch.equal(t, r16(t)), name                  # (fp16 values, exactly)
            assert torch.isfinite(out).all()

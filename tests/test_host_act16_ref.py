"""Host checks of the fp16-storage eval forward: tests/_act16_ref.py against a by-hand float64 composition of the h1 layer emulations, and the plan
(ConvPolicy.h1_act16, Plan.act16) in the manner of tests/test_host_h1_plan.py.  No GPU."""
import torch

from _act16_ref import act16_unet_forward, r16
from _h1_ref import _pool64, conv64, h1_conv
from _h1pw_ref import h1_convt, h1pw_unet_forward

CH = [32, 64, 128, 256, 512]


def _sd(scale=3.0):
    from oracle import net_torch as O
    return {k: v.double() * scale for k, v in O.init_state(O.unet_param_shapes(nf=32), seed=5).items()}


def test_act16_ref_equals_the_layer_emulations_with_fp16_rounding_between_them():
    """UNet 1x4x32x32: every layer is tests/_h1_ref.py / _h1pw_ref.py's emulation (which rounds its input with the tensor's own amax -- exact for a tensor of
    fp16 values below 2^15), every stored map is rounded once in between.  Equal to the last bit in float64."""
    sd = _sd()
    x = torch.rand(1, 4, 32, 32, generator=torch.Generator().manual_seed(11)).double()
    c = lambda n, t, t2=None: h1_conv(t, t2, sd[n + '.weight'], sd[n + '.bias'], 1)
    cur, skips = x, []
    for i in range(1, 6):
        cur = r16(c(f'conv{i}_2', r16(c(f'conv{i}_1', cur))))
        if i < 5:
            skips.append(cur); cur = _pool64(cur)
    for i in range(6, 10):
        u = r16(h1_convt(cur, sd[f'upv{i}.weight'], sd[f'upv{i}.bias']))
        cur = c(f'conv{i}_2', r16(c(f'conv{i}_1', u, skips[9 - i])))
        if i < 9:
            cur = r16(cur)
    want = conv64(cur, sd['conv10_1.weight'], sd['conv10_1.bias'])
    got = act16_unet_forward(sd, x)
    assert float(cur.abs().max()) < 2.0 ** 15
    assert torch.equal(got, want)
    assert torch.equal(act16_unet_forward(sd, x, res=True), want + x)
    # without the store's rounding it is the fp16_all emulation up to where THAT rounds an activation; with it the result moves, by about 2^-11
    names = [f'conv{i}_{j}' for i in range(1, 10) for j in (1, 2)] + [f'upv{i}' for i in range(6, 10)]
    all16 = h1pw_unet_forward(sd, x, names)
    e = float((got - all16).norm() / all16.norm())
    assert 1e-5 < e < 1e-2, e


def _pol(**kw):
    from pnnp_amd.archs import plan as P
    pol = P.ConvPolicy()
    for k, v in kw.items():
        setattr(pol, k, v)
    return pol


def test_act16_plan():
    from pnnp_amd.archs import plan as P
    base = P.ConvPolicy()
    assert base.h1_act16 is False and 'h1_act16' not in repr(base.key())
    # alone it changes nothing
    p0 = P.resolve_unet(CH, 4, 4, _pol(), False, 1, 512, 512)
    p1 = P.resolve_unet(CH, 4, 4, _pol(h1_act16=True), False, 1, 512, 512)
    assert p1.table() == p0.table() and not p1.act16
    p2 = P.resolve_unet(CH, 4, 4, _pol(h1_eval=True, h1_act16=True), False, 1, 512, 512)
    assert not p2.act16 and p2.table() == P.resolve_unet(CH, 4, 4, _pol(h1_eval=True), False, 1, 512, 512).table()
    # with both other switches: a UNet eval plan marks fp16 storage -- same launches as fp16_all -- and a training plan does not
    for shape in ((1, 512, 512), (2, 64, 64), (1, 80, 112), (16, 512, 512)):
        all16 = P.resolve_unet(CH, 4, 4, _pol(h1_eval=True, h1_pointwise=True), False, *shape)
        act = P.resolve_unet(CH, 4, 4, _pol(h1_eval=True, h1_pointwise=True, h1_act16=True), False, *shape)
        assert act.act16 and not all16.act16 and act.table() == all16.table() and act.packs == all16.packs
        assert [s.ks for s in act.steps.values()] == [s.ks for s in all16.steps.values()]
        tr = P.resolve_unet(CH, 4, 4, _pol(h1_eval=True, h1_pointwise=True, h1_act16=True), True, *shape)
        assert not tr.act16 and tr.table() == P.resolve_unet(CH, 4, 4, _pol(), True, *shape).table()
    # a layer held on another family keeps the whole plan on float32 storage: the head outside conv9_2's epilogue, the pointwise layers on bf16x3
    for off in (dict(head_fused=False), dict(h2_pointwise=False)):
        held = P.resolve_unet(CH, 4, 4, _pol(h1_eval=True, h1_pointwise=True, h1_act16=True, **off), False, 1, 512, 512)
        assert not held.act16 and held.table() == P.resolve_unet(CH, 4, 4, _pol(h1_eval=True, h1_pointwise=True, **off), False, 1, 512, 512).table()
    # ResUnet: its fp16_all plan, unchanged
    r0 = P.resolve_resunet(CH, 4, 4, _pol(h1_eval=True, h1_pointwise=True), False, 1, 256, 256)
    r1 = P.resolve_resunet(CH, 4, 4, _pol(h1_eval=True, h1_pointwise=True, h1_act16=True), False, 1, 256, 256)
    assert not r1.act16 and r1.table() == r0.table() and r1.packs == r0.packs
    # the plan key differs, the pack key does not
    a, b = _pol(h1_eval=True, h1_pointwise=True), _pol(h1_eval=True, h1_pointwise=True, h1_act16=True)
    assert a.plan_key() != b.plan_key() and a.key() == b.key()


def test_act16_exports_and_the_abi_version():
    import os
    from pnnp_amd import _lib, ops
    L = _lib.lib()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'pnnp_hip.h')).read()
    for name in ('pnnp_conv3x3_h1_fwd_et', 'pnnp_conv3x3_h1_fwd_splitk_et', 'pnnp_conv3x3_h1_fwd_head_et', 'pnnp_conv3x3_h1_fwd_pool_et', 'pnnp_convt_h1_fwd_et',
                 'pnnp_image_fits_es', 'pnnp_maxpool2_fwd_f16'):
        assert hasattr(L, name) and name + '(' in hdr, name
    assert L.pnnp_abi_version() == ops.ABI_VERSION == 9               # entries only: the version stays
    assert ops.image_fits(1424, 2128, 32) and ops.image_fits(4096, 8000, 32, 2) and not ops.image_fits(4096, 8000, 32, 4)
    assert not ops.image_fits(4096, 8000, 32, 3) and not ops.image_fits(0, 8, 32, 2)
    for H, W, C in ((1424, 2128, 32), (4096, 4096, 32), (4096, 8000, 32), (16, 16, 8)):
        assert ops.image_fits(H, W, C, 4) == ops.x3_image_fits(H, W, C)


def test_act16_precision_argument_is_known_on_the_host():
    from pnnp_amd import evaluate
    assert evaluate._PRECISION_STORAGE == {'fp16_act': dict(h1_eval=True, h1_pointwise=True, h1_act16=True)}
    assert evaluate._PRECISION['fp16_all'] == dict(h1_eval=True, h1_pointwise=True) and 'fp16_act' not in evaluate._PRECISION

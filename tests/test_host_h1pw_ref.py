"""Pins tests/_h1pw_ref.py, the float64 restatement the fp16x1 pointwise GPU tests compare against (no GPU): with the rounding off every layer is
the plain float64 torch op to 1e-13, with it on every operand is a multiple of its fp16 step and the two K segments of a 1x1 layer share the
LARGER amax.  Then the host side of the feature: the new exports, the shape table of pnnp_h1_pointwise_supported, the pack sizes, and which
steps of a plan ConvPolicy.h1_pointwise moves."""
import ctypes as C

import pytest
import torch

from _h1_ref import h1_round, h1_scale_exp, h1_resunet_forward, h1_unet_forward
from _h1pw_ref import h1_conv1x1, h1_conv_s2, h1_convt, h1pw_resunet_forward, h1pw_unet_forward
from pnnp_amd.archs import plan
from pnnp_amd.archs.unet import _EngineBase

F = torch.nn.functional
CH = [32, 64, 128, 256, 512]


def _ops(seed=0):
    g = torch.Generator().manual_seed(seed)
    x1 = torch.randn(2, 8, 6, 10, generator=g)
    x2 = torch.randn(2, 8, 6, 10, generator=g) * 50.0
    return g, x1, x2


def _on_fp16_grid(t, amax):
    """every element of t is a multiple of its fp16 step at the scale of ``amax``: t 2^se is an fp16 number"""
    s = t.double() * 2.0 ** h1_scale_exp(amax)
    return torch.equal(s.half().double(), s)


def test_unrounded_layers_are_the_plain_float64_ops():
    g, x1, x2 = _ops()
    wt, bt = torch.randn(8, 12, 2, 2, generator=g) * 0.2, torch.randn(12, generator=g)
    ref = F.conv_transpose2d(x1.double(), wt.double(), bt.double(), stride=2)
    assert torch.allclose(h1_convt(x1, wt, bt, rounded=False), ref, rtol=1e-13, atol=1e-13)
    w1, b1 = torch.randn(12, 16, 1, 1, generator=g) * 0.2, torch.randn(12, generator=g)
    r = torch.randn(2, 12, 6, 10, generator=g)
    ref = F.leaky_relu(F.conv2d(torch.cat([x1, x2], 1).double(), w1.double(), b1.double()) + r.double(), 0.2)
    assert torch.allclose(h1_conv1x1(x1, x2, w1, b1, 1, residual=r, rounded=False), ref, rtol=1e-13, atol=1e-13)
    ref = F.conv2d(x1.double(), w1[:, :8].double(), None)
    assert torch.allclose(h1_conv1x1(x1, None, w1[:, :8], None, 0, rounded=False), ref, rtol=1e-13, atol=1e-13)
    w3, b3 = torch.randn(12, 8, 3, 3, generator=g) * 0.2, torch.randn(12, generator=g)
    ref = F.relu(F.conv2d(x1.double(), w3.double(), b3.double(), stride=2, padding=1))
    assert torch.allclose(h1_conv_s2(x1, w3, b3, 2, rounded=False), ref, rtol=1e-13, atol=1e-13)


def test_rounded_layers_are_the_ops_on_operands_of_the_fp16_grid():
    g, x1, x2 = _ops(1)
    a1, a2 = float(x1.abs().max()), float(x2.abs().max())
    wt, bt = torch.randn(8, 12, 2, 2, generator=g) * 0.2, torch.randn(12, generator=g)
    xr, wr = h1_round(x1), h1_round(wt)
    assert _on_fp16_grid(xr, a1) and _on_fp16_grid(wr, float(wt.abs().max())) and not torch.equal(xr, x1.double())
    assert torch.equal(h1_convt(x1, wt, bt), h1_convt(xr, wr, bt, rounded=False))
    e = float((h1_convt(x1, wt, bt) - h1_convt(x1, wt, bt, rounded=False)).norm() / h1_convt(x1, wt, bt, rounded=False).norm())
    assert 1e-5 < e < 2e-3
    # two K segments: ONE scale from the LARGER slot.  fp16 is a floating-point format, so the shared scale shows only where it pushes the smaller
    # segment below fp16's normal range: x2 2^30 times larger -> x1 lands among the subnormals of x2's grid (a few bits left), not on its own grid
    w1 = torch.randn(12, 16, 1, 1, generator=g) * 0.2
    x2 = x2 * 2.0 ** 30
    a2 = float(x2.abs().max())
    x1r, x2r = h1_round(x1, a2), h1_round(x2, a2)
    assert _on_fp16_grid(x1r, a2) and _on_fp16_grid(x2r, a2) and not torch.equal(x1r, h1_round(x1, a1))
    want = F.conv2d(torch.cat([x1r, x2r], 1), h1_round(w1))
    assert torch.allclose(h1_conv1x1(x1, x2, w1, None, 0), want, rtol=1e-13, atol=1e-13)
    assert torch.equal(h1_conv1x1(x1, x2, w1, None, 0), h1_conv1x1(x1, x2, w1, None, 0, amax_x1=a1, amax_x2=a2))
    assert torch.equal(h1_conv1x1(x2, x1, w1, None, 0, amax_x1=a2, amax_x2=a1), h1_conv1x1(x2, x1, w1, None, 0))      # whichever segment is larger
    # explicit slots: a slot larger than the tensor's own maximum moves the grid only for fp16-subnormal elements
    w3 = torch.randn(12, 8, 3, 3, generator=g) * 0.2
    assert torch.equal(h1_conv_s2(x1, w3, None, 0), h1_conv_s2(h1_round(x1), h1_round(w3), None, 0, rounded=False))
    assert _on_fp16_grid(h1_round(x1, 64.0 * a1), 64.0 * a1)


def test_network_emulations_extend_the_3x3_ones():
    from oracle import net_torch as O
    x = torch.rand(1, 4, 32, 32, generator=torch.Generator().manual_seed(3))
    for arch, shapes, old, new, pw in (('unet', O.unet_param_shapes(nf=8), h1_unet_forward, h1pw_unet_forward, [f'upv{i}' for i in range(6, 10)]),
                                       ('resunet', O.resunet_param_shapes(nf=8), h1_resunet_forward, h1pw_resunet_forward,
                                        [f'{k}{i}' for i in range(6, 10) for k in ('upv', 'sc')] + [f'pool{i}' for i in range(1, 5)])):
        sd = {k: v * 6.0 for k, v in O.init_state(shapes, seed=1).items()}
        c3 = ([f'conv{i}_{j}' for i in range(1, 10) for j in (1, 2)] if arch == 'unet' else
              ['conv_in'] + [f'b{i}_{j}' for i in range(1, 10) for j in (0, 1)])
        exact = old(sd, x)
        assert torch.equal(new(sd, x), exact)                                  # no layer named: the exact forward
        assert torch.equal(new(sd, x, c3), old(sd, x, c3))                     # the 3x3 layers alone: tests/_h1_ref.py's emulation
        both = new(sd, x, c3 + pw)
        assert not torch.equal(both, old(sd, x, c3))                           # ... and the pointwise layers do round
        e = float((both - exact).norm() / exact.norm())
        assert 1e-5 < e < 1e-2


# ------------------------------------------------------------------ the library's host side
NEW_EXPORTS = ['pnnp_convt_h1_fwd_f32', 'pnnp_conv1x1_h1_fwd_f32', 'pnnp_conv_s2_h1_fwd_f32', 'pnnp_h1_pointwise_supported',
               'pnnp_h1_pointwise_weight_bytes', 'pnnp_pack_jobs_add_h1_convt', 'pnnp_pack_jobs_add_h1_1x1', 'pnnp_pack_jobs_add_h1_s2']


def test_new_exports_and_the_abi_version():
    import os
    from pnnp_amd import _lib, ops
    L = _lib.lib()
    for name in NEW_EXPORTS:
        assert hasattr(L, name), name
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'pnnp_hip.h')).read()
    for name in NEW_EXPORTS:
        assert name + '(' in hdr, name
    assert L.pnnp_abi_version() == ops.ABI_VERSION == 9                       # entries only: the version stays
    for name in ('convt_h1_fwd', 'conv1x1_h1_fwd', 'conv_s2_h1_fwd', 'h1_pointwise_weight_bytes', 'h1_pointwise_supported'):
        assert callable(getattr(ops, name)), name
    for name in ('add_h1_convt', 'add_h1_1x1', 'add_h1_s2'):
        assert callable(getattr(ops.PackJobs, name)), name


@pytest.mark.parametrize('K,N,ok', [(32, 32, True), (32, 96, True), (64, 128, True), (512, 1024, True), (2304, 512, True), (32, 64, True),
                                    (16, 32, False), (48, 64, False), (32, 16, False), (32, 48, False), (0, 32, False), (32, 0, False),
                                    (-32, 32, False), (32, -32, False), (8, 32, False)])
def test_refusal_table_of_h1_pointwise_supported(K, N, ok):
    from pnnp_amd import ops
    assert ops.h1_pointwise_supported(K, N) is ok
    assert ops.h1_pointwise_supported(K, N) == ops.gemm_h2_supported(K, N)    # the shapes of its fp16x2 twin


def test_pack_sizes_and_builders_refuse_on_the_host():
    """2 bytes per weight: half of the kind-6 pack.  The builders validate before anything runs: null pointers, channel counts off the 32 grid, a
    misaligned destination -> PNNP_E_INVALID (-1), a full table -> PNNP_E_WORKSPACE (-4); the table is not advanced."""
    from pnnp_amd import ops
    assert ops.h1_pointwise_weight_bytes(512, 1024) == 512 * 1024 * 2 == ops.h2mat_bytes(512, 1024) // 2
    assert ops.h1_pointwise_weight_bytes(9 * 32, 64) == 9 * 32 * 64 * 2
    L = ops._prep()
    jobs = (ops.PackJob * 16)()
    n = C.c_int(0)
    w, dst, slot = C.c_void_p(0x1000), C.c_void_p(0x2000), C.c_void_p(0x3000)
    for fn, a, b in ((L.pnnp_pack_jobs_add_h1_convt, 64, 32), (L.pnnp_pack_jobs_add_h1_1x1, 32, 64), (L.pnnp_pack_jobs_add_h1_s2, 64, 32)):
        assert fn(jobs, C.byref(n), 16, w, dst, a, 48, slot) == -1 and fn(jobs, C.byref(n), 16, w, dst, 40, b, slot) == -1
        assert fn(jobs, C.byref(n), 16, w, dst, 0, b, slot) == -1
        assert fn(jobs, C.byref(n), 16, None, dst, a, b, slot) == -1 and fn(jobs, C.byref(n), 16, w, None, a, b, slot) == -1
        assert fn(jobs, C.byref(n), 16, w, dst, a, b, None) == -1
        assert fn(jobs, C.byref(n), 16, w, C.c_void_p(0x2008), a, b, slot) == -1          # the pack is read by 16-byte LDS-DMA lanes
        assert n.value == 0
    assert L.pnnp_pack_jobs_add_h1_convt(jobs, C.byref(n), 16, w, dst, 64, 32, slot) == 0 and n.value == 4       # one job per sub-pixel
    assert all(jobs[i].kind == 8 and jobs[i].T == 2 and jobs[i].Ndst == 128 and jobs[i].n_off == 32 * i for i in range(4))
    assert L.pnnp_pack_jobs_add_h1_1x1(jobs, C.byref(n), 16, w, dst, 32, 64, slot) == 0 and n.value == 5 and jobs[4].kind == 8 and jobs[4].T == 2
    assert L.pnnp_pack_jobs_add_h1_s2(jobs, C.byref(n), 16, w, dst, 64, 32, slot) == 0 and n.value == 14         # one job per tap
    assert all(jobs[5 + t].kind == 8 and jobs[5 + t].T == 9 and jobs[5 + t].st == 32 * t for t in range(9))
    assert L.pnnp_pack_jobs_add_h1_s2(jobs, C.byref(n), 16, w, dst, 64, 32, slot) == -4                          # the table is full


# ------------------------------------------------------------------ the plan and the policy
def _engine(**kw):
    e = _EngineBase()
    e._init_base()
    e.set_policy(**kw)
    return e


POINTWISE = {'unet': [f'upv{i}' for i in range(6, 10)],
             'resunet': [f'upv{i}' for i in range(6, 10)] + [f'sc{i}' for i in range(6, 10)] + [f'pool{i}' for i in range(1, 5)]}


@pytest.mark.parametrize('arch', ['unet', 'resunet'])
@pytest.mark.parametrize('shape', [(1, 64, 64), (16, 512, 512)])
def test_eval_plan_moves_exactly_the_pointwise_h2_steps(arch, shape):
    resolve = plan.resolve_unet if arch == 'unet' else plan.resolve_resunet
    p_h1 = resolve(CH, 4, 4, _engine(h1_eval=True).policy, False, *shape)
    p_all = resolve(CH, 4, 4, _engine(h1_eval=True, h1_pointwise=True).policy, False, *shape)
    for name in p_h1.steps:
        if name in POINTWISE[arch]:
            assert p_h1[name].fwd == 'h2' and p_all[name].fwd == 'h1' and p_all[name].pack == ('h1', None), name
        else:
            assert p_all[name].families() == p_h1[name].families() and p_all[name].pack == p_h1[name].pack and p_all[name].ks == p_h1[name].ks, name
    assert not any(p_all[n].fwd == 'h2' for n in POINTWISE[arch])
    assert p_all.h2 and p_all.packs != p_h1.packs


@pytest.mark.parametrize('arch', ['unet', 'resunet'])
def test_the_switch_alone_and_training_plans_change_nothing(arch):
    resolve = plan.resolve_unet if arch == 'unet' else plan.resolve_resunet
    base = _engine().policy
    alone = _engine(h1_pointwise=True).policy
    assert alone.h1_pointwise and not alone.h1_eval
    for train in (False, True):
        p0, p1 = resolve(CH, 4, 4, base, train, 2, 64, 64), resolve(CH, 4, 4, alone, train, 2, 64, 64)
        assert p1.table() == p0.table() and p1.packs == p0.packs
    both = _engine(h1_eval=True, h1_pointwise=True).policy
    p0, p1 = resolve(CH, 4, 4, base, True, 2, 64, 64), resolve(CH, 4, 4, both, True, 2, 64, 64)
    assert p1.table() == p0.table() and p1.packs == p0.packs
    assert [(s.ks, s.codes, s.unpool) for s in p1.steps.values()] == [(s.ks, s.codes, s.unpool) for s in p0.steps.values()]


def test_policy_keys_sub_switch_and_environment(monkeypatch):
    base = _engine().policy
    assert not base.h1_pointwise
    e = _engine(h1_eval=True, h1_pointwise=True)
    assert e.policy.key() == base.key() and len(e.policy.key()) == 12
    assert e.policy.plan_key() != _engine(h1_eval=True).policy.plan_key() != base.plan_key()
    e.set_policy(x3=True)
    assert e.policy.h1_pointwise and e.policy.h1_eval                    # overrides survive a call that does not name them
    e.set_policy(h2=False)
    assert not e.policy.h1_pointwise
    p = plan.resolve_resunet(CH, 4, 4, e.policy, False, 1, 64, 64)
    assert not any(str(f).startswith('h1') for fam in p.table().values() for f in fam)
    e.set_policy(h2=True, h1_pointwise=False)
    assert e.policy.h1_eval and not e.policy.h1_pointwise
    assert e.policy.plan_key() == _engine(h1_eval=True).policy.plan_key()
    monkeypatch.setenv('PNNP_H1_POINTWISE', '1')
    assert plan.ConvPolicy().h1_pointwise and not plan.ConvPolicy(h2=False).h1_pointwise and not plan.ConvPolicy().h1_eval
    monkeypatch.delenv('PNNP_H1_POINTWISE')
    assert not plan.ConvPolicy().h1_pointwise


def test_precision_argument_names():
    from pnnp_amd._lib import PnnpError
    from pnnp_amd.evaluate import _precision

    class NoEngine:
        pass
    with _precision(NoEngine(), None):
        pass
    with _precision(NoEngine(), 'fp32'):
        pass
    for p in ('fp16', 'fp16_all', 'bf16'):
        with pytest.raises(PnnpError):
            with _precision(NoEngine(), p):
                pass

    class Net:
        engine = _engine()
    net = Net()
    with _precision(net, 'fp16_all'):
        assert net.engine.policy.h1_eval and net.engine.policy.h1_pointwise
    assert not net.engine.policy.h1_eval and not net.engine.policy.h1_pointwise and not net.engine._h2_sub
    with pytest.raises(ZeroDivisionError):
        with _precision(net, 'fp16_all'):
            1 / 0
    assert not net.engine.policy.h1_eval and not net.engine.policy.h1_pointwise and not net.engine._h2_sub
    net.engine.set_policy(h1_eval=True)                                  # an engine already serving 'fp16': only the pointwise switch is borrowed
    with _precision(net, 'fp16_all'):
        assert net.engine.policy.h1_eval and net.engine.policy.h1_pointwise
    assert net.engine.policy.h1_eval and not net.engine.policy.h1_pointwise and set(net.engine._h2_sub) == {'h1_eval'}
    with _precision(net, 'fp16'):                                        # 'fp16' and 'fp32' as before: they move h1_eval only
        assert net.engine.policy.h1_eval and not net.engine.policy.h1_pointwise
    with _precision(net, 'fp32'):
        assert not net.engine.policy.h1_eval
    assert net.engine.policy.h1_eval


@pytest.mark.parametrize('precision', ['fp16', 'fp32', 'fp16_all'])
def test_precision_restores_what_it_found(precision):
    """One path over a table of forced switches (evaluate._PRECISION): whatever the engine had comes back, overrides that were not there are
    removed again, also when the body raises; a switch the precision does not name is not touched; nothing at all is touched when the
    switches already have the wanted values."""
    from pnnp_amd.evaluate import _PRECISION, _precision
    assert _PRECISION == {'fp32': dict(h1_eval=False), 'fp16': dict(h1_eval=True), 'fp16_all': dict(h1_eval=True, h1_pointwise=True)}
    want = _PRECISION[precision]
    for start in (dict(), dict(h1_eval=True), dict(h1_pointwise=True), dict(h1_eval=True, h1_pointwise=True), dict(h1_eval=False)):
        class Net:
            engine = _engine(**start)
        net = Net()
        pol = net.engine.policy
        before = (pol.h1_eval, pol.h1_pointwise, dict(net.engine._h2_sub))
        inside = {'h1_eval': pol.h1_eval, 'h1_pointwise': pol.h1_pointwise, **want}
        for body_raises in (False, True):
            try:
                with _precision(net, precision):
                    p = net.engine.policy
                    assert (p.h1_eval, p.h1_pointwise) == (inside['h1_eval'], inside['h1_pointwise']), (start, precision)
                    assert (p is pol) == (inside == dict(h1_eval=before[0], h1_pointwise=before[1])), (start, precision)     # untouched when already as wanted
                    if body_raises:
                        1 / 0
            except ZeroDivisionError:
                assert body_raises
            p = net.engine.policy
            assert (p.h1_eval, p.h1_pointwise, net.engine._h2_sub) == before, (start, precision, body_raises)


def test_precision_fp16_under_pointwise_engine_and_messages():
    from pnnp_amd._lib import PnnpError
    from pnnp_amd.evaluate import _precision

    class Net:
        engine = _engine(h1_pointwise=True)                              # serves nothing yet: the pointwise switch alone changes no plan
    net = Net()
    with _precision(net, 'fp16'):                                        # 'fp16' leaves h1_pointwise as it finds it: here that is fp16_all's plan
        p = net.engine.policy
        assert p.h1_eval and p.h1_pointwise
        assert p.plan_key() == _engine(h1_eval=True, h1_pointwise=True).policy.plan_key()
    assert not net.engine.policy.h1_eval and net.engine.policy.h1_pointwise and net.engine._h2_sub == {'h1_pointwise': True}
    with pytest.raises(ZeroDivisionError):
        with _precision(net, 'fp16'):
            1 / 0
    assert not net.engine.policy.h1_eval and net.engine.policy.h1_pointwise and net.engine._h2_sub == {'h1_pointwise': True}
    net.engine.set_policy(h2=False)
    for precision in ('fp16', 'fp16_all'):                               # the messages name the precision asked for
        with pytest.raises(PnnpError, match=f"precision='{precision}' needs the fp16x2 family"):
            with _precision(net, precision):
                pass
    with _precision(net, 'fp32'):                                        # nothing to force: h1_eval is off without h2
        pass

    class NoEngine:
        pass
    for precision in ('fp16', 'fp16_all'):
        with pytest.raises(PnnpError, match=f"precision='{precision}' needs a network with a HIP engine"):
            with _precision(NoEngine(), precision):
                pass
    with pytest.raises(PnnpError, match="got 'bf16'"):
        with _precision(NoEngine(), 'bf16'):
            pass

"""Host logic of the opt-in fp16x1 eval forward (ConvPolicy.h1_eval, no GPU): which layers of an eval plan take the 'h1' kernels, that
nothing else in any plan moves, and how the switch travels through set_policy."""
import pytest

from pnnp_amd.archs import plan
from pnnp_amd.archs.unet import _EngineBase

CH = [32, 64, 128, 256, 512]
H1_OF = {'h2': 'h1', 'h2+pool': 'h1+pool', 'h2+splitk': 'h1+splitk', 'h2+head': 'h1+head'}


def _engine(**kw):
    e = _EngineBase()
    e._init_base()
    e.set_policy(**kw)
    return e


def _is_conv3(name):
    return name.startswith('conv') and name != 'conv10_1' and name != 'conv10' or name.startswith('b')


@pytest.mark.parametrize('shape', [(1, 512, 512), (1, 1424, 2128), (16, 512, 512)])
def test_unet_eval_plan_takes_h1_exactly_where_it_was_h2(shape):
    base, h1 = _engine().policy, _engine(h1_eval=True).policy
    assert not base.h1_eval and h1.h1_eval
    p0 = plan.resolve_unet(CH, 4, 4, base, False, *shape)
    p1 = plan.resolve_unet(CH, 4, 4, h1, False, *shape)
    t0, t1 = p0.table(), p1.table()
    assert list(t0) == list(t1)
    seen = set()
    for name in t0:
        f0, f1 = t0[name][0], t1[name][0]
        if _is_conv3(name) and f0 in H1_OF:
            assert f1 == H1_OF[f0], (name, f0, f1)
            assert p1[name].pack == ('h1', None) and p1[name].ks == p0[name].ks and p1[name].codes == p0[name].codes
            seen.add(f1)
        else:
            assert t1[name] == t0[name] and p1[name].pack == p0[name].pack, name
        assert t1[name][1:] == t0[name][1:]
    assert {'h1', 'h1+pool', 'h1+head'} <= seen
    assert ('h1+splitk' in seen) == (shape[0] == 1 and shape[1] == 512)      # one crop: the deep levels' grids are small
    assert t1['conv10_1'][0] == 'fused' and t1['upv6'][0] == 'h2'
    assert p1.h2 and p0.h2
    assert p1.packs != p0.packs


def test_resunet_eval_plan_takes_h1_on_the_stride_1_3x3_layers_only():
    base, h1 = _engine().policy, _engine(h1_eval=True).policy
    p0 = plan.resolve_resunet(CH, 4, 4, base, False, 16, 512, 512)
    p1 = plan.resolve_resunet(CH, 4, 4, h1, False, 16, 512, 512)
    t0, t1 = p0.table(), p1.table()
    n_h1 = 0
    for name in t0:
        if (name == 'conv_in' or name.startswith('b')) and t0[name][0] == 'h2':
            assert t1[name][0] == 'h1' and p1[name].pack == ('h1', None), name
            n_h1 += 1
        else:
            assert t1[name] == t0[name] and p1[name].pack == p0[name].pack, name
    assert n_h1 >= 18                                            # b1_0 .. b9_1 (conv_in too where it is not the streaming first layer)
    assert all(t1[f'pool{i}'][0] == 'h2' for i in range(1, 5)) and p1.h2


@pytest.mark.parametrize('resolve', [plan.resolve_unet, plan.resolve_resunet])
def test_train_plan_ignores_the_switch(resolve):
    base, h1 = _engine().policy, _engine(h1_eval=True).policy
    p0, p1 = resolve(CH, 4, 4, base, True, 16, 512, 512), resolve(CH, 4, 4, h1, True, 16, 512, 512)
    assert p1.table() == p0.table() and p1.packs == p0.packs
    assert [(s.ks, s.codes, s.unpool) for s in p1.steps.values()] == [(s.ks, s.codes, s.unpool) for s in p0.steps.values()]
    assert not any('h1' in str(f) for fam in p1.table().values() for f in fam)


def test_switch_off_is_todays_plan():
    e = _engine(h1_eval=True)
    e.set_policy(h1_eval=False)
    base = _engine().policy
    for train in (False, True):
        assert plan.resolve_unet(CH, 4, 4, e.policy, train, 1, 512, 512).table() == plan.resolve_unet(CH, 4, 4, base, train, 1, 512, 512).table()
    assert e.policy.plan_key() == base.plan_key()


def test_policy_keys_and_sub_switch_rule():
    e = _engine(h1_eval=True)
    base = _engine().policy
    assert len(e.policy.key()) == 12 and e.policy.key() == base.key()
    assert e.policy.plan_key() != base.plan_key()
    e.set_policy(x3=True)                                        # a later call that does not name it: the override stays
    assert e.policy.h1_eval
    e.set_policy(h2=False)                                       # only meaningful with the fp16x2 family
    assert not e.policy.h1_eval
    p = plan.resolve_unet(CH, 4, 4, e.policy, False, 1, 512, 512)
    assert not any(str(f).startswith('h1') for fam in p.table().values() for f in fam)
    e2 = _engine(h2=False, h1_eval=True)
    assert not e2.policy.h1_eval
    p = plan.resolve_resunet(CH, 4, 4, e2.policy, False, 1, 512, 512)
    assert not any(str(f).startswith('h1') for fam in p.table().values() for f in fam)
    e.set_policy(h2=True)
    assert e.policy.h1_eval


def test_default_comes_from_the_host_environment_only(monkeypatch):
    monkeypatch.setenv('PNNP_H1_EVAL', '1')
    assert plan.ConvPolicy().h1_eval and not plan.ConvPolicy(h2=False).h1_eval
    monkeypatch.delenv('PNNP_H1_EVAL')
    assert not plan.ConvPolicy().h1_eval

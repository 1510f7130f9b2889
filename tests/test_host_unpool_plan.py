"""The plan's per-layer `unpool` flag (pnnp_amd/archs/plan.py) without a GPU: the decoder layers whose skip-gradient launch carries MaxPool2d's
backward in its epilogue.  Not a kernel family: Plan.table() does not show it."""
import importlib
import os

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEC = [f'conv{i}_1' for i in range(6, 10)]


@pytest.fixture(scope='module', autouse=True)
def _built():
    if not os.path.exists(os.path.join(REPO, 'pnnp_amd', 'libpnnp_hip.so')):
        import __graft_entry__ as g
        g.build()


def _engine(**policy):
    from pnnp_amd.archs import UNetSeeInDark
    e = UNetSeeInDark(dict(nframes=1, res=False, nf=32, in_nc=4, out_nc=4)).engine
    if policy:
        e.set_policy(**policy)
    return e


def _flags(plan):
    return {n: s.unpool for n, s in plan.steps.items() if s.unpool}


def test_flag_is_set_for_the_decoder_skip_layers_in_training():
    p = _engine()._plan_for(16, 512, 512, True)
    assert _flags(p) == {n: True for n in DEC}
    for i in range(1, 5):                                   # what the deferred launch reads: sign bits (an fp16x2 forward) and codes
        s = p[f'conv{i}_2']
        assert s.fwd.startswith('h2') and s.codes


def test_flag_is_clear_in_eval_and_without_the_fp16x2_family():
    assert _flags(_engine()._plan_for(1, 512, 512, False)) == {}
    assert _flags(_engine(h2=False)._plan_for(16, 512, 512, True)) == {}
    assert _flags(_engine(x3=False, h2=False)._plan_for(16, 512, 512, True)) == {}
    assert _flags(_engine(unpool_fused=False)._plan_for(16, 512, 512, True)) == {}


def test_flag_is_per_level():
    p = _engine(unpool_levels=(1, 3))._plan_for(16, 512, 512, True)
    assert _flags(p) == {'conv9_1': True, 'conv7_1': True}  # level L belongs to conv{10 - L}_1


def test_environment_switch(monkeypatch):
    from pnnp_amd.archs import plan
    monkeypatch.setenv('PNNP_UNPOOL_FUSED', '0')
    assert plan.ConvPolicy().unpool_fused is False
    monkeypatch.setenv('PNNP_UNPOOL_FUSED', '1')
    monkeypatch.setenv('PNNP_UNPOOL_LEVELS', '234')
    pol = plan.ConvPolicy()
    assert pol.unpool_fused is True and pol.unpool_levels == (2, 3, 4)
    assert plan.ConvPolicy(h2=False).unpool_fused is False
    monkeypatch.delenv('PNNP_UNPOOL_LEVELS')
    assert plan.ConvPolicy().unpool_levels == (1, 2, 3, 4)
    assert plan.ConvPolicy().plan_key() != pol.plan_key()   # plans are cached per plan key


def test_an_engine_built_under_the_switch_runs_the_old_sequence(monkeypatch):
    monkeypatch.setenv('PNNP_UNPOOL_FUSED', '0')
    from pnnp_amd.archs import plan
    pol = plan.ConvPolicy()
    p = plan.resolve_unet([32, 64, 128, 256, 512], 4, 4, pol, True, 16, 512, 512)
    assert _flags(p) == {}


def test_table_is_unchanged_by_the_flag():
    on = _engine()._plan_for(16, 512, 512, True)
    off = _engine(unpool_fused=False)._plan_for(16, 512, 512, True)
    assert on.table() == off.table() and on.ws == off.ws and on.packs == off.packs
    assert all(len(t) == 3 for t in on.table().values())

"""The per-layer kernel-family plan (pnnp_amd/archs/plan.py) without a GPU: for each case, the (forward / backward-data / backward-weight)
family of every layer and the backward-weight workspace, as recorded from the launch sequence of a training step (or an eval forward)
on the MI355X before the plan existed.  nf = 32, 4 -> 4 channels, 512 x 512 crops; FAMILIES as in tests/test_gpu_fullsize.py."""
import ctypes
import os

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = {'x3': dict(x3=True, wino=True, thin=True, h2=False), 'wino': dict(x3=False, wino=True, thin=True, h2=False),
            'direct': dict(x3=False, wino=False, thin=False, h2=False), 'h2': dict(x3=True, wino=True, thin=True, h2=True)}
WS = 37814272                  # backward-weight workspace floats of every training case below (UNet and ResUnet, B = 16 and 64)

# (arch, family, B, train, the family of most layers, the layers that differ): 'fwd/dgrad/wgrad', '-' = the pass does not run
CASES = [
    ('unet', 'h2', 16, True, 'h2/h2/h2', {
        'conv1_1': 'h2/-/thin',
        'conv1_2': 'h2+pool/h2/h2',
        'conv2_2': 'h2+pool/h2/h2',
        'conv3_2': 'h2+pool/h2/h2',
        'conv4_2': 'h2+pool/h2/h2',
        'conv9_2': 'h2+head/h2/h2',
        'conv10_1': 'fused/thin/thin'}),
    ('unet', 'x3', 16, True, 'x3/x3/x3', {
        'conv1_1': 'thin/-/thin',
        'conv1_2': 'x3+pool/x3/x3',
        'conv2_2': 'x3+pool/x3/x3',
        'conv3_2': 'x3+pool/x3/x3',
        'conv4_2': 'x3+pool/x3/x3',
        'conv10_1': 'thin/thin/thin'}),
    ('unet', 'wino', 16, True, 'wino/wino/wino', {
        'conv1_1': 'thin/-/thin',
        'conv1_2': 'direct/direct/direct',
        'conv2_1': 'wino/direct/direct',
        'upv6': 'direct/direct/direct',
        'upv7': 'direct/direct/direct',
        'upv8': 'direct/direct/direct',
        'upv9': 'direct/direct/direct',
        'conv9_1': 'direct/wino/direct',
        'conv9_2': 'direct/direct/direct',
        'conv10_1': 'thin/thin/thin'}),
    ('unet', 'direct', 16, True, 'direct/direct/direct', {
        'conv1_1': 'direct/-/direct'}),
    ('resunet', 'h2', 16, True, 'h2/h2/h2', {
        'conv_in': 'thin/-/thin',
        'b1_0': 'h2/h2+res/h2',
        'b2_0': 'h2/h2+res/h2',
        'b3_0': 'h2/h2+res/h2',
        'b4_0': 'h2/h2+res/h2',
        'b5_0': 'h2/h2+res/h2',
        'conv10': 'thin/thin/thin'}),
    ('resunet', 'x3', 16, True, 'x3/x3/x3', {
        'conv_in': 'thin/-/thin',
        'b1_0': 'x3/x3+res/x3',
        'pool1': 'x3/x3/direct',
        'b2_0': 'x3/x3+res/x3',
        'b3_0': 'x3/x3+res/x3',
        'b4_0': 'x3/x3+res/x3',
        'b5_0': 'x3/x3+res/x3',
        'sc9': 'x3/x3/direct',
        'conv10': 'thin/thin/thin'}),
    ('resunet', 'wino', 16, True, 'direct/direct/direct', {
        'conv_in': 'thin/-/thin',
        'b1_0': 'direct/direct+res/direct',
        'b2_0': 'wino/wino+res/wino',
        'b2_1': 'wino/wino/wino',
        'b3_0': 'wino/wino+res/wino',
        'b3_1': 'wino/wino/wino',
        'b4_0': 'wino/wino+res/wino',
        'b4_1': 'wino/wino/wino',
        'b5_0': 'wino/wino+res/wino',
        'b5_1': 'wino/wino/wino',
        'b6_0': 'wino/wino/wino',
        'b6_1': 'wino/wino/wino',
        'b7_0': 'wino/wino/wino',
        'b7_1': 'wino/wino/wino',
        'b8_0': 'wino/wino/wino',
        'b8_1': 'wino/wino/wino',
        'b9_0': 'direct/wino/direct',
        'conv10': 'thin/thin/thin'}),
    ('resunet', 'direct', 16, True, 'direct/direct/direct', {
        'conv_in': 'direct/-/direct',
        'b1_0': 'direct/direct+res/direct',
        'b2_0': 'direct/direct+res/direct',
        'b3_0': 'direct/direct+res/direct',
        'b4_0': 'direct/direct+res/direct',
        'b5_0': 'direct/direct+res/direct'}),
    ('unet', 'h2', 64, True, 'h2/h2/h2', {
        'conv1_1': 'h2/-/thin',
        'conv1_2': 'h2+pool/h2/direct',
        'conv2_2': 'h2+pool/h2/h2',
        'conv3_2': 'h2+pool/h2/h2',
        'conv4_2': 'h2+pool/h2/h2',
        'upv8': 'h2/h2/direct',
        'upv9': 'h2/h2/direct',
        'conv9_1': 'h2/h2/direct',
        'conv9_2': 'h2+head/h2/direct',
        'conv10_1': 'fused/thin/thin'}),
    ('unet', 'h2', 1, False, 'h2+splitk/-/-', {
        'conv1_1': 'h2/-/-',
        'conv1_2': 'h2+pool/-/-',
        'conv2_1': 'h2/-/-',
        'conv2_2': 'h2+pool/-/-',
        'upv6': 'h2/-/-',
        'upv7': 'h2/-/-',
        'upv8': 'h2/-/-',
        'conv8_1': 'h2/-/-',
        'conv8_2': 'h2/-/-',
        'upv9': 'h2/-/-',
        'conv9_1': 'h2/-/-',
        'conv9_2': 'h2+head/-/-',
        'conv10_1': 'fused/-/-'}),
]


@pytest.fixture(scope='module')
def plan_mod():
    so = os.path.join(REPO, 'pnnp_amd', 'libpnnp_hip.so')
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    if ctypes.CDLL(so).pnnp_device_cus() != 256:
        pytest.skip('the plan below is stated for 256 compute units')
    from pnnp_amd.archs import plan
    return plan


@pytest.mark.parametrize('arch,family,B,train,common,diff', CASES, ids=[f'{c[0]}-{c[1]}-B{c[2]}-{"train" if c[3] else "eval"}' for c in CASES])
def test_plan_matches_recorded_launches(plan_mod, arch, family, B, train, common, diff):
    """The plan the engine itself runs from (its policy set as the tests on the GPU set it)."""
    from pnnp_amd.archs import ResUnet, UNetSeeInDark
    net = (UNetSeeInDark if arch == 'unet' else ResUnet)(dict(nframes=1, res=False, nf=32, in_nc=4, out_nc=4))
    e = net.engine
    e.set_policy(**FAMILIES[family])
    p = e._plan_for(B, 512, 512, train)
    got = {k: '/'.join('-' if f is None else f for f in t) for k, t in p.table().items()}
    names = [f'conv{i}_{j}' for i in range(1, 10) for j in (1, 2)] + [f'upv{i}' for i in range(6, 10)] + ['conv10_1'] if arch == 'unet' else \
        ['conv_in', 'conv10'] + [f'b{i}_{j}' for i in range(1, 10) for j in (0, 1)] + [f'pool{i}' for i in range(1, 5)] + [f'{k}{i}' for i in range(6, 10) for k in ('upv', 'sc')]
    assert sorted(got) == sorted(names)
    assert got == {n: diff.get(n, common) for n in names}
    if train:
        assert p.ws == WS


def test_engines_share_the_plan():
    from pnnp_amd.archs import plan, resunet, unet
    assert unet.ConvPolicy is plan.ConvPolicy and unet.DEFAULT_POLICY is plan.DEFAULT_POLICY
    assert unet.resolve_unet is plan.resolve_unet and resunet.resolve_resunet is plan.resolve_resunet

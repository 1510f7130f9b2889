"""What tests/test_gpu_thin_f64.py covers, without a GPU.  Its case tables, read through the launch rules tests/_thin_ref.py restates, give every head kernel
(forward and backward, LPP = 4, 8, 16) a launch where no wave takes a second 64-pixel group, one where some waves of an uncapped grid do, and one where the
grid is capped and the shares are uneven; and every first-layer kernel (forward and weight gradient, Cout 32 and 64) a launch with a tile per workgroup and
one with more tiles than workgroups in uneven shares -- at 256 compute units and, the capped and many-tile shapes being functions of the count, at 64 and
304.  The float64 references are checked against F.conv2d and autograd on two tiny shapes, so that a wrong reference cannot pass on the GPU by agreeing with
a wrong kernel."""
import math

import pytest
import torch
import torch.nn.functional as F

import _thin_ref as R
from test_gpu_thin_f64 import FIRST_FWD_CASES, FIRST_WGRAD_CASES, HEAD_BWD_CASES, HEAD_FWD_CASES, resolve

CU_COUNTS = (256, 64, 304)
BUDGET = 400 << 20          # bytes of float32 a capped or many-tile case moves to and from the device (inputs and destinations of one launch)


def _head(cus):
    """(kernel, per_cu, name, (B, H, W), cin, cout, labelled class) of every head launch in the tables."""
    return ([('fwd', R.HEAD_FWD_PER_CU, c[0], resolve(c[1], cus, R.HEAD_FWD_PER_CU), c[2], c[3], c[4]) for c in HEAD_FWD_CASES] +
            [('bwd', R.HEAD_BWD_PER_CU, c[0], resolve(c[1], cus, R.HEAD_BWD_PER_CU), c[2], c[3], c[5]) for c in HEAD_BWD_CASES])


def _first(cus):
    return ([('fwd', c[0], resolve(c[1], cus, cout=c[3]), c[2], c[3], c[7]) for c in FIRST_FWD_CASES] +
            [('wgrad', c[0], resolve(c[1], cus, cout=c[3]), c[2], c[3], c[5]) for c in FIRST_WGRAD_CASES])


@pytest.mark.parametrize('cus', CU_COUNTS)
def test_the_head_tables_reach_every_class_with_every_lpp(cus):
    got, straddle, idle, cap_straddle = {}, set(), set(), set()
    for kern, per_cu, name, (B, H, W), cin, cout, cls in _head(cus):
        npix = B * H * W
        assert npix % 64 == 0 and R.head_lpp(cin) and 1 <= cout <= 4, name
        L = R.head_launch(npix, per_cu, cus)
        assert L['cls'] == cls, (kern, name, L)
        got.setdefault((kern, R.head_lpp(cin)), set()).add(cls)
        if (H * W) % 64:
            straddle.add(kern)
            if B >= 3 and cls != 'one':
                cap_straddle.add((kern, cls))
        if L['ngroups'] < 4:
            idle.add(kern)
        if cls == 'second':
            assert L['trips'] == 2 and L['blocks'] < per_cu * cus and L['ngroups'] <= 15, (name, L)
        if cls == 'capped':
            ratio = L['ngroups'] / (4 * per_cu * cus)
            assert L['blocks'] == per_cu * cus and R.WINDOW[0] <= ratio <= R.WINDOW[1] and L['trips'] == 2, (name, L, ratio)
            moved = 4 * npix * ((cin + 2 * cout) if kern == 'fwd' else (2 * cin + 8))
            assert moved <= BUDGET, (name, moved)
    assert set(got) == {(k, lpp) for k in ('fwd', 'bwd') for lpp in (4, 8, 16)}
    for key, classes in got.items():
        assert classes == {'one', 'second', 'capped'}, (key, classes)
    assert straddle == {'fwd', 'bwd'} and idle == {'fwd', 'bwd'}
    assert cap_straddle >= {('fwd', 'second'), ('fwd', 'capped'), ('bwd', 'second'), ('bwd', 'capped')}
    assert {c[3] for c in HEAD_FWD_CASES} == {1, 2, 3, 4} == {c[3] for c in HEAD_BWD_CASES}
    assert {c[4] for c in HEAD_BWD_CASES} == {0, 1, 2}
    assert {c[4] for c in HEAD_BWD_CASES if c[5] != 'one'} == {0, 1, 2}
    assert any(c[6] for c in HEAD_FWD_CASES) and any(c[7] for c in HEAD_BWD_CASES)
    for cls in ('one', 'second', 'capped'):
        assert {r for c in HEAD_FWD_CASES if c[4] == cls for r in c[5]} == {0, 1}, cls


@pytest.mark.parametrize('cus', CU_COUNTS)
def test_the_first_layer_tables_reach_both_classes_and_every_ragged_width(cus):
    got, nws = {}, {}
    for kern, name, (B, H, W), cin, cout, cls in _first(cus):
        assert H % (512 // cout) == 0 and W % 16 == 0 and 1 <= cin <= 4, name
        L = R.first_launch(B, H, W, cout, cus)
        assert L['cls'] == cls, (kern, name, L)
        got.setdefault((kern, cout), set()).add(cls)
        nws.setdefault(kern, set()).update(L['nws'])
        if cls == 'many':
            ratio = L['ntiles'] / (R.FW_PER_CU * cus)
            assert R.WINDOW[0] <= ratio <= R.WINDOW[1] and L['per_wg'] == 2 and B >= 2 and L['tiles_h'] >= 2 and L['tiles_w'] >= 2, (name, L, ratio)
            assert min(L['nws']) in (16, 32), name
            assert 4 * B * H * W * (8 + cout) <= BUDGET, name
    assert set(got) == {(k, co) for k in ('fwd', 'wgrad') for co in (32, 64)}
    for key, classes in got.items():
        assert classes == {'one', 'many'}, (key, classes)
    assert nws == {'fwd': {16, 32, 48}, 'wgrad': {16, 32, 48}}
    for table, kcls in ((FIRST_FWD_CASES, 7), (FIRST_WGRAD_CASES, 5)):
        small = [c for c in table if c[kcls] == 'one']
        assert {c[2] for c in small} == {1, 3, 4}
        assert any(R.first_launch(*c[1], c[3], cus)['ntiles'] == 1 for c in small)                       # a one-tile map: H = TR, W = 16
        assert any(c[1][0] > 1 and R.first_launch(*c[1], c[3], cus)['tiles_h'] > 1 and R.first_launch(*c[1], c[3], cus)['tiles_w'] > 1 for c in small)
    assert {c[4] for c in FIRST_FWD_CASES} == {0, 1, 2} and {c[5] for c in FIRST_FWD_CASES} == {0, 1}
    assert any(c[6] for c in FIRST_FWD_CASES) and any(c[4] for c in FIRST_WGRAD_CASES)
    assert {min(R.first_launch(*resolve(c[1], cus, cout=c[3]), c[3], cus)['nws']) for t, k in ((FIRST_FWD_CASES, 7), (FIRST_WGRAD_CASES, 5))
            for c in t if c[k] == 'many'} == {16, 32}


def test_launch_rules_on_known_values():
    assert [R.head_lpp(c) for c in (16, 32, 64, 24, 8, 128)] == [4, 8, 16, 0, 0, 0]
    assert R.thin_blocks(0, 8, 256) == 1 and R.thin_blocks(5, 8, 256) == 5 and R.thin_blocks(2048, 8, 256) == 2048 and R.thin_blocks(3000, 8, 256) == 2048
    # 320 pixels: 5 groups, one workgroup, its wave 0 takes groups 0 and 4
    assert R.head_launch(320, 8, 256) == dict(ngroups=5, blocks=1, waves=4, trips=2, cls='second')
    assert R.head_launch(64 * 8192, 8, 256)['cls'] == 'one' and R.head_launch(64 * 16384, 8, 256)['cls'] == 'even'
    assert R.head_launch(64 * 8193, 8, 256)['cls'] == 'capped' and R.head_launch(64 * 4097, 4, 256)['cls'] == 'capped'
    # the full-size training map: 16 crops of 512 x 512
    assert R.head_launch(16 * 512 * 512, 4, 256) == dict(ngroups=65536, blocks=1024, waves=4096, trips=16, cls='even')
    L = R.first_launch(16, 512, 512, 32, 256)
    assert (L['tr'], L['tiles_w'], L['tiles_h'], L['ntiles'], L['blocks'], L['nws']) == (16, 11, 32, 5632, 1536, {48, 32})
    assert R.first_launch(1, 8, 16, 64, 256)['ntiles'] == 1 and R.first_launch(1, 16, 64, 32, 256)['nws'] == {48, 16}
    assert R.head_bwd_workspace(576, 64, 256) == 2 * 260 and R.first_wgrad_workspace(2, 32, 80, 32, 256) == 8 * 37 * 32
    # depths: one trip of LPP additions, log2(64 / LPP) shuffles, 2 waves, one reduce step, 15 slices, the product
    assert R.head_bwd_depth(256, 16, 256) == 4 + 4 + 2 + 1 + 15 + 1 and R.head_bwd_depth(256, 64, 256, bias=True) == 16 + 2 + 2 + 1 + 15
    assert R.first_wgrad_depth(1, 16, 16, 32, 256) == 96 + 7 + 1 + 15 + 1 and R.first_wgrad_depth(16, 512, 512, 64, 256, bias=True) == 8 * 96 + 3 + 96 + 15
    for cus in CU_COUNTS:
        for per_cu in (4, 8):
            assert R.head_bwd_depth(math.prod(R.head_capped_shape(cus, per_cu, True)), 64, cus) < 400


def _r(*shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g) * 2 - 1


@pytest.mark.parametrize('shape', [(2, 5, 6), (1, 3, 4)])
def test_the_references_against_conv2d_and_autograd(shape):
    B, H, W = shape
    for cin, cout in ((16, 3), (32, 1)):
        x, w, b, r = _r(B, cin, H, W, seed=1), _r(cout, cin, 1, 1, seed=2), _r(cout, seed=3), _r(B, cout, H, W, seed=4)
        g = _r(B, cout, H, W, seed=5)
        ref = R.head_fwd(x, w, b, r)
        assert torch.allclose(ref.ref, F.conv2d(x.double(), w.double(), b.double()) + r.double(), rtol=1e-13, atol=1e-13)
        assert (ref.n, ref.e) == (cin, 2) and R.head_fwd(x, w, b).e == 1 and bool((ref.S >= ref.ref.abs()).all())
        for mode in (0, 1, 2):
            # gx: x is the OUTPUT of the activation before the head and has the sign of its input, so act applied to x has the derivative the kernel takes
            xd = x.double().requires_grad_(True)
            a = xd if mode == 0 else torch.where(xd > 0, xd, R.SLOPE * xd if mode == 1 else 0.0 * xd)
            F.conv2d(a, w.double(), b.double()).backward(g.double())
            rgx, rW, rb = R.head_bwd(g, x, w, mode)
            assert torch.allclose(rgx.ref, xd.grad, rtol=1e-13, atol=1e-13) and (rgx.n, rgx.e) == (4, int(mode == 1))
            # dW, db: of the head on x itself
            w2 = w.double().requires_grad_(True); b2 = b.double().requires_grad_(True)
            F.conv2d(x.double(), w2, b2).backward(g.double())
            assert torch.allclose(rW.ref, w2.grad, rtol=1e-13, atol=1e-13) and torch.allclose(rb.ref, b2.grad, rtol=1e-13, atol=1e-13)
            assert rW.n == rb.n == B * H * W and bool((rW.S >= rW.ref.abs()).all())
    for cin, cout in ((3, 5), (4, 2)):
        x, w, b, g = _r(B, cin, H, W, seed=6), _r(cout, cin, 3, 3, seed=7), _r(cout, seed=8), _r(B, cout, H, W, seed=9)
        for act in (0, 1, 2):
            z = F.conv2d(x.double(), w.double(), b.double(), padding=1)
            want = {0: z, 1: torch.where(z > 0, z, R.SLOPE * z), 2: F.relu(z)}[act]
            ref = R.first_fwd(x, w, b, act)
            assert torch.allclose(ref.ref, want, rtol=1e-13, atol=1e-13) and (ref.n, ref.e) == (36, 1 + (act == 1))
        assert R.first_fwd(x, w, None, 0).e == 0
        w2 = torch.zeros(cout, cin, 3, 3, dtype=torch.float64, requires_grad=True); b2 = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
        F.conv2d(x.double(), w2, b2, padding=1).backward(g.double())
        rW, rb = R.first_bwd_weight(g, x)
        assert torch.allclose(rW.ref, w2.grad, rtol=1e-13, atol=1e-13) and torch.allclose(rb.ref, b2.grad, rtol=1e-13, atol=1e-13)
        assert bool((rW.S >= rW.ref.abs()).all()) and rW.n == B * H * W
    # an inf of g at an interior pixel meets no padding zero in the einsum reference
    x, g = _r(1, 2, 5, 6, seed=10).abs() + 0.1, _r(1, 3, 5, 6, seed=11)
    g[0, 1, 2, 3] = float('inf')
    rW, rb = R.first_bwd_weight(g, x)
    assert bool(torch.isinf(rW.ref[1]).all()) and not torch.isnan(rW.ref).any() and int(torch.isinf(rW.ref).sum()) == 18 and rb.ref[1] == float('inf')

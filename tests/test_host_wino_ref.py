"""tests/_wino_ref.py checked without a GPU: its float64 Winograd equals the plain float64 operations; the float32 emulation of the kernels, on the inputs
of tests/test_gpu_wino_f64.py, stays inside the stated bounds (so the reference and the bound alone pass); the case tables of that file reach every class of
the two kernels, by the restated launch rules at 256 compute units and by the library's own workspace query; and the raw C entries refuse frames past their
32-bit limits before they touch a device."""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

import _direct_ref as R
import _wino_ref as W
import test_gpu_wino_f64 as T

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, E_INVALID, E_UNSUPPORTED, E_WORKSPACE = 0, -1, -2, -4


def _lib():
    so = os.path.join(REPO, 'pnnp_amd', 'libpnnp_hip.so')
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(so)
    lib.pnnp_wino_wgrad_workspace_floats.restype = ctypes.c_int64
    return lib


def test_float64_winograd_equals_the_plain_operations():
    x = T._rand(2, 24, 17, 31, seed=1); w = T._rand(64, 24, 3, 3, seed=3, scale=0.2); g = T._rand(2, 64, 17, 31, seed=5)
    assert float((W.wino_conv(x, w) - F.conv2d(x.double(), w.double(), padding=1)).abs().max()) < 1e-12
    assert float((W.wino_conv(g, W.dgrad_filter(w)) - F.conv_transpose2d(g.double(), w.double(), padding=1)).abs().max()) < 1e-12
    x = T._rand(3, 16, 12, 24, seed=1); g = T._rand(3, 8, 12, 24, seed=5)
    dW, _ = R._wgrad(lambda x, w, b: F.conv2d(x, w, b, padding=1), (8, 16, 3, 3), 8, x.double(), g.double())
    assert float((W.wino_wgrad(g, x) - dW).abs().max()) < 1e-12
    for shape in ((1, 1, 1), (1, 15, 17), (1, 33, 1)):
        x = T._rand(shape[0], 8, *shape[1:], seed=2); w = T._rand(64, 8, 3, 3, seed=3)
        assert float((W.wino_conv(x, w) - F.conv2d(x.double(), w.double(), padding=1)).abs().max()) < 1e-12


def _hold(what, got, ref, depth=None, direct=None):
    err = (got.double() - ref.ref).abs()
    ratio = float((err / (W.U * ref.S).clamp_min(1e-300)).max())
    extra = ''
    if direct is not None:
        extra = (f'  S_w / S_direct = {float((ref.S / direct.clamp_min(1e-300)).min()):.1f} .. {float((ref.S / direct.clamp_min(1e-300)).max()):.1f},'
                 f' err / (2^-24 S_direct) = {float((err / (W.U * direct).clamp_min(1e-300)).max()):.3f}')
    print(f'wino_ref | emulated {what}: worst err / (2^-24 S_w) = {ratio:.3f}  (bound {(ref.n + ref.e) * 1.01:.1f}' + (f', by depth {(depth + ref.e) * 1.01:.1f})' if depth else ')') + extra)
    assert bool((err <= W.bound(ref)).all()), (what, ratio)
    if depth:
        assert bool((err <= W.bound(ref._replace(n=depth))).all()), (what, ratio, depth)


@pytest.mark.parametrize('case', T.FWD_CASES, ids=[c[0] for c in T.FWD_CASES])
def test_emulated_forward_stays_inside_the_bound(case):
    name, (B, H, W_), C1, C2, Co, variants = case
    x1, x2, w, b, r = T.fwd_inputs(B, H, W_, C1, C2, Co)
    xin = torch.cat([x1, x2], 1) if C2 else x1
    core = W.emulate_core(xin, w)
    u, (uref, uS) = W.emulate_filter(w), W.filter_transform(w)
    assert bool(((u.double() - uref).abs() <= 4 * W.U * uS * 1.01).all())
    for act, use_b, use_r in variants:
        got = W.emulate_epilogue(core, b if use_b else None, r if use_r else None, act)
        _hold(f'fwd {name} act {act} bias {use_b} residual {use_r}', got, W.conv_fwd(xin, w, b if use_b else None, r if use_r else None, act),
              direct=R.conv_fwd(xin, w, b if use_b else None, r if use_r else None, act).S)


@pytest.mark.parametrize('case', T.BWD_CASES, ids=[c[0] for c in T.BWD_CASES])
def test_emulated_backward_data_stays_inside_the_bound(case):
    name, Co, C1, C2 = case
    w, g, m1, m2, base1, base2 = T.bwd_inputs(Co, C1, C2)
    core = W.emulate_core(g, w, dgrad=True)
    for mo1, ac1, mo2, ac2 in (T.TWO_DST if C2 else [(mo, ac, 0, 0) for mo, ac in T.ONE_DST]):
        got = W.emulate_epilogue(core[:, :C1], mask=m1 if mo1 else None, mode=mo1, base=base1 if ac1 else None)
        _hold(f'bwd_data {name} dx1 mode {mo1} accumulate {ac1}', got, W.conv_bwd_data(g, w, 0, C1, m1 if mo1 else None, mo1, base1 if ac1 else None),
              direct=R.conv_bwd_data(g, w, 0, C1, m1 if mo1 else None, mo1, base1 if ac1 else None).S)
        if C2:
            got = W.emulate_epilogue(core[:, C1:], mask=m2 if mo2 else None, mode=mo2, base=base2 if ac2 else None)
            _hold(f'bwd_data {name} dx2 mode {mo2} accumulate {ac2}', got, W.conv_bwd_data(g, w, C1, C1 + C2, m2 if mo2 else None, mo2, base2 if ac2 else None))


@pytest.mark.parametrize('case', T.RES_CASES, ids=[c[0] for c in T.RES_CASES])
def test_emulated_shortcut_stays_inside_the_bound(case):
    name, (B, H, W_), Co, C1, mode = case
    w, g, add, m = T.res_inputs(B, H, W_, Co, C1)
    got = W.emulate_epilogue(W.emulate_core(g, w, dgrad=True), residual=add, mask=m if mode else None, mode=mode)
    _hold(f'bwd_data_res {name}', got, W.conv_bwd_data(g, w, mask=m if mode else None, mode=mode, addsrc=add))


@pytest.mark.parametrize('name', T.WG_NAMES)
def test_emulated_weight_gradient_stays_inside_both_bounds(name):
    """The first 4 x 4 channels of dW (every element sums alone) and the whole bias gradient, plain and accumulated, at the splits of 256 compute units."""
    case = next(c for c in T.wg_cases(256) if c[0] == name)
    _, (B, H, W_), Co, C1, C2, gcs, xcs, *_ = case
    N = C1 + C2
    Z, per = W.ww_splits(B, H, W_, Co, N), W.ww_per(B, H, W_, Co, N)
    g, x1, x2 = T.wg_inputs(B, H, W_, Co, C1, C2, gcs, xcs)
    rW, dep_w, rb, dep_b = T.wg_refs(B, H, W_, Co, C1, C2, gcs, xcs, Z, per)
    ew, eb = W.emulate_bwd_weight(g[:, :Co], x1[:, :C1], Z, per)
    cut = lambda r: r._replace(ref=r.ref[:4, :4], S=r.S[:4, :4])
    sd = R.conv_bwd_weight(g[:, :4], x1[:, :4], 3, Z)[0].S
    _hold(f'bwd_weight {name} dW Z {Z} per {per}', ew, cut(rW), dep_w, direct=sd)
    _hold(f'bwd_weight {name} dbias', eb, rb, dep_b)
    base_w, base_b = T._rand(Co, N, 3, 3, seed=12, scale=10.0), T._rand(Co, seed=13, scale=10.0)
    _hold(f'bwd_weight {name} dW accumulated', base_w[:4, :4] + ew, cut(W.accumulated(rW, base_w)), dep_w)
    _hold(f'bwd_weight {name} dbias accumulated', base_b + eb, W.accumulated(rb, base_b), dep_b)


def test_case_tables_reach_every_class():
    depth = {W.depth_class(W.wino_grid(*c[1], c[2] + c[3], c[4])[3]) for c in T.FWD_CASES} | {W.depth_class(c[1] // 8) for c in T.BWD_CASES}
    assert depth == {1, 2, 3, 4, '5+'}, depth
    sw = {W.switch_class(c[2], c[3]) for c in T.FWD_CASES} - {None}
    assert sw == {1, 2, 3, '4+'}, sw
    assert sum(c[2] != c[3] for c in T.FWD_CASES if c[3]) >= 5                                     # the two sources' pixel strides differ
    assert {c[2] % 64 for c in T.BWD_CASES if c[3]} == {0, 32}                                     # a split between the two waves of a 64-column block
    grids = {W.wino_grid(*c[1], c[2] + c[3], c[4])[:3] for c in T.FWD_CASES}
    assert (1, 1, (1, 1)) in grids and (2, 1, (2, 1)) in grids and (1, 2, (2, 1)) in grids and (3, 2, (18, 2)) in grids and (2, 1, (2, 3)) in grids, grids
    lib = _lib()
    cus = lib.pnnp_device_cus()
    cases = T.wg_cases(256)
    for c in cases:
        T.wg_assert_class(c, 256)
    assert {c[7] for c in cases} == {'one', 'two', 'three', 'many'}
    assert any(c[8] for c in cases) and any(c[7] == 'many' and c[9] == 1 for c in cases)
    assert cases[5][1] == (3, 68, 136) and W.ww_splits(3, 68, 136, 64, 64) == 217 and W.ww_nloc(3, 68, 136, 64, 64)[-1] == 3
    for _, (B, H, W_), Co, C1, C2, *_ in T.wg_cases(cus):
        assert lib.pnnp_wino_wgrad_supported(H, W_, Co, C1, C2) == 1
        assert lib.pnnp_wino_wgrad_workspace_floats(B, H, W_, Co, C1 + C2) == W.ww_workspace_floats(B, H, W_, Co, C1 + C2, cus)
    for K, N in ((8, 64), (12, 64), (16, 32), (64, 192)):
        assert lib.pnnp_wino_supported(K, N) == int(W.wino_supported(K, N))
    largest = max(max(B * H * W_ * max(gcs, xcs + C2) for _, (B, H, W_), Co, C1, C2, gcs, xcs, *_ in cases), max(c[1][0] * c[1][1] * c[1][2] * 192 for c in T.FWD_CASES))
    assert largest * 4 < 10e6, largest


def test_raw_entries_refuse_frames_past_their_32_bit_limits():
    """Just past a limit: PNNP_E_UNSUPPORTED.  Just inside, with a misaligned destination: PNNP_E_INVALID -- the limit check let the frame through and the next check
    stopped it (the weight-gradient entry has no alignment check: there the next stop is PNNP_E_WORKSPACE for a workspace of 0 floats).  The limit refusals sit
    in front of every HIP call; the just-inside path of the weight-gradient entry asks pnnp_device_cus for the split count (hipGetDevice: 256 without a
    device) before it refuses the workspace.  Nothing is launched and no pointer is dereferenced."""
    lib = _lib()
    buf = torch.zeros(64)
    p = ctypes.c_void_p(buf.data_ptr()); off = ctypes.c_void_p(buf.data_ptr() + 4)
    assert buf.data_ptr() % 16 == 0
    i64 = ctypes.c_int64
    fwd = lambda y, C1, Co, H, W_: lib.pnnp_conv3x3_wino_fwd_f32(p, C1, None, 0, p, None, None, y, 1, H, W_, Co, 0, None)
    bwd = lambda dx, Co, C1, H, W_: lib.pnnp_conv3x3_wino_bwd_data_f32(p, Co, p, dx, C1, None, 0, 0, None, 0, None, 0, 0, 1, H, W_, None)
    bwd2 = lambda dx2, Co, C1, C2, H, W_: lib.pnnp_conv3x3_wino_bwd_data_f32(p, Co, p, p, C1, None, 0, 0, dx2, C2, None, 0, 0, 1, H, W_, None)
    res = lambda dx, Co, C1, H, W_: lib.pnnp_conv3x3_wino_bwd_data_res_f32(p, Co, p, dx, C1, p, None, 0, 1, H, W_, None)
    # destination 64 times the source: 8 -> 512 channels at 1024 x 1024 is 2^31 bytes per image of the destination, 2^25 of the source
    for fn in (fwd, bwd, res):
        assert fn(p, 8, 512, 1024, 1024) == E_UNSUPPORTED
        assert fn(off, 8, 512, 1024, 1023) == E_INVALID
        assert fn(p, 512, 64, 1024, 1024) == E_UNSUPPORTED                    # the source side, as before
        assert fn(off, 512, 64, 1024, 1023) == E_INVALID
    assert bwd2(p, 8, 32, 544, 1024, 1024) == E_UNSUPPORTED                  # the second destination alone: 480 x 4 x 2^20 < 2^31 <= 544 x 4 x 2^20
    assert bwd2(off, 8, 32, 480, 1024, 1024) == E_INVALID
    wg = lambda gcs, x1cs, x2cs, H, W_, ws=0: lib.pnnp_conv3x3_wino_bwd_weight_f32(p, gcs, 64, p, x1cs, 64, p if x2cs else None, x2cs, 64 if x2cs else 0, p, None,
                                                                                   1, H, W_, 0, p, i64(ws), None)
    # (H W + W + 1) cs 4 >= 2^31 although B H W cs = 2^29 < 2^31 elements
    assert wg(64, 64, 0, 2048, 4096) == E_UNSUPPORTED
    assert wg(64, 64, 0, 2044, 4096) == E_WORKSPACE
    assert (2044 * 4096 + 4097) * 64 * 4 < 2 ** 31 <= (2048 * 4096 + 4097) * 64 * 4
    for strides in ((128, 64, 0), (64, 128, 0), (64, 64, 128)):
        assert wg(*strides, 1024, 4096) == E_UNSUPPORTED, strides
        assert wg(*strides, 1020, 4096) == E_WORKSPACE, strides
    assert wg(64, 64, 0, 8, 16) == E_WORKSPACE                                  # (a small frame takes the same way)

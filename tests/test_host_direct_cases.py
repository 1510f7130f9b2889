"""What tests/test_gpu_direct_f64.py covers, without a GPU.  With 256 compute units its case tables reach every reachable instantiation of launch_taps
(csrc/conv_igemm.hip) and all four output-tile shapes of each weight-gradient geometry (csrc/wgrad.hip), each of them once with a single tile per workgroup and
once with two or more and uneven shares.  The rules are the ones tests/_direct_ref.py restates; if one of them or a shape changes, this tells that the tables
have stopped covering a class before anyone runs them on a card."""
import ctypes
import os

import pytest

import _direct_ref as R
from test_gpu_direct_f64 import (BWD_CASES, CONVT_CASES, FWD_CASES, RES_CASES, S2_CASES, WGRAD_CASES, bwd_launch, convt_launches, fwd_launch, res_launch,
                                 s2_launches)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUS = 256


def _igemm_launches():
    """(what, labelled instantiation or None, instantiation by the mirror, tiles, labelled class or None) of every implicit-GEMM launch in the tables."""
    out = []
    for c in FWD_CASES:
        out.append(('fwd ' + c[0], c[6], *fwd_launch(c), c[7]))
    for c in BWD_CASES:
        out.append(('bwd ' + c[0], c[6], *bwd_launch(c), c[7]))
    for c in RES_CASES:
        out.append(('res ' + c[0], c[5], *res_launch(c), c[6]))
    for table, fn in ((CONVT_CASES, convt_launches), (S2_CASES, s2_launches)):
        for c in table:
            f, b = fn(c)
            if f:
                out.append(('fwd ' + c[0], c[4], *f, None))
            out.append(('bwd ' + c[0], c[5], *b, c[6]))
    return out


def test_kc_32_is_never_picked():
    """launch_taps<1> has three `kc == 32` arms; pick_kc starts at 16 for one tap and caps at 16 for nine, so for every channel count a launch accepts
    (multiples of 8: pnnp_igemm_launch refuses the rest) and every N block it returns 8 or 16."""
    for taps in (9, 1):
        for bn in (32, 64, 128):
            for chan in range(8, 513, 8):
                kc = R.pick_kc(bn, chan, taps)
                assert kc in (8, 16) and chan % kc == 0, (taps, bn, chan, kc)
                assert kc == (16 if chan % 16 == 0 and not (taps == 9 and bn == 128) else 8)
    assert len(R.IGEMM_INSTANCES) == 11 and all(kc != 32 for _, kc, _ in R.IGEMM_INSTANCES)
    assert {R.igemm_inst(t, n, c) for t in (9, 1) for n in range(4, 513, 4) for c in range(8, 513, 8)} == R.IGEMM_INSTANCES


def test_the_tables_reach_every_instantiation_of_launch_taps_in_both_classes():
    got = {}
    for what, label, inst, tiles, cls in _igemm_launches():
        assert label == inst, what
        actual = R.igemm_class(tiles, CUS)
        assert actual in ('one', 'many') and (cls is None or cls == actual), (what, tiles, actual)
        got.setdefault(inst, set()).add(actual)
    assert set(got) == R.IGEMM_INSTANCES
    for inst, classes in got.items():
        assert classes == {'one', 'many'}, (inst, classes)


def test_the_small_forward_cases_are_ragged_and_cover_the_ragged_n_tiles():
    small = [c for c in FWD_CASES if c[7] == 'one']
    for name, taps, (B, H, W), C1, C2, Co, inst, *_ in small:
        assert H <= 34 and W <= 70 and W % 32 and H % R.igemm_th(inst[2]), name
    assert {4, 8, 16, 48, 96, 160} <= {c[5] for c in small}
    assert any(c[2][0] == 2 for c in small) and any(c[4] for c in small)
    for taps in (9, 1):
        assert {c[6][2] for c in small if c[1] == taps} == {32, 64, 128} and {c[6][1] for c in small if c[1] == taps} == {8, 16}
    # the four persistent shapes of the issue, 2244 tiles each
    for c in FWD_CASES:
        if c[7] == 'many':
            assert fwd_launch(c)[1] == 2244, c[0]


def test_the_shortcut_cases():
    """9 taps and 1 tap; no mask, modes 1 and 2; C = 32 and 64; a ragged map and the persistent shape."""
    small = {(c[1], c[3], c[4]) for c in RES_CASES if c[6] == 'one'}
    assert small == {(t, c, m) for t in (9, 1) for c in (32, 64) for m in (0, 1, 2)}
    for c in RES_CASES:
        (B, H, W), th = c[2], R.igemm_th(c[5][2])
        assert c[6] == 'many' or (W % 32 and H % th), c[0]
    assert {c[1] for c in RES_CASES if c[6] == 'many'} == {9, 1}


def test_the_weight_gradient_tables_reach_every_tile_shape_in_both_classes():
    got, two = {}, set()
    for name, taps, (B, H, W), M, N1, N2, shape, cls in WGRAD_CASES:
        N = N1 + N2
        assert R.pick_shape(M, N) == shape and R.wgrad_class(B, H, W, M, N, taps) == cls, name
        got.setdefault((taps, shape), set()).add(cls)
        if N2 and N1 % (64 if shape & 2 else 32):
            two.add(taps)
        if cls == 'many':
            assert R.wgrad_tiles(B, H, W, M, N, taps) > R.wgrad_splits(B, H, W, M, N, taps)
    assert set(got) == {(t, s) for t in (9, 1, 4, 18) for s in range(4)}
    for key, classes in got.items():
        assert classes == {'one', 'many'}, (key, classes)
    assert two == {9, 1}                                    # a two-tensor input whose boundary falls inside an N tile
    assert R.wgrad_splits(2, 34, 130, 128, 128, 9) == 128 and R.wgrad_tiles(2, 34, 130, 128, 128, 9) == 170


def test_wgrad_splits_mirror_equals_the_library():
    so = os.path.join(REPO, 'pnnp_amd', 'libpnnp_hip.so')
    try:
        lib = ctypes.CDLL(so)
    except OSError as e:
        pytest.skip(f'the library does not load here: {e}')
    for taps in (9, 1, 4, 18):
        for B, H, W in ((1, 1, 1), (1, 7, 45), (2, 34, 130), (2, 17, 130), (4, 66, 260), (16, 512, 512), (3, 33, 31)):
            for M in (4, 16, 32, 36, 64, 96, 128, 256, 512):
                for N in (4, 8, 32, 40, 64, 72, 128, 512, 1024):
                    assert lib.pnnp_wgrad_splits(B, H, W, M, N, taps) == R.wgrad_splits(B, H, W, M, N, taps), (B, H, W, M, N, taps)

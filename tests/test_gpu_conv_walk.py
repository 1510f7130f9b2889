"""The persistent tile walk of the 3x3 forward / backward-data kernels (csrc/conv_s_body.h: ONE text for the bf16x3 and the fp16x2 family, csrc/conv_x3s.hip and
csrc/conv_h2s.hip), op by op against torch float32 on the CPU at the bars of tests/test_gpu_conv.py::close: the plain forward (bias, LeakyReLU) and the plain
backward-data of shapes that set how many tiles a workgroup walks -- one, two, three, four or more, and uneven shares, so that the producers' look-ahead crosses
one and two tile boundaries -- with one, two and three (odd: the halo image parity and bf16x3's three-stage weight ring flip between tiles) chunks of K, on 32- and
on 64-column tiles.  tests/test_gpu_x3.py::CASES gives every workgroup one tile, tests/test_gpu_wide_tiles.py::WIDE_CASES at most two.

Tiles = ceil(W / 32) ceil(H / 16) B ceil(N / BN) on 256 compute units, workgroup i walking tiles i', i' + 256, ...; every case asserts its tile width through
ops.h2_tile_columns (one rule for both families, csrc/igemm.h) and the table itself is checked without a GPU by tests/test_host_conv_walk_cases.py.  Backward-data
runs the layer with Cin and Cout exchanged, so that it writes the N columns and walks the K chunks its row states: the same width, chunks and tiles."""
import functools

import pytest
import torch
import torch.nn.functional as F

from test_gpu_conv import close, nchw, nhwc, _rand

pytestmark = pytest.mark.gpu
LRELU = 1

# ((B, H, W, Cin, Cout), tile columns, chunks of K (Cin / 16; 0.5 = a half-empty chunk), tiles per workgroup on 256 compute units)
CASES = [
    ((8, 192, 256, 16, 32), 32, 1, {3}),           # 768 tiles: exactly 3; the look-ahead reaches two tiles on
    ((8, 160, 256, 8, 32), 32, 0.5, {2, 3}),       # 640
    ((4, 192, 256, 32, 32), 32, 2, {1, 2}),        # 384
    ((17, 120, 250, 48, 32), 32, 3, {4, 5}),       # 1088, a map that fills neither its last tile row nor its last tile column
    ((8, 192, 256, 16, 64), 64, 1, {3}),           # 768
    ((5, 120, 250, 32, 64), 64, 2, {1, 2}),        # 320, ragged
    ((8, 120, 250, 48, 64), 64, 3, {2}),           # 512, ragged
    ((3, 120, 250, 16, 128), 64, 1, {1, 2}),       # 384; two column tiles per pixel tile: the n0 carry of `advance`
    ((17, 120, 250, 16, 64), 64, 1, {4, 5}),       # 1088, ragged: four and five tiles per workgroup on the wide tiles too
]
IDS = ['x'.join(map(str, c[0])) for c in CASES]


def _columns(B, H, W, N, cus=256):
    """pnnp_conv3_tile_columns (csrc/igemm.h) without the pooled forward: 64 unless the layer is narrower or 64-column tiles would fill under 3/4 of the chip."""
    if N < 64:
        return 32
    return 64 if ((W + 31) // 32) * ((H + 15) // 16) * B * ((N + 63) // 64) * 4 >= cus * 3 else 32


def _per_workgroup(B, H, W, N, cus=256):
    """The set of tile counts of a launch's workgroups: min(tiles, cus) workgroups share the tiles round-robin (pnnp_persistent_grid, csrc/common.h)."""
    bn = _columns(B, H, W, N, cus)
    tiles = ((W + 31) // 32) * ((H + 15) // 16) * B * ((N + bn - 1) // bn)
    g = min(tiles, cus)
    return {tiles // g, (tiles + g - 1) // g}


def _assert_width(B, H, W, N, columns):
    from pnnp_amd import ops
    assert ops.h2_tile_columns(B, H, W, N, False) == columns, (B, H, W, N, columns)


@functools.lru_cache(maxsize=None)
def _fwd_data(shape):
    """Inputs of the forward case and LeakyReLU(conv2d(x, w, b)) in float32 on the CPU (shared by both families, left unchanged)."""
    B, H, W, Ci, Co = shape
    x = _rand(B, Ci, H, W, seed=1); w = _rand(Co, Ci, 3, 3, seed=3, scale=0.2); b = _rand(Co, seed=4)
    return x, w, b, F.leaky_relu(F.conv2d(x, w, b, padding=1), 0.2)


@functools.lru_cache(maxsize=None)
def _bwd_data(shape):
    """The layer with the case's Cin and Cout exchanged: its weights [Cin][Cout][3][3], a gradient with Cin channels and autograd's d/d(input) (Cout channels)."""
    B, H, W, Ci, Co = shape
    w = _rand(Ci, Co, 3, 3, seed=3, scale=0.2)
    g = _rand(B, Ci, H, W, seed=5)
    xin = _rand(B, Co, H, W, seed=6).requires_grad_(True)
    F.conv2d(xin, w, None, padding=1).backward(g)
    return w, g, xin.grad


@pytest.mark.parametrize('family', ['x3', 'h2'])
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_conv_walk_fwd(case, family):
    from pnnp_amd import ops
    (B, H, W, Ci, Co), columns, _, _ = case
    _assert_width(B, H, W, Co, columns)
    x, w, b, ref = _fwd_data(case[0])
    xc = nhwc(x).cuda()
    y = torch.full((B, H, W, Co), float('nan'), device='cuda')
    if family == 'x3':
        from test_gpu_x3 import _packs
        f, _ = _packs(w.cuda(), dgrad=False)
        ops.conv_x3_fwd(xc, None, f, b.cuda(), y, Co, LRELU)
    else:
        from test_gpu_h2 import _packs, _slot
        f, _, sw = _packs(w.cuda(), dgrad=False)
        ops.conv_h2_fwd(xc, None, f, sw, b.cuda(), y, Co, LRELU, _slot(xc))
    close(nchw(y), ref, what=f'{family} fwd {case[0]}')


@pytest.mark.parametrize('family', ['x3', 'h2'])
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_conv_walk_bwd_data(case, family):
    from pnnp_amd import ops
    (B, H, W, Ci, Co), columns, _, _ = case
    _assert_width(B, H, W, Co, columns)                                  # (the launch writes the exchanged layer's input channels: N = Co)
    w, g, ref = _bwd_data(case[0])
    gc = nhwc(g).cuda()
    dx = torch.full((B, H, W, Co), float('nan'), device='cuda')
    if family == 'x3':
        from test_gpu_x3 import _packs
        _, d = _packs(w.cuda(), fwd=False)
        ops.conv_x3_bwd_data(gc, d, dx)
    else:
        from test_gpu_h2 import _packs, _slot
        _, d, sw = _packs(w.cuda(), fwd=False)
        ops.conv_h2_bwd_data(gc, _slot(gc), d, sw, dx)
    close(nchw(dx), ref, what=f'{family} dgrad {case[0]}')

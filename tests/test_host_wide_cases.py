"""Why tests/test_gpu_wide_tiles.py exists, without a GPU: the tile width of the fp16x2 / bf16x3 3x3 kernels is a host function of the launch's shape
(pnnp_h2_tile_columns; csrc/conv_x3s.hip asks the same helper, csrc/igemm.h), and the benchmark's layers resolve to 64 columns while the shape list the
reference tests share (tests/test_gpu_x3.py::CASES) resolves to 32.  If the width rule changes, this file tells which reference tests have stopped
covering the instantiation the benchmark runs."""
import ctypes
import os

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CH = [32, 64, 128, 256, 512]


@pytest.fixture(scope='module')
def tc():
    so = os.path.join(REPO, 'pnnp_amd', 'libpnnp_hip.so')
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    if ctypes.CDLL(so).pnnp_device_cus() != 256:
        pytest.skip('the widths below are stated for 256 compute units')
    from pnnp_amd import ops
    return ops.h2_tile_columns


def _policy():
    from pnnp_amd.archs import plan
    return plan.ConvPolicy()


def test_benchmark_layers_resolve_to_64_columns(tc):
    """UNet nf = 32 at B = 16 and ResUnet at B = 12, 512 x 512 crops, a training step: every 3x3 launch of an fp16x2 layer that writes 64 or more channels
    runs on 64-column tiles -- forward (N = the layer's output channels; the pooled forward by its own rule) and backward-data (N = the channels one launch
    writes: a decoder layer's cat([up, skip]) gradient is one launch of 2 c columns, or two column ranges of c where the skip half carries MaxPool2d's
    backward).  The one exception is stated: UNet's conv5_1 backward-data writes 256 channels on 32 x 32 maps, 128 tiles, below the threshold of 192."""
    from pnnp_amd.archs import plan
    B, S = 16, 512
    p = plan.resolve_unet(CH, 4, 4, _policy(), True, B, S, S)
    wide, narrow = [], []
    for i in range(1, 10):
        lvl = i - 1 if i <= 5 else 9 - i
        c, s = CH[lvl], S >> lvl
        for j in (1, 2):
            st = p[f'conv{i}_{j}']
            assert st.fwd.startswith('h2') and (st.dgrad == 'h2' or (i, j) == (1, 1))
            if c >= 64:
                assert st.fwd in ('h2', 'h2+pool')
                assert tc(B, s, s, c, st.fwd == 'h2+pool') == 64, (i, j, 'forward')
                wide.append(f'conv{i}_{j}')
            if j == 2 or i <= 5:
                written = [c if j == 2 else (0 if i == 1 else CH[lvl - 1])]
            else:
                written = [c, c] if st.unpool else [2 * c]
            for n in written:
                if n >= 64:
                    (wide if tc(B, s, s, n) == 64 else narrow).append(f'conv{i}_{j} dgrad')
    # 14 forwards (conv2_1 .. conv8_2); backward-data: conv{2..8}_2, conv3_1, conv4_1 and two column ranges each of conv{6,7,8}_1
    assert len(wide) == 14 + 15 and narrow == ['conv5_1 dgrad']
    assert tc(B, S >> 4, S >> 4, 256) == 32                                     # (128 tiles)
    B = 12
    p = plan.resolve_resunet(CH, 4, 4, _policy(), True, B, S, S)
    n_checked = 0
    for i in range(1, 10):
        lv = i - 1 if i <= 5 else 9 - i
        c, s = CH[lv], S >> lv
        for j in (0, 1):
            st = p[f'b{i}_{j}']
            assert st.fwd == 'h2' and st.dgrad in ('h2', 'h2+res')
            written = 2 * c if (j == 0 and i >= 6) else c
            if c >= 64:
                assert tc(B, s, s, c) == 64, (i, j, 'forward')
                n_checked += 1
            if written >= 64:
                assert tc(B, s, s, written) == 64, (i, j, 'backward-data')
                n_checked += 1
    assert n_checked == 14 + 15                                                  # (b9_0's backward-data writes 32 + 32 = 64 columns)
    lv = 4                                                                       # level 5 at B = 12 clears the threshold exactly: 1 x 2 x 12 x 8 = 192 tiles
    assert tc(B, S >> lv, S >> lv, 512) == 64 and tc(B - 1, S >> lv, S >> lv, 512) == 32


def test_wide_cases_are_wide_and_the_shared_cases_are_narrow(tc):
    from test_gpu_wide_tiles import UNPOOL_CASES, WIDE_CASES
    from test_gpu_x3 import CASES
    for B, H, W, C1, C2, Co in WIDE_CASES:
        assert tc(B, H, W, Co) == 64 and tc(B, H, W, Co, True) == 64 and tc(B, H, W, C1 + C2) == 64, (B, H, W, C1, C2, Co)
        assert H % 2 == 0 and W % 2 == 0
    for B, H, W, Cg, C in UNPOOL_CASES:
        assert tc(B, H, W, C) == 64
    tiles = lambda B, H, W, N: ((W + 31) // 32) * ((H + 15) // 16) * B * ((N + 63) // 64)
    assert min(tiles(B, H, W, Co) for B, H, W, C1, C2, Co in WIDE_CASES) == 192 and max(tiles(B, H, W, Co) for B, H, W, C1, C2, Co in WIDE_CASES) >= 512
    assert any(W % 32 and H % 16 for B, H, W, *_ in WIDE_CASES)
    for B, H, W, C1, C2, Co in CASES:
        assert tc(B, H, W, Co) == 32 and tc(B, H, W, C1 + C2) == 32, (B, H, W, C1, C2, Co)

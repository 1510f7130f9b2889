"""Every instantiation of the 3x3 weight-gradient kernel (csrc/wgrad_s.h: four output tiles on the bf16x3 scheme, csrc/wgrad_x3s.hip, and four on the fp16x2
scheme, csrc/wgrad_h2s.hip), op by op against the float64 sums of tests/test_gpu_x3.py::_f64_wgrad, at shapes that PICK each tile and set how many pixel tiles a
workgroup walks: one (no loop), two (no rolling iteration of the producers), three, four (rolling iterations) and uneven shares (some workgroups one tile more than
others).  One output tile per case, so a case has one slab per compute unit and its batch and map set the pixel tiles per workgroup.  The dispatch rule, the two
tile-height rules and the pixel-split rule are restated below; every case asserts the instantiation it is labelled with (tests/test_host_wgrad_cases.py checks the
table itself, without a GPU).

Bars: relative L2 < 2e-6 and a bias error below 1e-5 of the largest column sum of |g| -- those of tests/test_gpu_h2.py::test_h2_bwd_weight_tiles_per_workgroup,
for both schemes: on these cases the bf16x3 kernel as it was before the two shared one source measured at most 2.39e-7 relative L2 and 7.9e-9 of that column sum
(256 compute units; fp16x2: 1.84e-7 / 7.9e-9), so it needs no bar of its own."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

E_DW, E_BIAS = 2e-6, 1e-5


def _tile(Co, Ci):
    """pnnp_wx3s_launch / pnnp_wh2s_launch: the output tile (M = Cout, N = Cin) by the channel counts alone."""
    return (64 if Co % 64 == 0 else 32, 64 if Ci % 64 == 0 else 32)


TH = {'x3': {(64, 64): 2, (64, 32): 3, (32, 64): 2, (32, 32): 4},      # pnnp_wx3s_th: what the LDS holds twice at three planes per operand
      'h2': {(64, 64): 2, (64, 32): 3, (32, 64): 3, (32, 32): 4}}      # pnnp_wh2s_th: two planes leave the 32 x 64 tile a third row


def _inst(scheme, Co, Ci):
    """wgrad_s_kernel<Scheme, MO, NO, TH, MW> of a launch: fp16x2's 64 x 64 tile has one consumer wave own both 32-row blocks (MW = 2)."""
    t = _tile(Co, Ci)
    return (t[0] // 32, t[1] // 32, TH[scheme][t], 2 if (scheme == 'h2' and t == (64, 64)) else 1)


def _per_workgroup(scheme, B, H, W, Co, Ci, cus, share=1):
    """wx3_splits: Z workgroups per output tile, at most one per pixel tile; workgroup z walks tiles z, z + Z, ...  -> the set of tile counts."""
    t = _tile(Co, Ci)
    tiles = ((W + 31) // 32) * ((H + TH[scheme][t] - 1) // TH[scheme][t]) * B
    out_tiles = (Co // t[0]) * (Ci // t[1])
    z = max(1, min((cus * share + out_tiles - 1) // out_tiles, tiles))
    return {tiles // z, (tiles + z - 1) // z}


def _classes(counts):
    c = {'1' if n == 1 else '2' if n == 2 else '3' if n == 3 else '4+' for n in counts}
    return c | ({'uneven'} if len(counts) > 1 else set())


# (name, schemes, (B, H, W), (Cout, C1, C2), {scheme: instantiation}, pixel tiles per workgroup on 256 compute units)
X3, H2, BOTH = ('x3',), ('h2',), ('x3', 'h2')
CASES = [
    ('64x64 one tile, ragged map', BOTH, (1, 37, 70), (64, 64, 0), {'x3': (2, 2, 2, 1), 'h2': (2, 2, 2, 2)}, {1}),             # 3 x 19 = 57 pixel tiles
    ('64x64 two tiles', BOTH, (4, 64, 128), (64, 64, 0), {'x3': (2, 2, 2, 1), 'h2': (2, 2, 2, 2)}, {2}),                        # 4 x 32 x 4 = 512
    ('64x64 three and four tiles, two tensors', BOTH, (7, 64, 128), (64, 32, 32), {'x3': (2, 2, 2, 1), 'h2': (2, 2, 2, 2)}, {3, 4}),   # 896; n_split = 32 inside the N tile
    ('64x32 one tile', BOTH, (2, 30, 64), (64, 32, 0), {'x3': (2, 1, 3, 1), 'h2': (2, 1, 3, 1)}, {1}),                          # 2 x 10 x 2 = 40
    ('64x32 two tiles', BOTH, (8, 48, 128), (64, 32, 0), {'x3': (2, 1, 3, 1), 'h2': (2, 1, 3, 1)}, {2}),                        # 4 x 16 x 8 = 512
    ('64x32 three and four tiles, ragged map', BOTH, (10, 64, 120), (64, 32, 0), {'x3': (2, 1, 3, 1), 'h2': (2, 1, 3, 1)}, {3, 4}),    # 4 x 22 x 10 = 880
    ('32x64 one tile', BOTH, (1, 64, 128), (32, 64, 0), {'x3': (1, 2, 2, 1), 'h2': (1, 2, 3, 1)}, {1}),                         # 128 / 88
    ('32x64 two tiles of 2 rows', X3, (4, 64, 128), (32, 64, 0), {'x3': (1, 2, 2, 1)}, {2}),
    ('32x64 two tiles of 3 rows', H2, (8, 48, 128), (32, 64, 0), {'h2': (1, 2, 3, 1)}, {2}),
    ('32x64 three and four tiles of 2 rows, two tensors', X3, (7, 64, 128), (32, 32, 32), {'x3': (1, 2, 2, 1)}, {3, 4}),
    ('32x64 three and four tiles of 3 rows, two tensors', H2, (10, 64, 128), (32, 32, 32), {'h2': (1, 2, 3, 1)}, {3, 4}),
    ('32x32 one tile', BOTH, (1, 64, 128), (32, 32, 0), {'x3': (1, 1, 4, 1), 'h2': (1, 1, 4, 1)}, {1}),                         # 4 x 16 = 64
    ('32x32 two tiles', BOTH, (8, 64, 128), (32, 32, 0), {'x3': (1, 1, 4, 1), 'h2': (1, 1, 4, 1)}, {2}),                        # 512
    ('32x32 three and four tiles, ragged map', BOTH, (14, 62, 100), (32, 32, 0), {'x3': (1, 1, 4, 1), 'h2': (1, 1, 4, 1)}, {3, 4}),    # 4 x 16 x 14 = 896
]
RUNS = [(s, c) for c in CASES for s in c[1]]


@functools.lru_cache(maxsize=1)
def _data(name):
    """Inputs and float64 references of a case, shared by its two schemes."""
    from test_gpu_x3 import _f64_wgrad
    (B, H, W), (Co, C1, C2) = next((c[2], c[3]) for c in CASES if c[0] == name)
    gen = torch.Generator(device='cuda').manual_seed(sum(map(ord, name)))
    g = torch.randn(B, H, W, Co, device='cuda', generator=gen)
    x1 = torch.randn(B, H, W, C1, device='cuda', generator=gen)
    x2 = torch.randn(B, H, W, C2, device='cuda', generator=gen) * 3 if C2 else None
    ref = _f64_wgrad(g, torch.cat([x1, x2], 3) if C2 else x1)
    return g, x1, x2, ref, g.double().sum((0, 1, 2)), float(g.double().abs().sum((0, 1, 2)).max())


def _slot(t):
    from pnnp_amd import ops
    return ops.amax(t, torch.zeros(1, dtype=torch.int32, device='cuda'))


@pytest.mark.parametrize('scheme,case', RUNS, ids=[f'{s} {c[0]}' for s, c in RUNS])
def test_wgrad_instantiation_vs_float64(scheme, case):
    from pnnp_amd import _lib, ops
    name, _, (B, H, W), (Co, C1, C2), inst, _ = case
    assert _inst(scheme, Co, C1 + C2) == inst[scheme], name
    counts = _per_workgroup(scheme, B, H, W, Co, C1 + C2, _lib.lib().pnnp_device_cus())
    g, x1, x2, ref, bref, bscale = _data(name)
    ws = torch.full((ops.x3_wgrad_workspace_floats(B, H, W, Co, C1 + C2),), float('nan'), device='cuda')
    if scheme == 'x3':
        run = lambda dW, db, acc=0: ops.conv_x3_bwd_weight(g, Co, x1, C1, x2, dW, db, ws, accumulate=acc)
    else:
        sg, s1, s2 = _slot(g), _slot(x1), _slot(x2) if C2 else None
        run = lambda dW, db, acc=0: ops.conv_h2_bwd_weight(g, sg, Co, x1, s1, C1, x2, s2, dW, db, ws, accumulate=acc)
    nan = lambda *s: torch.full(s, float('nan'), device='cuda')
    rel = lambda d, r: float((d.double() - r).norm() / r.norm())
    dW, db = nan(Co, C1 + C2, 3, 3), nan(Co)
    run(dW, db)
    first, e, eb = dW.clone(), rel(dW, ref), float((db.double() - bref).abs().max()) / bscale
    run(dW, db, 1)                                                  # a second call accumulates
    e2, eb2 = rel(dW, 2 * ref), float((db.double() - 2 * bref).abs().max()) / (2 * bscale)
    dW3 = nan(Co, C1 + C2, 3, 3)
    run(dW3, None)                                                  # no bias gradient asked for
    e3 = rel(dW3, ref)
    print(f'{name} [{scheme} <{",".join(map(str, inst[scheme]))}>, pixel tiles per workgroup {sorted(counts)}]: rel L2 vs float64 {e:.2e}, accumulated {e2:.2e}, '
          f'without dbias {e3:.2e} (bar {E_DW:.0e}); bias / largest column sum of |g| {eb:.2e}, accumulated {eb2:.2e} (bar {E_BIAS:.0e})')
    assert e < E_DW and e2 < E_DW and e3 < E_DW, (name, scheme, e, e2, e3)
    assert eb < E_BIAS and eb2 < E_BIAS, (name, scheme, eb, eb2)
    assert torch.equal(dW, 2 * first) and torch.equal(dW3, first), (name, scheme)      # the slabs are summed in a fixed order: the same bits every call

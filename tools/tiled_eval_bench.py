"""Tiled full-frame inference (pnnp_amd/tiles.py, evaluate.forward_tiled; csrc/tiles.hip) on the SID frame:

    python tools/tiled_eval_bench.py [--out profiles/r7/tiled_eval.txt] [--reps 15] [--inner 20]

Workload: one frame 4x1424x2128 (the SonyA7S2 eval frame), patch_size 512, base 64 -> 4 x 5 = 20 tiles, UNetSeeInDark nf = 32.
Everything is timed in ONE process with device events around back-to-back calls, the forms of a comparison alternated round by round
after warm-up rounds; per call: median [min .. max] over the rounds, so the run-to-run spread stands beside every figure.

  (a) the two gather kernels alone against a plain ``copy_`` of the same bytes.  Traffic is counted from the shapes: the crop reads the
      frame once (the overlap is re-read from cache) and writes the tiles; the merge reads the interiors and writes the frame once.
  (b) ``forward_tiled`` against the composition a user could write before it existed, all on the device: F.pad(reflect), one slice copy
      and one net() call per tile, one slice write per tile (in the reference's write order).
  (c) the whole-frame ``evaluate`` and ``evaluate(tiles=...)`` on the same frame, for context: tiling does (P / l)^2 = 1.31 x the
      convolution work.
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch
import torch.nn.functional as F

from pnnp_amd import ops, tiles
from pnnp_amd.archs import UNetSeeInDark, initialize_weights
from pnnp_amd.evaluate import evaluate, forward_tiled

H, W, P, BASE = 1424, 2128, 512, 64


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / inner            # us per call


def rounds(forms, reps, inner, warm=3):
    """{name: [us per call per round]}: the forms alternate inside every round"""
    out = {k: [] for k in forms}
    for r in range(warm + reps):
        for k, fn in forms.items():
            t = timed(fn, inner)
            if r >= warm:
                out[k].append(t)
    return out


def stat(v):
    return f'{np.median(v):10.1f} us [{min(v):.1f} .. {max(v):.1f}]'


def by_hand(net, x, grid):
    """the reference's eval_crop / per-tile net / eval_merge as device tensor ops (syn_datasets.py:109-159, trainer_SID.py:351-357)"""
    d, l, p, nh, nw = grid.d, grid.l, grid.patch_size, grid.nh, grid.nw
    pad = F.pad(x, (d, d, d, d), mode='reflect')
    out = torch.empty_like(x)
    rows = [slice(i * l, i * l + p) for i in range(nh - 1)] + [slice(pad.shape[2] - p, pad.shape[2])]
    cols = [slice(j * l, j * l + p) for j in range(nw - 1)] + [slice(pad.shape[3] - p, pad.shape[3])]
    drow = [slice(i * l, i * l + l) for i in range(nh - 1)] + [slice(grid.h - l, grid.h)]
    dcol = [slice(j * l, j * l + l) for j in range(nw - 1)] + [slice(grid.w - l, grid.w)]
    order = [(i, j) for i in range(nh - 1) for j in range(nw - 1)] + [(i, nw - 1) for i in range(nh - 1)] + [(nh - 1, j) for j in range(nw - 1)] + [(nh - 1, nw - 1)]
    for i, j in order:
        y = net(pad[..., rows[i], cols[j]].contiguous())
        out[..., drow[i], dcol[j]] = y[..., d:-d, d:-d]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'r7', 'tiled_eval.txt'))
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--inner', type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tiled_eval_bench needs the GPU: nothing here is measured without one')
    torch.manual_seed(0)
    net = UNetSeeInDark(dict(nframes=1, res=False, nf=32, in_nc=4, out_nc=4)); initialize_weights(net); net = net.cuda().eval()
    g = torch.Generator(device='cuda').manual_seed(1)
    hr = torch.rand(1, 4, H, W, device='cuda', generator=g)
    x = (hr + 0.02 * torch.randn(1, 4, H, W, device='cuda', generator=g)).clamp(0, 1)
    grid = tiles.TileGrid(H, W, P, BASE, network=True)
    T, l = grid.T, grid.l
    L = [f'tiled inference on {torch.cuda.get_device_name(0)}: frame 4x{H}x{W}, patch_size {P}, base {BASE}: {grid.nh} x {grid.nw} = {T} tiles, UNetSeeInDark nf = 32',
         f'per call, median [min .. max] over {a.reps} rounds, the forms of a block alternated inside every round; device events', '']

    # ---- (a) the kernels alone
    nchw = torch.empty(T, 4, P, P, device='cuda'); nhwc = torch.empty(T, P, P, 8, device='cuda')
    slot = torch.zeros(1, dtype=torch.int32, device='cuda')
    frame = torch.empty_like(x)
    src_c, dst_c = torch.empty(T * 4 * P * P, device='cuda'), torch.empty(T * 4 * P * P, device='cuda')
    fb = 4 * H * W * 4
    cases = {
        'crop -> NCHW tiles (eval_crop)': (lambda: ops.tile_crop(x, grid, 0, T, nchw=nchw), fb + nchw.numel() * 4),
        'crop -> engine layout [T,P,P,8] + amax': (lambda: ops.tile_crop(x, grid, 0, T, nhwc=nhwc, amax=slot), fb + nhwc.numel() * 4),
        'merge (eval_merge)': (lambda: ops.tile_merge(nchw, frame, grid, 0, T), 2 * fb),
        'merge with x ratio and clamp': (lambda: ops.tile_merge(nchw, frame, grid, 0, T, ratio=2.0, clamp=True), 2 * fb),
    }
    L.append('(a) the gather kernels alone, each beside a plain copy_ of as many bytes as it moves (read + written)')
    for name, (fn, nbytes) in cases.items():
        n = nbytes // 8                                   # a copy_ of n floats moves 8 n bytes
        res = rounds({'kernel': fn, 'copy': lambda: dst_c[:n].copy_(src_c[:n])}, a.reps, 10 * a.inner)
        k, c = np.median(res['kernel']), np.median(res['copy'])
        L.append(f'  {name:42s} {nbytes / 1e6:7.1f} MB  kernel {stat(res["kernel"])} = {nbytes / k / 1e6:6.2f} TB/s   copy_ {stat(res["copy"])} = {nbytes / c / 1e6:6.2f} TB/s   kernel / copy time {k / c:.2f}')
    L.append("  (a copy_ of 50-110 MB per array runs out of the Infinity Cache on this chip; the gathers also pay index arithmetic per row, reflected groups at the frame's edges and,\n   into the engine layout, 4-byte loads from four channel planes per 16-byte store)")
    L.append('')

    # ---- (b) forward_tiled against the hand-written composition
    with torch.no_grad():
        ref = by_hand(net, x, grid)
        got = forward_tiled(net, x, P, BASE)
    L.append(f'(b) forward_tiled against the composition by hand (F.pad, {T} slice copies, {T} net() calls, {T} slice writes)')
    L.append(f'  outputs: max |difference| {float((got - ref).abs().max()):.3e} (max |value| {float(ref.abs().max()):.3e}): the batch size selects other kernels per layer (plan.py)')

    def hand():
        with torch.no_grad():
            by_hand(net, x, grid)
    forms = {'by hand': hand, 'forward_tiled, one batch': lambda: forward_tiled(net, x, P, BASE),
             'forward_tiled, tile_batch 4': lambda: forward_tiled(net, x, P, BASE, tile_batch=4)}
    res = rounds(forms, a.reps, max(1, a.inner // 5))
    for k, v in res.items():
        L.append(f'  {k:32s} {stat(v)}')
    hm = np.median(res['by hand'])
    L.append(f'  speed-up over the composition by hand: one batch {hm / np.median(res["forward_tiled, one batch"]):.2f} x, tile_batch 4 {hm / np.median(res["forward_tiled, tile_batch 4"]):.2f} x '
             f'(spread of the by-hand rounds: {100 * (max(res["by hand"]) - min(res["by hand"])) / hm:.1f} % of their median)')
    L.append('')

    # ---- (c) whole-frame evaluate for context
    tl = dict(patch_size=P, base=BASE)
    res = rounds({'whole frame': lambda: evaluate(net, x, hr), 'tiles': lambda: evaluate(net, x, hr, tiles=tl)}, a.reps, max(1, a.inner // 5))
    L.append(f'(c) evaluate on the whole frame and in tiles (network + tail + IlluminanceCorrect + PSNR / SSIM); convolution work x {(P / l) ** 2:.2f} in tiles')
    for k, v in res.items():
        L.append(f'  {k:32s} {stat(v)}')
    L.append(f'  tiles / whole frame: {np.median(res["tiles"]) / np.median(res["whole frame"]):.2f} x')
    text = '\n'.join(L) + '\n'
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()

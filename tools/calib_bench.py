"""The dark-frame calibration passes (csrc/calib.hip) against a plain copy and against the same results from torch ops:

    python tools/calib_bench.py [--out profiles/r7/calib.txt] [--frames 64] [--chunk 16] [--h 2848] [--w 4256] [--reps 7] [--no-fit]

Stack: ``frames`` dark frames of h x w uint16 (bl 512, Gaussian read noise and row noise, rounded), held on the device in chunks of
``chunk``.  Timed in ONE process with device events around a walk over all chunks, alternated round by round after warm-up rounds; us per
chunk, median [min .. max]:
  * accum: ``DarkStack.add`` (its launch and the allocation of the chunk's row sums); residual: ``calibrate.residuals``;
  * torch ops: the same results from tensor ops -- ``frames.to(int64).sum(0)``, the squares, the strided row sums; the broadcast
    subtractions -- checked equal before anything is timed;
  * copy: Tensor.copy_ of half the bytes the kernel moves (a copy reads and writes each byte), the roof of streaming that much.
Traffic is counted from the shape: accum reads 2 B per pixel and frame, reads and writes sum and sumsq once per chunk (24 B per pixel)
and writes the row sums; residual reads 2 B and writes 4 B per pixel and frame and reads the shading once (4 B per pixel).
Then the whole ``fit_dark`` over the chunk list (both passes, the float64 variances, the quantile select, the host fit), host clock
around a call that ends in the host's reads, after one warm-up call."""
import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch

from pnnp_amd import calibrate as K


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'r7', 'calib.txt'))
    ap.add_argument('--frames', type=int, default=64)
    ap.add_argument('--chunk', type=int, default=16)
    ap.add_argument('--h', type=int, default=2848)
    ap.add_argument('--w', type=int, default=4256)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--no-fit', action='store_true')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'this benchmark needs the GPU'
    H, W, n = a.h, a.w, a.chunk
    g = torch.Generator(device='cuda').manual_seed(0)
    chunks = []
    for _ in range(a.frames // n):
        x = 512 + 6.0 * torch.randn(n, H, W, device='cuda', generator=g) + 1.0 * torch.randn(n, H, 1, device='cuda', generator=g)
        chunks.append(x.round().clamp(0, 65535).to(torch.uint16))
        del x
    nch = len(chunks)
    lines = [f'dark-frame calibration, us per chunk, median [min .. max] of {a.reps} alternated rounds (each a walk over the {nch} chunks) after '
             f'{a.warmup} warm-up rounds; device {torch.cuda.get_device_name(0)}',
             f'{nch * n} frames of {H}x{W} uint16 in chunks of {n} ({n * H * W * 2 / 1e6:.1f} MB per chunk)']

    # ---- the same results from torch ops, checked before anything is timed
    def t_accum(c, s, ss):
        f = c.to(torch.int64)
        s += f.sum(0)
        ss += (f * f).sum(0)
        return f.view(n, H, W // 2, 2).sum(2)

    def t_residual(c, ds, ro):
        return (c.to(torch.float32) - ds[None]) - ro[:, :, None, :].expand(n, H, W // 2, 2).reshape(n, H, W)

    st = K.DarkStack(H, W).add(chunks[0])
    s64, ss64 = torch.zeros(H, W, dtype=torch.int64, device='cuda'), torch.zeros(H, W, dtype=torch.int64, device='cuda')
    rows = t_accum(chunks[0], s64, ss64)
    same = bool(torch.equal(st.sum.to(torch.int64), s64) and torch.equal(st.sumsq, ss64) and torch.equal(st.rowsum.to(torch.int64), rows))
    ds = st.dark_shading()
    ro = torch.randn(n, H, 2, device='cuda', generator=g)
    same_res = bool(torch.equal(K.residuals(chunks[0], ds, ro), t_residual(chunks[0], ds, ro)))
    lines.append(f'kernel == torch ops on the first chunk: accum {same}, residual {same_res}')
    del rows, st
    torch.cuda.empty_cache()

    px = H * W
    cases = {}
    stack = {'s': None}

    def k_accum():
        stack['s'] = K.DarkStack(H, W)
        for c in chunks:
            stack['s'].add(c)

    def o_accum():
        s64.zero_(); ss64.zero_()
        for c in chunks:
            t_accum(c, s64, ss64)

    def k_res():
        for c in chunks:
            K.residuals(c, ds, ro)

    def o_res():
        for c in chunks:
            t_residual(c, ds, ro)

    cases['accum'] = (n * px * 2 + px * 24 + n * H * 8, k_accum, o_accum)
    cases['residual'] = (n * px * 6 + px * 4 + n * H * 8, k_res, o_res)
    for name, (nbytes, f_kernel, f_ops) in cases.items():
        half = torch.empty(nbytes // 2, dtype=torch.uint8, device='cuda')
        half2 = torch.empty_like(half)

        def f_copy():
            for _ in range(nch):
                half2.copy_(half)

        forms = (('kernel', f_kernel), ('torch ops', f_ops), ('copy', f_copy))
        t = {k: [] for k, _ in forms}
        for r in range(a.warmup + a.reps):
            for k, fn in forms:
                us = timed(fn) / nch
                if r >= a.warmup:
                    t[k].append(us)
        med = {k: float(np.median(v)) for k, v in t.items()}
        lines.append(f'  {name:10s} {nbytes / 1e6:8.1f} MB moved per chunk')
        for k, _ in forms:
            v = np.array(t[k])
            rate = f'{nbytes / med[k] / 1e6:8.3f} TB/s' if k != 'torch ops' else ' ' * 13
            lines.append(f'    {k:10s} {np.median(v):10.1f} [{v.min():10.1f} .. {v.max():10.1f}]  {rate}   spread {(v.max() - v.min()) / np.median(v) * 100:.1f} %')
        lines.append(f'    kernel / copy = {med["kernel"] / med["copy"]:.2f} x the time;  torch ops / kernel = {med["torch ops"] / med["kernel"]:.1f} x')
        del half, half2
        torch.cuda.empty_cache()

    def flush():
        text = '\n'.join(lines) + '\n'
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(text)
        return text

    flush()                                  # the kernel timings are kept whatever becomes of the long call below
    if not a.no_fit:
        ts = []
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fit = K.fit_dark(chunks, 100, 1.0, 16383, 512)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        lines.append(f'  fit_dark over the {nch} chunks (nq 1000, 121 values of lam): {ts[1]:.3f} s (first call {ts[0]:.3f} s); '
                     f'sigGs {fit["sigGs"]:.4f} sigTL {fit["sigTL"]:.4f} lam {fit["lam"]:+.3f} sigR {fit["sigR"]:.4f} (drawn: Gaussian 6.0, rows 1.0)')
    print(flush(), end='')


if __name__ == '__main__':
    main()

"""The classical raw filters (csrc/isp_algos.hip) against the same arithmetic as torch ops on the device and a plain copy:

    python tools/isp_algos_bench.py [--out profiles/r7/isp_algos.txt] [--reps 9] [--inner 5]

Workloads: one frame 4x1424x2128 (the SonyA7S2 eval frame) and 16 crops of 4x512x512, layout 'chw', data in [0, 1).  Functions:
GuidedFilter at d = 7 and d = 25, FastGuidedFilter at d = 7, stdfilt at k = 5, vst_denoise at d = 7.  Three forms, timed in ONE process with
device events around `inner` back-to-back calls, alternated round by round after warm-up rounds; us per call, median [min .. max]:
  * kernel: the public function (its launches and the allocation of its result and intermediates);
  * composition: the same arithmetic as torch ops on the device -- box sums as F.pad + avg_pool2d on float64 copies (what equal results
    cost there), products and everything after the means in float32;
  * copy: Tensor.copy_ of half the bytes the kernels move (a copy reads and writes each byte), the roof of streaming that much.
Traffic is counted from the shape, per pixel: GuidedFilter 32 B (p, I in, a, b out; a, b, I in, result out), FastGuidedFilter 24 B,
stdfilt 8 B, vst_denoise 44 B (two elementwise launches of 8 B and the self-guided filter's 28 B).
The arithmetic per pixel and box mean of window d is 2 d float64 additions and 2 d LDS reads (more at the tile's halo)."""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch
import torch.nn.functional as F

from pnnp_amd import isp_algos as A


def t_box(x, d, mode):
    """float32 [N,H,W] -> float32: the box mean with float64 sums"""
    r = d // 2
    return F.avg_pool2d(F.pad(x.double()[None], (r, r, r, r), mode=mode), d, stride=1)[0].float()


def t_guided(p, I, d, eps, fast=False):
    mode = 'reflect' if fast else 'replicate'
    full = I
    if fast:
        p = (p[:, 0::2, 0::2] + p[:, 0::2, 1::2]) * 0.25 + (p[:, 1::2, 0::2] + p[:, 1::2, 1::2]) * 0.25
        I = (I[:, 0::2, 0::2] + I[:, 0::2, 1::2]) * 0.25 + (I[:, 1::2, 0::2] + I[:, 1::2, 1::2]) * 0.25
    mu_p, mu_I = t_box(p, d, mode), t_box(I, d, mode)
    var = t_box(I * I, d, mode) - mu_I * mu_I
    cov = t_box(I * p, d, mode) - mu_I * mu_p
    a = cov / (var + eps)
    b = mu_p - a * mu_I
    mu_a, mu_b = t_box(a, d, mode), t_box(b, d, mode)
    if fast:
        mu_a = F.interpolate(mu_a[None], scale_factor=2, mode='bilinear', align_corners=False)[0]
        mu_b = F.interpolate(mu_b[None], scale_factor=2, mode='bilinear', align_corners=False)[0]
    return mu_a * full + mu_b


def t_stdfilt(x, k):
    m = t_box(x, k, 'reflect')
    return torch.sqrt(torch.clamp_min(t_box(x * x, k, 'reflect') - m * m, 0))


def t_vst_denoise(x, gain, sigma, d, eps, scale):
    st = torch.full((1,), scale, dtype=torch.float32, device=x.device)
    v = x * st
    t = gain * v + (gain ** 2) * 3.0 / 8.0 + sigma ** 2
    v = (2.0 / gain) * torch.sqrt(torch.clamp_min(t, 0))
    g = t_guided(v, v, d, eps)
    y = (g / 2.0) ** 2 - 3.0 / 8.0 - sigma ** 2 / gain ** 2
    return (y * gain) / st


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'r7', 'isp_algos.txt'))
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--inner', type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'this benchmark needs the GPU'
    lines = [f'classical raw filters, us per call, median [min .. max] of {a.reps} alternated rounds of {a.inner} back-to-back calls after '
             f'{a.warmup} warm-up rounds; device {torch.cuda.get_device_name(0)}']
    g = torch.Generator(device='cuda').manual_seed(0)
    lost = []
    for shape in ((4, 1424, 2128), (64, 512, 512)):
        N, H, W = shape
        px = N * H * W
        I = torch.rand(shape, device='cuda', generator=g)
        p = (I + 0.05 * torch.randn(shape, device='cuda', generator=g)).contiguous()
        raw = (I * 0.05).contiguous()
        lines.append(f'{N} planes of {H}x{W} ({px / 1e6:.2f} Mpx)')
        variants = (('GuidedFilter d=7', 32, lambda: A.GuidedFilter(p, I, 7, 1e-2, layout='chw'), lambda: t_guided(p, I, 7, 1e-2)),
                    ('GuidedFilter d=25', 32, lambda: A.GuidedFilter(p, I, 25, 1e-2, layout='chw'), lambda: t_guided(p, I, 25, 1e-2)),
                    ('FastGuidedFilter d=7', 24, lambda: A.FastGuidedFilter(p, I, 7, 1e-2, layout='chw'), lambda: t_guided(p, I, 7, 1e-2, fast=True)),
                    ('stdfilt k=5', 8, lambda: A.stdfilt(I, 5, layout='chw'), lambda: t_stdfilt(I, 5)),
                    ('vst_denoise d=7', 44, lambda: A.vst_denoise(raw, 2.0, 4.0, 7, 1.0, 15871.0), lambda: t_vst_denoise(raw, 2.0, 4.0, 7, 1.0, 15871.0)))
        for name, bpp, f_kernel, f_comp in variants:
            got, want = f_kernel(), f_comp()
            differ = int((got.view(torch.int32) != want.view(torch.int32)).sum())
            worst = float((got - want).abs().max())
            del got, want
            nbytes = px * bpp
            half = torch.empty(nbytes // 2, dtype=torch.uint8, device='cuda')
            half2 = torch.empty_like(half)

            def f_copy():
                half2.copy_(half)

            forms = (('kernel', f_kernel), ('composition', f_comp), ('copy', f_copy))
            t = {k: [] for k, _ in forms}
            for r in range(a.warmup + a.reps):
                for k, fn in forms:
                    us = timed(fn, a.inner if k != 'composition' else max(1, a.inner // 5))
                    if r >= a.warmup:
                        t[k].append(us)
            med = {k: float(np.median(v)) for k, v in t.items()}
            lines.append(f'  {name:22s} {nbytes / 1e6:7.1f} MB algorithmic ({bpp} B per pixel); kernel vs composition: {differ} of {px} elements differ in bits, '
                         f'max |difference| {worst:.3e}')
            for k, _ in forms:
                v = np.array(t[k])
                rate = f'{nbytes / med[k] / 1e6:8.3f} TB/s' if k != 'composition' else ' ' * 13
                lines.append(f'    {k:12s} {np.median(v):10.1f} [{v.min():10.1f} .. {v.max():10.1f}]  {rate}   spread {(v.max() - v.min()) / np.median(v) * 100:.1f} %')
            beats = min(t['composition']) > max(t['kernel'])
            if not beats:
                lost.append(f'{name} on {N}x{H}x{W}')
            lines.append(f'    kernel / copy = {med["kernel"] / med["copy"]:.2f} x the time;  composition / kernel = {med["composition"] / med["kernel"]:.1f} x '
                         f'(composition min {min(t["composition"]):.1f} us, kernel max {max(t["kernel"]):.1f} us: '
                         f'{"beats it in every round" if beats else "DOES NOT beat it in every round"})')
            del half, half2
            torch.cuda.empty_cache()
    lines.append('lost to the composition in some round: ' + (', '.join(lost) if lost else 'none'))
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write(text)


if __name__ == '__main__':
    main()

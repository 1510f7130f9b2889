"""The sRGB -> packed raw kernel (csrc/unprocess.hip) against the torch-op composition it replaces and a plain byte mover:

    python tools/unprocess_bench.py [--out profiles/r7/unprocess.txt] [--reps 25] [--inner 10]

Workload: 16 crops of 1024x1024x3 -> 16x4x512x512 (what HipTrainStep.step_rgb feeds a step of 16 crops of patch 512), per-crop parameters,
data in [-0.1, 1.2] (float32) or all byte values (uint8).  Inputs float32 [B,H,W,3] and uint8 [B,H,W,3]; outputs packed only, and packed
plus the float32 RGB.  Three forms, timed in ONE process with device events around `inner` back-to-back calls, alternated round by round
after warm-up rounds; us per call, median [min .. max]:
  * kernel: pnnp_unprocess_f32 on a parameter table and output buffers that are already on the device;
  * composition: the reference's lines as torch ops on the device (unprocess.inverse_smoothstep, gamma_expansion, apply_ccm,
    safe_invert_gains, clamp, mosaic, permute to planes), one shared parameter set (the reference's functions take one), uint8 input
    first cast and divided by 255 -- what a user of the reference's functions would run there;
  * plain: tools/ubench/isp_roof.hip, loads and stores with no arithmetic, on a shape [16][4][H'][1024] -> float planes (28 B per pixel)
    whose H' makes its byte count that of the workload to within 0.1 %.
Traffic is counted from the shape: 12 B (float32) or 3 B (uint8) read per pixel, 4 B written for the packed raw, 12 B more for the RGB.

Then the golden cases of tests/golden/unprocess.npz on this device: the kernel's largest absolute and relative error against the float64
restatement beside the reference's own (tests/_unprocess_ref.py), and the same for the composition on case a."""
import argparse
import ctypes as C
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch

from pnnp_amd import _lib, unprocess as U
from tests import _unprocess_ref as R


def composition(x, m, rgb_gain, red_gain, blue_gain):
    if x.dtype == torch.uint8:
        x = x.float() / 255
    t = U.apply_ccm(U.gamma_expansion(U.inverse_smoothstep(x)), m)
    t = torch.clamp(U.safe_invert_gains(t, rgb_gain, red_gain, blue_gain), min=0.0, max=1.0)
    return t, U.mosaic(t).permute(0, 3, 1, 2).contiguous()


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / inner


def golden_errors():
    gold = dict(np.load(os.path.join(REPO, 'tests', 'golden', 'unprocess.npz')))
    meta = json.load(open(os.path.join(REPO, 'tests', 'golden', 'unprocess.json')))['cases']
    lines = []
    for tag in ('a', 'b', 'c', 'd', 'e', 'quad', 'nan'):
        x, m, g, gains = gold[tag + '_x'], gold[tag + '_m'], gold[tag + '_g'], gold[tag + '_gains']
        rows = U.unprocess_rows(m, g[:, 0], g[:, 1], g[:, 2], len(g))
        got = U.unprocess_batch(torch.from_numpy(x).cuda(), rows)[0].cpu().numpy()
        e_abs, e_rel = R.errors(got, R.batch_f64(x, m, gains))
        lines.append(f'  case {tag:5s} kernel abs {e_abs:.3e} rel {e_rel:.3e};  reference abs {meta[tag]["E_abs"]:.3e} rel {meta[tag]["E_rel"]:.3e}')
    x, m, g = gold['a_x'], gold['a_m'], gold['a_g'][0]
    d = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()
    comp = composition(d(x), d(m[0]), d(g[0:1]), d(g[1:2]), d(g[2:3]))[0].cpu().numpy()
    e_abs, e_rel = R.errors(comp, R.batch_f64(x, m, gold['a_gains']))
    lines.append(f'  case a     composition (torch ops on this device) abs {e_abs:.3e} rel {e_rel:.3e}')
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'r7', 'unprocess.txt'))
    ap.add_argument('--reps', type=int, default=25)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--inner', type=int, default=10)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--size', type=int, default=1024)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'this benchmark needs the GPU'
    roof = C.CDLL(os.path.join(REPO, 'tools', 'ubench', 'libisp_roof.so'))
    lib = _lib.lib()
    B, H, W = a.batch, a.size, a.size
    px = B * H * W
    lines = [f'sRGB -> packed raw, {B} x {H}x{W}x3 -> {B}x4x{H // 2}x{W // 2} ({px / 1e6:.2f} Mpx), us per call, median [min .. max] of {a.reps} alternated '
             f'rounds of {a.inner} back-to-back calls after {a.warmup} warm-up rounds; device {torch.cuda.get_device_name(0)}']
    g = torch.Generator(device='cuda').manual_seed(0)
    rng = np.random.RandomState(0)
    m = torch.from_numpy(R.CCMS['IMX686'])
    rows = U.unprocess_rows(m, 1 + 0.4 * rng.rand(B), 1.4 + 0.9 * rng.rand(B), 1.4 + 0.5 * rng.rand(B), B)
    md, gains = m.cuda(), [torch.tensor([v], device='cuda') for v in (1.25, 1.9, 1.6)]
    out_rgb = torch.empty((B, H, W, 3), dtype=torch.float32, device='cuda')
    out_pk = torch.empty((B, 4, H // 2, W // 2), dtype=torch.float32, device='cuda')
    st = _lib.stream()
    for kind, name, rd in ((U.UNP_IN_HWC_F32, 'float32 [B,H,W,3]', 12), (U.UNP_IN_HWC_U8, 'uint8 [B,H,W,3]', 3)):
        if kind == U.UNP_IN_HWC_U8:
            x = torch.randint(0, 256, (B, H, W, 3), device='cuda', generator=g, dtype=torch.uint8)
        else:
            x = torch.rand((B, H, W, 3), device='cuda', generator=g) * 1.3 - 0.1
        for both in (False, True):
            nbytes = px * (rd + 4 + (12 if both else 0))
            rh = max(1, int(round(nbytes / (16 * 1024 * 28))))
            rin = torch.empty((16, 4, rh, 1024), dtype=torch.float32, device='cuda').uniform_(0, 1)
            rout = torch.empty((16, 3, rh, 1024), dtype=torch.float32, device='cuda')
            rbytes = 16 * rh * 1024 * 28
            assert abs(rbytes - nbytes) <= 1e-3 * nbytes or px < 1 << 20
            orgb = out_rgb if both else None

            def f_kernel():
                _lib.check(lib.pnnp_unprocess_f32(_lib.ptr(x), kind, B, H, W, _lib.ptr(rows), C.c_uint(0), _lib.ptr(orgb), _lib.ptr(out_pk), st), 'unprocess')

            def f_comp():
                composition(x, md, *gains)

            def f_plain():
                assert roof.isp_roof_launch(_lib.ptr(rin), 16, rh, 1024, _lib.ptr(rout), None, st) == 0

            forms = (('kernel', f_kernel), ('composition', f_comp), ('plain', f_plain))
            t = {n: [] for n, _ in forms}
            for r in range(a.warmup + a.reps):
                for n, fn in forms:
                    us = timed(fn, a.inner)
                    if r >= a.warmup:
                        t[n].append(us)
            med = {k: float(np.median(v)) for k, v in t.items()}
            lines.append(f'input {name}, output {"packed + float32 RGB" if both else "packed only"}: {nbytes / 1e6:.1f} MB algorithmic '
                         f'({nbytes // px} B per pixel); plain moves {rbytes / 1e6:.1f} MB')
            for n, _ in forms:
                v = np.array(t[n])
                nb = rbytes if n == 'plain' else nbytes
                rate = f'{nb / med[n] / 1e6:8.3f} TB/s of algorithmic bytes' if n != 'composition' else ''
                lines.append(f'    {n:12s} {np.median(v):9.1f} [{v.min():9.1f} .. {v.max():9.1f}]  {rate}')
            lines.append(f'    kernel / plain = {med["kernel"] / med["plain"]:.2f} x the time;  composition / kernel = {med["composition"] / med["kernel"]:.1f} x '
                         f'(composition min {min(t["composition"]):.1f} us, kernel max {max(t["kernel"]):.1f} us)')
            del rin, rout
    lines.append('golden cases on this device: largest error against the float64 restatement (rule: every element within max(4 x the reference\'s, one ulp)):')
    lines += golden_errors()
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write(text)


if __name__ == '__main__':
    main()

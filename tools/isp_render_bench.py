"""The packed-raw -> sRGB render kernel (csrc/isp.hip) against the torch-op composition it replaces and a plain byte mover:

    python tools/isp_render_bench.py [--out profiles/r7/isp_render.txt] [--reps 25] [--inner 20]

Workloads: one frame 4x1424x2128 (the SonyA7S2 eval frame) and 16 crops of 4x512x512, Sony white balance and matrix, data in [-0.1, 1.3];
each for uint8-only output and for both outputs (uint8 [N,H,W,3] and float32 [N,3,H,W]).  Three forms, timed in ONE process with device
events around `inner` back-to-back calls, alternated round by round after warm-up rounds; us per call, median [min .. max]:
  * kernel: pnnp_isp_process_f32 on a parameter table and output buffers that are already on the device;
  * composition: apply_gains, clamp, raw2LRGB, apply_ccms, clamp, clamp(min) ** (1/2.2), * 255, .int(), clamp, then the permute / cast to
    uint8 (and / 255 for the float planes) as torch ops on the device -- what a user of the reference's functions would run there;
  * plain: tools/ubench/isp_roof.hip, the same grid, loads and stores with no arithmetic (the roof of this access pattern).
Traffic is counted from the shape: 16 B read per pixel, 3 B written for uint8, 12 B more for the float planes.

Then the golden cases of tests/golden/isp.npz on this device: how many values per case used the one-level exception of the agreement rule
(tests/_isp_ref.py)."""
import argparse
import ctypes as C
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch

from pnnp_amd import _lib, process as P
from tests import _isp_ref as R


def composition(x, wb, ccm, both):
    v = torch.clamp(P.apply_gains(x, wb), min=0.0, max=1.0)
    v = torch.clamp(P.apply_ccms(P.raw2LRGB(v), ccm), min=0.0, max=1.0)
    lv = torch.clamp((torch.clamp(v, min=1e-8) ** (1 / 2.2) * 255).int(), min=0, max=255)
    u8 = lv.permute(0, 2, 3, 1).to(torch.uint8).contiguous()
    return (lv.float() / 255 if both else None), u8


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / inner


def golden_counts():
    gold = dict(np.load(os.path.join(REPO, 'tests', 'golden', 'isp.npz')))
    lines = []
    for tag in 'abcde':
        x = gold[tag + '_x']
        x = np.repeat(x, 4, axis=1) if tag == 'd' else x
        wb, ccm, k = gold[tag + '_wb'], gold[tag + '_ccm'], gold[tag + '_k'].astype(np.int64)
        got = R.to_levels(P.process(torch.from_numpy(x).cuda(), torch.from_numpy(wb).cuda(), torch.from_numpy(ccm).cuda()).cpu().numpy())
        n_diff, n_bad = R.disagreements(got, k, R.process_pre(x, wb, ccm))
        n_once = int((got != R.process_levels(x, wb, ccm, once=True)).sum())
        lines.append(f'  case {tag}: {n_diff} of {k.size} values one level from the reference ({100.0 * n_diff / k.size:.3f} %), {n_bad} outside the rule; '
                     f'{n_once} differ from the round-once float64 restatement')
    got = R.to_levels(P.gamma_compression(torch.from_numpy(gold['g_x']).cuda()).cpu().numpy())
    n_diff, n_bad = R.disagreements(got, gold['g_k'], R.pre(gold['g_x']))
    lines.append(f'  gamma_compression: {n_diff} of {got.size}, {n_bad} outside the rule')
    for tag, args, add in (('f_sid', ('f_sid_lr', 'f_sid_pred', 'f_sid_hr'), False), ('f_nf', ('f_nf_hr', 'f_nf_sample', 'f_nf_lr'), True)):
        a = [gold[n] for n in args]
        lin = R.preview_linear(*a, gold['f_wb'], add_inputs_to_output=add)
        got = P.preview_strip(*[torch.from_numpy(v).cuda() for v in a], gold['f_wb'], add_inputs_to_output=add).cpu().numpy()
        n_diff, n_bad = R.disagreements(got, gold[tag + '_u8'], R.pre(lin, floor=False))
        lines.append(f'  preview {tag}: {n_diff} of {got.size}, {n_bad} outside the rule')
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'r7', 'isp_render.txt'))
    ap.add_argument('--reps', type=int, default=25)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--inner', type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'this benchmark needs the GPU'
    roof = C.CDLL(os.path.join(REPO, 'tools', 'ubench', 'libisp_roof.so'))
    lib = _lib.lib()
    lines = [f'packed raw -> sRGB render, us per call, median [min .. max] of {a.reps} alternated rounds of {a.inner} back-to-back calls after '
             f'{a.warmup} warm-up rounds; device {torch.cuda.get_device_name(0)}']
    g = torch.Generator(device='cuda').manual_seed(0)
    wb, ccm = torch.from_numpy(R.SONY_WB[None]).cuda(), torch.from_numpy(R.SONY_CCM[None]).cuda()
    for shape in ((1, 4, 1424, 2128), (16, 4, 512, 512)):
        N, _, H, W = shape
        x = torch.rand(shape, device='cuda', generator=g) * 1.4 - 0.1
        rows = P.isp_rows(wb, ccm, N)
        out_f = torch.empty((N, 3, H, W), dtype=torch.float32, device='cuda')
        out_b = torch.empty((N, H, W, 3), dtype=torch.uint8, device='cuda')
        # results first: kernel against composition under the agreement rule (the composition's pow is the device's float32 pow)
        f, u = P.isp_render(x, rows, f32=True, u8=True)
        cf, cu = composition(x, wb, ccm, True)
        n_diff = int((u != cu).sum())
        n_two = int(((u.int() - cu.int()).abs() > 1).sum())
        px = N * H * W
        lines.append(f'{N} x 4x{H}x{W} ({px / 1e6:.2f} Mpx): kernel vs composition: {n_diff} of {3 * px} values differ, {n_two} by more than one level')
        for both in (False, True):
            of = out_f if both else None
            st = _lib.stream()

            def f_kernel():
                _lib.check(lib.pnnp_isp_process_f32(_lib.ptr(x), N, H, W, _lib.ptr(rows), C.c_uint(0), _lib.ptr(of), _lib.ptr(out_b), st), 'isp')

            def f_plain():
                assert roof.isp_roof_launch(_lib.ptr(x), N, H, W, _lib.ptr(of), _lib.ptr(out_b), st) == 0

            def f_comp():
                composition(x, wb, ccm, both)

            forms = (('kernel', f_kernel), ('composition', f_comp), ('plain', f_plain))
            t = {name: [] for name, _ in forms}
            for r in range(a.warmup + a.reps):
                for name, fn in forms:
                    us = timed(fn, a.inner)
                    if r >= a.warmup:
                        t[name].append(us)
            nbytes = px * (16 + 3 + (12 if both else 0))
            med = {k: float(np.median(v)) for k, v in t.items()}
            lines.append(f'  output {"uint8 + float32" if both else "uint8 only":16s} {nbytes / 1e6:7.1f} MB algorithmic ({nbytes // px} B per pixel)')
            for name, _ in forms:
                v = np.array(t[name])
                rate = f'{nbytes / med[name] / 1e6:8.3f} TB/s' if name != 'composition' else ' ' * 13
                lines.append(f'    {name:12s} {np.median(v):9.1f} [{v.min():9.1f} .. {v.max():9.1f}]  {rate}')
            lines.append(f'    kernel / plain = {med["kernel"] / med["plain"]:.2f} x the time;  composition / kernel = {med["composition"] / med["kernel"]:.1f} x '
                         f'(composition min {min(t["composition"]):.1f} us, kernel max {max(t["kernel"]):.1f} us)')
    lines.append('golden cases on this device (agreement rule: equal, or one level apart with the float64 value within 1e-4 of an integer; cap 0.5 % per case):')
    lines += golden_counts()
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write(text)


if __name__ == '__main__':
    main()

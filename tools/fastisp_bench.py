"""The full-resolution render kernel (csrc/demosaic.hip) against the same arithmetic as torch ops on the device and a plain copy:

    python tools/fastisp_bench.py [--out profiles/r7/fastisp.txt] [--reps 15] [--inner 10]

Workloads: one frame 4x1424x2128 (the SonyA7S2 eval frame, 2848x4256 rendered) and 16 crops of 4x512x512, Sony gains and matrix, data in
[-0.1, 1.3].  Variants: FastISP to uint8, to float32 planes, to both, and the uint16 stencil alone on the mosaic of the same data.  Three
forms, timed in ONE process with device events around `inner` back-to-back calls, alternated round by round after warm-up rounds; us per
call, median [min .. max]:
  * kernel: pnnp_fastisp_f32 / pnnp_demosaic_ea_u16 on a parameter table and output buffers that are already on the device;
  * composition: the restatement (tests/_fastisp_ref.py) op by op as torch ops on the device: the float32 front, the stencil on int32
    slices, the float64 tail, then the casts a caller needs;
  * copy: Tensor.copy_ of half the bytes the variant moves (a copy reads and writes each byte), the roof of streaming that much.
Traffic is counted from the shape, per output pixel: 4 B read (one float32 mosaic element; 2 B for the stencil alone), 3 B written for
uint8, 12 B for the float planes, 6 B for the stencil's uint16 triple.
The condition: in every round each variant's kernel beats its composition by more than the run-to-run spread (composition min > kernel max)."""
import argparse
import ctypes as C
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch

from pnnp_amd import _lib, process as P
from tests._isp_ref import SONY_CCM, SONY_WB


def t_front(x, wb0, wb2):
    N, _, h, w = x.shape
    raw = torch.empty((N, 2 * h, 2 * w), dtype=torch.float32, device=x.device)
    raw[:, 0::2, 0::2] = x[:, 0] * wb0
    raw[:, 0::2, 1::2] = x[:, 1]
    raw[:, 1::2, 1::2] = x[:, 2] * wb2
    raw[:, 1::2, 0::2] = x[:, 3]
    return torch.nan_to_num(raw.clamp(0, 1) * 16383.0, nan=0.0).to(torch.int32)


def t_demosaic(s):
    """int32 [N,H,W] -> int32 [N,H,W,3]"""
    N, H, W = s.shape
    c, u, d, l, r = s[:, 1:-1, 1:-1], s[:, :-2, 1:-1], s[:, 2:, 1:-1], s[:, 1:-1, :-2], s[:, 1:-1, 2:]
    hz, vt = (l + r + 1) >> 1, (u + d + 1) >> 1
    diag = (s[:, :-2, :-2] + s[:, :-2, 2:] + s[:, 2:, :-2] + s[:, 2:, 2:] + 2) >> 2
    g = torch.where((l - r).abs() > (u - d).abs(), vt, hz)
    yy = torch.arange(1, H - 1, device=s.device)[:, None]
    xx = torch.arange(1, W - 1, device=s.device)[None, :]
    even, colour = ((yy & 1) == 0).expand(H - 2, W - 2), ((yy ^ xx) & 1) == 0
    Rc = torch.where(colour, torch.where(even, c, diag), torch.where(even, hz, vt))
    Gc = torch.where(colour, g, c)
    Bc = torch.where(colour, torch.where(even, diag, c), torch.where(even, vt, hz))
    inner = torch.stack([Rc, Gc, Bc], dim=-1)
    iy = torch.arange(H, device=s.device).clamp(1, H - 2) - 1
    ix = torch.arange(W, device=s.device).clamp(1, W - 2) - 1
    return inner[:, iy][:, :, ix]


def t_tail(D, ccm64):
    v = D.to(torch.float64) / 16383
    lin = (v[..., None, :] * ccm64[None, None, None]).sum(-1)
    return lin.clamp(0, 1) ** (1 / 2.2)


def composition(x, wb0, wb2, ccm64, f32, u8):
    out = t_tail(t_demosaic(t_front(x, wb0, wb2)), ccm64)
    return (out.to(torch.float32).permute(0, 3, 1, 2).contiguous() if f32 else None), ((out * 255).floor().to(torch.uint8) if u8 else None)


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
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'r7', 'fastisp.txt'))
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--inner', type=int, default=10)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'this benchmark needs the GPU'
    lib = _lib.lib()
    lines = [f'full-resolution render (FastISP), us per call, median [min .. max] of {a.reps} alternated rounds of {a.inner} back-to-back calls after '
             f'{a.warmup} warm-up rounds; device {torch.cuda.get_device_name(0)}']
    g = torch.Generator(device='cuda').manual_seed(0)
    ccm64 = torch.from_numpy(SONY_CCM.astype(np.float64)).cuda()
    wb0, wb2 = float(SONY_WB[0]), float(SONY_WB[2])
    ok = True
    for shape in ((1, 4, 1424, 2128), (16, 4, 512, 512)):
        N, _, h, w = shape
        H, W = 2 * h, 2 * w
        px = N * H * W
        x = torch.rand(shape, device='cuda', generator=g) * 1.4 - 0.1
        rows = P.isp_rows(SONY_WB, SONY_CCM, N)
        out_f = torch.empty((N, 3, H, W), dtype=torch.float32, device='cuda')
        out_b = torch.empty((N, H, W, 3), dtype=torch.uint8, device='cuda')
        mosaic = t_front(x, wb0, wb2).to(torch.uint16)
        mosaic32 = mosaic.to(torch.int32)
        out_s = torch.empty((N, H, W, 3), dtype=torch.uint16, device='cuda')
        # results first: kernel against composition
        f, u = P.fastisp_render(x, rows, f32=True, u8=True)
        cf, cu = composition(x, wb0, wb2, ccm64, True, True)
        _lib.check(lib.pnnp_demosaic_ea_u16(_lib.ptr(mosaic), N, H, W, _lib.ptr(out_s), _lib.stream()), 'demosaic')
        same_s = bool((out_s.to(torch.int32) == t_demosaic(mosaic32)).all())
        lines.append(f'{N} x 4x{h}x{w} -> {N} x {H}x{W} ({px / 1e6:.2f} Mpx): kernel vs composition: {int((u != cu).sum())} of {3 * px} levels differ, '
                     f'float planes max |difference| {float((f - cf).abs().max()):.3e}, stencil {"equal" if same_s else "DIFFERS"}')
        del f, u, cf, cu
        st = _lib.stream()
        variants = (('uint8', False, True, 4 + 3), ('float32', True, False, 4 + 12), ('uint8 + float32', True, True, 4 + 15), ('stencil uint16', None, None, 2 + 6))
        for name, f32, u8, bpp in variants:
            nbytes = px * bpp
            half = torch.empty(nbytes // 2, dtype=torch.uint8, device='cuda')
            half2 = torch.empty_like(half)
            if f32 is None:
                def f_kernel():
                    _lib.check(lib.pnnp_demosaic_ea_u16(_lib.ptr(mosaic), N, H, W, _lib.ptr(out_s), st), 'demosaic')

                def f_comp():
                    t_demosaic(mosaic32).to(torch.uint16)
            else:
                of, ob = (out_f if f32 else None), (out_b if u8 else None)

                def f_kernel():
                    _lib.check(lib.pnnp_fastisp_f32(_lib.ptr(x), N, h, w, _lib.ptr(rows), C.c_uint(0), _lib.ptr(of), _lib.ptr(ob), st), 'fastisp')

                def f_comp():
                    composition(x, wb0, wb2, ccm64, f32, u8)

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
            lines.append(f'  {name:16s} {nbytes / 1e6:7.1f} MB algorithmic ({bpp} B per output pixel)')
            for k, _ in forms:
                v = np.array(t[k])
                rate = f'{nbytes / med[k] / 1e6:8.3f} TB/s' if k != 'composition' else ' ' * 13
                lines.append(f'    {k:12s} {np.median(v):10.1f} [{v.min():10.1f} .. {v.max():10.1f}]  {rate}   spread {(v.max() - v.min()) / np.median(v) * 100:.1f} %')
            beats = min(t['composition']) > max(t['kernel'])
            ok = ok and beats
            lines.append(f'    kernel / copy = {med["kernel"] / med["copy"]:.2f} x the time;  composition / kernel = {med["composition"] / med["kernel"]:.1f} x '
                         f'(composition min {min(t["composition"]):.1f} us, kernel max {max(t["kernel"]):.1f} us: {"beats it in every round" if beats else "DOES NOT beat it in every round"})')
            del half, half2
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write(text)
    if not ok:
        sys.exit('a kernel variant did not beat its composition in every round')


if __name__ == '__main__':
    main()

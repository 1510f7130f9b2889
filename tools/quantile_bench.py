#!/usr/bin/env python3
"""Cost of the device-side QuantileLoss (csrc/quantile.hip; losses.QuantileLoss) at K = 1000 probabilities on 16 crops of 4x512x512 float32
values per operand (normal samples of different scale), pooled (one row of N = 16.7 M) and per crop (16 rows of N = 1 M).

HIP events around EVERY call; ROUNDS rounds in ONE process, each round timing every candidate once, in turn (alternated), after WARM
warm-up rounds; median [min .. max] over the rounds:
  forward              losses.QuantileLoss under no_grad (memset, range, census, scan, gather, finish, eval; allocates its outputs per call)
  forward + backward   losses.QuantileLoss(...).backward() with both operands requiring grad
  torch.quantile       the reference's composition (utils/kld_div.py:49-53) from torch.quantile on the same device, forward and forward +
                       backward; if torch refuses the size or runs out of memory that is recorded instead of a time
  CDFLoss              losses.CDFLoss on the same tensors (flattened), points over the range of both, forward and forward + backward
  plain read           pnnp_noise_score_read_f32 over (output, gt, output): 12 N bytes with one 1024-thread workgroup per CU
Algorithmic bytes of the forward, counted here: three passes read both operands (3 x 8 N bytes); the gather writes and the finish reads
8 bytes per gathered sample (the gathered share is read back from the workspace after a call).

--kernels N: nothing but N forward + backward calls of each form, for a `rocprofv3 --kernel-trace --stats` run around this script (a run of
its own; the qt_* rows of its kernel_stats.csv are appended to profiles/r7/quantile.txt by hand).
usage: quantile_bench.py [--out FILE] [--kernels N] [--rounds R]"""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

K = 1000
CROPS, PER_CROP = 16, 4 * 512 * 512
WARM = 2


def event_us(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def show(ts):
    if isinstance(ts, str):
        return ts
    return f'{statistics.median(ts):10.1f} [{min(ts):10.1f} .. {max(ts):10.1f}]'


def gathered_share(o, g, q):
    """the share of the samples that the gather appended, read from the workspace of one call on the C entry"""
    from pnnp_amd import _lib, losses
    L = losses._quantile_lib()
    r, k = o.shape[0], q.numel()
    ws = torch.empty(int(L.pnnp_quantile_ws_bytes(r, o.shape[1], g.shape[1], k)), dtype=torch.uint8, device='cuda')
    buf = [torch.empty(2 * k * r, device='cuda'), torch.empty(4 * k * r, dtype=torch.int32, device='cuda'), torch.empty(2 * k, device='cuda'),
           torch.empty(1, device='cuda'), torch.empty(2 * k * r, device='cuda')]
    _lib.check(L.pnnp_quantile_loss_f32(_lib.ptr(o), C.c_int64(o.shape[1]), _lib.ptr(g), C.c_int64(g.shape[1]), r, _lib.ptr(q), k, _lib.ptr(ws),
                                        *[_lib.ptr(b) for b in buf], _lib.stream()), 'pnnp_quantile_loss_f32')
    words = 32768 + 1024 + 8 + 14 * k                          # the table of one (row, operand) pair, 32-bit words (csrc/quantile.hip)
    tables = ws[:2 * r * words * 4].view(torch.int32).view(2 * r, words).cpu()
    total = 0
    for t in tables:
        ns = int(t[32768 + 1024 + 2])
        total += int(t[32768 + 1024 + 8 + 4 * k:32768 + 1024 + 8 + 4 * k + ns].sum())         # slot_cnt
    return total / float(o.numel() + g.numel())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'r7', 'quantile.txt'))
    ap.add_argument('--kernels', type=int, default=0)
    ap.add_argument('--rounds', type=int, default=7)
    args = ap.parse_args()
    from pnnp_amd import _lib, losses
    L = _lib.lib()
    gen = torch.Generator(device='cuda').manual_seed(1)
    out4 = torch.randn(CROPS, PER_CROP, device='cuda', generator=gen)
    gt4 = torch.randn(CROPS, PER_CROP, device='cuda', generator=gen) * 1.2 + 0.1
    q = losses.get_x(size=K, mode='uniform').cuda()
    x = (torch.minimum(out4.min(), gt4.min()) + q * (torch.maximum(out4.max(), gt4.max()) - torch.minimum(out4.min(), gt4.min()))).contiguous()
    forms = {'pooled': (out4.reshape(1, -1), gt4.reshape(1, -1)), 'per crop': (out4, gt4)}
    if args.kernels:
        for name, (o, g) in forms.items():
            a, b = o.clone().requires_grad_(True), g.clone().requires_grad_(True)
            for _ in range(args.kernels):
                a.grad = b.grad = None
                losses.QuantileLoss(a.squeeze(0), b.squeeze(0), q).backward()
        torch.cuda.synchronize()
        return
    lines = [f'QuantileLoss, K = {K}, {CROPS} crops of 4x512x512 per operand; us per call, median [min .. max] of {args.rounds} alternated rounds '
             f'after {WARM} warm-up rounds; device {torch.cuda.get_device_name(0)}']
    sink = torch.zeros(256, dtype=torch.int32, device='cuda')
    for name, (o, g) in forms.items():
        o1, g1 = o.squeeze(0), g.squeeze(0)
        n_all = o.numel()
        a, b = o1.clone().requires_grad_(True), g1.clone().requires_grad_(True)

        def ours_f():
            with torch.no_grad():
                losses.QuantileLoss(o1, g1, q)

        def ours_fb():
            a.grad = b.grad = None
            losses.QuantileLoss(a, b, q).backward()

        def ref(u, v):
            return torch.nn.functional.l1_loss(torch.quantile(u, q, dim=-1, interpolation='linear').squeeze(),
                                               torch.quantile(v, q, dim=-1, interpolation='linear').squeeze())

        def torch_f():
            with torch.no_grad():
                ref(o1, g1)

        def torch_fb():
            a.grad = b.grad = None
            ref(a, b).backward()

        def cdf_f():
            with torch.no_grad():
                losses.CDFLoss(o1, g1, x, assume_sorted=True)

        def cdf_fb():
            a.grad = b.grad = None
            losses.CDFLoss(a, b, x, assume_sorted=True).backward()

        def read():
            _lib.check(L.pnnp_noise_score_read_f32(_lib.ptr(o), _lib.ptr(g), _lib.ptr(o), 1, C.c_int64(n_all), _lib.ptr(sink), _lib.stream()), 'read')

        cands = [('forward', ours_f), ('forward + backward', ours_fb), ('torch.quantile forward', torch_f), ('torch.quantile forward + backward', torch_fb),
                 ('CDFLoss forward', cdf_f), ('CDFLoss forward + backward', cdf_fb), ('plain read of 12 N bytes', read)]
        times = {c: [] for c, _ in cands}
        for rnd in range(WARM + args.rounds):
            for c, fn in cands:
                if isinstance(times[c], str):
                    continue
                try:
                    t = event_us(fn)
                except (RuntimeError, torch.OutOfMemoryError) as e:                  # torch refuses the size, or no memory: recorded
                    times[c] = 'refused: ' + str(e).splitlines()[0][:120]
                    torch.cuda.empty_cache()
                    continue
                if rnd >= WARM:
                    times[c].append(t)
        share = gathered_share(o.contiguous(), g.contiguous(), q)
        fwd_bytes = 3 * 8 * n_all + 2 * 8 * share * 2 * n_all
        lines.append(f'--- {name}: rows = {o.shape[0]}, N = {o.shape[1]} per row and operand; gathered share of the samples {share:.4f}')
        for c, _ in cands:
            lines.append(f'  {c:36s} {show(times[c])}')
        f_med, r_med = statistics.median(times['forward']), statistics.median(times['plain read of 12 N bytes'])
        read_rate = 12 * n_all / r_med / 1e3
        lines.append(f'  plain read rate {read_rate:8.1f} GB/s; forward: {fwd_bytes / 1e6:8.1f} MB algorithmic = {fwd_bytes / f_med / 1e3:8.1f} GB/s = '
                     f'{100 * fwd_bytes / f_med / 1e3 / read_rate:5.1f} % of the plain read rate; one pass over both operands at the read rate {8 * n_all / read_rate / 1e3:8.1f} us')
        for tag, ours, theirs in (('forward', 'forward', 'torch.quantile forward'), ('forward + backward', 'forward + backward', 'torch.quantile forward + backward'),
                                  ('forward vs CDFLoss', 'forward', 'CDFLoss forward'), ('forward + backward vs CDFLoss', 'forward + backward', 'CDFLoss forward + backward')):
            if isinstance(times[theirs], str):
                lines.append(f'  ratio {tag}: no yardstick ({times[theirs]})')
            else:
                lines.append(f'  ratio {tag}: yardstick / ours = {statistics.median(times[theirs]) / statistics.median(times[ours]):6.2f} '
                             f'(ours max {max(times[ours]):.1f} us, yardstick min {min(times[theirs]):.1f} us)')
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()

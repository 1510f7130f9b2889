#!/usr/bin/env python3
"""Cost of the device-side distribution loss (csrc/ddl.hip; losses.CDFLoss) at K = 1000 points on two sample sets of N = 4x512x512 and of
N = 16x4x512x512 float32 values each (normal samples of different scale; the points span both).

Per size, HIP events around EVERY call, 20 calls after 5 warm-ups, median [min .. max]:
  forward              pnnp_cdf_loss_f32 through the C entry with its buffers allocated once (2 memsets, range, census, finish, loss)
  forward + backward   losses.CDFLoss(...).backward() with both operands requiring grad (allocates its outputs per call)
  torch ops            the sort-based restatement (tests/_ddl_ref.py: sort + searchsorted + gather, autograd) on the same device, same two cases
  plain read           pnnp_noise_score_read_f32 over (output, gt, output): 12 N bytes with one 1024-thread workgroup per CU; the census
                       pass reads 8 N bytes, so "census bytes at the plain read's rate" = 2/3 of its time
The one condition: the device path is faster than the torch ops at both sizes beyond the spread of the 20 calls (its max below their min).

--variants: also time the forward through measurement builds of the library (tools/build_variant.sh, -DDD_AB=1/2/3: no binary search, no
LDS atomics, no minimum / maximum; wrong results on purpose), each in a child process with PNNP_LIB set.
--kernels N: nothing but N forward + backward calls at each size, for a `rocprofv3 --kernel-trace --stats` run around this script.
usage: ddl_bench.py [--out FILE] [--variants] [--kernels N]"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

K = 1000
SIZES = [4 * 512 * 512, 16 * 4 * 512 * 512]
CALLS, WARM = 20, 5
VARIANTS = [('no binary search', 'ddl_ab1'), ('no LDS atomics', 'ddl_ab2'), ('count only (no min / max)', 'ddl_ab3')]


def timed(fn):
    """us of each of CALLS calls after WARM warm-ups"""
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(CALLS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    return out


def show(ts):
    return f'{statistics.median(ts):9.1f} [{min(ts):9.1f} .. {max(ts):9.1f}]'


def inputs(n):
    g = torch.Generator(device='cuda').manual_seed(n)
    out = torch.randn(n, device='cuda', generator=g)
    gt = torch.randn(n, device='cuda', generator=g) * 1.2 + 0.1
    lo, hi = torch.minimum(out.min(), gt.min()), torch.maximum(out.max(), gt.max())
    from pnnp_amd import losses
    x = (lo + losses.get_x(size=K, mode='uniform').cuda() * (hi - lo)).contiguous()
    return out, gt, x


def forward_entry(out, gt, x):
    from pnnp_amd import _lib, losses
    L = losses._ddl_lib()
    ws = losses._workspace(L, 2, K, out.device)
    cdf = torch.empty(2, K, device='cuda'); dcdf = torch.empty(2, K, device='cuda')
    br = torch.empty(2, 2 * K + 2, dtype=torch.int32, device='cuda'); loss = torch.empty(1, device='cuda')
    n = out.numel()

    def call():
        _lib.check(L.pnnp_cdf_loss_f32(_lib.ptr(out), C.c_int64(n), _lib.ptr(gt), C.c_int64(n), _lib.ptr(x), K, _lib.ptr(ws), _lib.ptr(cdf), _lib.ptr(br),
                                       _lib.ptr(loss), _lib.ptr(dcdf), _lib.stream()), 'cdf_loss')
    return call, loss


def forward_times():
    res = {}
    for n in SIZES:
        out, gt, x = inputs(n)
        call, _ = forward_entry(out, gt, x)
        res[str(n)] = timed(call)
    return res


def kernels_only(reps):
    from pnnp_amd import losses
    for n in SIZES:
        out, gt, x = inputs(n)
        out.requires_grad_(True); gt.requires_grad_(True)
        for _ in range(reps):
            out.grad = gt.grad = None
            losses.CDFLoss(out, gt, x, assume_sorted=True).backward()
        torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--variants', action='store_true')
    ap.add_argument('--kernels', type=int, default=0)
    ap.add_argument('--forward-json', action='store_true', help='(child of --variants) print the forward times as JSON')
    a = ap.parse_args()
    if a.kernels:
        return kernels_only(a.kernels)
    if a.forward_json:
        print('FORWARD ' + json.dumps(forward_times()))
        return
    variant_times = {}
    if a.variants:                                             # children first: this process has not touched the GPU yet
        for name, tag in VARIANTS:
            lib = os.path.join(REPO, 'tools', 'scratch', 'variants', f'libpnnp_{tag}.so')
            if not os.path.exists(lib):
                raise SystemExit(f'{lib} not found: tools/build_variant.sh {tag} ddl.hip -DDD_AB=...')
            r = subprocess.run([sys.executable, os.path.abspath(__file__), '--forward-json'], env=dict(os.environ, PNNP_LIB=lib), capture_output=True,
                               text=True, timeout=300, check=True)
            variant_times[name] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('FORWARD ')][-1][8:])
    from pnnp_amd import _lib, losses
    from tests import _ddl_ref as R
    L = _lib.lib()
    lines = [f'distribution loss (csrc/ddl.hip, CDFLoss) on {torch.cuda.get_device_name(0)}: K = {K} points, two operands of N float32 samples each; HIP events around every '
             f'call, {CALLS} calls after {WARM} warm-ups; us, median [min .. max]']
    ok = True
    for n in SIZES:
        out, gt, x = inputs(n)
        call, loss = forward_entry(out, gt, x)
        t_fwd = timed(call)
        sink = torch.zeros(256, dtype=torch.int32, device='cuda')
        t_read = timed(lambda: _lib.check(L.pnnp_noise_score_read_f32(_lib.ptr(out), _lib.ptr(gt), _lib.ptr(out), 1, C.c_int64(n), _lib.ptr(sink), _lib.stream()), 'read'))
        a_, b_ = out.clone().requires_grad_(True), gt.clone().requires_grad_(True)

        def ours_fb():
            a_.grad = b_.grad = None
            losses.CDFLoss(a_, b_, x, assume_sorted=True).backward()

        def torch_f():
            with torch.no_grad():
                return R.cdf_loss(out, gt, x)

        def torch_fb():
            a_.grad = b_.grad = None
            R.cdf_loss(a_, b_, x).backward()

        t_fb, t_tf, t_tfb = timed(ours_fb), timed(torch_f), timed(torch_fb)
        ours, theirs = float(losses.CDFLoss(out, gt, x, assume_sorted=True)), float(torch_f())
        med = statistics.median
        read_census = med(t_read) * 2 / 3
        lines += [f'N = {n}  ({8 * n / 1e6:.0f} MB in the two operands; the forward reads them twice: range, census)   CDFLoss device {ours:.8f}  torch ops {theirs:.8f}',
                  f'  forward, C entry            {show(t_fwd)}    {16 * n / med(t_fwd) / 1e6:6.2f} TB/s of the 16 N bytes the two passes read',
                  f'  forward + backward, python  {show(t_fb)}',
                  f'  torch ops forward           {show(t_tf)}    x{med(t_tf) / med(t_fwd):.1f} the device forward',
                  f'  torch ops forward+backward  {show(t_tfb)}    x{med(t_tfb) / med(t_fb):.1f} the device forward + backward',
                  f'  plain read of 12 N bytes    {show(t_read)}    {12 * n / med(t_read) / 1e6:6.2f} TB/s; the census pass\'s 8 N bytes at that rate: {read_census:.1f} us']
        for name, tms in variant_times.items():
            v = tms[str(n)]
            lines.append(f'  forward, build with {name:<26s} {show(v)}    {med(t_fwd) - med(v):+9.1f} us to the full forward')
        faster = max(t_fwd) < min(t_tf) and max(t_fb) < min(t_tfb)
        ok = ok and faster
        lines.append(f'  device path faster than the torch ops beyond the spread (max of ours < min of theirs), forward and forward + backward: {faster}')
    print('\n'.join(lines), flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    if not ok:
        raise SystemExit('the device path is NOT faster than the torch ops beyond the spread')


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""Cost of the float-edge histogram KL on the device (csrc/hist_kl.hip; metrics.kl_div_3_data, metrics.kl_div_range) on 16 crops of
4x512x512 float32 (2 x 64 MB read), pooled and per crop:

  default   kl_div_3_data at the default 1000 bins on [0, 1], N(0.5, 0.1) against N(0.5, 0.11);
  noiseflow kl_div_3_data at the 103 Noise Flow edges, N(0, 0.03) against N(0, 0.033);
  range     kl_div_range at 16383 bins over the pooled range of the default case's data (pooled only; its one synchronisation included).

Per case, in the same run and on the same buffers, two yardsticks:
  (a) the same result from torch ops on the device: torch.bucketize(x.double(), edges, right=True) - 1 with the last-bin fix, bincount,
      the KL lines (for `range`: torch min / max, the same host arange, then those);
  (b) metrics.kl_div_norm (the integer-DN score, csrc/noise_score.hip) over the same bytes.
HIP events over `--reps` calls after a warm-up, alternating between two sets of buffers (2 x 128 MB: no call finds its input cached by the
call before), `--runs` times over: the mean of the runs and their spread (max - min).  The condition: every case is faster than (a) by
more than the two spreads together.  The ratio to (b) is reported, not gated.  Beside them, to show what binds the count pass, the default
case's call on inputs that change the LDS traffic only: uniform samples (a wave's 64 adds go to 64 different words), and a constant (one add
per wave).
usage: kl_data_bench.py [--out FILE] [--reps N] [--runs N]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, S = 16, 512


def _us(fns, reps):
    """mean time of one call, alternating over `fns`"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for f in fns:
        f()
    torch.cuda.synchronize()
    e0.record()
    for i in range(reps):
        fns[i % len(fns)]()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def _runs(fns, reps, runs):
    t = [_us(fns, reps) for _ in range(runs)]
    return float(np.mean(t)), max(t) - min(t)


def _torch_hist(x, edges, per_crop):
    """np.histogram's counts / n with torch ops: [rows, nb] float64"""
    nb = edges.numel() - 1
    xd = x.double().reshape(x.shape[0] if per_crop else 1, -1)
    idx = torch.bucketize(xd, edges, right=True) - 1                        # the largest i with e[i] <= x; -1 below, nb at and beyond the last edge (and for a NaN)
    idx = torch.where(xd == edges[-1], nb - 1, idx)                         # the last bin is closed
    idx = torch.where((idx >= 0) & (idx < nb), idx, nb)                     # slot nb: in no bin
    rows = xd.shape[0]
    idx = idx + torch.arange(rows, device=x.device).reshape(rows, 1) * (nb + 1)
    counts = torch.bincount(idx.reshape(-1), minlength=rows * (nb + 1)).reshape(rows, nb + 1)[:, :nb]
    return counts.double() / xd.shape[1]


def _torch_kl3(p, q, edges, per_crop):
    yp, yq = _torch_hist(p, edges, per_crop), _torch_hist(q, edges, per_crop)
    both = (yp > 0) & (yq > 0)
    one = torch.ones_like(yp)
    lp, lq = torch.log(torch.where(both, yp, one)), torch.log(torch.where(both, yq, one))
    fwd, inv = (yp * (lp - lq)).sum(1), (yq * (lq - lp)).sum(1)
    return fwd, inv, (fwd + inv) / 2, yp, yq


def _torch_range(p, q, wp):
    v = torch.stack([p.min(), q.min(), p.max(), q.max()]).cpu().numpy()     # the same one synchronisation
    l, r = min(v[0], v[1]), max(v[2], v[3])
    bw = (r - l) / wp
    edges = torch.from_numpy(np.arange(l, r + bw, bw)).to(p.device)
    return _torch_kl3(p, q, edges, False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--runs', type=int, default=3)
    a = ap.parse_args()
    from pnnp_amd import metrics
    nbytes = 2 * B * 4 * S * S * 4
    g = torch.Generator(device='cuda').manual_seed(7)
    rn = lambda mu, sig: torch.randn(B, 4, S, S, device='cuda', generator=g) * sig + mu
    data = {'default': [(rn(0.5, 0.1), rn(0.5, 0.11)) for _ in range(2)], 'noiseflow': [(rn(0, 0.03), rn(0, 0.033)) for _ in range(2)]}
    data['range'] = data['default']
    data['uniform'] = [(torch.rand(B, 4, S, S, device='cuda', generator=g), torch.rand(B, 4, S, S, device='cuda', generator=g)) for _ in range(2)]
    data['constant'] = [(torch.full((B, 4, S, S), 0.25, device='cuda'), torch.full((B, 4, S, S), 0.75, device='cuda')) for _ in range(2)]
    nf = metrics.noise_flow_edges()
    e_default = torch.from_numpy(np.arange(0.0, 1.0 + 1 / 1000, 1 / 1000)).cuda()
    e_nf = torch.from_numpy(nf).cuda()
    lines = [f'float-edge histogram KL (csrc/hist_kl.hip) on {torch.cuda.get_device_name(0)}: {B} crops of 4x{S}x{S} float32, two sample sets, {nbytes / 1e6:.0f} MB '
             f'read once; HIP events, {a.runs} runs of {a.reps} calls after a warm-up, alternating two sets of buffers; mean of the runs +- their spread (max - min); '
             f'TB/s = {nbytes / 1e6:.0f} MB / time',
             f'{"case":<22s} {"kernel us":>10s} {"spread":>7s} {"TB/s":>6s} {"(a) torch ops us":>17s} {"spread":>7s} {"(a) / kernel":>13s} {"faster by more than the spreads":>32s} '
             f'{"(b) kl_div_norm us":>19s} {"kernel / (b)":>13s}   kl_fwd (crop 0)']
    ok_all = True
    for case, per_crop in (('default', False), ('default', True), ('noiseflow', False), ('noiseflow', True), ('range', False), ('uniform', False), ('constant', False)):
        sets = data[case]
        if case == 'range':
            kern = [lambda s=s: metrics.kl_div_range(s[0], s[1], wp=16383) for s in sets]
            ref = [lambda s=s: _torch_range(s[0], s[1], 16383) for s in sets]
            r, t = kern[0](), ref[0]()
            same = torch.equal(r['hist_p'][0], t[3][0]) and torch.equal(r['hist_q'][0], t[4][0])
            kl0, kl0_ref = float(r['kl_fwd']), float(t[0][0])
        else:
            kw = {'bin_edges': nf} if case == 'noiseflow' else {}
            ed = e_nf if case == 'noiseflow' else e_default
            kern = [lambda s=s: metrics.kl_div_3_data(s[0], s[1], per_crop=per_crop, return_hist=True, **kw) for s in sets]
            ref = [lambda s=s: _torch_kl3(s[0], s[1], ed, per_crop) for s in sets]
            r, t = kern[0](), ref[0]()
            same = torch.equal(r[3][0].reshape(t[3].shape), t[3]) and torch.equal(r[3][1].reshape(t[4].shape), t[4])
            kl0, kl0_ref = float(r[0].reshape(-1)[0]), float(t[0][0])
        assert same, f'{case}: the torch yardstick counts differently'
        assert abs(kl0 - kl0_ref) <= 1e-10 * max(abs(kl0_ref), 1e-3), (case, kl0, kl0_ref)
        score = [lambda s=s: metrics.kl_div_norm(s[0], s[1], per_crop=per_crop) for s in sets]
        t_k, s_k = _runs(kern, a.reps, a.runs)
        t_a, s_a = _runs(ref, max(a.reps // 4, 2), a.runs)
        t_b, _ = _runs(score, a.reps, a.runs)
        faster = t_a - t_k > s_a + s_k
        gated = case in ('default', 'noiseflow', 'range')
        ok_all &= faster or not gated
        lines.append(f'{case + (" per crop" if per_crop else " pooled"):<22s} {t_k:10.1f} {s_k:7.1f} {nbytes / t_k / 1e6:6.2f} {t_a:17.1f} {s_a:7.1f} {t_a / t_k:13.1f} '
                     f'{("yes" if faster else "NO") + ("" if gated else " (not gated)"):>32s} {t_b:19.1f} {t_k / t_b:13.2f}   {kl0:.6f}')
        print(lines[-1], flush=True)
    lines.append('every gated case faster than (a) by more than the spreads: ' + ('yes' if ok_all else 'NO'))
    print(lines[-1], flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    return 0 if ok_all else 1


if __name__ == '__main__':
    sys.exit(main())

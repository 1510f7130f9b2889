#!/usr/bin/env python3
"""Cost and calibration of the fp16x2 range census (csrc/range_census.hip; HipTrainStep range_every / range_max_share).

  1. census time and algorithmic TB/s (bytes of every split tensor read once) on the train step's tensors: config 3 (UNet nf=32,
     B=16, 512x512), config 5 (ResUnet nf=32, B=12, 512x512 with the random-init NoiseFlow proxy of bench.py) and B=1;
     the step time without a census; the amortised share at period P and the smallest power-of-two period at or below 0.1 %;
  2. calibration: the worst per-census low-bit share (16 bits) over a SID-like run (the soak's crops: rand^2.2 x 0.1, 0.1 % saturated,
     physics sampler with ratio ~ U(100, 300), clip 2) with a census every step, against range_max_share;
  3. the outlier case: one input pixel at 1e8 x the rest.
usage: range_census_bench.py [--out FILE] [--calib-steps N]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _net(arch, seed=1997):
    from pnnp_amd.archs import ResUnet, UNetSeeInDark, initialize_weights
    torch.manual_seed(seed); np.random.seed(seed)
    net = (UNetSeeInDark if arch == 'unet' else ResUnet)(dict(nframes=1, res=False, nf=32, in_nc=4, out_nc=4))
    initialize_weights(net)
    return net.cuda()


def _proxy(S):
    from pnnp_amd.archs import NoiseFlow
    proxy = NoiseFlow({'x_shape': (4, S, S), 'arch': 'sdn|unc|unc|unc|unc|giso|unc|unc|unc|unc'})
    with torch.no_grad():
        for k, v in proxy.state_dict().items():
            if k.endswith('conv2d_3.weight'):
                v.normal_(0, 0.05)
    return proxy.cuda().train()


def _ms(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def cost(label, arch, B, S, proxy=False, period=128):
    from pnnp_amd import ops
    from pnnp_amd.trainer import HipTrainStep
    net = _net(arch)
    px = _proxy(S) if proxy else None
    ts = HipTrainStep(net, lr=1e-4, clip=2, range_every=0, proxy_net=px, proxy_ratio_choices=(1, 2, 4, 8, 16) if proxy else None, proxy_iso=6400)
    hr = torch.rand(B, 4, S, S, device='cuda') * (0.01 if proxy else 1.0)
    step = lambda: ts.step(hr)
    for _ in range(3):
        step()
    step_ms = _ms(step, 10)
    # the census of the last step's tensors, alone (what HipTrainStep adds on a census step)
    step()
    rc = ops.RangeCensus(hr.device)
    pairs = net.engine.census_pairs()
    nbytes = sum(4 * t.numel() for _, _, t, _ in pairs)
    rc.run(pairs, 1)
    cen_ms = _ms(lambda: net.engine.range_census(rc, 1), 20)
    share = cen_ms / (period * step_ms)
    p = 1
    while cen_ms / (p * step_ms) > 1e-3:
        p *= 2
    return (f'{label:<34s} jobs {len(pairs):3d}  {nbytes / 1e9:6.2f} GB  census {cen_ms:7.3f} ms  {nbytes / cen_ms / 1e9:5.2f} TB/s   step {step_ms:7.2f} ms  '
            f'census / step {cen_ms / step_ms * 100:5.2f} %  amortised at period {period}: {share * 100:.4f} %  smallest period <= 0.1 %: {p}')


def _sid_like(B, S, gen):
    hr = torch.rand(B, 4, S, S, device='cuda', generator=gen) ** 2.2 * 0.1
    sat = torch.rand(B, 4, S, S, device='cuda', generator=gen) < 1e-3
    return torch.where(sat, torch.ones_like(hr), hr)


def calibrate(steps, B=4, S=256, max_share=1e-3):
    from pnnp_amd.trainer import HipTrainStep
    net = _net('unet', seed=5)
    ts = HipTrainStep(net, lr=1e-4, camera_type='SonyA7S2', noise_code='pr', clip=2, seed=1997, range_every=1, range_max_share=max_share)
    gen = torch.Generator(device='cuda').manual_seed(21)
    pool = [_sid_like(B, S, gen) for _ in range(6)]
    for s in range(steps):
        np.random.seed(1997 + s)
        ts.step(pool[s % 6])
    rows = ts.census.read()
    ts.census.reset()
    rows.sort(key=lambda r: -r['worst_share'])
    worst = rows[0]
    out = [f'calibration: {steps} steps, UNet nf=32, {B} crops of 4x{S}x{S} (rand^2.2 x 0.1, 0.1 % saturated; physics sampler SonyA7S2 pr, ratio U(100, 300), clip 2), '
           f'a census every step, 16 bits (bins k >= 24)',
           f'  worst per-census low-bit share {worst["worst_share"]:.3e} ({worst["kind"]} {worst["name"]}, step {worst["worst_step"]}); range_max_share {max_share:.0e}: '
           f'margin {max_share / max(worst["worst_share"], 1e-30):.1f}x' + (' (no element below 16 bits in any census)' if worst['worst_share'] == 0 else ''),
           f'  over {sum(r["over"] for r in rows)}, nonfinite {sum(r["nonfinite"] for r in rows)} over all {len(rows)} jobs',
           '  top 8 jobs: ' + ', '.join(f'{r["kind"]} {r["name"]} {r["worst_share"]:.2e} (median bin {r["log2_ratio"]:.0f}, k>=18 {r["frac_small"]:.2e})' for r in rows[:8])]
    return out


def outlier(B=2, S=256):
    import warnings
    from pnnp_amd._lib import PnnpRangeWarning
    from pnnp_amd.trainer import HipTrainStep
    net = _net('unet', seed=5)
    ts = HipTrainStep(net, lr=1e-4, clip=2, range_every=1)
    gen = torch.Generator(device='cuda').manual_seed(3)
    hr = _sid_like(B, S, gen)
    noisy = hr.clone() * 100
    noisy[0, 0, 17, 23] = float(noisy.max()) * 1e8
    ts.step(hr, noisy=noisy)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        rows = ts.check_range()
    trips = [r for r in rows if r['worst_share'] > ts.range_max_share or r['over'] or r['nonfinite']]
    return [f'outlier: one input pixel at 1e8 x the rest ({B} crops of 4x{S}x{S}): {len(trips)} of {len(rows)} jobs trip, '
            f'{sum(issubclass(w.category, PnnpRangeWarning) for w in rec)} warning(s)',
            '  ' + ', '.join(f'{r["kind"]} {r["name"]} {r["worst_share"]:.3f}' for r in trips[:10]) + (' ...' if len(trips) > 10 else '')]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--calib-steps', type=int, default=120)
    a = ap.parse_args()
    lines = [f'range census (csrc/range_census.hip) on {torch.cuda.get_device_name(0)}; census = the census launch + its summary, timed alone over 20 repeats '
             f'after a warm-up; TB/s = bytes of the split tensors (each read once) / time']
    for label, arch, B, proxy in (('config 3: UNet B=16 512x512', 'unet', 16, False), ('config 5: ResUnet+NF B=12 512x512', 'resunet', 12, True),
                                  ('UNet B=1 512x512', 'unet', 1, False)):
        lines.append(cost(label, arch, B, 512, proxy))
        print(lines[-1], flush=True)
    lines += calibrate(a.calib_steps)
    print('\n'.join(lines[-4:]), flush=True)
    lines += outlier()
    print('\n'.join(lines[-2:]), flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""Cost of the device-side noise-model score (csrc/noise_score.hip; metrics.noise_model_score), pair mode, 16 crops of 4x512x512
(3 x 64 MB read), on three inputs:

  narrow    physics-sampler noise, SonyA7S2 at ISO 1600, ratio 1;
  wide      the same x ratio 300;
  constant  a constant image, sampled noise 0 (every sample of p and of q in one bin).

Per input: the score (memset + the one-pass count + finish) through the C entry with its buffers allocated once, HIP events over `--reps`
calls after a warm-up, alternating between two sets of buffers (2 x 192 MB: more than the 256 MB Infinity Cache holds, so no call finds
its input cached by the call before); us and TB/s of the bytes read (3 images once); and the same through metrics.noise_model_score
(which allocates its outputs per call: host time shows there).  Beside it, in the same run and on the same buffers:
the plain read (pnnp_noise_score_read_f32: the score's grid -- one 1024-thread workgroup per CU, which the 132 KB of LDS force on the
score but not on a read -- and its loads, nothing else), a free-grid read (torch.sum of each image: three launches), and the host path the score replaces for ONE crop
(device-to-host copy of three 4 MB images + numpy with the reference's definition; the reference scores crop 0 only).
usage: noise_score_bench.py [--out FILE] [--reps N]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, S = 16, 512
BL, WP = 512, 16383


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


def _inputs(kind, seed):
    from pnnp_amd import process
    g = torch.Generator(device='cuda').manual_seed(seed)
    if kind == 'constant':
        clean = torch.full((B, 4, S, S), 0.25, device='cuda')
        return clean, clean.clone(), torch.zeros_like(clean)
    clean = torch.rand(B, 4, S, S, device='cuda', generator=g) ** 2.2 * 0.1                 # SID-like crops
    np.random.seed(seed)
    ratio = 300.0 if kind == 'wide' else 1.0
    prm = process.sample_params_max(camera_type='SonyA7S2', ratio=ratio, iso=1600)
    rows = process.pack_params([prm] * B, clean.device)
    flags = process.noise_flags('prq', torch_mode=True)
    real = process.noise_sample(clean, rows, flags, seed=seed, offset=1)
    noise = process.noise_sample(clean, rows, flags, seed=seed, offset=2) - clean
    return clean, real, noise


def _host_score(clean, real, noise):
    """The path the device score replaces (one crop): three copies to the host, then numpy with the reference's definition."""
    from pnnp_amd import metrics
    t0 = time.perf_counter()
    inputs = clean[0].cpu().numpy().clip(0, 1)
    output = noise[0].cpu().numpy() + inputs
    target = real[0].cpu().numpy()
    t1 = time.perf_counter()
    s = np.float32(WP - BL)
    p = np.round((target - inputs).flatten() * s); q = np.round((output - inputs).flatten() * s)
    if p.min() < 0:
        p = p + np.float32(512); q = q + np.float32(512)
    edges = metrics._kld_edges(16383)
    ys = [np.histogram((np.round(x).clip(0, 16383) / np.float32(16383)).astype(np.float32), edges)[0] / x.size for x in (p, q)]
    idx = (ys[0] > 0) & (ys[1] > 0)
    a, b = ys[0][idx], ys[1][idx]
    kl = float(np.sum(a * (np.log(a) - np.log(b))))
    stds = float(target.std()), float(output.std())
    t2 = time.perf_counter()
    return kl, stds, (t1 - t0) * 1e6, (t2 - t1) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=40)
    a = ap.parse_args()
    from pnnp_amd import _lib, metrics
    L = _lib.lib()
    nbytes = 3 * B * 4 * S * S * 4
    lines = [f'noise-model score (csrc/noise_score.hip) on {torch.cuda.get_device_name(0)}: pair mode, {B} crops of 4x{S}x{S}, {nbytes / 1e6:.0f} MB read once by the '
             f'algorithm; HIP events, mean of {a.reps} calls after a warm-up, alternating two sets of buffers; TB/s = {nbytes / 1e6:.0f} MB / time',
             f'{"input":<10s} {"score us":>9s} {"TB/s":>6s} {"plain read us":>14s} {"TB/s":>6s} {"score / read":>13s} {"torch.sum x3 us":>16s} {"TB/s":>6s} {"python call us":>15s}   kl_int of crop 0, std']
    sink = torch.zeros(B * 256, dtype=torch.int32, device='cuda')
    for kind in ('narrow', 'wide', 'constant'):
        sets = [_inputs(kind, 7), _inputs(kind, 8)]
        score = [lambda s=s: metrics.noise_model_score(*s, bl=BL, wp=WP, per_crop=True) for s in sets]
        n = 4 * S * S
        lut, edges = metrics._score_tables(16383, 512.0, sink.device)
        L = metrics._score_lib()
        ws = torch.empty(int(L.pnnp_noise_score_ws_bytes(B, C.c_int64(n))), dtype=torch.uint8, device='cuda')
        hist = torch.empty(B, 2, edges.numel() - 1, dtype=torch.float64, device='cuda'); out = torch.empty(B, 8, dtype=torch.float64, device='cuda')
        score_c = [lambda s=s: _lib.check(L.pnnp_noise_score_f32(*[_lib.ptr(t) for t in s], B, C.c_int64(n), C.c_float(WP - BL), C.c_float(512.0), 16383,
                                                                  _lib.ptr(lut), edges.numel() - 1, _lib.ptr(ws), _lib.ptr(hist), _lib.ptr(out), _lib.stream()), 'score')
                   for s in sets]
        read = [lambda s=s: _lib.check(L.pnnp_noise_score_read_f32(*[_lib.ptr(t) for t in s], B, C.c_int64(4 * S * S), _lib.ptr(sink), _lib.stream()), 'read')
                for s in sets]
        free = [lambda s=s: [t.sum() for t in s] for s in sets]
        t_free = _us(free, a.reps)
        t_read = _us(read, a.reps)
        t_score = _us(score_c, a.reps)
        t_py = _us(score, a.reps)
        t_read2 = _us(read, a.reps)
        res = score[0]()
        score_c[0]()
        assert torch.equal(out[:, 0], res['kl_int']) and torch.equal(out[:, 3], res['gt_std'])
        lines.append(f'{kind:<10s} {t_score:9.1f} {nbytes / t_score / 1e6:6.2f} {min(t_read, t_read2):14.1f} {nbytes / min(t_read, t_read2) / 1e6:6.2f} '
                     f'{t_score / min(t_read, t_read2):13.2f} {t_free:16.1f} {nbytes / t_free / 1e6:6.2f} {t_py:15.1f}   {metrics.score_log_line(res)}   (plain read before / after: {t_read:.1f} / {t_read2:.1f} us)')
        print(lines[-1], flush=True)
        if kind != 'constant':
            _host_score(*sets[0])
            kl, stds, t_copy, t_np = _host_score(*sets[0])
            lines.append(f'           host path, ONE crop (3 x {4 * S * S * 4 / 1e6:.1f} MB): copies {t_copy:.0f} us + numpy {t_np:.0f} us = {t_copy + t_np:.0f} us; '
                         f'kl_int {kl:.6f} (device crop 0: {float(res["kl_int"][0]):.6f}), std {stds[1]:.3f} vs {stds[0]:.3f}')
            print(lines[-1], flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

"""The paired-data preprocess branch, batched pass against the per-crop loop it replaces:

    python tools/sna_batch_bench.py [--out profiles/r7/sna_batch.txt] [--reps 25]

Workload: 16 crops of 4x512x512, SonyA7S2 (ISO 1600), ratio ~ U(100, 300), 'augv2' gains, clip: 2 -- the shape of runfiles/SonyA7S2/PMN.yml.
Three forms, timed in ONE process with device events around each call, alternated round by round after warm-up rounds; median [min .. max]:
  * batched: process.sna_rows (host K draws, table upload) + process.sna_batch (one launch);
  * kernel only: process.sna_batch on a table that is already on the device (the figure behind the B/s);
  * composition: the loop of trainer_SID.py:436-447,481-485 on process.SNA_torch -- per crop the digital gain, SNA_torch, two adds, two stores
    into the batch, then the two clamps over the batch.
The kernel's traffic is counted from the shape: 16 B per element (lr and hr read once, written once)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from pnnp_amd import process as P


def composition(lr, hr, aug, ratio_dev, ratio_host, iso, ori, clip):
    """-> (lr_out, hr_out, launches): the reference's loop, its ops counted as they are issued"""
    lr, hr = lr.clone(), hr.clone()                                          # the loop writes into the batch (2 launches, not counted)
    launches = 0
    for i in range(lr.shape[0]):
        if not ori:
            lr[i] = lr[i] * ratio_dev[i]; launches += 2                      # mul + store into the batch
        if np.abs(aug[i]).max() != 0:
            dn, dy = P.SNA_torch(hr[i], aug[i], camera_type='SonyA7S2', ratio=ratio_host[i], black_lr=False, ori=ori, iso=iso)
            lr[i] = lr[i] + dn
            hr[i] = hr[i] + dy
            launches += 5                                                    # sna_kernel, 2 adds, 2 stores
    if clip:
        lr = lr.clamp(-np.inf if clip == P.HALF_CLIP else 0, 1)
        hr = hr.clamp(0, 1)
        launches += 2
    return lr, hr, launches


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'r7', 'sna_batch.txt'))
    ap.add_argument('--reps', type=int, default=25)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--crops', type=int, default=16)
    ap.add_argument('--patch', type=int, default=512)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'this benchmark needs the GPU'
    B, S, iso, ori, clip = a.crops, a.patch, 1600, False, P.HALF_CLIP
    g = torch.Generator(device='cuda').manual_seed(0)
    hr = torch.rand(B, 4, S, S, device='cuda', generator=g) ** 2
    np.random.seed(0); torch.manual_seed(0)                                  # seed 0: the randint(4) != 0 path, gains are drawn
    ar, ag, ab = P.get_aug_param_torch({}, b=B, command='augv2')
    ratio_host = torch.from_numpy(np.random.uniform(100, 300, B)).float()
    ratio_dev = ratio_host.cuda()
    lr = (hr + 0.01 * torch.randn(hr.shape, device='cuda', generator=g)) / ratio_dev.view(B, 1, 1, 1)
    aug_wbs = torch.stack((ar, ag, ab, ag), dim=1)
    aug = aug_wbs.numpy()
    active = int((np.abs(aug).max(axis=1) != 0).sum())
    assert active > 0
    rows, K = P.sna_rows(aug_wbs, ratio_host, [iso], 'SonyA7S2', False, B)
    rates = (hr.reshape(B, 4, -1).mean(-1).cpu().numpy() * (16383 - 512) / ratio_host.numpy()[:, None] * aug / np.where(K > 0, K, 1)[:, None])
    out_l, out_h = torch.empty_like(lr), torch.empty_like(hr)
    launches = [0]

    def f_batched():
        r, _ = P.sna_rows(aug_wbs, ratio_host, [iso], 'SonyA7S2', False, B)
        P.sna_batch(lr, hr, r, ori, clip, seed=1997, offset=0, out_lr=out_l, out_hr=out_h)

    def f_kernel():
        P.sna_batch(lr, hr, rows, ori, clip, seed=1997, offset=0, out_lr=out_l, out_hr=out_h)

    def f_comp():
        launches[0] = composition(lr, hr, aug, ratio_dev, ratio_host, iso, ori, clip)[2]

    forms = (('batched: sna_rows + sna_batch', f_batched), ('kernel only: sna_batch', f_kernel), ('composition: SNA_torch loop + adds + clamps', f_comp))
    t = {name: [] for name, _ in forms}
    for r in range(a.warmup + a.reps):
        for name, fn in forms:
            us = timed(fn)
            if r >= a.warmup:
                t[name].append(us)
    n_el = hr.numel()
    lines = [f'paired-data preprocess, {B} crops of 4x{S}x{S}, SonyA7S2 ISO {iso}, ratio U(100,300), augv2 ({active} of {B} crops active), ori False, clip 2; '
             f'us per call, median [min .. max] of {a.reps} alternated rounds after {a.warmup} warm-up rounds; device {torch.cuda.get_device_name(0)}',
             f'mean Poisson rate per active crop and plane: min {rates[rates > 0].min():.2f}, median {np.median(rates[rates > 0]):.2f}, max {rates.max():.2f}']
    med = {}
    for name, _ in forms:
        v = np.array(t[name])
        med[name] = float(np.median(v))
        lines.append(f'  {name:50s} {np.median(v):10.1f} [{v.min():10.1f} .. {v.max():10.1f}]')
    k = med['kernel only: sna_batch']
    lines.append(f'  launches: batched 1 (+ 1 table upload), composition {launches[0]} (counted as its ops are issued)')
    lines.append(f'  kernel only: {16 * n_el / 1e6:.1f} MB algorithmic (16 B per element) = {16 * n_el / k / 1e3:.1f} GB/s; '
                 f'{k * 1e6 / n_el:.2f} ps per element')
    lines.append(f'  ratio composition / batched = {med[forms[2][0]] / med[forms[0][0]]:.2f} '
                 f'(batched max {max(t[forms[0][0]]):.1f} us, composition min {min(t[forms[2][0]]):.1f} us)')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()

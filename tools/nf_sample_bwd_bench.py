"""NoiseFlow.sample's backward against the NLL backward at the same shape (default 16 x 4 x 512 x 512, training mode): in one run it
times  sample()  |  sample(differentiable=True) and its backward  |  loss() and its backward,  each after a warm-up, with device events
(forward and backward separately), and states the algorithmic HBM bytes each moves (4-plane fp32 maps; halo re-reads and the
per-workgroup partial rows are not counted) and the rate that gives.  The kernels are HBM-bound, so the figure of merit is the sample
backward's achieved rate as a fraction of the NLL backward's.  Needs a GPU.
python tools/nf_sample_bwd_bench.py [--B 16] [--P 512] [--steps 10] [--eval]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# maps ([B][4][P][P] fp32) read + written per pair, from the pass lists in DESIGN.md section 4.7
SAMPLE_EVAL = 2.0                            # step: u in, out
SAMPLE_TRAIN = 0.5 + 1 + 2 + 2.0             # statistics: u[0:2] -> h1; h1 -> h2; then the step
SAMPLE_BWD = 2.5 + 2 + 6 + 4 + 3.5           # hidden, out3, couple, conv2, conv1
NLL_FWD, NLL_BWD = 8.0, 14.0                 # nf_train.hip: conv1 2, conv2 2, couple 4 | couple 5, conv2 4, conv1 5


def timed(fwd, steps, backward):
    """mean ms of fwd() and of .backward() on its result over `steps` runs (device events), after two warm-up runs"""
    ev = lambda: torch.cuda.Event(enable_timing=True)
    tf = tb = 0.0
    for i in range(steps + 2):
        e0, e1, e2 = ev(), ev(), ev()
        e0.record()
        out = fwd()
        e1.record()
        if backward:
            out.backward()
        e2.record(); torch.cuda.synchronize()
        if i >= 2:
            tf += e0.elapsed_time(e1); tb += e1.elapsed_time(e2)
    return tf / steps, tb / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--B', type=int, default=16); ap.add_argument('--P', type=int, default=512)
    ap.add_argument('--steps', type=int, default=10); ap.add_argument('--eval', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('nf_sample_bwd_bench needs a GPU (no CPU path)')
    from pnnp_amd.archs import NoiseFlow
    np.random.seed(0); torch.manual_seed(0)
    net = NoiseFlow({'x_shape': (4, a.P, a.P), 'arch': 'sdn|unc|unc|unc|unc|giso|unc|unc|unc|unc'}).cuda()
    with torch.no_grad():                                            # off the zero inits, so that every ReLU mask and gradient is live
        for k, p in net.named_parameters():
            if 'conv2d_3' in k or k.endswith('logs'):
                p.normal_(0.0, 0.05)
    net.train(not a.eval)
    clean = torch.rand(a.B, 4, a.P, a.P, device='cuda') * 0.05
    noise = torch.randn_like(clean) * torch.sqrt(clean * 2e-3 + 1e-5)
    cot = torch.randn_like(clean)
    M = clean.numel() * 4                                            # bytes of one map
    pairs = 8
    s_fwd = pairs * (SAMPLE_EVAL if a.eval else SAMPLE_TRAIN) + 1    # + clean on the last pair
    rows = [('sample()', lambda: net.sample(clean=clean, iso=1600.0), False, s_fwd, 0.0),
            ('sample(differentiable=True) + backward', lambda: (net.sample(clean=clean, iso=1600.0, differentiable=True) * cot).sum(), True,
             s_fwd + 2, pairs * SAMPLE_BWD + 1 + 2),                 # + the objective's product and its backward (2 maps each)
            ('loss() + backward (training mode)', lambda: net.loss(noise=noise, clean=clean, iso=1600.0)[0], True,
             pairs * NLL_FWD + 2 + 2, pairs * NLL_BWD + 2)]         # + clean twice on the first pair, + the copy of the input | + clean twice
    print(f'shape {a.B} x 4 x {a.P} x {a.P}, one map = {M / 1e6:.1f} MB, BatchNorm mode of the sample rows: {"eval" if a.eval else "training"}, '
          f'{a.steps} timed runs after 2 warm-up runs, device events')
    rate = {}
    for name, fn, bwd, mf, mb in rows:
        if name.startswith('loss'):
            net.train()
        net.zero_grad(set_to_none=True)
        tf, tb = timed(fn, a.steps, bwd)
        line = f'{name:48s} forward {tf:8.3f} ms  {mf * M / 1e9:6.2f} GB  {mf * M / tf / 1e6:7.0f} GB/s'
        if bwd:
            line += f' | backward {tb:8.3f} ms  {mb * M / 1e9:6.2f} GB  {mb * M / tb / 1e6:7.0f} GB/s'
            rate[name[:4]] = mb * M / tb
        print(line)
    print(f'sample backward rate / NLL backward rate (same shape, algorithmic bytes): {rate["samp"] / rate["loss"]:.3f}')


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""How much of a small-batch train step is host time: the question a graph-captured step would answer (nf = 32, 4 x 512 x 512 crops,
noise code 'pr', clip 2 -- the bench.py workload at other batch sizes).  Results: profiles/r7/graph_step.txt.

    python tools/graph_step_bench.py --batches 1,2,4,16
        per batch size: the eager step's wall time (`--rounds` rounds of `--steps` steps, median and spread of the per-round ms / step),
        and the host's issue time of one step: how long HipTrainStep.step takes to return when it starts on an idle GPU (median of
        `--issue-steps` steps, each followed by a synchronisation).  One JSON line per batch size.

    rocprofv3 --kernel-trace --stats -d DIR -o NAME -- python tools/graph_step_bench.py --batches 1 --rounds 1 --steps 20 --issue-steps 0
    python tools/graph_step_bench.py --analyze DIR [--wall-ms 2.88]
        the kernels of each step of the trace (a step ends with the Adam kernel; the first complete step is not counted): the summed
        kernel time per step, the trace's step span and the share of it in which no kernel runs, and -- with the wall time of the
        un-profiled run -- the share of the real step in which no kernel runs.  That share is all a graph replay of the step can save."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def run(args):
    import numpy as np
    import torch
    from pnnp_amd.archs import UNetSeeInDark, initialize_weights
    from pnnp_amd.trainer import HipTrainStep
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    for B in [int(b) for b in args.batches.split(',')]:
        torch.manual_seed(1997)
        np.random.seed(1997)
        net = UNetSeeInDark(dict(nframes=1, res=False, nf=32, in_nc=4, out_nc=4))
        initialize_weights(net)
        net = net.to(dev)
        ts = HipTrainStep(net, lr=1e-4, camera_type='SonyA7S2', noise_code='pr', ori=False, clip=2, seed=1997)
        hr = torch.rand(B, 4, args.size, args.size, device=dev, generator=torch.Generator(device=dev).manual_seed(1234))
        step = 0

        def one():
            nonlocal step
            np.random.seed(1997 + step)
            ts.step(hr)
            step += 1

        for _ in range(args.warmup):
            one()
        torch.cuda.synchronize()
        per = []
        for _ in range(args.rounds):
            t0 = time.perf_counter()
            for _ in range(args.steps):
                one()
            torch.cuda.synchronize()
            per.append(1e3 * (time.perf_counter() - t0) / args.steps)
        issue = []
        for _ in range(args.issue_steps):
            t0 = time.perf_counter()
            one()
            issue.append(1e3 * (time.perf_counter() - t0))
            torch.cuda.synchronize()
        r = dict(batch=B, ms_per_step=round(statistics.median(per), 4), min=round(min(per), 4), max=round(max(per), 4), rounds=len(per), steps=args.steps)
        if issue:
            r['host_issue_ms'] = round(statistics.median(issue), 4)
        print(json.dumps(r), flush=True)
        del ts, net, hr
        torch.cuda.empty_cache()


def summarize(kernels, wall_ms=None):
    """``kernels``: (start_ns, end_ns, name) of one stream's launches.  Per step (ending with an Adam launch; the steps before the first and
    after the last one are not counted, nor the first complete one, which may still carry set-up): launches, summed kernel time, span from the
    previous step's Adam end to this one's."""
    ks = sorted(kernels)
    ends = [i for i, k in enumerate(ks) if 'adam_kernel' in k[2]]
    if len(ends) < 3:
        raise ValueError(f'{len(ends)} Adam launches in the trace: too few steps')
    steps = []
    for a, b in zip(ends[:-1], ends[1:]):
        seg = ks[a + 1:b + 1]
        steps.append((len(seg), sum(e - s for s, e, _ in seg), ks[b][1] - ks[a][1]))
    steps = steps[1:]
    n = len(steps)
    ksum = sum(s[1] for s in steps) / n / 1e6
    span = sum(s[2] for s in steps) / n / 1e6
    out = dict(steps=n, kernels_per_step=statistics.median(s[0] for s in steps), kernel_ms_per_step=round(ksum, 4),
               trace_span_ms=round(span, 4), trace_gap_share=round(1 - ksum / span, 4))
    if wall_ms:
        out.update(wall_ms=wall_ms, gap_share=round(1 - ksum / wall_ms, 4))
    return out


def analyze(args):
    files = sorted(glob.glob(os.path.join(args.analyze, '**', '*kernel_trace.csv'), recursive=True))
    if not files:
        raise SystemExit(f'no *kernel_trace.csv under {args.analyze}')
    ks = []
    for f in files:
        with open(f) as fh:
            ks += [(int(r['Start_Timestamp']), int(r['End_Timestamp']), r['Kernel_Name']) for r in csv.DictReader(fh)]
    print(json.dumps(dict(trace=args.analyze, **summarize(ks, args.wall_ms))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='1,2,4,16')
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--issue-steps', type=int, default=20, help='steps that each start on an idle GPU, for the host issue time (0: none)')
    ap.add_argument('--analyze', metavar='DIR', help='summarise the rocprofv3 kernel trace(s) under DIR instead of running')
    ap.add_argument('--wall-ms', type=float, help='with --analyze: the un-profiled ms / step, for the gap share of the real step')
    args = ap.parse_args()
    if args.analyze:
        analyze(args)
    else:
        run(args)


if __name__ == '__main__':
    main()

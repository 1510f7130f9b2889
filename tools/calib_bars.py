#!/usr/bin/env python3
"""How well the dark-frame estimators recover known parameters: the bars of tests/test_gpu_calib.py::test_round_trip_through_the_sampler.

Runs on the CPU and touches no product code: the stack is drawn by the C oracle sampler (oracle/cbind.noise_sample) over SEEDS seeds and
fitted by the float64 restatement (tests/_calib_ref.py) alone.  Each bar is |mean error| + 5 std over the seeds of THIS reference run.

    python tools/calib_bars.py [--seeds 24] [--frames 32] [--h 32] [--w 64] [--lam-points 121]
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))

TRUE = dict(K=1.0, sigGs=3.0, sigTL=3.2, lam=-0.05, sigR=1.0, q=1 / 16384, ratio=1.0, wp=16383, bl=512, bias=0)


def main():
    import _calib_ref as R
    from oracle import cbind
    ap = argparse.ArgumentParser()
    ap.add_argument('--seeds', type=int, default=24)
    ap.add_argument('--frames', type=int, default=32)
    ap.add_argument('--h', type=int, default=32, help='rows of a packed plane')
    ap.add_argument('--w', type=int, default=64, help='columns of a packed plane')
    ap.add_argument('--lam-points', type=int, default=121, help='points of the lam grid over [-0.3, 0.3] (121: the default grid)')
    a = ap.parse_args()
    grid = np.linspace(-0.3, 0.3, a.lam_points)
    flags = cbind.noise_flags('pgr', ori=True, clip=False, torch_mode=True) | 0x8000
    want = dict(sigTL=TRUE['sigTL'], lam=TRUE['lam'], sigR=TRUE['sigR'], sigGs=R.matching_sigGs(TRUE['sigTL'], TRUE['lam']))
    got = {k: [] for k in want}
    for seed in range(a.seeds):
        z = cbind.noise_sample(np.zeros((a.frames, 4, a.h, a.w), np.float32), cbind.param_rows([TRUE] * a.frames), flags, seed=seed, offset=0)
        fit = R.fit_dark(R.planes_to_mosaics(z, TRUE['wp'], TRUE['bl']), TRUE['K'], TRUE['wp'], TRUE['bl'], lam_grid=grid)
        for k in want:
            got[k].append(fit[k])
    print(f'# {a.seeds} seeds, {a.frames} frames of [4,{a.h},{a.w}] -> mosaics {2 * a.h}x{2 * a.w}; drawn by the C oracle sampler, fitted by tests/_calib_ref.py, lam grid of {a.lam_points} points')
    print('# parameter   true        mean        mean error  std         bar = |mean error| + 5 std   bar / true')
    for k, t in want.items():
        e = np.array(got[k]) - t
        bar = abs(e.mean()) + 5 * e.std(ddof=1)
        print(f'{k:10s} {t:11.6f} {np.mean(got[k]):11.6f} {e.mean():+11.6f} {e.std(ddof=1):11.6f} {bar:11.6f} {bar / abs(t):28.3f}')


if __name__ == '__main__':
    main()

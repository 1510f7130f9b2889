"""bench.py's command line: --steps / --warmup validation, what --dump-outputs writes, and a plain run (the timed steps only)
against a --full run (roofline, per-class kernel table, CPU baseline) of the same small configuration."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args, timeout=600):
    return subprocess.run([sys.executable, os.path.join(REPO, 'bench.py')] + args, capture_output=True, text=True, timeout=timeout, cwd=REPO)


def _line(r):
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.parametrize('args', [['--steps', '0'], ['--warmup', '-1']])
def test_steps_and_warmup_are_checked(args):
    r = _bench(args, timeout=120)
    assert r.returncode == 2 and '--steps must be at least 1' in r.stderr


@pytest.mark.parametrize('arch', ['unet', 'resunet'])
def test_dump_outputs_float32_under_64mb(tmp_path, arch):
    """The benchmark's networks at nf=32: float32 files under 64 MB in all; params and grad keep the same positions (the full
    vectors when they fit, UNet; the same seeded sample when they do not, ResUnet).  Host buffers only: no kernel runs."""
    from pnnp_amd.archs import ResUnet, UNetSeeInDark, initialize_weights
    torch.manual_seed(1997)
    net = (UNetSeeInDark if arch == 'unet' else ResUnet)(dict(nframes=1, res=False, nf=32, in_nc=4, out_nc=4))
    initialize_weights(net)
    net.engine.params.ensure(torch.device('cpu'))
    for n, p in net.named_parameters():
        net.engine.params.grad_view(n, p.shape).copy_(p.detach() * 2 + 1)
    loss = torch.arange(17, dtype=torch.float32)
    bench.dump_outputs(str(tmp_path), loss, net)
    files = sorted(os.listdir(tmp_path))
    assert files == ['grad.npy', 'loss.npy', 'params.npy']
    assert sum(os.path.getsize(tmp_path / f) for f in files) < 64e6
    a = {f[:-4]: np.load(tmp_path / f) for f in files}
    assert all(v.dtype == np.float32 for v in a.values())
    assert np.array_equal(a['loss'], loss.numpy())
    assert np.array_equal(a['grad'], a['params'] * np.float32(2) + np.float32(1))
    flat = torch.cat([p.detach().reshape(-1) for _, p in net.named_parameters()]).numpy()
    if arch == 'unet':
        assert np.array_equal(a['params'], flat)
    else:
        assert a['params'].size < flat.size and np.isin(a['params'], flat).all()


@pytest.mark.gpu
def test_plain_and_full_runs(tmp_path):
    common = ['--gpus', '1', '--steps', '2', '--warmup', '1', '--size', '64', '--batch', '2']
    plain = _line(_bench(common + ['--dump-outputs', str(tmp_path / 'plain')]))
    assert plain['steps'] == 2 and plain['warmup'] == 1 and plain['ms_per_step'] > 0
    assert abs(plain['value'] - 2 * 2 / (plain['ms_per_step'] * 2e-3)) < 1e-6 * plain['value']
    assert 'cpu_baseline' not in plain and 'kernel_classes' not in plain and plain['roofline']['achieved'] is None
    lp = np.load(tmp_path / 'plain' / 'loss.npy')
    assert lp.shape == (3,) and lp[0] == np.float32(plain['final_loss'])
    full = _line(_bench(common + ['--full', '--cpu-baseline-seconds', '5', '--dump-outputs', str(tmp_path / 'full')]))
    assert full['roofline']['achieved'] > 0 and full['kernel_classes'] and full['cpu_baseline']['timed_steps'] >= 1
    # same arguments, same seeded inputs; --full's un-timed profiling steps run after the dump
    lf = np.load(tmp_path / 'full' / 'loss.npy')
    assert np.allclose(lf, lp, rtol=1e-5, atol=0), (lf, lp)
    pp, pf = np.load(tmp_path / 'plain' / 'params.npy'), np.load(tmp_path / 'full' / 'params.npy')
    assert pp.shape == pf.shape and float(np.mean(np.abs(pp - pf) < 1e-6)) > 0.999

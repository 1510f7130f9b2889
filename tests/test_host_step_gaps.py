"""tools/graph_step_bench.py's trace summary (CPU, no GPU): per train step, the summed kernel time, the span and the share of the
step in which no kernel runs -- what a graph-captured step could save (profiles/r7/graph_step.txt)."""
import csv
import json
import os
import subprocess
import sys

import pytest

from tools import graph_step_bench as gsb

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADAM = 'void (anonymous namespace)::adam_kernel(float*, float const*, float*, float*, long, float, float, float, float, float, float, float)'


def _trace(n_steps, gap_us, t0=10 ** 15):
    """n_steps steps of three kernels (100 + 300 + 50 us), `gap_us` before the second kernel of every step, 10 us between the others."""
    ks, t = [], t0
    for _ in range(n_steps):
        for name, dur, gap in (('noise_sample_kernel', 100000, 10000), ('igemm_h2s_kernel<64, 4>', 300000, 1000 * gap_us), (ADAM, 50000, 10000)):
            t += gap
            ks.append((t, t + dur, name))
            t += dur
    return ks


def test_summary_of_a_known_trace():
    ks = _trace(6, gap_us=40)
    s = gsb.summarize(ks[::-1])                      # any order: sorted by start
    assert s['steps'] == 4                           # 5 complete steps between 6 Adam launches, the first of them dropped
    assert s['kernels_per_step'] == 3
    assert s['kernel_ms_per_step'] == pytest.approx(0.45)
    assert s['trace_span_ms'] == pytest.approx(0.51)
    assert s['trace_gap_share'] == pytest.approx(1 - 450 / 510, abs=1e-4)
    w = gsb.summarize(ks, wall_ms=0.6)
    assert w['gap_share'] == pytest.approx(0.25, abs=1e-4)


def test_gapless_trace_and_too_few_steps():
    assert gsb.summarize(_trace(5, gap_us=0))['trace_span_ms'] == pytest.approx(0.47)
    with pytest.raises(ValueError):
        gsb.summarize(_trace(2, gap_us=0))


def test_analyze_reads_rocprofv3_csv(tmp_path):
    d = tmp_path / 'tr' / 'host'
    d.mkdir(parents=True)
    with open(d / 'b1_kernel_trace.csv', 'w', newline='') as f:
        w = csv.writer(f, quoting=csv.QUOTE_NONNUMERIC)
        w.writerow(['Kind', 'Kernel_Name', 'Start_Timestamp', 'End_Timestamp'])
        for s, e, n in _trace(4, gap_us=40):
            w.writerow(['KERNEL_DISPATCH', n, s, e])
    out = subprocess.run([sys.executable, os.path.join(REPO, 'tools', 'graph_step_bench.py'), '--analyze', str(tmp_path / 'tr'),
                          '--wall-ms', '0.51'], check=True, capture_output=True, text=True).stdout
    r = json.loads(out.strip().splitlines()[-1])
    assert r['steps'] == 2 and r['kernel_ms_per_step'] == pytest.approx(0.45) and r['gap_share'] == pytest.approx(1 - 450 / 510, abs=1e-4)

"""The CPU restatement of NoiseFlow.sample that the sample-backward tests differentiate (tests/_nf_sample_ref.py), pinned without a
GPU: its float32 eval-mode values are those of oracle.noiseflow_torch.sample, its training-mode values those of the reference's own
train-mode sample (goldens ts_out_iso*), fixed statistics equal to the batch's reproduce the batch-statistics values while the
gradients differ, and the public surface of the feature exists."""
import os

import numpy as np
import torch

from oracle import noiseflow_torch as O
from tests import _nf_sample_ref as R


def _golden(golden_dir):
    g = np.load(os.path.join(golden_dir, 'noiseflow.npz'))
    return g, {k: torch.from_numpy(g['sd:' + k]) for k in [str(x) for x in g['keys']]}


def test_float32_eval_values_equal_the_oracle(golden_dir):
    _g, sd = _golden(golden_dir)
    gen = torch.Generator().manual_seed(9)
    clean = torch.rand(3, 4, 50, 70, generator=gen) * 0.02; z = torch.randn(3, 4, 50, 70, generator=gen)
    for iso in (800.0, 3000.0):
        assert torch.equal(R.sample(sd, clean, iso, z, 'running', torch.float32), O.sample(sd, clean, torch.tensor(iso), z))


def test_training_mode_values_match_the_reference_golden(golden_dir):
    g, sd = _golden(golden_dir)
    clean = torch.from_numpy(g['tr_clean']); z = torch.from_numpy(g['ts_z'])
    for iso in (1600, 3000):
        ref = g[f'ts_out_iso{iso}']
        for dt in (torch.float32, torch.float64):
            got = R.sample(R._cast(sd, dt), clean.to(dt), iso, z.to(dt), 'batch', dt).numpy()
            scale = np.abs(ref).max(); err = np.abs(got - ref)                   # _close_chain's bar (tests/test_gpu_noiseflow.py)
            assert (err <= 2e-4 * np.abs(ref) + 2e-4 * scale).mean() >= 0.999
            assert (err <= 5e-2 * np.abs(ref) + 5e-3 * scale).all()


def test_matched_fixed_statistics_give_the_batch_values_and_other_gradients(golden_dir):
    _g, sd = _golden(golden_dir)
    gen = torch.Generator().manual_seed(1)
    z = torch.randn(2, 4, 16, 16, generator=gen); clean = torch.rand(2, 4, 16, 16, generator=gen) * 0.02
    cot = torch.randn(2, 4, 16, 16, generator=gen)
    stats = R.batch_stats(sd, clean, 1600.0, z)
    xb, gb = R.value_and_grads(sd, clean, 1600.0, z, cot, 'batch', torch.float64)
    xf, gf = R.value_and_grads(sd, clean, 1600.0, z, cot, stats, torch.float64)
    assert len(gb) == 126 and set(gb) == set(gf)                                # 125 trainable parameters and z
    assert float((xb - xf).abs().max()) <= 1e-12 * float(xb.abs().max())
    assert R.worst_rel(gf, gb) > 1.0                                             # the two modes are told apart
    assert R.check(gb, gb, 0.0) == [] and R.check(gf, gb, 2e-4) != []


def test_public_surface():
    import inspect
    from pnnp_amd.archs import NoiseFlow
    from pnnp_amd.trainer import NoiseFlowFitStep
    assert callable(NoiseFlowFitStep.ddl_step)
    assert list(inspect.signature(NoiseFlowFitStep.ddl_step).parameters)[1:] == ['hr', 'iso', 'kind', 'x', 'lr']
    assert 'differentiable' in NoiseFlow.sample.__doc__

"""The one-pair float64 reference of the NoiseFlow kernel tests (tests/_nf_pair_ref.py), pinned without a GPU.

1. Eight chained ``sample_pair`` calls on blocks built per the header from the golden state dict reproduce
   ``tests/_nf_sample_ref.sample(..., dtype=float64)`` (running and batch statistics); eight chained ``density_pair`` / ``train_pair``
   calls reproduce ``oracle.noiseflow_torch.forward`` / ``loss`` run in float64 (eval and training mode).  All are float64
   restatements of one another, only the order of sums differs: 1e-12 of the output's scale.
2. ``train_pair_bwd`` is the gradient of the function ``train_pair`` returns the values of (central differences in float64).
3. Sensitivity: each defect class that tests/test_gpu_nf_pairs.py exists to catch, planted in the reference itself, moves some element
   by more than 100x that test's bar (4 E32, plus the transcendental allowance for the sampling step) at every case shape that can
   reach it, with the very parameter draws of the GPU tests.
4. The seeds of the backward cases leave at most 2 % of the pixels out of the dx comparison."""
import os

import numpy as np
import pytest
import torch

from oracle import noiseflow_torch as O
from tests import _nf_pair_ref as P
from tests import _nf_sample_ref as R

F64 = torch.float64


def _golden(golden_dir):
    g = np.load(os.path.join(golden_dir, 'noiseflow.npz'))
    return g, {k: torch.from_numpy(g['sd:' + k]) for k in [str(x) for x in g['keys']]}


def _close(got, ref, what):
    err, scale = float((got - ref).abs().max()), float(ref.abs().max())
    assert err <= 1e-12 * scale, (what, err, scale)


# ------------------------------------------------------------------------------------------------------------ 1. the chains
@pytest.mark.parametrize('mode', ('running', 'batch'))
def test_eight_sample_pairs_are_the_sample_chain(golden_dir, mode):
    g, sd0 = _golden(golden_dir)
    sd = R._cast(sd0, F64)
    clean, z = torch.from_numpy(g['tr_clean']).double(), torch.from_numpy(g['ts_z']).double()
    for iso in (1600.0, 3000.0):                                            # a table hit and an interpolated ISO
        gs, a, b = P.chain_scalars(sd, iso)
        x = z
        for k in P.COUPLING_IDX[::-1]:
            winv = P.conv_matrices(sd, k - 1)[1] * (gs if k == 11 else 1.0)   # GainISO^-1 follows Conv2d1x1^-1 of model.10
            step = torch.cat([P.step_vector(sd, k, train=mode == 'batch'), winv.reshape(-1)])
            bn = P.stats(P.prm_block(sd, k), x) if mode == 'batch' else None
            x = P.sample_pair(step, x, clean if k == 2 else None, float(a), float(b), 1.0, bn_stats=bn)
        _close(x, R.sample(sd, clean, iso, z, mode, F64), (mode, iso))


def _density_chain(sd, noise, clean, iso, training):
    """-> (z, objective per crop, sum z^2 per crop) from eight density_pair / train_pair calls"""
    B, C, H, W = noise.shape
    gs, a, b = P.chain_scalars(sd, iso)
    obj = torch.zeros(B, dtype=F64)
    x = noise
    for k in P.COUPLING_IDX:
        w = P.conv_matrices(sd, k - 1)[0] / (gs if k == 11 else 1.0)          # GainISO precedes Conv2d1x1 model.10
        obj = obj + sd[f'model.{k - 1}.log_s'].sum() * W * W - (torch.log(gs) * C * H * W if k == 11 else 0.0)
        cl = clean if k == 2 else None
        if training:
            x, _h1, _h2, _o3, _bn, part = P.train_pair(P.prm_block(sd, k), w, torch.stack([a, b]), x, cl)
            obj = obj + part[:, 0].view(B, -1).sum(1)
            zz = part[:, 1].view(B, -1).sum(1)
        else:
            x, ld = P.density_pair(torch.cat([P.step_vector(sd, k), w.reshape(-1)]), x, cl, float(a), float(b))
            obj = obj + P.tile_sums(ld).sum(1)
            zz = (x * x).sum((1, 2, 3))
    return x, obj, zz


@pytest.mark.parametrize('training', (False, True))
def test_eight_density_pairs_are_the_oracle_forward_and_loss(golden_dir, training):
    g, sd0 = _golden(golden_dir)
    noise, clean = (torch.from_numpy(g['tr_noise' if training else 'fw_noise']).double(),
                    torch.from_numpy(g['tr_clean' if training else 'clean']).double())
    for iso in (1600.0, 3000.0):
        sd = R._cast(sd0, F64)
        z, obj, zz = _density_chain(sd, noise, clean, iso, training)
        zr, objr = O.forward(R._cast(sd0, F64), noise, clean, torch.tensor(iso), training)
        assert zr.dtype == F64 and objr.dtype == F64
        _close(z, zr, ('z', iso))
        _close(obj, objr, ('objective', iso))
        D = float(np.prod(noise.shape[1:]))
        nll = -(obj - 0.5 * (np.log(2 * np.pi) * D + zz)).mean() / D
        nllr, _sd = O.loss(R._cast(sd0, F64), noise, clean, torch.tensor(iso), training)
        assert abs(float(nll) - float(nllr)) <= 1e-12 * abs(float(nllr)), (float(nll), float(nllr))


# ------------------------------------------------------------------------------------------------------------ 2. the backward
def test_backward_is_the_gradient_of_train_pair():
    c = P.draw((3, 5, 3), P.SEEDS[(3, 5, 3)])
    args = [c['prm'].double(), c['m'].double().reshape(-1), c['ab'].double(), c['x'].double()]
    dx, sums = P.train_pair_bwd(*args, c['clean'], c['dz'], P.DZMUL, P.COBJ)
    assert sums.shape == (319,) and dx.shape == c['x'].shape
    assert float(sums[213:217].abs().max()) == 0 and float(sums[297:301].abs().max()) == 0       # dB2, dB1

    def objective(a):
        z, _h1, _h2, _o3, _bn, part = P.train_pair(a[0], a[1], a[2], a[3], c['clean'])
        return float((z * c['dz'].double()).sum() * P.DZMUL + P.COBJ * part[:, 0].sum())
    # central differences at a few entries of every input: (argument, flat index, position in dx / sums or None)
    probes = [(3, 7, None), (3, 100, None), (0, 5, 225 + 5), (0, 78, 221 + 2), (0, 82, 217 + 2), (0, 90, 197 + 6), (0, 105, 193 + 1),
              (0, 110, 189 + 2), (0, 112 + 4 * 9 + 3, 4 * 9 + 3), (0, 112 + 50, 50), (0, 293, 181), (0, 297, 185), (0, 300, 188),
              (1, 6, 301 + 6), (1, 13, 301 + 13), (2, 0, 317), (2, 1, 318)]
    for arg, i, at in probes:
        eps = 1e-6
        hi = [t.clone() for t in args]; lo = [t.clone() for t in args]
        hi[arg].view(-1)[i] += eps; lo[arg].view(-1)[i] -= eps
        fd = (objective(hi) - objective(lo)) / (2 * eps)
        an = float(dx.reshape(-1)[i]) if at is None else float(sums[at])
        assert abs(fd - an) <= 1e-6 * max(1.0, abs(an)), (arg, i, fd, an)


# ------------------------------------------------------------------------------------------------------------ 3. sensitivity
def _reach(defect, shape):
    """can this defect change anything at this shape?"""
    B, H, W = shape
    if defect == 'seam':
        return H > P.TS or W > P.TS                                        # a seam exists
    if defect == 'tail':
        return H >= 30                                                      # a tile has rows 29 .. 31 (fed by hidden positions >= 1024)
    if defect == 'cleanb':
        return B > 1
    return True


@pytest.mark.parametrize('shape', P.SHAPES)
def test_planted_defects_exceed_the_bar_a_hundredfold(shape):
    c = P.draw(shape, P.SEEDS[shape])
    with P.one_thread():
        for defect in P.DEFECTS:
            if not _reach(defect, shape):
                continue
            if defect == 'bias':                                            # only the bn_stats path forms the offset
                bn = P.stats(c['prm'], c['x'])
                run = lambda dt, d=None: P.sample_pair(c['step_train'], c['x'], c['clean'], P.SDN_A, P.SDN_B, P.OUT_MUL, bn_stats=bn,
                                                       dtype=dt, with_reach=True, _defect=d)
            else:
                run = lambda dt, d=None: P.sample_pair(c['step_eval'], c['x'], c['clean'], P.SDN_A, P.SDN_B, P.OUT_MUL, dtype=dt,
                                                       with_reach=True, _defect=d)
            ref, reach = run(F64)
            bar = 4 * P.e32_of(run(torch.float32)[0], ref) + 4e-7 * reach
            moved = float(((run(F64, defect)[0] - ref).abs() / bar).max())
            assert moved > 100, ('sample_pair', defect, shape, moved)
            if defect in ('bias', 'tail'):                                  # the step kernel's own: the bn_stats offset, its 2+2+1 rounds
                continue
            # the same defect in the density direction and in training mode
            run = lambda dt, d=None: P.density_pair(c['step_eval'], c['x'], c['clean'], P.SDN_A, P.SDN_B, dtype=dt, _defect=d)[0]
            ref = run(F64)
            moved = float((run(F64, defect) - ref).abs().max()) / (4 * P.e32_of(run(torch.float32), ref))
            assert moved > 100, ('density_pair', defect, shape, moved)
            run = lambda dt, d=None: P.train_pair(c['prm'], c['m'], c['ab'], c['x'], c['clean'], dtype=dt, _defect=d)[0]
            ref = run(F64)
            moved = float((run(F64, defect) - ref).abs().max()) / (4 * P.e32_of(run(torch.float32), ref))
            if shape != (1, 1, 1) or defect in ('ring', 'pad'):             # one pixel: BatchNorm's output is its bias whatever feeds it
                assert moved > 100, ('train_pair', defect, shape, moved)


def test_the_draws_cover_what_the_golden_state_dict_hides():
    cs = [P.draw(s, P.SEEDS[s]) for s in P.SHAPES] + [P.draw(*P.MEAN30, mean30=True)]
    assert {float(torch.sign(c['scale'])) for c in cs} == {-1.0, 1.0}
    for c in cs:
        for k in ('g1', 'g2'):
            assert float(c[k].min()) < 0 < float(c[k].max()) and 0.5 <= float(c[k].abs().min()) and float(c[k].abs().max()) <= 1.5
        assert np.linalg.cond(c['m'].double().numpy()) < 20
        assert P.OUT_MUL != 1.0
    x = cs[-1]['x'][:, 0]
    assert 25 < abs(float(x.mean())) / float(x.std()) < 35


# ------------------------------------------------------------------------------------------------------------ 4. the dx seeds
@pytest.mark.parametrize('shape', P.SHAPES)
@pytest.mark.parametrize('with_clean', (False, True))
def test_backward_seeds_leave_at_most_two_percent_out(shape, with_clean):
    c = P.draw(shape, P.SEEDS[shape])
    out = P.dx_excluded(c['prm'], c['m'].reshape(-1), c['ab'], c['x'], c['clean'] if with_clean else None)
    assert out.shape == (shape[0], shape[1], shape[2]) and float(out.double().mean()) <= 0.02, float(out.double().mean())

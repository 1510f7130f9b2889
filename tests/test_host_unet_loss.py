"""Unet_Loss without a GPU: the float64 restatement (tests/_unet_loss_ref.py) against the reference's recorded float32 outputs
(tests/golden/unet_loss.npz), its closed-form gradient against float64 autograd, the `hyper.loss` surface and the refusals that must come before
any device call."""
import json
import os
import types

import numpy as np
import pytest
import torch

import _unet_loss_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
U = 2.0 ** -24
MODES = [(c, p) for c in (0, 1) for p in (0, 1)]


@pytest.fixture(scope='module')
def golden(golden_dir):
    g = np.load(os.path.join(golden_dir, 'unet_loss.npz'))
    meta = json.load(open(os.path.join(golden_dir, 'unet_loss.json')))
    return g, meta


def test_restatement_equals_the_recorded_reference(golden):
    """float32 rounding: a mean of N float32 terms summed in torch's blocked order is within 64 x 2^-24 of the exact mean for these N <= 10 240
    (each term carries <= 3 roundings, the cascade adds ~log2 N), a gradient element carries <= 16 (four level terms, each a product of <= 3
    factors).  L1-family gradients agree at every element the restatement does not mark fragile; the generator found none flipped."""
    g, meta = golden
    for case in meta['cases']:
        tag = case['tag']
        pred, hr = g[f'{tag}_pred'], g[f'{tag}_hr']
        for c, p in MODES:
            if p and not case['pyramid']:
                continue
            ref = R.closed_form(pred, hr, charbonnier=bool(c), pyramid=bool(p))
            assert abs(float(g[f'{tag}_loss_c{c}p{p}']) - ref['loss']) <= 64 * U * ref['loss'], (tag, c, p)
            err = np.abs(g[f'{tag}_grad_c{c}p{p}'].astype(np.float64) - ref['grad'])
            # Charbonnier: f'(d) = d / sqrt(d^2 + 1e-6) has slope <= 1 / sqrt(1e-6) = 1000 at d = 0, and a pooled float32 d carries an absolute
            # error of up to ~8 x 2^-24 (values <= 1.2, three poolings, the subtraction), which that slope multiplies
            ok = err <= (16 + (8 * 1000 if c else 0)) * U * ref['coef'].max()
            assert (ok | (ref['fragile'] if not c else False)).all(), (tag, c, p, err.max() / ref['coef'].max())
            if p:
                assert np.all(np.abs(g[f'{tag}_terms_c{c}'].astype(np.float64) - ref['terms'][:4]) <= 64 * U * ref['terms'][:4]), (tag, c)
        ref = R.closed_form(pred, hr, grad=1.0, recon=False)
        assert abs(float(g[f'{tag}_edge_loss']) - ref['loss']) <= 64 * U * ref['loss'], tag
        assert ref['terms'][4] == ref['loss'] and not ref['terms'][:4].any()
        err = np.abs(g[f'{tag}_edge_grad'].astype(np.float64) - ref['grad'])
        assert ((err <= 16 * U * 8 * ref['coef_edge'].max()) | ref['fragile']).all(), (tag, 'edge')      # an element is up to 8 coefficients
        assert ref['fragile'].mean() <= meta['fragile_cap'] or tag == 'planted'


@pytest.mark.parametrize('kw', [dict(), dict(charbonnier=True), dict(pyramid=True), dict(charbonnier=True, pyramid=True), dict(grad=0.7),
                                dict(charbonnier=True, grad=0.3), dict(grad=1.0, recon=False)], ids=str)
def test_closed_form_gradient_equals_float64_autograd(golden, kw):
    """The identity the kernel is built on: all four levels of a pixel live in its own aligned 8x8 block, 1 / 4^l cancels the level's element count.
    Also through the ratio, both clamps and grad_weight, and for the edge term's transposed Sobel."""
    g, meta = golden
    for case in meta['cases']:
        tag = case['tag']
        if kw.get('pyramid') and not case['pyramid']:
            continue
        pred, hr = g[f'{tag}_pred'], g[f'{tag}_hr'] * 1.3 - 0.1
        B = pred.shape[0]
        for extra in (dict(), dict(scale=np.linspace(0.5, 1.75, B).astype(np.float32), clamp_target=True, grad_weight=0.6), dict(clamp_pred=False)):
            a, c = R.autograd(pred, hr, **kw, **extra), R.closed_form(pred, hr, **kw, **extra)
            top = np.abs(a['grad']).max()
            assert top > 0
            assert np.abs(a['grad'] - c['grad']).max() <= 1e-13 * top, (tag, extra, np.abs(a['grad'] - c['grad']).max() / top)
            assert a['loss'] == c['loss'] and np.array_equal(a['terms'], c['terms'])


def test_l1_family_integers_reproduce_the_gradient(golden):
    """k, ks, mask and the float32 coefficient chain (R.l1_family_expected) are the restatement's own gradient to float32 rounding: what the GPU test
    compares the kernel's bits with."""
    g, _ = golden
    pred, hr = g['e_pred'], g['e_hr']
    sc = np.array([0.5, 1.5], np.float32)
    for kw in (dict(), dict(pyramid=True), dict(grad=0.5), dict(grad=1.0, recon=False)):
        ref = R.closed_form(pred, hr, scale=sc, grad_weight=0.6, **kw)
        want = R.l1_family_expected(ref, grad_weight=0.6, scale=sc, grad=kw.get('grad', 0.0), pyramid=kw.get('pyramid', False))
        assert np.abs(want.astype(np.float64) - ref['grad']).max() <= 4 * U * np.abs(ref['grad']).max(), kw


def test_plain_tensor_helpers_match_the_reference(golden):
    """gradient / Pyramid_Sample / Pyramid_Loss (kept so that the reference's imports resolve) on the CPU against the recorded arrays."""
    from pnnp_amd import losses
    g, _ = golden
    pred, hr = torch.from_numpy(g['e_pred']).clamp(0, 1), torch.from_numpy(g['e_hr'])
    for d in 'xy':
        for w, t in (('low', pred), ('high', hr)):
            got = losses.gradient(t, d, device='cpu').numpy()
            np.testing.assert_allclose(got[:, 0], g[f'e_edge_{d}_{w}'], rtol=0, atol=64 * U * 16)
            assert got.shape == tuple(t.shape)
    lows, highs = [pred] + losses.Pyramid_Sample(pred, 8), [hr] + losses.Pyramid_Sample(hr, 8)
    assert [tuple(x.shape[2:]) for x in lows] == [(32, 40), (16, 20), (8, 10), (4, 5)]
    loss = losses.Pyramid_Loss(lows, highs, rate=0.5, norm=True)
    assert abs(float(loss) - float(g['e_loss_c0p1'])) <= 64 * U * float(loss)
    assert losses.gradient(hr, 'x', device='cpu', kernel='robert').shape == (2, 4, 33, 39)      # the reference's own shapes for its 2x2 kernel


def test_loss_options_and_refusals_touch_no_device(monkeypatch):
    from pnnp_amd import _lib, losses, ops
    from pnnp_amd.trainer import HipTrainStep

    def no_device(*a, **k):
        raise AssertionError('a refusal reached the library')
    monkeypatch.setattr(_lib, 'lib', no_device)
    monkeypatch.setattr(ops, 'lib', no_device)
    assert ops.unet_loss_options({}) == dict(charbonnier=False, pyramid=False, grad=0.0)
    assert ops.unet_loss_options(dict(pyramid=True, charbonnier=True)) == dict(charbonnier=True, pyramid=True, grad=0.0)
    assert ops.unet_loss_options(dict(grad=2)) == dict(charbonnier=False, pyramid=False, grad=2.0)
    net = types.SimpleNamespace(engine=None)
    for bad in (dict(pyramid=True, grad=0.1), dict(sobel=1.0), dict(grad=-1.0), dict(grad=float('nan')), dict(grad=float('inf')), dict(pyramid=1),
                dict(charbonnier='yes'), dict(grad=True), 'pyramid', ['pyramid']):
        with pytest.raises(_lib.PnnpError):
            ops.unet_loss_options(bad)
        with pytest.raises(_lib.PnnpError):
            HipTrainStep(net, loss=bad)
    assert HipTrainStep(net).loss_opt is None and HipTrainStep(net, loss=dict(charbonnier=True)).loss_opt['charbonnier'] is True
    x = torch.zeros(1, 4, 12, 16)
    out, ws = torch.zeros(2), torch.zeros(1024)
    with pytest.raises(_lib.PnnpError, match='multiples of 8'):                      # H % 8
        ops.unet_loss(x, x, None, out, ws, pyramid=True)
    with pytest.raises(_lib.PnnpError, match='multiples of 8'):                      # W % 8
        ops.unet_loss(x.transpose(2, 3).contiguous(), x.transpose(2, 3).contiguous(), None, out, ws, pyramid=True)
    with pytest.raises(_lib.PnnpError, match='pyramid'):
        ops.unet_loss(x, x, None, out, ws, pyramid=True, grad=0.5)
    with pytest.raises(_lib.PnnpError, match='GPU only'):                            # no CPU path
        ops.unet_loss(x, x, None, out, ws)
    with pytest.raises(_lib.PnnpError, match='GPU only'):
        losses.Unet_Loss()(x, x)
    assert not out.any() and not ws.any()


def test_hyper_loss_of_a_run_file():
    from pnnp_amd import _lib, runfile
    cfg = runfile.load(os.path.join(HERE, 'fixtures', 'runfile_sony_pyramid.yml'))
    assert cfg['hyper']['loss'] == dict(charbonnier=True, pyramid=True, grad=0.0)
    _, step, lr_of, shapes = runfile.build(cfg, device='cpu')
    assert step.loss_opt == dict(charbonnier=True, pyramid=True, grad=0.0) and step.loss_terms is None
    assert shapes['patch'] % 8 == 0 and lr_of(21) > 0
    plain = runfile.load(os.path.join(HERE, 'fixtures', 'runfile_sony.yml'))
    assert 'loss' not in plain['hyper'] and runfile.build(plain, device='cpu')[1].loss_opt is None
    cfg['hyper']['loss'] = dict(pyramid=True, grad=0.5)
    with pytest.raises(_lib.PnnpError):
        runfile.build(cfg, device='cpu')
    cfg['hyper']['loss'] = dict(piramid=True)
    with pytest.raises(_lib.PnnpError):
        runfile.build(cfg, device='cpu')

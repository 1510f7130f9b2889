#!/usr/bin/env python3
"""Generate tests/golden/unet_loss.npz + unet_loss.json by running the REAL reference on the CPU, in float32: ``Unet_Loss``
(losses/base_loss.py:75-107) with its ``Pyramid_Sample`` and ``gradient`` helpers.

Runs only where the reference is available (see make_golden.py, whose import stubs it uses); stores data only.

    python tests/golden/make_golden_unet_loss.py

Per case <tag> (pred reaches outside [0, 1], the trainers' call site clamps it: trainer_SID.py:99):

    <tag>_pred, <tag>_hr            float32 [B,C,H,W]
    <tag>_loss_c<c>p<p>             Unet_Loss(charbonnier=c)(pred.clamp(0, 1), hr, pyramid=p)            (the four pairs; p = 1 only where H, W % 8 == 0)
    <tag>_grad_c<c>p<p>             pred.grad after its backward()
    <tag>_terms_c<c>                the four level terms, composed from Pyramid_Sample and the module's own loss()       (where H, W % 8 == 0)
    <tag>_edge_{x,y}_{low,high}     gradient(., 'x' / 'y', device='cpu'), channel 0 (the generator asserts that all channels are the same array)
    <tag>_edge_loss, _edge_grad     grad_loss composed from them, mean(|x_low - x_high| + |y_low - y_high|), and pred.grad after its backward()

``Unet_Loss.grad_loss`` itself cannot run here: it calls ``gradient`` with its default ``device='cuda'`` (base_loss.py:15,81-82), so the same two
lines are composed with ``device='cpu'``.

The generator asserts, against tests/_unet_loss_ref.py, that in every L1-family record (c = 0, and the edge term) the reference's own float32 gradient
differs from the float64 closed form only at elements the restatement marks fragile (a sign within 1e-6 of flipping) and that those are at most
0.5 % of the case: the cap tests/test_gpu_unet_loss.py grants the kernel.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import import_reference  # noqa: E402

BELOW_0 = np.nextafter(np.float32(0), np.float32(-1))
ABOVE_1 = np.nextafter(np.float32(1), np.float32(2))
FRAGILE_CAP = 0.005

# (tag, B, C, H, W, seed): see the table in DESIGN.md section 7b, row f13
CASES = [('a', 2, 4, 32, 32, 11), ('b', 1, 3, 8, 8, 12), ('c', 3, 4, 16, 24, 13), ('d', 1, 8, 8, 8, 14), ('e', 2, 4, 32, 40, 15),
         ('f', 2, 4, 5, 7, 16), ('planted', 1, 4, 16, 16, 17)]


def make_inputs(tag, B, C, H, W, seed):
    rng = np.random.default_rng(seed)
    pred = (rng.random((B, C, H, W)) * 1.4 - 0.2).astype(np.float32)
    hr = rng.random((B, C, H, W)).astype(np.float32)
    if tag == 'planted':
        # channel 0, block (0, 0), row 0: the clamp's edges and their float32 neighbours, and d == 0 at level 0
        for i, (pv, hv) in enumerate([(0.0, 0.5), (1.0, 0.5), (-0.0, 0.5), (BELOW_0, 0.5), (ABOVE_1, 0.5), (0.375, 0.375)]):
            pred[0, 0, 0, i] = pv
            hr[0, 0, 0, i] = hv
        # channel 1, block (0, 1): pred == hr inside [0, 1], so every level is exactly zero (sign 0, Charbonnier value sqrt(1e-6))
        pred[0, 1, 0:8, 8:16] = hr[0, 1, 0:8, 8:16]
        # channel 2, block (1, 0): +-0.25 on the two halves: levels 0 to 2 do not vanish, the level-3 mean cancels exactly
        hr[0, 2, 8:16, 0:8] = 0.5
        pred[0, 2, 8:16, 0:4] = 0.75
        pred[0, 2, 8:16, 4:8] = 0.25
    return pred, hr


def main():
    import_reference()
    import torch
    import _unet_loss_ref as R
    BL = sys.modules['losses.base_loss']
    out, meta = {}, []
    for tag, B, C, H, W, seed in CASES:
        pred, hr = make_inputs(tag, B, C, H, W, seed)
        out[f'{tag}_pred'], out[f'{tag}_hr'] = pred, hr
        pyr_ok = H % 8 == 0 and W % 8 == 0
        t_hr = torch.from_numpy(hr)
        info = dict(tag=tag, B=B, C=C, H=H, W=W, pyramid=pyr_ok, fragile={})

        def check_l1(name, g32, **kw):
            ref = R.closed_form(pred, hr, **kw)
            bad = np.abs(g32.astype(np.float64) - ref['grad']) > 1e-4 * np.abs(ref['coef'] + ref['coef_edge']).max()
            assert not (bad & ~ref['fragile']).any(), (tag, name, int((bad & ~ref['fragile']).sum()))
            share = ref['fragile'].mean()
            if tag != 'planted':                                    # the planted case holds exact zeros on purpose
                assert share <= FRAGILE_CAP, (tag, name, share)
            info['fragile'][name] = dict(share=float(share), flipped=int(bad.sum()))

        for c in (0, 1):
            crit = BL.Unet_Loss(charbonnier=bool(c))
            for p in ((0, 1) if pyr_ok else (0,)):
                leaf = torch.from_numpy(pred).clone().requires_grad_(True)
                loss = crit(leaf.clamp(0, 1), t_hr, pyramid=bool(p))
                loss.backward()
                out[f'{tag}_loss_c{c}p{p}'] = np.float32(loss.item())
                out[f'{tag}_grad_c{c}p{p}'] = leaf.grad.numpy().copy()
                if c == 0:
                    check_l1(f'c0p{p}', leaf.grad.numpy(), charbonnier=False, pyramid=bool(p))
            if pyr_ok:
                with torch.no_grad():
                    low = torch.from_numpy(pred).clamp(0, 1)
                    lows, highs = [low] + BL.Pyramid_Sample(low, max_scale=8), [t_hr] + BL.Pyramid_Sample(t_hr, max_scale=8)
                    out[f'{tag}_terms_c{c}'] = np.array([crit.loss(a, b).item() for a, b in zip(lows, highs)], np.float32)
        leaf = torch.from_numpy(pred).clone().requires_grad_(True)
        low = leaf.clamp(0, 1)
        maps = {(d, w): BL.gradient(t, d, device='cpu') for d in 'xy' for w, t in (('low', low), ('high', t_hr))}
        edge = torch.mean(torch.abs(maps['x', 'low'] - maps['x', 'high']) + torch.abs(maps['y', 'low'] - maps['y', 'high']))
        edge.backward()
        for (d, w), m in maps.items():
            m = m.detach().numpy()
            assert all(np.array_equal(m[:, 0], m[:, k]) for k in range(C)), (tag, d, w)      # every output channel is the Sobel of the channel sum
            out[f'{tag}_edge_{d}_{w}'] = m[:, 0].copy()
        out[f'{tag}_edge_loss'] = np.float32(edge.item())
        out[f'{tag}_edge_grad'] = leaf.grad.numpy().copy()
        check_l1('edge', leaf.grad.numpy(), grad=1.0, recon=False)
        meta.append(info)
    np.savez_compressed(os.path.join(HERE, 'unet_loss.npz'), **out)
    json.dump(dict(cases=meta, fragile_cap=FRAGILE_CAP), open(os.path.join(HERE, 'unet_loss.json'), 'w'), indent=1)
    print('unet_loss fixtures written:', os.path.getsize(os.path.join(HERE, 'unet_loss.npz')), 'bytes')
    for m in meta:
        print(m['tag'], m['fragile'])


if __name__ == '__main__':
    main()

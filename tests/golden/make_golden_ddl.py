#!/usr/bin/env python3
"""Generate tests/golden/ddl.npz by running the REAL reference's CDFPPF.get_cdf, CDFLoss, KLD (with .backward()) and get_x
(utils/kld_div.py:21-98) on the CPU.

Runs only where the reference tree is present (see make_golden.py).  Stores seeded inputs and the reference's outputs -- data only,
no reference source text.

    python tests/golden/make_golden_ddl.py

Per case <c>: <c>_out, <c>_gt (float32 samples, different lengths), <c>_x (float32 ascending points), <c>_cdf_out, <c>_cdf_gt (float32 [K]),
<c>_cdfloss, <c>_kld (float32 scalars), <c>_gcdf_out, <c>_gcdf_gt, <c>_gkld_out, <c>_gkld_gt (float32 gradients of the two losses with
respect to the samples).  getx_<mode>: get_x(size=1000, mode=<mode>) under torch.manual_seed(SEED); getx_small: get_x(3, 64, 'icdf').
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402

SEED = 20240611
CASES = ['normal', 'distinct', 'ties', 'inside']


def cases():
    rng = np.random.default_rng(SEED)
    f = lambda a: np.ascontiguousarray(a, np.float32)
    out = {}
    # two normal samples of different size and scale; 1000 points that straddle both ends of both
    o, g = f(rng.normal(0.1, 1.0, 16384)), f(rng.normal(0.0, 1.2, 8192))
    out['normal'] = (o, g, f(np.linspace(-6.0, 6.0, 1000)))
    # distinct values (a scaled permutation): points equal to data values, to the minimum and the maximum, outside on both sides, repeated
    o, g = f((rng.permutation(4097) - 2048) / 64.0), f((rng.permutation(4096) - 1000) / 32.0)
    x = np.concatenate([[-200.0, -100.0, o.min(), g.min()], np.sort(rng.choice(o, 20, replace=False)), np.sort(rng.choice(g, 20, replace=False)),
                        rng.uniform(-30, 60, 14), [5.0, 5.0, 5.0], [o.max(), g.max(), 150.0]])
    out['distinct'] = (o, g, f(np.sort(x)))
    # integer-valued samples with heavy ties
    o, g = f(np.rint(rng.normal(0, 3.0, 4096))), f(np.rint(rng.normal(0.5, 3.5, 4099)))
    out['ties'] = (o, g, f(np.sort(np.concatenate([np.arange(-12, 13), rng.uniform(-14, 14, 39)]))))
    # every point strictly inside both ranges
    o, g = f(rng.normal(0, 1, 4100)), f(rng.normal(0, 1, 4097) * 1.1 + 0.05)
    out['inside'] = (o, g, f(np.linspace(-2.0, 2.0, 64)))
    return out


def main():
    make_golden.import_reference()
    import torch
    from utils.kld_div import CDFPPF, CDFLoss, KLD, get_x
    store = {}
    for name, (o, g, x) in cases().items():
        to, tg, tx = torch.from_numpy(o), torch.from_numpy(g), torch.from_numpy(x)
        store[name + '_out'], store[name + '_gt'], store[name + '_x'] = o, g, x
        store[name + '_cdf_out'] = CDFPPF(to).get_cdf(tx).numpy()
        store[name + '_cdf_gt'] = CDFPPF(tg).get_cdf(tx).numpy()
        for tag, fn in (('cdf', CDFLoss), ('kld', KLD)):
            a, b = to.clone().requires_grad_(True), tg.clone().requires_grad_(True)
            loss = fn(a, b, tx)
            loss.backward()
            store[f'{name}_{tag}loss' if tag == 'cdf' else f'{name}_kld'] = np.float32(loss.item())
            store[f'{name}_g{tag}_out'], store[f'{name}_g{tag}_gt'] = a.grad.numpy(), b.grad.numpy()
        print(name, 'N', o.size, g.size, 'K', x.size, 'CDFLoss', store[name + '_cdfloss'], 'KLD', store[name + '_kld'])
    for mode in ('uniform', 'cdf', 'icdf'):
        torch.manual_seed(SEED)
        store['getx_' + mode] = get_x(size=1000, mode=mode).numpy()
    torch.manual_seed(SEED)
    store['getx_small'] = get_x(3, 64, 'icdf').numpy()
    path = os.path.join(HERE, 'ddl.npz')
    np.savez_compressed(path, **store)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""Generate tests/golden/quantile.npz by running the REAL reference's QuantileLoss (utils/kld_div.py:49-53) and the torch.quantile it is
built on, with .backward(), on the CPU.

Runs only where the reference tree is present (see make_golden.py).  Stores seeded inputs and the reference's outputs -- data only,
no reference source text.

    python tests/golden/make_golden_quantile.py

Per case <c>: <c>_out, <c>_gt (float32 samples; 1-D, or [3, N] for 'rows'), <c>_q (float32 probabilities), <c>_pos_out, <c>_pos_gt (float32
[K]: q * (N - 1) as torch multiplies it), <c>_q_out, <c>_q_gt (torch.quantile(..., dim=-1, interpolation='linear'), [K, *leading]),
<c>_loss (float32 scalar), <c>_gloss_out, <c>_gloss_gt (gradients of QuantileLoss), <c>_g (float32 [K, *leading], seeded) and
<c>_gq_out (the gradient of sum(<c>_g * torch.quantile(out)) with respect to out).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402

SEED = 20240923
CASES = ['normal', 'edges', 'ties', 'rows', 'tiny1', 'tiny2', 'tiny3']
TIE_FREE = ['normal', 'edges', 'rows']


def cases():
    rng = np.random.default_rng(SEED)
    f = lambda a: np.ascontiguousarray(a, np.float32)
    out = {}
    out['normal'] = (f(rng.normal(0.1, 1.0, 16384)), f(rng.normal(0.0, 1.2, 8192)), f(np.linspace(1e-4, 1 - 1e-4, 1000)))
    # distinct values (scaled permutations); q: both ends, the median three times, exact ranks k / (N - 1), others; not ascending
    n = 4097
    o, g = f((rng.permutation(n) - 2048) / 64.0), f((rng.permutation(n) - 1000) / 32.0)
    q = np.concatenate([[0.0, 1.0, 0.5, 0.5, 0.5], rng.choice(n, 24, replace=False) / (n - 1.0), rng.uniform(0, 1, 35)])
    out['edges'] = (o, g, f(rng.permutation(q)))
    # integer-valued samples with heavy ties
    out['ties'] = (f(np.rint(rng.normal(0, 3.0, 4096))), f(np.rint(rng.normal(0.5, 3.5, 4099))), f(np.linspace(0.0, 1.0, 257)))
    # three rows per operand
    out['rows'] = (f(rng.normal(0, 1, (3, 4100)) * [[1.0], [2.0], [0.5]]), f(rng.normal(0.1, 1.1, (3, 4100))), f(rng.uniform(0, 1, 100)))
    for n in (1, 2, 3):
        out[f'tiny{n}'] = (f(rng.normal(0, 1, n)), f(rng.normal(0, 1, n)), f([0.0, 0.25, 0.5, 0.75, 1.0, 0.3]))
    return out


def main():
    make_golden.import_reference()
    import torch
    from utils.kld_div import QuantileLoss
    rng = np.random.default_rng(SEED + 1)
    store = {}
    for name, (o, g, q) in cases().items():
        to, tg, tq = torch.from_numpy(o), torch.from_numpy(g), torch.from_numpy(q)
        store[name + '_out'], store[name + '_gt'], store[name + '_q'] = o, g, q
        store[name + '_pos_out'] = (tq * (o.shape[-1] - 1)).numpy()
        store[name + '_pos_gt'] = (tq * (g.shape[-1] - 1)).numpy()
        store[name + '_q_out'] = torch.quantile(to, tq, dim=-1, keepdim=False, interpolation='linear').numpy()
        store[name + '_q_gt'] = torch.quantile(tg, tq, dim=-1, keepdim=False, interpolation='linear').numpy()
        a, b = to.clone().requires_grad_(True), tg.clone().requires_grad_(True)
        loss = QuantileLoss(a, b, tq)
        loss.backward()
        store[name + '_loss'] = np.float32(loss.item())
        store[name + '_gloss_out'], store[name + '_gloss_gt'] = a.grad.numpy(), b.grad.numpy()
        gk = rng.normal(size=store[name + '_q_out'].shape).astype(np.float32)
        a = to.clone().requires_grad_(True)
        (torch.quantile(a, tq, dim=-1, keepdim=False, interpolation='linear') * torch.from_numpy(gk)).sum().backward()
        store[name + '_g'], store[name + '_gq_out'] = gk, a.grad.numpy()
        print(name, 'N', o.shape, g.shape, 'K', q.size, 'QuantileLoss', store[name + '_loss'])
    path = os.path.join(HERE, 'quantile.npz')
    np.savez_compressed(path, **store)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""Generate tests/golden/kld.npz by running the REAL reference's kl_div_norm (utils/kld_div.py:163-200).

Runs only where the reference tree is present (see make_golden.py).  Stores seeded inputs and the reference's outputs -- data only,
no reference source text.  The reference mutates its arguments (``p_data += bl``), so it gets copies.

    python tests/golden/make_golden_kld.py

Per case <c>: <c>_p, <c>_q (float32 [4,64,64]), <c>_cp, <c>_cq (int32 counts = hist * n, [nbins]), <c>_kl (float64 [3]: fwd, inv, sym);
`edges` = the reference's second element of hist_p (bin_edges * wp - bl).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402

SHAPE = (4, 64, 64)


def cases():
    rng = np.random.default_rng(20240607)
    n = int(np.prod(SHAPE))
    f = lambda a: np.asarray(a, np.float32).reshape(SHAPE)
    out = {}
    out['narrow'] = (f(np.rint(rng.normal(0, 3.0, n))), f(np.rint(rng.normal(0, 3.2, n))))                 # the shift branch
    out['wide'] = (f(np.rint(rng.normal(0, 900.0, n))), f(np.rint(rng.normal(0, 950.0, n))))               # bin pairing above DN 1024
    pos = np.rint(rng.normal(40, 5.0, n))
    assert pos.min() > 0
    out['pos'] = (f(pos), f(np.rint(rng.normal(40, 5.5, n))))                                              # no shift
    out['posq'] = (f(pos), f(np.rint(rng.normal(40, 30.0, n))))                                            # q's negatives clip to 0, no shift
    # non-integer inputs: multiples of 0.5 (ties) and values one float32 step below a tie, where rint(x + 512) != rint(x) + 512
    tp = np.round(rng.uniform(-20, 60, n) * 2) / 2
    tq = np.round(rng.uniform(-22, 62, n) * 2) / 2
    near = np.array([0.49999997, 1.4999999, 2.4999998, -0.49999997, -1.4999999, 3.4999998, 0.5, 1.5, 2.5, -0.5, -1.5], np.float32)
    tp = tp.astype(np.float32); tq = tq.astype(np.float32)
    tp[rng.choice(n, 4000, replace=False)] = near[rng.integers(0, len(near), 4000)]
    tq[rng.choice(n, 4000, replace=False)] = near[rng.integers(0, len(near), 4000)]
    out['ties'] = (f(tp), f(tq))
    ip, iq = out['narrow'][0].copy(), out['narrow'][1].copy()
    iq.reshape(-1)[[5, 777, 9000]] = np.inf
    iq.reshape(-1)[[6, 12000]] = -np.inf
    out['inf'] = (ip, iq)                                                                                  # clipped to the ends
    npp, nq = out['narrow'][0].copy(), out['narrow'][1].copy()
    npp.reshape(-1)[4321] = np.nan
    out['nan'] = (npp, nq)                                                                                 # no shift; counted in n only
    return out


def main():
    make_golden.import_reference()
    from utils.kld_div import kl_div_norm
    store = {}
    n = int(np.prod(SHAPE))
    for name, (p, q) in cases().items():
        with np.errstate(all='ignore'):
            r = kl_div_norm(p.flatten().copy(), q.flatten().copy())
        cp, cq = np.rint(r['hist_p'][0] * n), np.rint(r['hist_q'][0] * n)
        assert np.array_equal(cp / n, r['hist_p'][0]) and np.array_equal(cq / n, r['hist_q'][0])
        store[name + '_p'], store[name + '_q'] = p, q
        store[name + '_cp'], store[name + '_cq'] = cp.astype(np.int32), cq.astype(np.int32)
        store[name + '_kl'] = np.array([r['kl_fwd'], r['kl_inv'], r['kl_sym']], np.float64)
        store['edges'] = np.asarray(r['hist_p'][1], np.float64)
        print(name, 'counts', int(cp.sum()), int(cq.sum()), 'kl', store[name + '_kl'])
    assert int(store['nan_cp'].sum()) == n - 1
    path = os.path.join(HERE, 'kld.npz')
    np.savez_compressed(path, **store)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()

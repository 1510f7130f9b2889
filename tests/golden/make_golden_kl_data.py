#!/usr/bin/env python3
"""Generate tests/golden/kl_data.npz by running the REAL reference's get_histogram, kl_div_3_data, kl_div_3 and kl_div_norm(bl=None)
(utils/kld_div.py:100-210).

Runs only where the reference tree is present (see make_golden.py).  Stores seeded inputs and the reference's outputs -- data only,
no reference source text.

    python tests/golden/make_golden_kl_data.py

Sample sets are stored once (`data_<name>`) and shared by the cases.  Per histogram case <c> (names in `cases`): <c>_pq (the two names
of its sample sets), <c>_e (float64 edges; absent = the defaults, 1000 bins on [0, 1]), <c>_cp, <c>_cq (int32 counts = hist * n),
<c>_kl (float64 [3]: fwd, inv, sym), <c>_cen (get_histogram's bin centres of p).  Per bl=None case <c> (names in `range_cases`): <c>_pq,
<c>_wp, <c>_x (the reference's second element of hist_p: bin_edges * wp - 0, in arange's dtype), <c>_cp, <c>_cq, <c>_kl.
`k3_p`, `k3_q`, `k3_vals`: two histograms (with zeros, a NaN and an inf) and kl_div_forward, kl_div_inverse, kl_div_sym, kl_div_3 of
them.  `numpy_version`: the float32 scalar arithmetic of the bl=None edges is numpy's.

wp + 2 edges: for float32 data bw = float32((r - l) / wp) and arange's length is ceil((float32(r + bw) - l) / bw) in float64, which is
wp + 2 whenever the rounded quotient exceeds wp + 1.  The 4x64x64 draws used here all give wp + 1; a 4x16x16 draw found by a search
over seeds (see data()) gives wp + 2, and main() asserts that the file has both.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402

SHAPE = (4, 64, 64)
NF_EDGES = np.concatenate(([-1000.0], np.arange(-0.1, 0.1 + 1e-9, 0.2 / 100), [1000.0]))      # the Noise Flow edges (103 of them)


def default_edges():
    bw = (1.0 - 0.0) / 1000
    return np.arange(0.0, 1.0 + bw, bw)


def data():
    rng = np.random.default_rng(20240911)
    n = int(np.prod(SHAPE))
    f = lambda a: np.asarray(a, np.float32).reshape(SHAPE)
    d = {}
    a, b = rng.normal(0.5, 0.1, n), rng.normal(0.5, 0.11, n)
    a[:8] = [0.5, 0.5, 0.0, 1.0, np.nextafter(0.5, 0), np.nextafter(0.5, 1), 0.3, -0.01]      # edges of the repeated- / one- / two-bin cases
    b[:4] = [0.5, 1.0, 1.0, 0.0]
    d['a'], d['b'] = f(a), f(b)
    d['short'] = np.asarray(rng.normal(0.5, 0.12, 3 * 50 * 50), np.float32).reshape(3, 50, 50)              # unequal n
    nfp, nfq = rng.normal(0, 0.03, n), rng.normal(0, 0.033, n)
    nfp[[3, 500, 9000]] = [0.5, -0.7, 999.0]                    # inside the catch-all bins ...
    nfq[[4, 600, 9100]] = [-999.5, 0.25, 1000.0]                # ... the closed last edge ...
    nfp[[7, 8]] = [1000.5, -1000.5]                             # ... and beyond them
    nfp[[11, 12, 13]] = [-0.1, 0.1, -1000.0]                    # edges themselves
    d['nfp'], d['nfq'] = f(nfp), f(nfq)
    # every float32(e[k]) of the default edges and its float32 neighbours on both sides
    e = default_edges()
    e32 = e.astype(np.float32)
    lo, hi = np.nextafter(e32, np.float32(-np.inf)), np.nextafter(e32, np.float32(np.inf))
    d['e32'] = np.concatenate([e32, lo, hi]).astype(np.float32)
    d['e32q'] = np.concatenate([lo, e32[::2], hi[1::3]]).astype(np.float32)
    # the same as float64, the edges themselves, their float64 neighbours, and values strictly between two float32 neighbours
    e32d, lod, hid = e32.astype(np.float64), lo.astype(np.float64), hi.astype(np.float64)
    d['e64'] = np.concatenate([e32d, lod, hid, e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf), (e32d + lod) / 2, (e32d + hid) / 2])
    d['e64q'] = np.concatenate([e, (e32d + e) / 2, np.nextafter(e, np.inf)[::2], hid[::5]])
    sub = np.float32(-1e-45)
    assert sub < 0 and sub > -np.finfo(np.float32).tiny
    d['spec'] = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1.0, np.nextafter(np.float32(1), np.float32(2)), sub, 0.25, 0.5, 0.999, 0.9995,
                          np.nextafter(np.float32(1), np.float32(0)), -1e-3, 3.0, np.nan], np.float32)
    d['specq'] = np.array([1.0, 1.0, -0.0, sub, np.inf, 0.25, 0.2505, 0.5, 0.9995, np.nan, 7.0], np.float32)
    d['above'] = np.linspace(2, 3, 257).astype(np.float32)     # all out of range
    d['below'] = np.linspace(-1, -0.5, 100).astype(np.float32)
    # float64 samples that no float32 holds (25 explicit mantissa bits: the low 27 cleared, which also lets the file compress)
    cut = lambda a: (np.asarray(a, np.float64).view(np.uint64) & ~np.uint64((1 << 27) - 1)).view(np.float64).reshape(SHAPE)
    d['dp'], d['dq'] = cut(rng.normal(0.1, 2.0, n)), cut(rng.normal(0.1, 2.1, n))
    assert not np.array_equal(d['dp'].astype(np.float32).astype(np.float64), d['dp'])
    # the bl=None edges number wp + 2 for about one draw in six; among seeds 1 .. 39 of this small draw, 7 is the first with wp + 2
    # edges (at wp = 1000 and at 255; no seed gave them at 16383)
    r7 = np.random.default_rng(7)
    d['w7p'] = r7.normal(0.5, 0.1, 1024).astype(np.float32).reshape(4, 16, 16)
    d['w7q'] = r7.normal(0.5, 0.11, 1024).astype(np.float32).reshape(4, 16, 16)
    return d


CASES = {                        # name -> (p, q, edges or None)
    'default': ('a', 'b', None),
    'nf': ('nfp', 'nfq', NF_EDGES),
    'edge32': ('e32', 'e32q', None),
    'edge64': ('e64', 'e64q', None),
    'special': ('spec', 'specq', None),
    'allout': ('above', 'below', None),
    'halfout': ('above', 'a', None),
    'repeat': ('a', 'b', np.array([0.0, 0.5, 0.5, 1.0])),
    'onebin': ('a', 'b', np.array([0.0, 1.0])),
    'twobin': ('a', 'b', np.array([0.0, 0.3, 1.0])),
    'unequal': ('a', 'short', None),
    'default64': ('dp', 'dq', np.linspace(-6.0, 6.5, 778)),
}
RANGE_CASES = {'range16383': ('a', 'b', 16383), 'range1000': ('a', 'b', 1000), 'range255': ('a', 'b', 255), 'range1000s': ('a', 'short', 1000),
               'range255n': ('nfp', 'nfq', 255), 'range1000w': ('w7p', 'w7q', 1000), 'range255w': ('w7p', 'w7q', 255), 'range64': ('dp', 'dq', 1000), 'range64s': ('dp', 'dq', 255)}


def main():
    make_golden.import_reference()
    from utils.kld_div import get_histogram, kl_div_3, kl_div_3_data, kl_div_forward, kl_div_inverse, kl_div_norm, kl_div_sym
    d = data()
    store = {'data_' + k: v for k, v in d.items()}
    store['numpy_version'] = np.array(np.__version__)
    store['cases'] = np.array(list(CASES))
    store['range_cases'] = np.array(list(RANGE_CASES))
    for name, (pn, qn, e) in CASES.items():
        p, q = d[pn], d[qn]
        kw = {} if e is None else {'bin_edges': e}
        with np.errstate(all='ignore'):
            kl = kl_div_3_data(p.copy(), q.copy(), **kw)
            yp, cen = get_histogram(p.copy(), **kw)
            yq, _ = get_histogram(q.copy(), **kw)
        cp, cq = np.rint(yp * p.size), np.rint(yq * q.size)
        assert np.array_equal(cp / p.size, yp) and np.array_equal(cq / q.size, yq)
        store[name + '_pq'] = np.array([pn, qn])
        if e is not None:
            store[name + '_e'] = np.asarray(e, np.float64)
        store[name + '_cp'], store[name + '_cq'] = cp.astype(np.int32), cq.astype(np.int32)
        store[name + '_kl'] = np.array(kl, np.float64)
        store[name + '_cen'] = np.asarray(cen, np.float64)
        print(name, 'counts', int(cp.sum()), 'of', p.size, int(cq.sum()), 'of', q.size, 'kl', store[name + '_kl'])
    assert np.all(store['allout_kl'] == 0.0) and store['allout_cp'].sum() == 0 and store['allout_cq'].sum() == 0
    extra = set()
    for name, (pn, qn, wp) in RANGE_CASES.items():
        p, q = d[pn], d[qn]
        r = kl_div_norm(p.flatten().copy(), q.flatten().copy(), bl=None, wp=wp)
        yp, x = r['hist_p']
        yq, _ = r['hist_q']
        cp, cq = np.rint(yp * p.size), np.rint(yq * q.size)
        assert np.array_equal(cp / p.size, yp) and np.array_equal(cq / q.size, yq)
        store[name + '_pq'] = np.array([pn, qn])
        store[name + '_wp'] = np.array(wp)
        store[name + '_x'] = np.asarray(x)
        store[name + '_cp'], store[name + '_cq'] = cp.astype(np.int32), cq.astype(np.int32)
        store[name + '_kl'] = np.array([r['kl_fwd'], r['kl_inv'], r['kl_sym']], np.float64)
        extra.add((p.dtype.name, len(x) - wp))
        print(name, p.dtype, 'wp', wp, 'edges', len(x), x.dtype, 'counts', int(cp.sum()), int(cq.sum()), 'kl', store[name + '_kl'])
    print('edges - wp per dtype:', sorted(extra))
    assert ('float32', 1) in extra and ('float32', 2) in extra, 'no float32 case with wp + 2 edges: look for another draw'
    for bad in (np.array([1.0, np.nan, 2.0], np.float32), np.array([1.0, np.inf], np.float32), np.full(5, 0.25, np.float32)):
        try:
            with np.errstate(all='ignore'):
                kl_div_norm(bad.copy(), bad.copy(), bl=None)
        except ValueError as err:
            print('bl=None refuses', bad[:3], ':', err)
        else:
            raise AssertionError('the reference accepted ' + repr(bad))
    # histograms for kl_div_forward / inverse / sym / 3: the default case's, with zeros, and a NaN and an inf put in
    hp, hq = store['default_cp'] / d['a'].size, store['default_cq'] / d['b'].size
    hp[[400, 401]] = [np.nan, 0.01]; hq[[401, 520]] = [np.inf, np.nan]
    with np.errstate(all='ignore'):
        store['k3_vals'] = np.array([kl_div_forward(hp, hq), kl_div_inverse(hp, hq), kl_div_sym(hp, hq), *kl_div_3(hp, hq)], np.float64)
    store['k3_p'], store['k3_q'] = hp, hq
    print('k3', store['k3_vals'])
    path = os.path.join(HERE, 'kl_data.npz')
    np.savez_compressed(path, **store)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()

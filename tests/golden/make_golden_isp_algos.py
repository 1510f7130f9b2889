#!/usr/bin/env python3
"""Generate tests/golden/isp_algos.npz + isp_algos.json by running the REAL reference: ``VST``, ``inverse_VST``, ``stdfilt``,
``GuidedFilter`` and ``FastGuidedFilter`` of utils/isp_algos.py and ``bayer2gray`` / ``repair_bad_pixels`` of utils/isp_ops.py.

Runs only where the reference is available (see make_golden.py, whose import stubs it uses); stores data only.

    python tests/golden/make_golden_isp_algos.py

OpenCV is not here, and parity with one build of it is not a goal (include/pnnp_hip.h defines the box mean, the two resizes, the 3 x 3
filter and the 3 x 3 median): the stubbed cv2 gets ``boxFilter``, ``blur``, ``resize``, ``filter2D`` and ``medianBlur`` from the
restatement (tests/_isp_algos_ref.py), each wrapped so that it asserts the window, the border and the dtype the real function hands it.
Everything around those calls is the real function's own numpy; VST / inverse_VST call nothing outside numpy.

Stored per filter case <tag>: the inputs (<tag>_p, <tag>_I, or <tag>_x for stdfilt), <tag>_ref32, the real function's float32 output, and
the same function's output on the float64 copies of the inputs, ref64, as <tag>_d64 = ref64 - float64(ref32), which is exact (asserted) and
compresses where ref64 itself does not: ref64 = float64(ref32) + d64.  Case B lies in isp_algos_b.npz, everything else in isp_algos.npz.  The json lists per case the function, window, eps, shape,
e_ref = max |ref32 - ref64| and the number of elements on which the separable-order restatement differs from the 2-D-order one.  Filter
cases (issue letters): A [8,8] d=3; B [2,4,37,150] d=7 (run plane by plane: the real functions take one image); C d=51 on [52,60] and,
GuidedFilter only, [8,60]; D a constant frame and a two-level step edge; E DN-scale data (0..16383) with eps 1 and 1e-4 * 16383^2 and
unit-scale data with eps 1, 1e-2, 1e-4.  Case B's inputs are 8-bit levels so that its file stays below 1 MiB.

Before anything is written the generator asserts that e_ref is non-zero for every filter case, that the separable order differs from the
2-D order on at most 0.1 % of a case's elements, and that the restatement of each whole function equals the real function bit for bit."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import import_reference  # noqa: E402
import _isp_algos_ref as R  # noqa: E402


class Expect:
    """what the stubbed cv2 calls must receive while one real function runs"""
    d = border = dtype = None
    calls = 0


def install(cv2):
    def check(src, dtype=None):
        assert isinstance(src, np.ndarray) and src.ndim == 2 and src.dtype == (dtype or Expect.dtype), (src.shape, src.dtype, Expect.dtype)
        Expect.calls += 1

    def boxFilter(src, ddepth, ksize, borderType=R.BORDER_DEFAULT):
        check(src)
        assert ddepth == -1 and tuple(ksize) == (Expect.d, Expect.d) and borderType == Expect.border, (ksize, borderType)
        return R.boxFilter(src, ddepth, ksize, borderType=borderType)

    def blur(src, ksize):
        check(src)
        assert tuple(ksize) == (Expect.d, Expect.d) and Expect.border == R.BORDER_DEFAULT
        return R.blur(src, ksize)

    def resize(src, dsize, fx=None, fy=None, interpolation=None):
        check(src)
        assert dsize is None and fx == fy and fx in (0.5, 2) and interpolation == R.INTER_LINEAR
        return R.resize(src, dsize, fx=fx, fy=fy, interpolation=interpolation)

    def filter2D(src, ddepth, kernel, borderType=R.BORDER_DEFAULT):
        check(src)
        assert ddepth == -1 and borderType == R.BORDER_REFLECT and kernel.dtype == np.float32 and np.array_equal(kernel, R.GRAY_KERNEL)
        return R.filter2D(src, ddepth, kernel, borderType=borderType)

    def medianBlur(src, ksize):
        check(np.ascontiguousarray(src))
        assert ksize == 3
        return R.medianBlur(np.ascontiguousarray(src), ksize)

    for k in ('BORDER_REPLICATE', 'BORDER_REFLECT', 'BORDER_REFLECT_101', 'BORDER_DEFAULT', 'INTER_LINEAR'):
        setattr(cv2, k, getattr(R, k))
    cv2.boxFilter, cv2.blur, cv2.resize, cv2.filter2D, cv2.medianBlur = boxFilter, blur, resize, filter2D, medianBlur


def run(fn, args, d, border, dtype, calls, kw):
    Expect.d, Expect.border, Expect.dtype, Expect.calls = d, border, np.dtype(dtype), 0
    out = fn(*[a.astype(dtype) for a in args], **kw)
    assert Expect.calls == calls and out.dtype == np.dtype(dtype), (fn.__name__, Expect.calls, out.dtype)
    return out


def main():
    _, _, isp, _, _, _ = import_reference()
    import utils.isp_algos as algos
    assert algos.cv2 is isp.cv2
    install(isp.cv2)
    rng = np.random.RandomState(2026)
    out, meta = {}, {'filters': [], 'versions': dict(numpy=np.__version__)}

    # ------------------------------------------------------------------ the filters
    def pair(shape, scale=1.0, noise=0.05, levels=None):
        """a smooth guide with texture and a noisy copy of it"""
        H, W = shape[-2:]
        yy, xx = np.mgrid[0:H, 0:W]
        I = 0.5 + 0.3 * np.sin(xx / 5.0 + rng.rand(*shape[:-2], 1, 1) * 6) * np.cos(yy / 7.0) + 0.15 * rng.rand(*shape)
        p = I + noise * rng.randn(*shape)
        if levels:
            I, p = np.round(I * levels) / levels, np.round(p * levels) / levels
        return (p * scale).astype(np.float32), (I * scale).astype(np.float32)

    step = np.full((16, 24), 0.2, np.float32)
    step[:, 11:] = 0.8
    const = np.full((16, 24), 0.7, np.float32)          # with d = 7 the float64 run differs from the float32 one (at d = 5 both return the constant)
    pA, pB, pC, pC8, pE, pEd = pair((8, 8)), pair((2, 4, 37, 150), levels=255), pair((52, 60)), pair((8, 60)), pair((20, 24)), pair((20, 24), 16383.0, 0.02)
    dn2 = 1e-4 * 16383.0 ** 2
    G, F, S = 'GuidedFilter', 'FastGuidedFilter', 'stdfilt'
    cases = [('A_g', G, pA, 3, 1), ('A_f', F, pA, 3, 1), ('A_s', S, pA, 3, None),
             ('B_g', G, pB, 7, 1), ('B_s', S, pB, 7, None),
             ('C_g', G, pC, 51, 1), ('C_f', F, pC, 51, 1), ('C_s', S, pC, 51, None), ('C8_g', G, pC8, 51, 1),
             ('Dc_g', G, (const, const), 7, 1), ('Dc_f', F, (const, const), 7, 1), ('Dc_s', S, (const, const), 7, None),
             ('Ds_g', G, (step, step), 5, 1e-2), ('Ds_f', F, (step, step), 5, 1e-2), ('Ds_s', S, (step, step), 5, None),
             ('Edn1_g', G, pEd, 7, 1), ('Edn1_f', F, pEd, 7, 1), ('Edn2_g', G, pEd, 7, dn2), ('Edn2_f', F, pEd, 7, dn2), ('Edn_s', S, pEd, 5, None),
             ('Eu1_g', G, pE, 7, 1), ('Eu1_f', F, pE, 7, 1), ('Eu2_g', G, pE, 7, 1e-2), ('Eu2_f', F, pE, 7, 1e-2),
             ('Eu4_g', G, pE, 7, 1e-4), ('Eu4_f', F, pE, 7, 1e-4), ('Eu_s', S, pE, 5, None)]
    stored = {}
    for tag, name, (p, I), d, eps in cases:
        real, mine = getattr(algos, name), getattr(R, name)
        planes_p, planes_I = p.reshape(-1, *p.shape[-2:]), I.reshape(-1, *I.shape[-2:])
        res = {np.float32: [], np.float64: []}
        sep_diff = 0
        for pp, ii in zip(planes_p, planes_I):
            for dt in (np.float32, np.float64):
                if name == S:
                    o = run(real, (ii,), d, R.BORDER_DEFAULT, dt, 2, dict(k=d))
                    m, ms = mine(ii.astype(dt), d), mine(ii.astype(dt), d, separable=True)
                else:
                    o = run(real, (pp, ii), d, R.BORDER_REPLICATE if name == G else R.BORDER_DEFAULT, dt, 6 if name == G else 10, dict(d=d, eps=eps))
                    m, ms = mine(pp.astype(dt), ii.astype(dt), d, eps), mine(pp.astype(dt), ii.astype(dt), d, eps, separable=True)
                assert np.array_equal(o.view(np.uint8), m.view(np.uint8)), (tag, 'the restatement is not the real function')
                if dt == np.float32:
                    sep_diff += int((m.view(np.int32) != ms.view(np.int32)).sum())
                res[dt].append(o)
        ref32, ref64 = np.stack(res[np.float32]).reshape(p.shape), np.stack(res[np.float64]).reshape(p.shape)
        e_ref = float(np.abs(ref32.astype(np.float64) - ref64).max())
        assert e_ref > 0, (tag, 'e_ref is zero')
        assert sep_diff <= 1e-3 * ref32.size, (tag, sep_diff, ref32.size)
        if name == S:
            key = stored.setdefault(id(I), tag + '_x')
            if key == tag + '_x':
                out[key] = I
            ins = dict(x=key)
        else:
            kp, ki = stored.setdefault(id(p), tag + '_p'), stored.setdefault(id(I), tag + '_I')
            if kp == tag + '_p':
                out[kp] = p
            if ki == tag + '_I':
                out[ki] = I
            ins = dict(p=kp, I=ki)
        # ref64 is stored as its exact difference from ref32 (the two lie within a factor of two of each other, or the difference is
        # asserted exact anyway): the trailing mantissa bytes of that difference are zero, which the compression removes
        d64 = ref64 - ref32.astype(np.float64)
        assert np.array_equal((ref32.astype(np.float64) + d64).view(np.uint64), ref64.view(np.uint64)), tag
        out[tag + '_ref32'], out[tag + '_d64'] = ref32, d64
        meta['filters'].append(dict(tag=tag, fn=name, d=d, eps=eps, shape=list(p.shape), e_ref=e_ref, max_ref64=float(np.abs(ref64).max()),
                                    sep_diff=sep_diff, **ins))

    # ------------------------------------------------------------------ VST / inverse_VST: no stub; float32 in, float32 out
    n = 1003                                                      # not a multiple of 4
    x = (rng.rand(n) * 1200 - 100).astype(np.float32)             # negatives that the max clamps
    x[:40] = 0
    x[40:80] = -rng.rand(40).astype(np.float32) * 1e4
    y = (rng.rand(n) * 80).astype(np.float32)
    y[:8] = 0
    out['vst_x'], out['ivst_x'] = x, y
    meta['vst'] = []
    for gain in (0.5, 1, 3.7):
        for wp in (1, 16383):
            for sigma, mu in ((0, 0), (2.5, 0), (1.25, 37.5)):
                tag = f'g{gain}_w{wp}_s{sigma}_m{mu}'
                f = algos.VST(x, sigma, mu=mu, gain=gain, wp=wp)
                b = algos.inverse_VST(y, sigma, gain=gain, wp=wp)
                assert f.dtype == np.float32 and b.dtype == np.float32
                assert np.array_equal(f.view(np.int32), R.VST(x, sigma, mu, gain, wp).view(np.int32)), tag
                assert np.array_equal(b.view(np.int32), R.inverse_VST(y, sigma, gain, wp).view(np.int32)), tag
                out['vst_' + tag], out['ivst_' + tag] = f, b
                meta['vst'].append(dict(tag=tag, gain=gain, wp=wp, sigma=sigma, mu=mu))
    d0 = algos.VST(x, 1.5)                                         # the defaults
    assert np.array_equal(d0.view(np.int32), R.VST(x, 1.5).view(np.int32))
    out['vst_default'] = d0

    # ------------------------------------------------------------------ bayer2gray
    for H, W in ((6, 10), (34, 70)):
        m = (rng.rand(H, W) * 16383).astype(np.float32)
        Expect.dtype, Expect.calls = np.dtype(np.float32), 0
        g = isp.bayer2gray(m)
        assert Expect.calls == 1 and g.dtype == np.float32 and np.array_equal(g.view(np.int32), R.bayer2gray(m).view(np.int32))
        out[f'gray_{H}x{W}_x'], out[f'gray_{H}x{W}_out'] = m, g

    # ------------------------------------------------------------------ repair_bad_pixels
    H, W = 8, 12
    small = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1),                    # the corners
             (0, 5), (H - 1, 6), (3, 0), (4, W - 1),                            # the edges
             (2, 4), (2, 6), (4, 4),                                            # neighbours within one colour plane
             (5, 7), (5, 7),                                                    # a duplicate
             (3, 3)]
    meta['repair'] = []
    for tag, dt, shape, pts in (('u16', np.uint16, (H, W), small), ('f32', np.float32, (H, W), small), ('empty', np.uint16, (H, W), []),
                                ('big', np.uint16, (64, 64), [tuple(v) for v in rng.randint(0, 64, size=(4096, 2))])):
        raw = rng.randint(0, 16384, size=shape).astype(dt)
        if dt == np.float32:
            raw = raw + rng.rand(*shape).astype(np.float32)
        for y_, x_ in pts[:: max(1, len(pts) // 64)]:                           # hot pixels, so that a median differs from what it replaces
            raw[y_, x_] = 65535 if dt == np.uint16 else 1e6
        Expect.dtype, Expect.calls = np.dtype(dt), 0
        fixed = isp.repair_bad_pixels(raw.copy(), pts)
        assert Expect.calls == 4 and fixed.dtype == dt
        assert np.array_equal(fixed, R.repair_bad_pixels(raw.copy(), pts)), tag
        untouched = np.ones(shape, bool)
        for y_, x_ in pts:
            untouched[y_, x_] = False
        assert np.array_equal(fixed[untouched], raw[untouched])
        out[f'repair_{tag}_in'], out[f'repair_{tag}_pts'], out[f'repair_{tag}_out'] = raw, np.asarray(pts, np.int32).reshape(-1, 2), fixed
        meta['repair'].append(dict(tag=tag, dtype=np.dtype(dt).name, shape=list(shape), n=len(pts), changed=int((fixed != raw).sum())))
    # the neighbours (2,4), (2,6), (4,4) are hot in the input: a median taken from an already repaired frame would differ
    assert meta['repair'][0]['changed'] >= 10

    # case B goes to a file of its own: every committed file stays below 1 MiB
    for name, keep in (('isp_algos.npz', lambda k: not k.startswith('B_')), ('isp_algos_b.npz', lambda k: k.startswith('B_'))):
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **{k: v for k, v in out.items() if keep(k)})
        size = os.path.getsize(path)
        assert size < (1 << 20), (name, size)
        print(name, 'written:', size, 'bytes')
    json.dump(meta, open(os.path.join(HERE, 'isp_algos.json'), 'w'), indent=1)
    for c in meta['filters']:
        print(c['tag'], c['fn'], c['d'], c['eps'], c['shape'], 'e_ref %.3g' % c['e_ref'], 'sep_diff', c['sep_diff'])
    print(meta['repair'])


if __name__ == '__main__':
    main()

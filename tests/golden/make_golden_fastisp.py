#!/usr/bin/env python3
"""Generate tests/golden/fastisp.npz + fastisp.json by running the REAL reference: ``FastISP`` and ``SimpleISP`` of utils/isp_ops.py:125-158.

Runs only where the reference is available (see make_golden.py, whose import stubs it uses); stores data only.

    python tests/golden/make_golden_fastisp.py

FastISP's one outside call is cv2.cvtColor(raw.astype(np.uint16), cv2.COLOR_BAYER_BG2RGB_EA).  OpenCV is not here, and parity with one
build of it is not a goal (include/pnnp_hip.h defines the demosaic): the stubbed cv2 gets the colour code and a ``cvtColor`` that asserts a
uint16 mosaic and that code, records the mosaic it receives and returns the restatement's demosaic (tests/_fastisp_ref.py).  Everything
around the call -- the gained mosaic, the clip, the 14-bit quantisation, / 16383, the colour matrix, the clip, gamma 2.2 -- is then the real
function's own numpy.  Stored per case: the input, wb, ccm (absent where the call passes None), the captured mosaic, the float64 result
and floor(255 * result).  Cases (each at most 4x24x36):
  a  random data in [-0.1, 1.3], Sony gains, the Sony matrix as float32 (widened by numpy's promotion, as the device table is)
  b  defaults: wb=None, ccm=None (gains 2, the float64 default matrix)
  c  saturated: every plane at least 1 / gain, exactly 1, and 1 - 2^-24
  d  zeros and negative values
  e  the identity matrix, gains 1
  q  quantisation-dense: float32(k / 16383) displaced by -2..+2 ulp on the green planes, the same divided by the gain on R and B

Before anything is written the generator asserts that the restatement equals the real function's output bit for bit, that case q straddles
the front's truncation at many k, and that no stored 255 * result lies within 1e-9 of an integer other than exactly 0 or 255 (so a test
may compare levels exactly)."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import import_reference  # noqa: E402
import _fastisp_ref as R  # noqa: E402
from _isp_ref import SONY_CCM, SONY_WB  # noqa: E402

BAYER_BG2RGB_EA = 137          # OpenCV's value of the colour code; only its identity matters here


def ulp_shift(v, d):
    return (np.asarray(v, np.float32).view(np.int32) + np.asarray(d, np.int32)).view(np.float32)


def main():
    archs, proc, isp, losses, data_process, base_trainer = import_reference()
    seen = []

    def cvt(src, code):
        assert isinstance(src, np.ndarray) and src.dtype == np.uint16 and src.ndim == 2 and code == BAYER_BG2RGB_EA
        seen.append(src.copy())
        return R.demosaic_ea(src)

    isp.cv2.COLOR_BAYER_BG2RGB_EA = BAYER_BG2RGB_EA
    isp.cv2.cvtColor = cvt

    rng = np.random.RandomState(2025)
    wb, ccm = SONY_WB, SONY_CCM
    one, eye = np.ones(4, np.float32), np.eye(3, dtype=np.float32)
    h, w = 24, 36

    sat = np.empty((4, 12, 36), np.float32)
    sat[..., :12] = 1 + rng.rand(4, 12, 12).astype(np.float32) * 0.3
    sat[..., 12:24] = 1.0
    sat[..., 24:] = np.float32(1) - np.float32(2.0 ** -24)
    sat[:, :6] /= wb.reshape(4, 1, 1)

    neg = np.zeros((4, 8, 12), np.float32)
    neg[..., 4:8] = -rng.rand(4, 8, 4).astype(np.float32)
    neg[..., 8:] = rng.rand(4, 8, 4).astype(np.float32) * 1e-4

    ks = rng.randint(1, 16384, size=(4, h, w))
    dense = ulp_shift((ks / 16383).astype(np.float32), rng.randint(-2, 3, size=ks.shape))
    dense[0] /= wb[0]
    dense[2] /= wb[2]

    cases = [('a', (rng.rand(4, h, w) * 1.4 - 0.1).astype(np.float32), wb, ccm),
             ('b', (rng.rand(4, 12, 18) * 0.7 - 0.05).astype(np.float32), None, None),
             ('c', sat, wb, ccm),
             ('d', neg, wb, ccm),
             ('e', (rng.rand(4, 7, 9) * 1.2 - 0.1).astype(np.float32), one, eye),
             ('q', dense, wb, ccm)]
    out, meta = {}, {'cases': [], 'versions': dict(numpy=np.__version__)}
    for tag, x, g, m in cases:
        del seen[:]
        ref = isp.FastISP(x, wb=g, ccm=m, gamma=2.2)
        assert len(seen) == 1 and ref.dtype == np.float64 and ref.shape == (2 * x.shape[1], 2 * x.shape[2], 3)
        mosaic = seen[0]
        assert np.array_equal(R.front(x, g), mosaic), tag
        assert np.array_equal(R.fastisp(x, g, m).view(np.uint64), ref.view(np.uint64)), tag
        s = 255 * ref
        near = (np.abs(s - np.rint(s)) < 1e-9) & (s != 0) & (s != 255)
        assert not near.any(), (tag, int(near.sum()))
        out[tag + '_x'], out[tag + '_mosaic'], out[tag + '_out'], out[tag + '_u8'] = x, mosaic, ref, R.levels(ref)
        if g is not None:
            out[tag + '_wb'], out[tag + '_ccm'] = g, m
        meta['cases'].append(dict(tag=tag, shape=list(x.shape), defaults=g is None, levels=[int(out[tag + '_u8'].min()), int(out[tag + '_u8'].max())]))
    # the dense case: the truncation yields k for some displacements and k - 1 for others, on every plane
    S = out['q_mosaic']
    got = np.stack([S[0::2, 0::2], S[0::2, 1::2], S[1::2, 1::2], S[1::2, 0::2]])
    straddle = [int((got[p] == ks[p]).sum()) for p in range(4)], [int((got[p] == ks[p] - 1).sum()) for p in range(4)]
    assert set(np.unique(got.astype(np.int64) - ks)) <= {-1, 0} and min(straddle[0]) > 100 and min(straddle[1]) > 100, straddle
    meta['dense_straddle'] = dict(at_k=straddle[0], below_k=straddle[1])
    # saturated: the mosaic is 16383 wherever the gained value reaches 1, 16382 where it stays an ulp below
    assert (out['c_mosaic'] >= 16382).all() and (out['c_mosaic'][12:, :48] == 16383).all() and (out['c_mosaic'][12:, 48:] == 16382).any()
    assert out['c_u8'].max() == 255

    # SimpleISP (utils/isp_ops.py:125-132): [h,w,4] RGGB -> float64 [h,w,3]
    raw = rng.randint(400, 16500, size=(10, 14, 4)).astype(np.uint16)
    swb = [2.13, 1.0, 1.0, 1.57]
    simple = isp.SimpleISP(raw, bl=512, wp=16383, wb=swb, gamma=2.2)
    assert simple.dtype == np.float64 and simple.shape == (10, 14, 3)
    out['simple_raw'], out['simple_wb'], out['simple_out'] = raw, np.array(swb), simple
    simple_d = isp.SimpleISP(raw)
    out['simple_default_out'] = simple_d

    np.savez_compressed(os.path.join(HERE, 'fastisp.npz'), **out)
    json.dump(meta, open(os.path.join(HERE, 'fastisp.json'), 'w'), indent=1)
    print('fastisp fixtures written:', os.path.getsize(os.path.join(HERE, 'fastisp.npz')), 'bytes')
    for c in meta['cases']:
        print(c)
    print(meta['dense_straddle'])


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""Generate tests/golden/unprocess.npz + unprocess.json by running the REAL reference: ``inverse_smoothstep``, ``gamma_expansion``,
``apply_ccm``, ``safe_invert_gains``, ``mosaic``, ``mosaic_GBRG``, ``unprocess`` and ``random_ccm`` of data_process/unprocess.py, and
``process`` of data_process/process.py for the round trip.

Runs only where the reference is available (see make_golden.py, whose import stubs it uses); stores data only.

    python tests/golden/make_golden_unprocess.py

Cases (every image at most 64x130x3).  a-e, quad and nan run the lines of ``unprocess`` (:199-207) with given parameters:
  a     random data in [-0.1, 1.2], the IMX686 matrix, 64x66x3 (W / 2 = 33)
  b     B = 3 of 34x130x3, three different matrices and gains (per-image parameters)
  c     highlights: values in [0.85, 1] and exactly 1 under a matrix whose rows sum to 1.08, so that the mask spans 0..1 and beyond
        (asserted: gray below 0.9, between 0.9 and 1, and at or above 1)
  d     0, negative values, 1e-9, 1e-8, 1e-6, 1e-4 (the tone curve's cancellation near 0)
  e     the SonyA7S2 identity matrix with lock_wb = ([1.], [2.1], [1.7]), through ``unprocess`` itself
  quad  one 2x2x3 image;  nan: 4x8x3 with one NaN channel in one pixel
  f     ``unprocess`` under torch.manual_seed / np.random.seed for both cameras, on a 3-D image and a 4-D stack: outputs, metadata and the
        RNG states left behind
  g     ``mosaic`` and ``mosaic_GBRG`` on a 5-D stack [2,2,6,8,3]
  rt    round trip: mid-range values constant over each 2x2 quad, ``unprocess`` (locked gains) -> ``mosaic`` -> ``process`` with the
        inverse gains and cam2rgb -> smoothstep on the host; the reference's own largest |result - x| is recorded

Per case the generator records E_abs / E_rel, the reference's largest absolute / relative error against the float64 restatement
(tests/_unprocess_ref.py; E_rel over float64 values above 1e-6).  Before anything is written it asserts that the float32 restatement equals
the reference exactly on this host.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import import_reference  # noqa: E402
import _unprocess_ref as R  # noqa: E402


def main():
    import torch
    archs, proc, isp, losses, data_process, base_trainer = import_reference()
    import data_process.unprocess  # noqa: F401
    U = sys.modules['data_process.unprocess']                    # a function named `unprocess` shadows the attribute
    rng = np.random.RandomState(2025)
    out, meta = {}, {'cases': {}, 'versions': dict(numpy=np.__version__, torch=torch.__version__)}
    imx, sony = R.CCMS['IMX686'], R.CCMS['SonyA7S2']
    assert np.array_equal(U.random_ccm('IMX686').numpy(), imx) and np.array_equal(U.random_ccm('SonyA7S2').numpy(), sony)

    def reference_lines(x, m, rgb, red, blue):
        """unprocess.py:199-207 on one image with given parameters"""
        t = U.inverse_smoothstep(torch.from_numpy(x))
        t = U.gamma_expansion(t)
        t = U.apply_ccm(t, torch.from_numpy(m))
        t = U.safe_invert_gains(t, torch.tensor([rgb]), torch.tensor([red]), torch.tensor([blue]))
        return torch.clamp(t, min=0.0, max=1.0).numpy()

    def record(tag, x, ms, gs):
        """x [B,H,W,3]; ms [B,3,3]; gs [B,3] = (rgb_gain, red_gain, blue_gain) per image"""
        x, ms, gs = np.asarray(x, np.float32), np.asarray(ms, np.float32), np.asarray(gs, np.float32)
        ref = np.stack([reference_lines(x[i], ms[i], *[float(v) for v in gs[i]]) for i in range(len(x))])
        gains = np.stack([R.gains_f32(*gs[i]) for i in range(len(x))])
        mine = np.stack([R.unprocess_f32(x[i], ms[i], gains[i]) for i in range(len(x))])
        assert np.array_equal(mine.view(np.uint32), ref.view(np.uint32)), tag      # the float32 restatement IS the reference on this host
        e_abs, e_rel = R.errors(ref, R.batch_f64(x, ms, gains))
        out[tag + '_x'], out[tag + '_m'], out[tag + '_g'], out[tag + '_gains'], out[tag + '_ref'] = x, ms, gs, gains, ref
        meta['cases'][tag] = dict(shape=list(x.shape), E_abs=e_abs, E_rel=e_rel)
        return ref

    g0 = [1.25, 1.9, 1.6]
    record('a', rng.rand(1, 64, 66, 3) * 1.3 - 0.1, imx[None], [g0])
    mb = np.stack([imx, (imx * np.float32(0.95) + np.float32(0.01)).astype(np.float32), sony])
    record('b', rng.rand(3, 34, 130, 3) * 1.3 - 0.1, mb, [g0, [1.1, 2.3, 1.45], [1.4, 1.75, 2.6]])

    hi = (0.85 + 0.15 * rng.rand(1, 32, 48, 3)).astype(np.float32)
    hi[:, :, 32:] = 1.0
    hi[:, :8, :16] = np.float32(0.85) + np.float32(0.05) * rng.rand(1, 8, 16, 3).astype(np.float32)
    mc = (imx * np.float32(1.08)).astype(np.float32)
    record('c', hi, mc[None], [g0])
    x64 = np.clip(hi.astype(np.float64), 0, 1)
    l64 = np.maximum(0.5 - np.sin(np.arcsin(1 - 2 * x64) / 3), 1e-8) ** 2.2
    gray = (l64 @ mc.astype(np.float64).T).mean(-1)
    assert (gray < 0.9).any() and ((gray > 0.9) & (gray < 1.0)).any() and (gray >= 1.0).any()      # the mask spans 0..1 and beyond
    meta['cases']['c']['gray'] = [float(gray.min()), float(gray.max())]

    small = np.zeros((1, 8, 28, 3), np.float32)
    for k, v in enumerate([0.0, -0.05, -1.0, 1e-9, 1e-8, 1e-6, 1e-4]):
        small[:, :, 4 * k:4 * k + 4] = np.float32(v)
    small[:, 4:, :, 1] = np.float32(0.3)                         # lower half: a mid-range green beside them
    record('d', small, imx[None], [g0])

    record('quad', rng.rand(1, 2, 2, 3), imx[None], [g0])
    xn = rng.rand(1, 4, 8, 3).astype(np.float32)
    xn[0, 1, 5, 2] = np.nan
    refn = record('nan', xn, imx[None], [g0])
    assert np.isnan(refn[0, 1, 5]).all() and np.isnan(refn).sum() == 3                            # through the matrix: all three channels

    # e: the identity matrix with locked gains, through unprocess() itself
    xe = rng.rand(32, 40, 3).astype(np.float32)
    lock = ([1.], [2.1], [1.7])
    refe, md = U.unprocess(torch.from_numpy(xe), lock_wb=lock, camera_type='SonyA7S2')
    assert [float(md[k]) for k in ('rgb_gain', 'red_gain', 'blue_gain')] == [1.0, float(np.float32(2.1)), float(np.float32(1.7))]
    rece = record('e', xe[None], sony[None], [[1.0, 2.1, 1.7]])
    assert np.array_equal(rece[0].view(np.uint32), refe.numpy().view(np.uint32))

    # f: unprocess() under seeds: the host draws, the outputs, the RNG states left behind
    for cam in ('IMX686', 'SonyA7S2'):
        for tag, shape in (('3d', (16, 20, 3)), ('4d', (2, 8, 12, 3))):
            x = rng.rand(*shape).astype(np.float32)
            torch.manual_seed(11); np.random.seed(13)
            ref, md = U.unprocess(torch.from_numpy(x), camera_type=cam)
            key = f'f_{cam}_{tag}'
            out[key + '_x'], out[key + '_ref'] = x, ref.numpy()
            for k in ('cam2rgb', 'rgb_gain', 'red_gain', 'blue_gain'):
                out[f'{key}_{k}'] = md[k].numpy()
            st = np.random.get_state()
            out[key + '_torch_state'], out[key + '_np_keys'], out[key + '_np_pos'] = torch.get_rng_state().numpy(), st[1], np.int64(st[2])
            gains = R.gains_f32(md['rgb_gain'].numpy(), md['red_gain'].numpy(), md['blue_gain'].numpy())
            flat = x.reshape((-1,) + shape[-3:])
            mine = np.stack([R.unprocess_f32(v, R.CCMS[cam], gains) for v in flat]).reshape(shape)
            assert np.array_equal(mine.view(np.uint32), ref.numpy().view(np.uint32)), key
            e_abs, e_rel = R.errors(ref.numpy(), R.batch_f64(flat, R.CCMS[cam], gains).reshape(shape))
            meta['cases'][key] = dict(shape=list(shape), E_abs=e_abs, E_rel=e_rel, seeds=dict(torch=11, numpy=13))

    # g: the gathers on a 5-D stack
    xg = rng.rand(2, 2, 6, 8, 3).astype(np.float32)
    out['g_x'] = xg
    out['g_rggb'], out['g_gbrg'] = U.mosaic(torch.from_numpy(xg)).numpy(), U.mosaic_GBRG(torch.from_numpy(xg)).numpy()
    assert out['g_rggb'].shape == (2, 2, 3, 4, 4)
    assert np.array_equal(R.mosaic(xg), out['g_rggb']) and np.array_equal(R.mosaic(xg, gbrg=True), out['g_gbrg'])
    # ... and as index maps: a tensor that holds its own flat index
    idx = np.arange(4 * 6 * 3, dtype=np.float32).reshape(4, 6, 3)
    out['g_idx_rggb'], out['g_idx_gbrg'] = U.mosaic(torch.from_numpy(idx)).numpy(), U.mosaic_GBRG(torch.from_numpy(idx)).numpy()

    # rt: the round trip through the reference's own ISP
    base = (0.25 + 0.5 * rng.rand(16, 24, 3)).astype(np.float32)
    xr = np.repeat(np.repeat(base, 2, axis=0), 2, axis=1)                                         # constant over each 2x2 quad
    lock = ([1.2], [1.9], [1.6])
    un, md = U.unprocess(torch.from_numpy(xr), lock_wb=lock, camera_type='IMX686')
    assert float(un.max()) < 1.0 and float(un.min()) > 0.0                                        # no clamp binds
    pk = U.mosaic(un[None]).permute(0, 3, 1, 2).contiguous()
    rgb_gain, red, blue = [float(md[k]) for k in ('rgb_gain', 'red_gain', 'blue_gain')]
    wb = torch.tensor([[red * rgb_gain, rgb_gain, blue * rgb_gain, rgb_gain]])
    back = proc.process(pk, wbs=wb, cam2rgbs=md['cam2rgb'][None], gamma=2.2).numpy()[0].transpose(1, 2, 0)
    s = back.astype(np.float64)
    e_rt = float(np.abs(3 * s ** 2 - 2 * s ** 3 - base).max())
    out['rt_x'], out['rt_lock'], out['rt_wb'], out['rt_cam2rgb'] = xr, np.array(lock, np.float32), wb.numpy(), md['cam2rgb'].numpy()
    meta['cases']['rt'] = dict(shape=list(xr.shape), E_roundtrip=e_rt)

    np.savez_compressed(os.path.join(HERE, 'unprocess.npz'), **out)
    json.dump(meta, open(os.path.join(HERE, 'unprocess.json'), 'w'), indent=1)
    print('unprocess fixtures written:', os.path.getsize(os.path.join(HERE, 'unprocess.npz')), 'bytes')
    for k, c in meta['cases'].items():
        print(k, c)


if __name__ == '__main__':
    main()

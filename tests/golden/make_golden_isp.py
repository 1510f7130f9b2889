#!/usr/bin/env python3
"""Generate tests/golden/isp.npz + isp.json by running the REAL reference: ``process``, ``raw2rgb_v2`` and ``gamma_compression`` of
data_process/process.py:104-184, and the numpy lines of the trainers' preview strip.

Runs only where the reference is available (see make_golden.py, whose import stubs it uses); stores data only.

    python tests/golden/make_golden_isp.py

Renders are stored as uint8 levels k; the generator asserts that the reference's float result is exactly float32(k) / 255.  Cases (every one
at most 4x64x100 per image):
  a  random data in [-0.1, 1.3], Sony white balance and the Sony matrix (utils/isp_ops.py:151-153), N = 1
  b  N = 2, one shared wb [1,4], two matrices
  c  saturated: blocks where all four planes are at least 1, exactly 1, and 1 - 2^-24
  d  boundary-dense: identity matrix, wb = 1, R = G1 = G2 = B; every value is float32((k/255)^2.2) displaced by -32..+31 ulp, for every k in
     1..255 (64 offsets per k, so every quantisation threshold is straddled: asserted below); 16 320 values as 3 images of 64x85; only
     plane R is stored
  e  zeros, negative values, 1e-8, 1e-9
  g  gamma_compression alone on [1,3,24,36] in [-0.1, 1.3];  v2: raw2rgb_v2 on [4,16,20]
  f  preview strips, wb [2.13, 1, 1.57, 1], 4x32x40.  The preview lines are inline in train() and cannot be called; the lines below are
     those of trainer_SID.py:150-157 and trainer_NF_SID.py:166-167,175-179 (quoted beside them), applied to tensors as the trainers hold
     them.  trainer_SID does not clip before the power, so its strip is recorded on data whose gained values stay inside [0,1]
     (inputs may be negative: they are clipped at :150); the NF strip, which clips at :179, is recorded on data in [-0.1, 1.2].

Before anything is written the generator asserts, on the CPU, that in every case the reference against the round-once float64 restatement
(tests/_isp_ref.py) stays under HALF the cap of the agreement rule, and that the float32 restatement equals the reference exactly.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import import_reference  # noqa: E402
import _isp_ref as R  # noqa: E402


def ulp_shift(v, d):
    """float32 values moved by d units in the last place (positive finite values)"""
    return (np.asarray(v, np.float32).view(np.int32) + np.asarray(d, np.int32)).view(np.float32)


def inv_gain(t, w, ge):
    """the float32 x nearest to t / w with float32(x * w) >= t (``ge``) or <= t: equal to t wherever t has a preimage under the gain"""
    t, w = np.broadcast_arrays(np.asarray(t, np.float32), np.asarray(w, np.float32))
    x0 = (t / w).astype(np.float32)
    x = np.full(t.shape, np.nan, np.float32)
    for d in (range(-4, 5) if ge else range(4, -5, -1)):
        c = ulp_shift(x0, np.full(t.shape, d, np.int32))
        p = (c * w).astype(np.float32)
        hit = np.isnan(x) & ((p >= t) if ge else (p <= t))
        x[hit] = c[hit]
    assert not np.isnan(x).any()
    return x


def main():
    import torch
    archs, proc, isp, losses, data_process, base_trainer = import_reference()
    rng = np.random.RandomState(2024)
    out, meta = {}, {'cases': [], 'versions': dict(numpy=np.__version__, torch=torch.__version__)}
    wb, ccm = R.SONY_WB, R.SONY_CCM
    ccm2 = (ccm * np.array([[0.9, 1.1, 1.0]], np.float32) + np.float32(0.01)).astype(np.float32)
    eye = np.eye(3, dtype=np.float32)
    one = np.ones(4, np.float32)

    sat = np.empty((1, 4, 16, 48), np.float32)
    sat[..., :16] = 1 + rng.rand(1, 4, 16, 16).astype(np.float32) * 0.3
    sat[..., 16:32] = 1.0
    sat[..., 32:] = np.float32(1) - np.float32(2.0 ** -24)
    w4 = wb.reshape(1, 4, 1, 1)
    sat[..., :32] = inv_gain(sat[..., :32], w4, True)        # x * wb >= 1 (exactly 1 where 1 has a preimage under the gain)
    sat[..., 32:] = inv_gain(sat[..., 32:], w4, False)       # x * wb = 1 - 2^-24 on the green planes (gain 1), the nearest value below it elsewhere
    sat[:, :, 8:] = np.maximum(sat[:, :, 8:], np.float32(1.0))   # lower half: raw values of at least 1 themselves

    ks = np.arange(1, 256)
    base = ((ks / 255.0) ** 2.2).astype(np.float32)
    dense = ulp_shift(np.repeat(base, 64), np.tile(np.arange(-32, 32), 255)).reshape(3, 1, 64, 85)
    dense4 = np.repeat(dense, 4, axis=1)

    edge = np.zeros((1, 4, 8, 16), np.float32)
    edge[..., 4:8] = -rng.rand(1, 4, 8, 4).astype(np.float32)
    edge[..., 8:12] = np.float32(1e-8)
    edge[..., 12:] = np.float32(1e-9)
    edge[:, :, 4:, 8:] /= wb.reshape(1, 4, 1, 1)              # ... and gained values next to 1e-8 / 1e-9

    cases = [('a', (rng.rand(1, 4, 64, 100) * 1.4 - 0.1).astype(np.float32), wb[None], ccm[None]),
             ('b', (rng.rand(2, 4, 32, 52) * 1.4 - 0.1).astype(np.float32), wb[None], np.stack([ccm, ccm2])),
             ('c', sat, wb[None], ccm[None]),
             ('d', dense4, one[None], eye[None]),
             ('e', edge, wb[None], ccm[None])]
    half_cap = R.CAP / 2
    for tag, x, w, m in cases:
        N = x.shape[0]
        ref = proc.process(torch.from_numpy(x), wbs=torch.from_numpy(w), cam2rgbs=torch.from_numpy(m).repeat(N // m.shape[0], 1, 1), gamma=2.2).numpy()
        k = R.to_levels(ref)
        assert np.array_equal(R.process_levels(x, w, m), k), tag           # the float32 restatement IS the reference on this host
        n_diff, n_bad = R.disagreements(R.process_levels(x, w, m, once=True), k, R.process_pre(x, w, m))
        assert n_bad == 0 and n_diff <= half_cap * k.size, (tag, n_diff, n_bad, k.size)
        out[tag + '_x'] = x[:, :1] if tag == 'd' else x
        out[tag + '_wb'], out[tag + '_ccm'], out[tag + '_k'] = w, m, k.astype(np.uint8)
        meta['cases'].append(dict(tag=tag, shape=list(x.shape), once_vs_reference=n_diff, values=int(k.size)))
    # coverage of the boundary-dense case: every level 1..255 has values on both sides of its threshold
    kd = out['d_k'][:, 0].reshape(255, 64).astype(np.int64)
    assert all((kd[i] == i).any() and (kd[i] == i + 1).any() for i in range(255))
    # saturated: the three kinds of row sum are all there
    lin_c = R.linear(sat, wb, ccm).numpy()
    assert (np.clip(sat * w4, 0, 1)[..., :32] == 1).all() and (np.clip(sat * w4, 0, 1)[:, :, :8, 32:] < 1).all()
    assert (sat[:, 1, :8, 32:] == np.float32(1) - np.float32(2.0 ** -24)).all()
    assert set(np.unique(lin_c[..., :32])) <= {np.float32(1), np.float32(1) - np.float32(2.0 ** -24)} and set(np.unique(out['c_k'])) == {254, 255}

    g = (rng.rand(1, 3, 24, 36) * 1.4 - 0.1).astype(np.float32)
    kg = R.to_levels(proc.gamma_compression(torch.from_numpy(g)).numpy())
    assert np.array_equal(R.levels(g), kg)
    n_diff, n_bad = R.disagreements(R.levels_once(g), kg, R.pre(g))
    assert n_bad == 0 and n_diff <= half_cap * kg.size
    out['g_x'], out['g_k'] = g, kg.astype(np.uint8)

    v2 = (rng.rand(4, 16, 20) * 1.4 - 0.1).astype(np.float32)
    r2 = proc.raw2rgb_v2(v2, wb, ccm)
    assert r2.shape == (16, 20, 3) and r2.dtype == np.float32
    k2 = R.to_levels(r2)
    assert np.array_equal(R.process_levels(v2[None], wb, ccm)[0].transpose(1, 2, 0), k2)
    out['v2_x'], out['v2_k'] = v2, k2.astype(np.uint8)

    # ---- preview strips
    pwb = torch.tensor([[2.13, 1.0, 1.57, 1.0]])
    data = {'wb': pwb}
    # trainer_SID.py:143,150-157 -- values whose gained result stays inside [0,1]
    imgs_lr = torch.from_numpy((rng.rand(1, 4, 32, 40) * 0.5 - 0.05).astype(np.float32)) / pwb.view(1, 4, 1, 1)
    pred = torch.from_numpy(rng.rand(1, 4, 32, 40).astype(np.float32)) / pwb.view(1, 4, 1, 1)
    imgs_hr = torch.from_numpy(rng.rand(1, 4, 32, 40).astype(np.float32)) / pwb.view(1, 4, 1, 1)
    wbn = data['wb'][0].numpy()                                                          # :143
    inputs = imgs_lr[0].detach().cpu().numpy().clip(0, 1)                                # :150
    output = pred[0].detach().cpu().numpy()                                              # :151
    target = imgs_hr[0].detach().cpu().numpy()                                           # :152
    temp_img = np.concatenate((inputs, output, target), axis=2)[:3]                      # :153
    temp_img[0] = temp_img[0] * wbn[0]                                                   # :154
    temp_img[2] = temp_img[2] * wbn[2]                                                   # :155
    temp_img = temp_img.transpose(1, 2, 0)[:, :, ::-1] ** (1 / 2.2)                      # :157
    assert temp_img.dtype == np.float32 and np.isfinite(temp_img).all() and temp_img.min() >= 0 and temp_img.max() <= 1
    sid = np.uint8(temp_img * 255)                                                       # :158 (what cv2.imwrite receives)
    out['f_sid_lr'], out['f_sid_pred'], out['f_sid_hr'], out['f_sid_u8'] = imgs_lr.numpy()[0], pred.numpy()[0], imgs_hr.numpy()[0], sid
    # trainer_NF_SID.py:161,166-168,175-180
    imgs_hr = torch.from_numpy((rng.rand(1, 4, 32, 40) * 1.3 - 0.1).astype(np.float32))
    imgs_nf = torch.from_numpy((rng.randn(1, 4, 32, 40) * 0.2).astype(np.float32))
    imgs_lr = torch.from_numpy((rng.rand(1, 4, 32, 40) * 1.3 - 0.1).astype(np.float32))
    inputs = imgs_hr[0].detach().cpu().numpy().clip(0, 1)                                # :166
    output = imgs_nf[0].detach().cpu().numpy() + inputs                                  # :167
    target = imgs_lr[0].detach().cpu().numpy()                                           # :168
    temp_img = np.concatenate((inputs, output, target), axis=2)[:3]                      # :175
    temp_img[0] = temp_img[0] * wbn[0]                                                   # :176
    temp_img[2] = temp_img[2] * wbn[2]                                                   # :177
    temp_img = temp_img.transpose(1, 2, 0)[:, :, ::-1].clip(0, 1) ** (1 / 2.2)           # :179
    assert temp_img.dtype == np.float32
    nf = np.uint8(temp_img * 255)                                                        # :180
    out['f_nf_hr'], out['f_nf_sample'], out['f_nf_lr'], out['f_nf_u8'] = imgs_hr.numpy()[0], imgs_nf.numpy()[0], imgs_lr.numpy()[0], nf
    out['f_wb'] = wbn
    for tag, args, add in (('f_sid', ('f_sid_lr', 'f_sid_pred', 'f_sid_hr'), False), ('f_nf', ('f_nf_hr', 'f_nf_sample', 'f_nf_lr'), True)):
        lin = R.preview_linear(*[out[a] for a in args], wbn, add_inputs_to_output=add)
        n_diff, n_bad = R.disagreements(R.levels_once(lin, floor=False), out[tag + '_u8'], R.pre(lin, floor=False))
        assert n_bad == 0 and n_diff <= half_cap * lin.size, (tag, n_diff, n_bad)
        meta['cases'].append(dict(tag=tag, shape=list(lin.shape), once_vs_reference=n_diff, values=int(lin.size)))

    np.savez_compressed(os.path.join(HERE, 'isp.npz'), **out)
    json.dump(meta, open(os.path.join(HERE, 'isp.json'), 'w'), indent=1)
    print('isp fixtures written:', os.path.getsize(os.path.join(HERE, 'isp.npz')), 'bytes')
    for c in meta['cases']:
        print(c)


if __name__ == '__main__':
    main()

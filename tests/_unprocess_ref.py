"""The restatement of the reference's sRGB -> raw unprocessing (data_process/unprocess.py:79-121, 199-207) and of its Bayer gathers
(:123-167) that csrc/unprocess.hip is tested against; tests/test_oracle_unprocess.py pins it to the reference's own outputs
(tests/golden/unprocess.npz, written by tests/golden/make_golden_unprocess.py).

Per pixel of a channel-last image, with m = rgb2cam and gains = (1 / red, 1, 1 / blue) / rgb_gain:

    x = clamp(image, 0, 1);  s = 0.5 - sin(asin(1 - 2x) / 3);  l = max(s, 1e-8) ** 2.2;  c = l . m^T
    gray = mean(c);  mask = (max(gray - 0.9, 0) / (1 - 0.9)) ** 2;  safe = max(mask + (1 - mask) gains, gains);  out = clamp(c safe, 0, 1)

``unprocess_f32`` runs these lines with torch's CPU float32 ops (what the reference ran: the generator asserts it EQUALS the reference on the
generating host); ``unprocess_f64`` runs them in float64 on the float32 inputs and parameters, the quantity the agreement rule looks at.

The agreement rule (``assert_within``): a bit-for-bit match with torch's CPU asin / sin / pow cannot be asked of a device, so the rule is
against float64.  The generator records per case E_abs and E_rel, the reference's own largest absolute and largest relative error against
``unprocess_f64`` (E_rel over elements whose float64 value exceeds REL_FLOOR = 1e-6).  A result must stay, in every element, within
max(4 E_abs, one float32 ulp of the value) absolutely and within max(4 E_rel, that ulp over the value) relatively; no element is excepted.
4 x is the margin the project gives reference-relative bars; the ulp floor keeps an exact case from demanding
exactness.  A NaN must stand exactly where the float64 restatement has one."""
import numpy as np
import torch

REL_FLOOR = 1e-6
MARGIN = 4.0

CCMS = {'SonyA7S2': np.eye(3, dtype=np.float32),
        'IMX686': np.array([[0.61093086, 0.31565922, 0.07340994], [0.09433191, 0.7658969, 0.1397712], [0.03532438, 0.3020709, 0.6626047]], np.float32)}


def gains_f32(rgb_gain, red_gain, blue_gain):
    """float32 [3]: (1 / red, 1, 1 / blue) / rgb_gain with torch's float32 tensor ops, as safe_invert_gains forms it"""
    t = [torch.as_tensor(np.asarray(v, np.float32).reshape(1)) for v in (rgb_gain, red_gain, blue_gain)]
    return (torch.stack((1.0 / t[1], torch.tensor([1.0]), 1.0 / t[2])) / t[0]).reshape(3).numpy()


def _lines(x, m, gains):
    """the lines above on torch tensors of one dtype: x [...,3], m [3,3], gains [3]"""
    x = torch.clamp(x, min=0.0, max=1.0)
    s = 0.5 - torch.sin(torch.asin(1.0 - 2.0 * x) / 3.0)
    l = torch.clamp(s, min=1e-8) ** 2.2
    c = torch.reshape(torch.tensordot(torch.reshape(l, [-1, 3]), m, dims=[[-1], [-1]]), l.size())
    gray = torch.mean(c, dim=-1, keepdim=True)
    mask = (torch.clamp(gray - 0.9, min=0.0) / (1.0 - 0.9)) ** 2.0
    g = gains.view(1, 1, 3)
    return torch.clamp(c * torch.max(mask + (1.0 - mask) * g, g), min=0.0, max=1.0)


def unprocess_f32(image, rgb2cam, gains):
    """one image [H,W,3] float32, torch CPU float32 -> numpy float32"""
    return _lines(torch.as_tensor(np.asarray(image, np.float32)), torch.as_tensor(np.asarray(rgb2cam, np.float32)),
                  torch.as_tensor(np.asarray(gains, np.float32))).numpy()


def unprocess_f64(image, rgb2cam, gains):
    """the same lines in float64 on the float32 inputs and parameters -> numpy float64"""
    f = lambda v: torch.as_tensor(np.asarray(v, np.float32).astype(np.float64))
    return _lines(f(image), f(rgb2cam), f(gains)).numpy()


def batch_f64(images, rgb2cams, gains):
    """[B,H,W,3] with per-image parameters [B,3,3] / [3,3] and [B,3] / [3]"""
    B = len(images)
    m = np.broadcast_to(np.asarray(rgb2cams, np.float32), (B, 3, 3))
    g = np.broadcast_to(np.asarray(gains, np.float32), (B, 3))
    return np.stack([unprocess_f64(images[i], m[i], g[i]) for i in range(B)])


def mosaic(image, gbrg=False):
    """[...,H,W,3] -> [...,H/2,W/2,4] channel-last: R, Gr, B, Gb (mosaic) or R, Gr, Gb, B on the GBRG pattern (mosaic_GBRG)"""
    a = np.asarray(image)
    if gbrg:
        return np.stack((a[..., 1::2, 0::2, 0], a[..., 1::2, 1::2, 1], a[..., 0::2, 0::2, 1], a[..., 0::2, 1::2, 2]), axis=-1)
    return np.stack((a[..., 0::2, 0::2, 0], a[..., 0::2, 1::2, 1], a[..., 1::2, 1::2, 2], a[..., 1::2, 0::2, 1]), axis=-1)


def packed(image, gbrg=False):
    """[B,H,W,3] -> [B,4,H/2,W/2]: the gather as the train step takes it (channel-first)"""
    return np.moveaxis(mosaic(image, gbrg), -1, 1)


def errors(got, want64):
    """-> (largest absolute error, largest relative error over elements whose float64 value exceeds REL_FLOOR); NaN positions must agree"""
    got, want64 = np.asarray(got, np.float64), np.asarray(want64, np.float64)
    assert got.shape == want64.shape, (got.shape, want64.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want64)), 'NaN positions differ'
    ok = ~np.isnan(want64)
    d = np.abs(got - want64)[ok]
    w = np.abs(want64[ok])
    big = w > REL_FLOOR
    return float(d.max()) if d.size else 0.0, float((d[big] / w[big]).max()) if big.any() else 0.0


def assert_within(got, want64, e_abs, e_rel, what=''):
    """the agreement rule, every element; -> the observed (abs, rel) errors, printed before anything is asserted"""
    got, want64 = np.asarray(got, np.float64), np.asarray(want64, np.float64)
    obs = errors(got, want64)
    print(f'unprocess agreement {what}: abs {obs[0]:.3e} (reference {e_abs:.3e}), rel {obs[1]:.3e} (reference {e_rel:.3e})')
    ok = ~np.isnan(want64)
    d, w = np.abs(got - want64)[ok], np.abs(want64[ok])
    ulp = np.spacing(w.astype(np.float32)).astype(np.float64)
    bad_abs = d > np.maximum(MARGIN * e_abs, ulp)
    big = w > REL_FLOOR
    bad_rel = big & (d > np.maximum(MARGIN * e_rel * w, ulp))
    assert not bad_abs.any(), f'{what}: {int(bad_abs.sum())} elements beyond max(4 x {e_abs:.3e}, ulp), worst {d.max():.3e}'
    assert not bad_rel.any(), f'{what}: {int(bad_rel.sum())} elements beyond max(4 x {e_rel:.3e}, ulp / value) relatively, worst {obs[1]:.3e}'
    return obs

"""The dark-frame calibration of pnnp_amd/calibrate.py restated in int64 / float64 numpy: every definition of its docstrings, including
the float32 residual expression and the 1-D bilateral filter of row_denoise.  The tests compare the device path against this file; the
file itself is checked against closed forms in tests/test_host_calib.py.  Nothing here imports pnnp_amd."""
import numpy as np
from scipy import stats


def accumulate(frames):
    """uint16 [N,H,W] -> sum int64 [H,W], sumsq int64 [H,W], rowsum int64 [N,H,2]"""
    v = np.asarray(frames).astype(np.int64)
    N, H, W = v.shape
    return v.sum(axis=0), (v * v).sum(axis=0), v.reshape(N, H, W // 2, 2).sum(axis=2)


def dark_shading(s, N):
    return (s.astype(np.float64) / N).astype(np.float32)


def var_map(s, ss, N):
    return (N * ss - s * s).astype(np.float64) / (N * (N - 1))


def black_level_error(s, N, bl):
    H, W = s.shape
    planes = [s[0::2, 0::2], s[0::2, 1::2], s[1::2, 1::2], s[1::2, 0::2]]               # raw2bayer's order: R, G1, B, G2
    return np.array([p.sum() for p in planes], np.float64) / (float(N) * (H // 2) * (W // 2)) - float(bl)


def residual(frames, ds, rowoff32):
    """the float32 expression of the kernel: (float32(v) - ds) - rowoff, each subtraction rounded on its own"""
    v = np.asarray(frames).astype(np.float32)
    N, H, W = v.shape
    d = (v - np.asarray(ds, np.float32)[None]).astype(np.float32)
    off = np.repeat(np.asarray(rowoff32, np.float32)[:, :, None, :], W // 2, axis=2).reshape(N, H, W)
    return (d - off).astype(np.float32)


def probabilities(nq):
    return ((np.arange(nq, dtype=np.float64) + 0.5) / nq).astype(np.float32)


def quantiles(res, p32):
    """linear-interpolated order statistics in float32, torch.quantile's arithmetic: pos = p (n - 1), lo + (hi - lo) w"""
    import torch
    r = torch.from_numpy(np.ascontiguousarray(res).reshape(res.shape[0], -1))
    return torch.quantile(r, torch.from_numpy(p32), dim=1).t().numpy()


def slope(t, q):
    t0 = t - t.mean()
    return (q * t0).sum(axis=-1) / (t0 * t0).sum()


def corr(t, q):
    t0 = t - t.mean()
    q0 = q - q.mean(axis=-1, keepdims=True)
    return (q0 * t0).sum(axis=-1) / np.sqrt((t0 * t0).sum() * (q0 * q0).sum(axis=-1))


def spread(x):
    return float(np.std(x, ddof=1)) if len(x) > 1 else 0.0


def fit_dark(frames, K, wp, bl, nq=1000, lam_grid=None, darkshading=None, quantile_fn=quantiles):
    frames = np.asarray(frames)
    N, H, W = frames.shape
    s, ss, rowsum = accumulate(frames)
    if darkshading is None:
        ds, c = dark_shading(s, N), N / (N - 1)
        base = s.reshape(H, W // 2, 2).sum(axis=1).astype(np.float64) / (N * (W // 2))
    else:
        ds, c = np.asarray(darkshading, np.float32), 1.0
        base = ds.astype(np.float64).reshape(H, W // 2, 2).sum(axis=1) / (W // 2)
    rowoff = rowsum.astype(np.float64) / (W // 2) - base[None]
    res = residual(frames, ds, rowoff.astype(np.float32))
    r64 = res.reshape(N, -1).astype(np.float64)
    v_res = (r64 * r64).mean(axis=1) - r64.mean(axis=1) ** 2
    v_row = rowoff.reshape(N, -1).var(axis=1, ddof=1)
    m_f = rowoff.reshape(N, -1).mean(axis=1)
    p32 = probabilities(nq)
    q32 = quantile_fn(res, p32)
    q = q32.astype(np.float64)
    p = p32.astype(np.float64)
    lam_grid = np.linspace(-0.3, 0.3, 121) if lam_grid is None else np.asarray(lam_grid, np.float64)
    lam_corr = np.array([corr(stats.tukeylambda.ppf(p, lam), q).mean() for lam in lam_grid])
    lam = float(lam_grid[int(np.argmax(lam_corr))])
    sigGs_f = np.sqrt(c) * slope(stats.norm.ppf(p), q)
    sigTL_f = np.sqrt(c) * slope(stats.tukeylambda.ppf(p, lam), q)
    sigR_f = np.sqrt(np.maximum(c * v_row - c * v_res / (W // 2), 0.0))
    return {'Kmax': K, 'lam': lam, 'sigGs': float(sigGs_f.mean()), 'sigGssig': spread(sigGs_f), 'sigTL': float(sigTL_f.mean()),
            'sigTLsig': spread(sigTL_f), 'sigR': float(sigR_f.mean()), 'sigRsig': spread(sigR_f), 'bias': 0, 'biassig': spread(m_f),
            'q': 1.0 / (wp + 1), 'wp': wp, 'bl': bl, 'n_frames': N, 'darkshading': ds, 'black_level_error': black_level_error(s, N, bl),
            'sigGs_f': sigGs_f, 'sigTL_f': sigTL_f, 'sigR_f': sigR_f, 'm_f': m_f, 'v_res': v_res, 'v_row': v_row, 'quantiles': q,
            'quantiles32': q32, 'rowoff': rowoff, 'lam_corr': lam_corr, 'sum': s, 'sumsq': ss, 'rowsum': rowsum, 'residual': res}


def matching_sigGs(sigTL, lam, nq=1000):
    """the normal-scale value of a Tukey-lambda law: the slope of its quantiles on the normal quantiles at the fit's probabilities"""
    p = probabilities(nq).astype(np.float64)
    return float(sigTL * slope(stats.norm.ppf(p), stats.tukeylambda.ppf(p, lam)))


def planes_to_mosaics(z, wp, bl):
    """the sampler's normalised planes [N,4,h,w] -> uint16 mosaics [N,2h,2w]: float32 z * (wp - bl) + bl, rounded, through rggb2bayer
    (plane c lands on row parity c >> 1, column parity c & 1)"""
    dn = np.rint(np.asarray(z, np.float32) * np.float32(wp - bl) + np.float32(bl)).clip(0, 65535).astype(np.uint16)
    N, _, h, w = dn.shape
    return np.ascontiguousarray(dn.reshape(N, 2, 2, h, w).transpose(0, 3, 1, 4, 2).reshape(N, 2 * h, 2 * w))


def bilateral_1d(m, iso, d=25, sc=10.0):
    m = np.asarray(m, np.float64)
    n, r = m.size, d // 2
    ss = 1.0 + iso / 200.0
    out = np.empty(n)
    for i in range(n):
        num = den = 0.0
        for k in range(-r, r + 1):
            v = m[min(max(i + k, 0), n - 1)]
            w = np.exp(-(k * k) / (2.0 * ss * ss)) * np.exp(-((v - m[i]) ** 2) / (2.0 * sc * sc))
            num += w * v
            den += w
        out[i] = num / den
    return out


def row_denoise(data, iso):
    x = np.asarray(data, np.float32)
    H, W = x.shape
    rows = np.stack([x[0::2], x[1::2]]).astype(np.float64)                              # bayer2rows
    out = np.empty_like(rows)
    for i in range(2):
        m = rows[i].mean(axis=1)
        out[i] = rows[i] - (m - bilateral_1d(m, iso))[:, None]
    y = np.empty((H, W), np.float64)
    y[0::2], y[1::2] = out[0], out[1]                                                   # rows2bayer
    return y

"""The float64 restatement of the eval epilogue that csrc/evalmetrics.hip is tested against: tensor2im + PSNR / SSIM
(utils/visualization.py:9-31 -> scikit-image's structural_similarity(data_range=255, channel_axis=-1) by its published definition) and
IlluminanceCorrect (data_process/__init__.py:144-175), and the input families of tests/test_gpu_metrics.py, so that the host test
(tests/test_host_ssim_ref.py) and the device test draw identical data.

Everything here is plain numpy float64.  The 7x7 window sums are 49 shifted slices added up, no running sums and no filter: the one
float32 step is tensor2im's product ``x * 255`` (the kernel's first operation, and the reference's), after which the clipped values move
to float64.  ``oracle_ssim_map`` is the other yardstick: oracle/metrics_np.ssim's per-window value (float32 maps out of
scipy's uniform_filter), kept per window instead of averaged; its distance from ``ssim_map`` is what float32 costs on a window."""
import numpy as np

WIN = 7
K1, K2, DATA_RANGE = 0.01, 0.03, 255.0
C1, C2 = (K1 * DATA_RANGE) ** 2, (K2 * DATA_RANGE) ** 2
COV_NORM = WIN * WIN / (WIN * WIN - 1.0)                      # use_sample_covariance=True

PSNR_BAR, SSIM_BAR = 1e-3, 2e-5                               # the project's standing bars (dB, SSIM units)

# (level, noise sigma) of the per-window conditioning families: three bright and flat, one dark and noisy
FLAT_FAMILIES = ((0.95, 0.002), (0.98, 0.0005), (0.5, 0.005))
DARK_FAMILY = (0.2, 0.03)
N_DRAWS = 200

IMPULSE_SHAPE = (2, 40, 70)
IMPULSE_BACKGROUND, IMPULSE_STEP = 0.4, 0.2


def impulse_positions(H=IMPULSE_SHAPE[1], W=IMPULSE_SHAPE[2]):
    """both sides of every 32-tile seam, the halo depth, the first and last valid rows and columns"""
    return ((0, 0), (2, 2), (3, 3), (H - 1, W - 1), (H - 4, W - 4), (31, 31), (32, 32), (28, 35), (35, 28), (36, 66), (3, W - 4))


# ---- the reference

def tensor2im(t):
    """[..., H, W] tensor units -> float64 of clip(float32(t) * 255, 0, 255): the product is rounded to float32 like the kernel's (and
    the reference's), the clip is exact, nothing after it is float32.  A NaN stays a NaN (np.clip)."""
    with np.errstate(invalid='ignore'):
        return np.clip(np.asarray(t, np.float32) * np.float32(255.0), np.float32(0), np.float32(255)).astype(np.float64)


def _window_sum(f):
    H, W = f.shape
    s = np.zeros((H - WIN + 1, W - WIN + 1), np.float64)
    for u in range(WIN):
        for v in range(WIN):
            s += f[u:u + H - WIN + 1, v:v + W - WIN + 1]
    return s


def ssim_map(x, y):
    """one channel of x255 clipped data [H, W] -> the (H-6) x (W-6) SSIM map, one value per full 7x7 window"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    assert x.shape == y.shape and x.ndim == 2 and min(x.shape) >= WIN
    n = float(WIN * WIN)
    ux, uy = _window_sum(x) / n, _window_sum(y) / n
    vx = COV_NORM * (_window_sum(x * x) / n - ux * ux)
    vy = COV_NORM * (_window_sum(y * y) / n - uy * uy)
    vxy = COV_NORM * (_window_sum(x * y) / n - ux * uy)
    return ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))


def ssim_channels(a, b):
    """[C, H, W] in tensor units -> float64 [C]: each channel's mean over its window-valid region"""
    X, Y = tensor2im(a), tensor2im(b)
    assert X.ndim == 3 and X.shape == Y.shape
    return np.array([ssim_map(X[c], Y[c]).mean() for c in range(X.shape[0])])


def ssim(a, b):
    return float(ssim_channels(a, b).mean())


def psnr(a, b):
    """over all elements; +inf for equal images, NaN when a NaN is in"""
    X, Y = tensor2im(a), tensor2im(b)
    with np.errstate(divide='ignore'):
        return float(10.0 * np.log10(DATA_RANGE ** 2 / np.mean((X - Y) ** 2)))


def oracle_ssim_map(x, y):
    """oracle/metrics_np.ssim's value per window (same statements, float32 maps, cropped by 3), before its mean"""
    from scipy.ndimage import uniform_filter
    x, y = np.asarray(x).astype(np.float32), np.asarray(y).astype(np.float32)
    ux, uy = uniform_filter(x, size=WIN), uniform_filter(y, size=WIN)
    uxx, uyy, uxy = uniform_filter(x * x, size=WIN), uniform_filter(y * y, size=WIN), uniform_filter(x * y, size=WIN)
    vx, vy, vxy = COV_NORM * (uxx - ux * ux), COV_NORM * (uyy - uy * uy), COV_NORM * (uxy - ux * uy)
    s = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
    p = (WIN - 1) // 2
    return s[p:-p, p:-p]


def illuminance_correct(pred, src):
    """one image, any shape: <p,s>/<p,p> * p with p = clamp(pred, 0, 1), dots over src != 1; float64 throughout (0/0 -> NaN)"""
    pred, src = np.asarray(pred, np.float32), np.asarray(src, np.float32)
    with np.errstate(invalid='ignore', divide='ignore'):
        p = np.clip(pred, np.float32(0), np.float32(1)).astype(np.float64)
        m = src != np.float32(1)
        s = src.astype(np.float64)
        return (p[m] * s[m]).sum() / (p[m] * p[m]).sum() * p


# ---- input families (float32 numpy, tensor units; first the output, then the target)

def existing_family(shape, seed):
    """tests/test_gpu_metrics.py::test_psnr_ssim_vs_oracle's inputs: rand**2 and 0.03 noise on it, clamped to [-0.1, 1.1]"""
    import torch
    g = torch.Generator().manual_seed(seed)
    t = torch.rand(1, *shape, generator=g) ** 2
    o = (t + 0.03 * torch.randn(1, *shape, generator=g)).clamp(-0.1, 1.1)
    return o.numpy(), t.numpy()


def well_conditioned(C, H, W, seed=0):
    """rand**2 + 0.03 randn with another gain and offset per channel; both frames leave [0, 1] on either side, so the clip matters"""
    rng = np.random.default_rng([11, C, H, W, seed])
    gain = np.linspace(1.25, 0.7, C, dtype=np.float32).reshape(C, 1, 1) if C > 1 else np.float32(1.25)
    off = np.linspace(-0.08, 0.12, C, dtype=np.float32).reshape(C, 1, 1) if C > 1 else np.float32(-0.08)
    t = (rng.random((C, H, W), dtype=np.float32) ** 2 * gain + off).astype(np.float32)
    o = (t + np.float32(0.03) * rng.standard_normal((C, H, W), dtype=np.float32)).astype(np.float32)
    return o, t


def impulse(pos, channel=0):
    """a == b == 0.4 except one pixel of one channel of ``a``, raised by 0.2"""
    b = np.full(IMPULSE_SHAPE, IMPULSE_BACKGROUND, np.float32)
    a = b.copy()
    a[channel, pos[0], pos[1]] += np.float32(IMPULSE_STEP)
    return a, b


def flat_family(level, sigma, shape=(N_DRAWS, 1, 7, 7), seed=0):
    """target = level + 0.001 randn, output = target + sigma randn"""
    rng = np.random.default_rng([13, int(round(level * 1000)), int(round(sigma * 1e6)), seed])
    t = (np.float32(level) + np.float32(0.001) * rng.standard_normal(shape, dtype=np.float32)).astype(np.float32)
    o = (t + np.float32(sigma) * rng.standard_normal(shape, dtype=np.float32)).astype(np.float32)
    return o, t


def window_errors(o, t):
    """[n, 1, 7, 7] pairs -> (float64 SSIM of each window [n], the oracle's value of each window [n])"""
    O, T = tensor2im(o), tensor2im(t)
    ref = np.array([ssim_map(T[i, 0], O[i, 0])[0, 0] for i in range(len(O))])
    orc = np.array([float(oracle_ssim_map(T[i, 0], O[i, 0])[0, 0]) for i in range(len(O))])
    return ref, orc


def illum_inputs(shape, seed=0, ones=0.3):
    """pred uniform in [-0.2, 1.3], src uniform in [0, 1) with a share ``ones`` of it set to exactly 1.0"""
    rng = np.random.default_rng([17, int(np.prod(shape)), seed])
    pred = (rng.random(shape, dtype=np.float32) * np.float32(1.5) - np.float32(0.2)).astype(np.float32)
    src = rng.random(shape, dtype=np.float32)
    src[rng.random(shape) < ones] = np.float32(1.0)
    return pred, src

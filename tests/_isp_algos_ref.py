"""The numpy restatement of the classical raw filters (csrc/isp_algos.hip): the definitions of include/pnnp_hip.h that stand in for the
OpenCV calls of the reference's utils/isp_algos.py and of bayer2gray / repair_bad_pixels in utils/isp_ops.py.  The first part has cv2's
names and call shapes (``boxFilter``, ``blur``, ``resize``, ``filter2D``, ``medianBlur`` and the border constants) so that
tests/golden/make_golden_isp_algos.py can hand it to the real functions as their ``cv2``; the second part restates those functions
themselves.  Everything works in the dtype of its input: float32 in -> float32 out with float64 sums, float64 in -> float64 throughout.

    box mean   d x d, d odd, anchor at the centre; the d^2 values summed in float64, times the float64 constant 1.0 / (d d), rounded once
    resize     0.5x: the 2 x 2 block's mean, f(f(x00 + x01) 0.25 + f(x10 + x11) 0.25); 2x: INTER_LINEAR, coordinate (x + 0.5) / 2 - 0.5, weights
               0.75 / 0.25 and 0 for a neighbour outside, horizontal pass first, each pass s0 (1 - w) + s1 w
    filter2D   the 3 x 3 kernel's nine float64 products summed in row-major order, rounded once
    median     3 x 3, BORDER_REPLICATE

All return numpy arrays."""
import numpy as np

BORDER_REPLICATE, BORDER_REFLECT, BORDER_REFLECT_101, BORDER_DEFAULT = 1, 2, 4, 4
INTER_LINEAR = 1
MAX_D = 51
_PAD = {BORDER_REPLICATE: 'edge', BORDER_REFLECT: 'symmetric', BORDER_REFLECT_101: 'reflect'}
GRAY_KERNEL = np.array([[1, 2, 1], [2, 4, 2], [1, 2, 1]], np.float32) / 16.


def _float2d(x):
    x = np.asarray(x)
    assert x.ndim == 2 and x.dtype in (np.float32, np.float64), (x.shape, x.dtype)
    return x


def box_mean(x, d, border=BORDER_REFLECT_101, separable=False):
    """[H,W] float32 / float64 -> the same dtype.  ``separable``: row sums first, then the column sums of those (the kernel's order);
    otherwise the window's d^2 values in row-major order."""
    x = _float2d(x)
    H, W = x.shape
    assert d % 2 == 1 and 1 <= d <= MAX_D, d
    r = d // 2
    if border == BORDER_REFLECT_101:
        assert r < min(H, W), 'REFLECT_101 needs d // 2 < min(H, W)'
    xp = np.pad(x.astype(np.float64), r, mode=_PAD[border]) if r else x.astype(np.float64)
    if separable:
        rows = xp[:, 0:W].copy()
        for k in range(1, d):
            rows += xp[:, k:k + W]
        acc = rows[0:H].copy()
        for k in range(1, d):
            acc += rows[k:k + H]
    else:
        acc = None
        for dy in range(d):
            for dx in range(d):
                t = xp[dy:dy + H, dx:dx + W]
                acc = t.copy() if acc is None else acc + t
    return (acc * (1.0 / (d * d))).astype(x.dtype)


def resize_half(x):
    x = _float2d(x)
    assert x.shape[0] % 2 == 0 and x.shape[1] % 2 == 0, x.shape
    q = x.dtype.type(0.25)                    # cv2's two passes, (x00 0.5 + x01 0.5) 0.5 + (x10 0.5 + x11 0.5) 0.5, round the same way
    return (x[0::2, 0::2] + x[0::2, 1::2]) * q + (x[1::2, 0::2] + x[1::2, 1::2]) * q


def _up_axis(n):
    """the 2x upsampling of a line of n samples: (index of s0, index of s1, weight of s1) per output sample"""
    X = np.arange(2 * n)
    i0 = np.where(X % 2 == 1, X // 2, X // 2 - 1)
    w1 = np.where(X % 2 == 1, 0.25, 0.75)
    low, high = i0 < 0, i0 >= n - 1
    i0 = np.where(low, 0, np.where(high, n - 1, i0))
    w1 = np.where(low | high, 0.0, w1)
    return i0, np.minimum(i0 + 1, n - 1), w1


def resize_double(x):
    x = _float2d(x)
    t = x.dtype.type
    h, w = x.shape
    xa, xb, wx = _up_axis(w)
    wx = wx.astype(x.dtype)[None, :]
    hz = x[:, xa] * (t(1) - wx) + x[:, xb] * wx
    ya, yb, wy = _up_axis(h)
    wy = wy.astype(x.dtype)[:, None]
    return hz[ya] * (t(1) - wy) + hz[yb] * wy


# ---------------------------------------------------------------------------- cv2's call shapes
def boxFilter(src, ddepth, ksize, borderType=BORDER_DEFAULT):
    assert ddepth == -1 and ksize[0] == ksize[1]
    return box_mean(src, ksize[0], borderType)


def blur(src, ksize):
    return boxFilter(src, -1, ksize)


def resize(src, dsize, fx=None, fy=None, interpolation=INTER_LINEAR):
    assert dsize is None and fx == fy and fx in (0.5, 2) and interpolation == INTER_LINEAR
    return resize_half(src) if fx == 0.5 else resize_double(src)


def filter2D(src, ddepth, kernel, borderType=BORDER_DEFAULT):
    src = _float2d(src)
    kernel = np.asarray(kernel)
    assert ddepth == -1 and kernel.shape == (3, 3)
    H, W = src.shape
    xp = np.pad(src.astype(np.float64), 1, mode=_PAD[borderType])
    acc = None
    for dy in range(3):
        for dx in range(3):
            t = xp[dy:dy + H, dx:dx + W] * np.float64(kernel[dy, dx])
            acc = t if acc is None else acc + t
    return acc.astype(src.dtype)


def medianBlur(src, ksize):
    src = np.asarray(src)
    assert ksize == 3 and src.ndim == 2 and src.dtype in (np.uint16, np.float32)
    H, W = src.shape
    xp = np.pad(src, 1, mode='edge')
    stack = np.stack([xp[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)])
    return np.sort(stack, axis=0)[4]


# ---------------------------------------------------------------------------- the reference's functions, restated
def _const(x, v):
    """a Python scalar as numpy takes it beside an array of x's dtype"""
    return np.asarray(x).dtype.type(v)


def VST(x, sigma, mu=0, gain=1.0, wp=1):
    x = np.asarray(x)
    y = _const(x, gain) * x + _const(x, (gain ** 2) * 3.0 / 8.0) + _const(x, sigma ** 2) - _const(x, gain * mu)
    y = np.sqrt(np.maximum(y, np.zeros_like(y)))
    y = y / _const(x, wp)
    return _const(x, 2.0 / gain) * y


def inverse_VST(x, sigma, gain=1.0, wp=1):
    x = np.asarray(x)
    x = x * _const(x, wp)
    h = x / _const(x, 2.0)
    y = h * h - _const(x, 3.0 / 8.0) - _const(x, sigma ** 2 / gain ** 2)
    return (y * _const(x, gain)) / _const(x, wp)


def stdfilt(img, k=5, separable=False):
    img = _float2d(img)
    m = box_mean(img, k, BORDER_REFLECT_101, separable)
    m2 = box_mean(img * img, k, BORDER_REFLECT_101, separable)
    return np.sqrt(np.maximum(m2 - m * m, 0))


def guided_ab(p, I, d, eps, border, separable=False):
    mu_p, mu_I = box_mean(p, d, border, separable), box_mean(I, d, border, separable)
    II, Ip = box_mean(I * I, d, border, separable), box_mean(I * p, d, border, separable)
    var = II - mu_I * mu_I
    cov = Ip - mu_I * mu_p
    a = cov / (var + _const(p, eps))
    return a, mu_p - a * mu_I


def GuidedFilter(p, I, d=7, eps=1, separable=False):
    p, I = _float2d(p), _float2d(I)
    a, b = guided_ab(p, I, d, eps, BORDER_REPLICATE, separable)
    return box_mean(a, d, BORDER_REPLICATE, separable) * I + box_mean(b, d, BORDER_REPLICATE, separable)


def FastGuidedFilter(p, I, d=7, eps=1, separable=False):
    p, I = _float2d(p), _float2d(I)
    a, b = guided_ab(resize_half(p), resize_half(I), d, eps, BORDER_REFLECT_101, separable)
    mu_a = resize_double(box_mean(a, d, BORDER_REFLECT_101, separable))
    mu_b = resize_double(box_mean(b, d, BORDER_REFLECT_101, separable))
    return mu_a * I + mu_b


def bayer2gray(raw):
    return filter2D(raw, -1, GRAY_KERNEL, borderType=BORDER_REFLECT)


def repair_bad_pixels(raw, bad_points):
    """in place, as the reference: every listed pixel takes the 3 x 3 median of its colour plane in the unmodified frame"""
    raw = np.asarray(raw)
    H, W = raw.shape
    fixed = np.empty_like(raw)
    for py in range(2):
        for px in range(2):
            fixed[py::2, px::2] = medianBlur(np.ascontiguousarray(raw[py::2, px::2]), 3)
    for y, x in bad_points:
        assert 0 <= y < H and 0 <= x < W
        raw[y, x] = fixed[y, x]
    return raw

"""The reference's classical raw toolbox (utils/isp_algos.py) with its names and signatures, on the device: csrc/isp_algos.hip.

    VST, inverse_VST              the generalised Anscombe transform for Poisson-Gaussian raw with gain K and read noise sigma
    stdfilt                       a local noise-level map
    GuidedFilter, FastGuidedFilter
    Blur1D                        torch ops, not on the path
    vst_denoise                   an extension: VST -> GuidedFilter -> inverse_VST, the non-learned baseline denoiser
    row_denoise                   the row-banding clean-up of a dark-shading map (pnnp_amd/calibrate.py, csrc/calib.hip)

Device tensors in, device tensors out, nothing synchronises.  The image functions take ``[H,W]`` or ``[H,W,C]`` (the reference's layout,
the default) or, with ``layout='chw'``, ``[..., H, W]``: every plane is filtered on its own.  float32 runs on the kernels; a float64
input runs as float64 torch ops (not on the path: there so that a float64 caller gets float64 arithmetic, as the reference gives it).

The OpenCV calls of the reference are replaced by the definitions in include/pnnp_hip.h (box sums in float64, rounded once): parity with
an OpenCV build is not a goal.  Deviations: the window ``d`` is odd and at most 51; ``VST`` keeps the reference's quirks (``wp`` only
divides, ``inverse_VST`` does not add ``mu`` back); ``row_denoise`` takes a loaded map only (its ``path`` is not read) and filters the row
means with the 1-D bilateral filter that include/pnnp_hip.h defines, the stand-in for cv2.bilateralFilter; ``AlgoDebugger`` (a GUI) has
no counterpart.
"""
import ctypes as C

import torch
import torch.nn.functional as F

from . import _lib
from ._lib import PnnpError

MAX_D = 51
_REFLECT_101, _HALF = 0x1, 0x2


def _entry(name):
    try:
        return getattr(_lib.lib(), name)
    except AttributeError:
        raise PnnpError(f'{_lib.LIB_PATH} has no {name}: an older build of the library; rebuild it') from None


def _check_window(d, what):
    if int(d) != d or d < 1 or d % 2 == 0:
        raise PnnpError(f'{what}: the window must be odd, got {d} (an even window has no centre; the reference\'s anchor rule is not implemented)')
    if d > MAX_D:
        raise PnnpError(f'{what}: the window is at most {MAX_D}, got {d}')
    return int(d)


def _check_float(what, *tensors):
    for t in tensors:
        if not torch.is_tensor(t) or t.dtype not in (torch.float32, torch.float64):
            raise PnnpError(f'{what}: expected float32 (the kernels) or float64 (torch ops) tensors, got {getattr(t, "dtype", type(t))}')
    if len({t.dtype for t in tensors}) != 1 or len({tuple(t.shape) for t in tensors}) != 1:
        raise PnnpError(f'{what}: the images must agree in dtype and shape')


def _geometry(x, layout, what):
    """-> (N, H, W, strides (plane, row, pixel) of the CONTIGUOUS tensor of that shape)"""
    if layout not in ('hwc', 'chw'):
        raise PnnpError(f"{what}: layout must be 'hwc' or 'chw', got {layout!r}")
    if x.dim() == 2:
        H, W = x.shape
        return 1, H, W, (H * W, W, 1)
    if layout == 'hwc':
        if x.dim() != 3:
            raise PnnpError(f"{what}: expected [H,W] or [H,W,C] (layout='chw': [...,H,W]), got {tuple(x.shape)}")
        H, W, Cn = x.shape
        return Cn, H, W, (1, W * Cn, Cn)
    H, W = x.shape[-2:]
    return x.numel() // (H * W) if H * W else 0, H, W, (H * W, W, 1)


def _check_size(N, H, W, d, reflect, half, what):
    if N < 1 or H < 1 or W < 1:
        raise PnnpError(f'{what}: empty image')
    if N > 65535:
        raise PnnpError(f'{what}: at most 65535 planes per call, got {N}')
    if half and (H % 2 or W % 2):
        raise PnnpError(f'{what}: the half-resolution filter needs even sides, got {H}x{W}')
    h, w = (H // 2, W // 2) if half else (H, W)
    if reflect and d // 2 >= min(h, w):
        raise PnnpError(f'{what}: the REFLECT_101 border needs d // 2 < min(H, W) = {min(h, w)}' + (' at half resolution' if half else '') + f', got d = {d}')


def _i64x3(s):
    return (C.c_int64 * 3)(*s)


# ---------------------------------------------------------------------------- float64: torch ops, not on the path
def _planes4(x, layout):
    """-> [1,N,H,W] view for the torch-op path, and the function that brings a result back to x's shape"""
    if x.dim() == 2:
        return x[None, None], lambda y: y[0, 0]
    if layout == 'hwc':
        return x.permute(2, 0, 1)[None], lambda y: y[0].permute(1, 2, 0)
    H, W = x.shape[-2:]
    return x.reshape(1, -1, H, W), lambda y: y.reshape(x.shape)


def _box_torch(x4, d, mode):
    r = d // 2
    return F.avg_pool2d(F.pad(x4, (r, r, r, r), mode=mode) if r else x4, d, stride=1)


def _guided_torch(p4, I4, d, eps, fast):
    if fast:
        full, p4, I4 = I4, F.interpolate(p4, scale_factor=0.5, mode='bilinear', align_corners=False), \
            F.interpolate(I4, scale_factor=0.5, mode='bilinear', align_corners=False)
    mode = 'reflect' if fast else 'replicate'
    mu_p, mu_I = _box_torch(p4, d, mode), _box_torch(I4, d, mode)
    var = _box_torch(I4 * I4, d, mode) - mu_I * mu_I
    cov = _box_torch(I4 * p4, d, mode) - mu_I * mu_p
    a = cov / (var + eps)
    b = mu_p - a * mu_I
    mu_a, mu_b = _box_torch(a, d, mode), _box_torch(b, d, mode)
    if fast:
        mu_a = F.interpolate(mu_a, scale_factor=2, mode='bilinear', align_corners=False)
        mu_b = F.interpolate(mu_b, scale_factor=2, mode='bilinear', align_corners=False)
        I4 = full
    return mu_a * I4 + mu_b


# ---------------------------------------------------------------------------- the kernels
def _vst_launch(x, inverse, sigma, mu, gain, wp, scale=None, group=1):
    out = torch.empty_like(x)
    if x.numel():
        _lib.check(_entry('pnnp_vst_f32')(_lib.ptr(x), C.c_int64(x.numel()), int(inverse), C.c_double(float(sigma)), C.c_double(float(mu)),
                                          C.c_double(float(gain)), C.c_double(float(wp)), _lib.ptr(scale), C.c_int64(group), _lib.ptr(out),
                                          _lib.stream()), 'vst')
    return out


def _check_vst(x, gain, wp, what):
    if not torch.is_tensor(x) or x.dtype not in (torch.float32, torch.float64):
        raise PnnpError(f'{what}: expected a float32 or float64 tensor, got {getattr(x, "dtype", type(x))}')
    if gain == 0 or wp == 0:
        raise PnnpError(f'{what}: gain and wp must not be 0')
    _lib.require_cuda(x)


def VST(x, sigma, mu=0, gain=1.0, wp=1):
    """utils/isp_algos.py:4-10: (2 / gain) * sqrt(max(gain x + gain^2 3/8 + sigma^2 - gain mu, 0)) / wp in the reference's operand order; its
    first line ``y = x * wp`` is dead code, so ``wp`` only divides.  Any shape; float32 on the kernel, float64 as torch ops."""
    _check_vst(x, gain, wp, 'VST')
    if x.dtype == torch.float64:
        y = gain * x + (gain ** 2) * 3.0 / 8.0 + sigma ** 2 - gain * mu
        return (2.0 / gain) * (torch.sqrt(torch.maximum(y, torch.zeros_like(y))) / wp)
    return _vst_launch(x.contiguous(), 0, sigma, mu, gain, wp)


def inverse_VST(x, sigma, gain=1.0, wp=1):
    """utils/isp_algos.py:13-18: ((x wp / 2)^2 - 3/8 - sigma^2 / gain^2) gain / wp; ``mu`` is not added back, as in the reference."""
    _check_vst(x, gain, wp, 'inverse_VST')
    if x.dtype == torch.float64:
        y = (x * wp / 2.0) ** 2 - 3.0 / 8.0 - sigma ** 2 / gain ** 2
        return y * gain / wp
    return _vst_launch(x.contiguous(), 1, sigma, 0.0, gain, wp)


def stdfilt(img, k=5, layout='hwc'):
    """utils/isp_algos.py:21-29: sqrt(max(blur(img^2) - blur(img)^2, 0)) with a k x k box (border REFLECT_101), per plane."""
    k = _check_window(k, 'stdfilt')
    _check_float('stdfilt', img)
    N, H, W, strides = _geometry(img, layout, 'stdfilt')
    _check_size(N, H, W, k, True, False, 'stdfilt')
    _lib.require_cuda(img)
    if img.dtype == torch.float64:
        x4, back = _planes4(img, layout)
        m = _box_torch(x4, k, 'reflect')
        return back(torch.sqrt(torch.clamp_min(_box_torch(x4 * x4, k, 'reflect') - m * m, 0)))
    x = img.contiguous()
    out = torch.empty_like(x)
    s = _i64x3(strides)
    _lib.check(_entry('pnnp_stdfilt_f32')(_lib.ptr(x), N, H, W, s, k, _lib.ptr(out), s, _lib.stream()), 'stdfilt')
    return out


def _guided(p, I, d, eps, layout, fast, what):
    d = _check_window(d, what)
    _check_float(what, p, I)
    N, H, W, strides = _geometry(p, layout, what)
    _check_size(N, H, W, d, fast, fast, what)
    _lib.require_cuda(p, I)
    if p.dtype == torch.float64:
        p4, back = _planes4(p, layout)
        return back(_guided_torch(p4, _planes4(I, layout)[0], d, eps, fast))
    same = p is I or (p.data_ptr() == I.data_ptr() and p.stride() == I.stride())
    pc = p.contiguous()
    Ic = pc if same else I.contiguous()
    flags = (_REFLECT_101 | _HALF) if fast else 0
    h, w = (H // 2, W // 2) if fast else (H, W)
    ab = torch.empty((2, N, h, w), dtype=torch.float32, device=p.device)
    ws = torch.empty((2, N, h, w), dtype=torch.float32, device=p.device) if fast else None
    out = torch.empty_like(pc)
    s = _i64x3(strides)
    _lib.check(_entry('pnnp_guided_ab_f32')(_lib.ptr(pc), _lib.ptr(Ic), N, H, W, s, d, C.c_float(float(eps)), flags, _lib.ptr(ab[0]),
                                            _lib.ptr(ab[1]), _lib.stream()), what + ' (a, b)')
    _lib.check(_entry('pnnp_guided_apply_f32')(_lib.ptr(ab[0]), _lib.ptr(ab[1]), _lib.ptr(Ic), N, H, W, s, d, flags, _lib.ptr(ws), _lib.ptr(out),
                                               s, _lib.stream()), what + ' (apply)')
    return out


def GuidedFilter(p, I, d=7, eps=1, layout='hwc'):
    """utils/isp_algos.py:64-82: the guided filter of ``p`` with guide ``I``, d x d box means with border REPLICATE: two launches
    (a = cov / (var + eps), b = mu_p - a mu_I; then box(a) I + box(b)).  ``p is I`` skips the duplicate means, bitwise the same."""
    return _guided(p, I, d, eps, layout, False, 'GuidedFilter')


def FastGuidedFilter(p, I, d=7, eps=1, layout='hwc'):
    """utils/isp_algos.py:42-62: a and b at half resolution (0.5x bilinear resize, border REFLECT_101), their means upsampled by 2
    (INTER_LINEAR) before box(a) I + box(b).  H and W must be even."""
    return _guided(p, I, d, eps, layout, True, 'FastGuidedFilter')


def Blur1D(data, c=0.5, log=True):
    """utils/isp_algos.py:31-40 as torch ops (not on the path): a [c, (1-c)/2] three-tap blur of a 1-D tensor's interior, in log2 when
    ``log``.  Returns a new tensor; note that the reference, with ``log=False``, writes into its argument."""
    t = torch.log2(data) if log else data.clone()
    src = t.clone()
    t[1:-1] = src[1:-1] * c + (src[:-2] + src[2:]) * (1 - c) / 2
    return 2 ** t if log else t


def vst_denoise(x, gain, sigma, d=7, eps=1.0, scale=1.0, layout='chw'):
    """The non-learned baseline: ``inverse_VST(GuidedFilter(v, v, d, eps), sigma, gain) / scale`` with ``v = VST(x * scale, sigma, 0, gain)``,
    bit-equal to that composition of the public functions (``x * scale`` a float32 product, ``/ scale`` a float32 division by a tensor).
    In the VST domain the noise has unit variance, which is why the reference's eps = 1 is the natural default.  ``scale``: a float, or a
    tensor [B] with one value per leading index of ``x`` (layout 'chw', ``x`` [B, ..., H, W]); it brings ``x`` to the DN scale in which
    ``gain`` and ``sigma`` are given.  Four launches: the product and the division ride on the two VST launches."""
    _check_float('vst_denoise', x)
    _check_vst(x, gain, 1, 'vst_denoise')
    if x.dtype == torch.float64:
        s = scale.to(x).reshape((-1,) + (1,) * (x.dim() - 1)) if torch.is_tensor(scale) else torch.tensor(float(scale), dtype=x.dtype, device=x.device)
        v = VST(x * s, sigma, 0, gain)
        return inverse_VST(GuidedFilter(v, v, d, eps, layout=layout), sigma, gain) / s
    xc = x.contiguous()
    if torch.is_tensor(scale) and scale.numel() > 1:
        if layout != 'chw' or x.dim() < 3 or scale.numel() != x.shape[0]:
            raise PnnpError(f"vst_denoise: a scale tensor has one value per leading index of a layout='chw' batch, got {tuple(scale.shape)} for {tuple(x.shape)}")
        st, group = scale.to(device=x.device, dtype=torch.float32).reshape(-1).contiguous(), xc.numel() // x.shape[0]
    else:
        st = scale.to(device=x.device, dtype=torch.float32).reshape(1) if torch.is_tensor(scale) else torch.full((1,), float(scale), dtype=torch.float32, device=x.device)
        group = max(xc.numel(), 1)
    v = _vst_launch(xc, 0, sigma, 0.0, gain, 1, st, group)
    g = GuidedFilter(v, v, d, eps, layout=layout)
    return _vst_launch(g, 1, sigma, 0.0, gain, 1, st, group)


def row_denoise(path, iso, data=None):
    """utils/isp_algos.py:84-99 with the reference's signature: ``calibrate.row_denoise(data, iso)``.  ``data`` is required: the
    reference's ``dataload(path)`` is not mirrored, so ``path`` is never read."""
    if data is None:
        raise PnnpError('row_denoise: pass the map as data= (a float32 [H,W] tensor or array); files are not read here')
    from . import calibrate
    return calibrate.row_denoise(data, iso)

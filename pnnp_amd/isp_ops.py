"""Bayer pack / unpack with the reference's names and signatures, executed by the
HIP kernels in csrc/pack.hip (bit-exact with the reference).

Mirrors utils/isp_ops.py:57-112 of the reference.  Inputs may be numpy arrays
(like the reference's DataLoader workers pass) or CUDA tensors; numpy inputs are
staged to the GPU, processed there and returned as numpy, CUDA tensors stay on the
device.  There is no CPU implementation here.

``FastISP`` / ``SimpleISP`` (utils/isp_ops.py:125-158) and ``demosaic_ea`` are the full-resolution render, csrc/demosaic.hip.
``bayer2gray`` and ``repair_bad_pixels`` (utils/isp_ops.py:70-74, 115-123) run on csrc/isp_algos.hip.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib

_NP2T = {np.dtype('uint16'): torch.uint16, np.dtype('float32'): torch.float32, np.dtype('float64'): torch.float64,
         np.dtype('int16'): torch.int16, np.dtype('int32'): torch.int32, np.dtype('uint8'): torch.uint8,
         np.dtype('int64'): torch.int64}


def _to_dev(a):
    """-> (cuda tensor, was_numpy)."""
    if torch.is_tensor(a):
        if a.is_cuda:
            return a.contiguous(), False
        return a.contiguous().cuda(), True
    a = np.ascontiguousarray(a)
    if a.dtype not in _NP2T:
        raise TypeError(f'unsupported dtype {a.dtype}')
    return torch.from_numpy(a).cuda(), True


def _ret(t, was_host):
    return t.cpu().numpy() if was_host else t


def raw2bayer(raw, wp=1023, bl=64, norm=True, clip=False, bias=np.array([0, 0, 0, 0])):
    """utils/isp_ops.py:84-96: [H,W] (or batched [B,H,W]) u16/f32 -> f32 [4,H/2,W/2]
    ([B,4,H/2,W/2]), planes R,G1,B,G2; (x-(bias+bl))/(wp-(bias+bl)) in float64."""
    x, host = _to_dev(raw)
    if x.dtype not in (torch.uint16, torch.float32):
        x = x.to(torch.float32)          # reference: raw.astype(np.float32)
    batched = x.dim() == 3
    if not batched:
        x = x[None]
    B, H, W = x.shape
    out = torch.empty((B, 4, H // 2, W // 2), dtype=torch.float32, device=x.device)
    black = (C.c_double * 4)(*[float(b) + float(bl) for b in np.broadcast_to(np.asarray(bias, np.float64).reshape(-1), (4,))])
    fn = _lib.lib().pnnp_pack_bayer_u16 if x.dtype == torch.uint16 else _lib.lib().pnnp_pack_bayer_f32
    _lib.check(fn(_lib.ptr(x), B, H, W, C.c_int64(W), C.c_int64(H * W), _lib.ptr(out), black,
                  C.c_double(float(wp)), int(bool(norm)), int(bool(clip)), _lib.stream()), 'pack_bayer')
    if not batched:
        out = out[0]
    return _ret(out, host)


def bayer2raw(packed_raw, wp=16383, bl=512, device_out=False):
    """utils/isp_ops.py:98-112: f32 [4,h,w] / [1,4,h,w] -> u16 [2h,2w].  Like the
    reference the result is a numpy array unless ``device_out``."""
    x, _ = _to_dev(packed_raw.detach() if torch.is_tensor(packed_raw) else packed_raw)
    x = x.float()
    if x.dim() == 4:
        x = x[0].contiguous()
    _, h, w = x.shape
    out = torch.empty((2 * h, 2 * w), dtype=torch.uint16, device=x.device)
    _lib.check(_lib.lib().pnnp_unpack_bayer_u16(_lib.ptr(x), 1, h, w, _lib.ptr(out), int(wp), int(bl), _lib.stream()),
               'unpack_bayer')
    return out if device_out else out.cpu().numpy()


def _move(fn_name, a, out_shape):
    x, host = _to_dev(a)
    out = torch.empty(out_shape, dtype=x.dtype, device=x.device)
    return x, out, host, getattr(_lib.lib(), fn_name)


def bayer2rggb(bayer):
    """utils/isp_ops.py:57-59: [H,W] -> [H/2,W/2,4] in order (0,0),(0,1),(1,0),(1,1)."""
    H, W = bayer.shape
    x, out, host, fn = _move('pnnp_bayer_to_rggb', bayer, (H // 2, W // 2, 4))
    _lib.check(fn(_lib.ptr(x), _lib.ptr(out), H, W, x.element_size(), _lib.stream()), 'bayer2rggb')
    return _ret(out, host)


def rggb2bayer(rggb):
    """utils/isp_ops.py:61-63."""
    h, w, _ = rggb.shape
    x, out, host, fn = _move('pnnp_rggb_to_bayer', rggb, (2 * h, 2 * w))
    _lib.check(fn(_lib.ptr(x), _lib.ptr(out), h, w, x.element_size(), _lib.stream()), 'rggb2bayer')
    return _ret(out, host)


def bayer2rows(bayer):
    """utils/isp_ops.py:65-68: [H,W] -> [2,H/2,W]."""
    H, W = bayer.shape
    x, out, host, fn = _move('pnnp_bayer_to_rows', bayer, (2, H // 2, W))
    _lib.check(fn(_lib.ptr(x), _lib.ptr(out), H, W, x.element_size(), _lib.stream()), 'bayer2rows')
    return _ret(out, host)


def rows2bayer(rows):
    """utils/isp_ops.py:76-81: [2,h,W] -> float64 [2h,W] (np.empty default dtype)."""
    _, h, W = rows.shape
    if not torch.is_tensor(rows):
        rows = np.asarray(rows, np.float64)
    x, host = _to_dev(rows)
    x = x.to(torch.float64)
    out = torch.empty((2 * h, W), dtype=torch.float64, device=x.device)
    _lib.check(_lib.lib().pnnp_rows_to_bayer(_lib.ptr(x), _lib.ptr(out), h, W, 8, _lib.stream()), 'rows2bayer')
    return _ret(out, host)


# ---------------------------------------------------------------------------- full-resolution render (csrc/demosaic.hip)
def demosaic_ea(mosaic_u16, out=None):
    """The edge-aware RGGB demosaic that include/pnnp_hip.h defines (the stand-in for cv2.cvtColor(COLOR_BAYER_BG2RGB_EA); parity with an
    OpenCV build is not a goal): uint16 [H,W] or [B,H,W], H and W even and at least 4, numpy or a tensor -> uint16 [..,H,W,3] in R, G, B
    order; numpy in -> numpy out.  ``out``: a contiguous uint16 device tensor of the result's shape to write into."""
    x, host = _to_dev(mosaic_u16)
    if x.dtype != torch.uint16 or x.dim() not in (2, 3):
        raise _lib.PnnpError(f'demosaic_ea: expected uint16 [H,W] or [B,H,W], got {x.dtype} {tuple(x.shape)}')
    batched = x.dim() == 3
    x3 = x if batched else x[None]
    B, H, W = x3.shape
    if H < 4 or W < 4 or H % 2 or W % 2:
        raise _lib.PnnpError(f'demosaic_ea: a Bayer frame has even sides of at least 4, got {H}x{W}')
    shape = (B, H, W, 3) if batched else (H, W, 3)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint16, device=x.device)
    elif not torch.is_tensor(out) or not out.is_cuda or out.dtype != torch.uint16 or tuple(out.shape) != shape or not out.is_contiguous():
        raise _lib.PnnpError(f'demosaic_ea: out must be a contiguous uint16 device tensor {shape}')
    try:
        entry = _lib.lib().pnnp_demosaic_ea_u16
    except AttributeError:
        raise _lib.PnnpError(f'{_lib.LIB_PATH} has no pnnp_demosaic_ea_u16: an older build of the library; rebuild it') from None
    _lib.check(entry(_lib.ptr(x3), B, H, W, _lib.ptr(out), _lib.stream()), 'demosaic_ea')
    return _ret(out, host)


def FastISP(img4c, wb=None, ccm=None, gamma=2.2, device_out=False, u8=False, bgr=False):
    """utils/isp_ops.py:134-158 in one kernel: packed [4,h,w] (planes R, G1, B, G2; numpy, staged through the GPU, or a tensor) -> the
    full-resolution sRGB picture [2h,2w,3], numpy unless ``device_out``.  wb: the gains wb[0] and wb[2] are taken as float32 (None: 2
    and 2); ccm: [3,3], rounded to float32 and widened (None: the reference's float64 Sony matrix, exactly).  ``u8=True`` returns
    floor(255 v) as uint8 instead (``bgr=True``: in B, G, R order).
    Deviations: the result is float32 (float32 of the float64 value; the reference returns float64); a NaN renders as 0; the demosaic is
    the one include/pnnp_hip.h defines, not OpenCV's; only gamma 2.2 has a kernel, another value raises PnnpError('unsupported ...')."""
    from . import process
    process._check_gamma(gamma)
    x, _ = _to_dev(img4c.detach() if torch.is_tensor(img4c) else img4c)
    if x.dim() != 3 or x.shape[0] != 4:
        raise _lib.PnnpError(f'FastISP: expected packed raw [4,h,w], got {tuple(x.shape)}')
    if wb is None:
        gains = [2.0, 1.0, 2.0, 1.0]
    else:
        g = torch.as_tensor(wb).detach().to(torch.float32).reshape(-1)
        gains = torch.stack([g[0], torch.ones_like(g[0]), g[2], torch.ones_like(g[0])])
    rows = process.isp_rows(gains, torch.eye(3) if ccm is None else ccm, 1, x.device)
    out_f, out_b = process.fastisp_render(x[None], rows, f32=not u8, u8=u8, bgr=bgr, default_ccm=ccm is None)
    out = out_b[0] if u8 else out_f[0].permute(1, 2, 0)
    return out if device_out else out.cpu().numpy()


def SimpleISP(raw, bl=512, wp=16383, wb=[2, 1, 1, 2], gamma=2.2, device_out=False):
    """utils/isp_ops.py:125-132 as torch ops on the device (not a kernel, not on the path: here so the module is complete): [h,w,4]
    RGGB -> float64 [h,w,3] = clip((float32(raw) - bl) / (wp - bl) * wb, 0, 1)[..., (0, 1, 3)] ** (1 / gamma); numpy unless ``device_out``."""
    x, _ = _to_dev(raw.detach() if torch.is_tensor(raw) else raw)
    # (a division by a host scalar would run as a multiplication by its reciprocal: divide by a device value, as numpy divides)
    v = (x.to(torch.float32) - bl) / torch.tensor(float(wp - bl), dtype=torch.float32, device=x.device)
    g =torch.as_tensor(np.asarray(wb, np.float64), device=x.device)
    v = (v.to(torch.float64) * g.reshape(1, 1, -1)).clamp(0, 1)[:, :, (0, 1, 3)] ** (1 / gamma)
    return v if device_out else v.cpu().numpy()


# ---------------------------------------------------------------------------- the OpenCV-backed helpers (csrc/isp_algos.hip)
def bayer2gray(raw):
    """utils/isp_ops.py:70-74: the bilinear Bayer-to-gray filter, [1 2 1; 2 4 2; 1 2 1] / 16 with BORDER_REFLECT, on a float32 mosaic [H,W]
    (or a batch [B,H,W]): nine exact float64 products, their sum rounded once (include/pnnp_hip.h defines it; parity with an OpenCV build
    is not a goal).  A uint16 mosaic is refused (OpenCV would return a saturated uint16 image: convert first).  numpy in -> numpy out."""
    if getattr(raw, 'dtype', None) not in (torch.float32, np.dtype('float32')):
        raise _lib.PnnpError(f'bayer2gray: expected a float32 mosaic, got {getattr(raw, "dtype", type(raw))}')
    if raw.ndim not in (2, 3) or 0 in tuple(raw.shape):
        raise _lib.PnnpError(f'bayer2gray: expected [H,W] or [B,H,W], got {tuple(raw.shape)}')
    x, host = _to_dev(raw)
    B = x.shape[0] if x.dim() == 3 else 1
    out = torch.empty_like(x)
    try:
        entry = _lib.lib().pnnp_bayer2gray_f32
    except AttributeError:
        raise _lib.PnnpError(f'{_lib.LIB_PATH} has no pnnp_bayer2gray_f32: an older build of the library; rebuild it') from None
    _lib.check(entry(_lib.ptr(x), B, x.shape[-2], x.shape[-1], _lib.ptr(out), _lib.stream()), 'bayer2gray')
    return _ret(out, host)


def repair_bad_pixels(raw, bad_points, method='median'):
    """utils/isp_ops.py:115-123: every listed pixel of the mosaic ``raw`` [H,W] (uint16 or float32, H and W even; a CONTIGUOUS device
    tensor) takes the 3 x 3 median of its own colour plane (REPLICATE at the plane's border), every median from the unmodified frame.
    In place, and returns ``raw``, as the reference does.  ``bad_points``: a sequence of (row, col), or an int tensor [n,2]; duplicates
    are allowed, an empty list is a no-op, a point outside the frame raises before anything is launched (a device tensor of points is
    read back for that check: the one synchronisation here; a host list costs none).  ``method`` is ignored, as in the reference.  A NaN in a float32 neighbourhood is not supported (the median
    is then unspecified)."""
    if not torch.is_tensor(raw) or raw.dtype not in (torch.uint16, torch.float32) or raw.dim() != 2:
        raise _lib.PnnpError(f'repair_bad_pixels: expected a uint16 or float32 tensor [H,W], got {getattr(raw, "dtype", type(raw))} '
                             f'{tuple(getattr(raw, "shape", ()))}')
    H, W = raw.shape
    if H < 2 or W < 2 or H % 2 or W % 2:
        raise _lib.PnnpError(f'repair_bad_pixels: a Bayer frame has even sides, got {H}x{W}')
    if not raw.is_contiguous():
        raise _lib.PnnpError('repair_bad_pixels works in place: the frame must be contiguous')
    pts = bad_points.detach() if torch.is_tensor(bad_points) else torch.as_tensor(np.asarray(bad_points, np.int64).reshape(-1, 2))
    if pts.dim() != 2 or pts.shape[1] != 2 or pts.dtype not in (torch.int32, torch.int64, torch.int16, torch.uint8):
        raise _lib.PnnpError(f'repair_bad_pixels: bad_points must be integer points [n,2], got {pts.dtype} {tuple(pts.shape)}')
    n = pts.shape[0]
    if n == 0:
        return raw
    host = pts.cpu()
    if int(host[:, 0].min()) < 0 or int(host[:, 0].max()) >= H or int(host[:, 1].min()) < 0 or int(host[:, 1].max()) >= W:
        raise _lib.PnnpError(f'repair_bad_pixels: a point lies outside the {H}x{W} frame')
    _lib.require_cuda(raw)
    pd = pts.to(device=raw.device, dtype=torch.int32).contiguous()
    tmp = torch.empty((n,), dtype=raw.dtype, device=raw.device)
    try:
        entry = _lib.lib().pnnp_repair_bad_pixels
    except AttributeError:
        raise _lib.PnnpError(f'{_lib.LIB_PATH} has no pnnp_repair_bad_pixels: an older build of the library; rebuild it') from None
    _lib.check(entry(_lib.ptr(raw), raw.element_size(), H, W, _lib.ptr(pd), n, _lib.ptr(tmp), _lib.stream()), 'repair_bad_pixels')
    return raw

"""sRGB -> realistic raw on the device: the reference's data_process/unprocess.py under its own names.

``unprocess`` (unprocess.py:170-217) turns an ordinary RGB image into clean linear camera RGB -- inverse tone curve, gamma expansion,
RGB -> camera matrix, inverted white balance and brightening with the highlight mask, clamp -- and ``mosaic`` / ``mosaic_GBRG`` (:123-167)
gather the Bayer planes.  The reference's datasets run them per crop on DataLoader workers to make training targets without a raw dataset
(``Img_Dataset``, syn_datasets.py:207-282).  Here the arithmetic and the gather are ONE kernel (csrc/unprocess.hip): ``unprocess_batch``
reads a batch of float32 or uint8 images and writes the un-mosaicked RGB and / or the packed raw [B,4,H/2,W/2] the train step takes as
``hr`` (``HipTrainStep.step_rgb``).  The host draws (``random_ccm``, ``random_gains``) are the reference's, in its order, from its RNGs.

``inverse_smoothstep``, ``gamma_expansion``, ``apply_ccm`` and ``safe_invert_gains`` are the reference's lines as torch ops on device
tensors, ``mosaic`` / ``mosaic_GBRG`` strided device gathers: not on the path (``unprocess`` and ``step_rgb`` run the kernel), here so the
reference's imports resolve and as an on-device composition to compare and time the kernel against.

Deviations: uint8 input (taken as v / 255; the reference has none); the tone curve keeps its accuracy below x ~ 6e-8, where the reference's
cancels to the 1e-8 floor (csrc/unprocess.hip); no CPU path.  ``Img_Dataset`` itself is NOT mirrored, it cannot run in the reference:
``default_args`` raises, its .h5 "is not packed yet", it indexes the list ``metadata`` as a dictionary (:257) and applies the channel-last
arithmetic to channel-first crops.  The functions are the contract, not the class.  ``random_noise_levels`` / ``add_noise`` (:220-242) are
left out: nothing in the reference calls them.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .augment import random_gains  # noqa: F401  (unprocess.py:60-77; re-exported under the reference module's name)

UNP_NPARAM = 16                                # PNNP_UNP_NPARAM: rgb2cam[9] row-major, gains[3], 4 unused
UNP_IN_HWC_F32, UNP_IN_CHW_F32, UNP_IN_HWC_U8 = 0, 1, 2
UNP_F_GBRG = 0x1

CCMS = {'SonyA7S2': [[1., 0., 0.], [0., 1., 0.], [0., 0., 1.]],                       # unprocess.py:33-42: the inverses of the cameras' matrices
        'IMX686': [[0.61093086, 0.31565922, 0.07340994], [0.09433191, 0.7658969, 0.1397712], [0.03532438, 0.3020709, 0.6626047]]}


def random_ccm(camera_type='IMX686'):
    """unprocess.py:7-46: the RGB -> camera matrix of the camera, float32 [3,3] on the host (nothing is random in the reference either).
    An unknown camera raises KeyError (the reference fails there on an unbound name)."""
    return torch.FloatTensor(CCMS[camera_type])


def inverse_smoothstep(image):
    """unprocess.py:79-85 as torch ops on a device tensor (not on the path)."""
    _lib.require_cuda(image)
    image = torch.clamp(image, min=0.0, max=1.0)
    return 0.5 - torch.sin(torch.asin(1.0 - 2.0 * image) / 3.0)


def gamma_expansion(image):
    """unprocess.py:88-94 as torch ops on a device tensor (not on the path)."""
    _lib.require_cuda(image)
    return torch.clamp(image, min=1e-8) ** 2.2


def apply_ccm(image, ccm):
    """unprocess.py:97-103 as torch ops on device tensors (not on the path): [...,3] times ccm [3,3] over the last axes."""
    _lib.require_cuda(image, ccm)
    shape = image.size()
    return torch.reshape(torch.tensordot(torch.reshape(image, [-1, 3]), ccm, dims=[[-1], [-1]]), shape)


def safe_invert_gains(image, rgb_gain, red_gain, blue_gain, use_gpu=True):
    """unprocess.py:106-121 as torch ops on device tensors (not on the path).  ``use_gpu`` is accepted for the signature: the tensors
    are on the device here whatever it says."""
    _lib.require_cuda(image, rgb_gain, red_gain, blue_gain)
    green = torch.tensor([1.0], device=image.device)
    gains = (torch.stack((1.0 / red_gain, green, 1.0 / blue_gain)) / rgb_gain).view(1, 1, 3)
    gray = torch.mean(image, dim=-1, keepdim=True)
    inflection = 0.9
    mask = (torch.clamp(gray - inflection, min=0.0) / (1.0 - inflection)) ** 2.0
    return image * torch.max(mask + (1.0 - mask) * gains, gains)


def _check_mosaic(image, what):
    if not torch.is_tensor(image) or image.dim() < 3 or image.shape[-1] != 3:
        raise _lib.PnnpError(f'{what}: expected a tensor [...,H,W,3], got {tuple(image.shape) if hasattr(image, "shape") else type(image)}')
    if image.shape[-3] % 2 or image.shape[-2] % 2:
        raise _lib.PnnpError(f'{what}: H and W must be even, got {image.shape[-3]}x{image.shape[-2]}')
    _lib.require_cuda(image)


def mosaic(image):
    """unprocess.py:123-144: [...,H,W,3] on the device -> [...,H/2,W/2,4], planes R, Gr, B, Gb channel-LAST as the reference returns them
    (its ``image.size() == 3`` compares a Size with an int, so every input takes its second branch).  Strided device gathers of the
    input's own bits; ``unprocess_batch(packed='RGGB')`` writes the same planes channel-first from inside the kernel."""
    _check_mosaic(image, 'mosaic')
    return torch.stack((image[..., 0::2, 0::2, 0], image[..., 0::2, 1::2, 1], image[..., 1::2, 1::2, 2], image[..., 1::2, 0::2, 1]), dim=-1)


def mosaic_GBRG(image):
    """unprocess.py:146-167: as ``mosaic`` for a GBRG sensor; the plane order is the reference's R, Gr, Gb, B (it differs from mosaic's)."""
    _check_mosaic(image, 'mosaic_GBRG')
    return torch.stack((image[..., 1::2, 0::2, 0], image[..., 1::2, 1::2, 1], image[..., 0::2, 0::2, 1], image[..., 0::2, 1::2, 2]), dim=-1)


def unprocess_draw(lock_wb=False, camera_type='IMX686'):
    """The host part of ``unprocess`` (unprocess.py:173-176), in the reference's order: the camera's matrix, its inverse, then the
    brightening gain from the torch RNG and the red gain from the numpy RNG (``random_gains``), or ``lock_wb=([rgb], [red], [blue])``
    taken as given (no draw).  -> (rgb2cam, cam2rgb, rgb_gain, red_gain, blue_gain), float32 host tensors of shapes [3,3], [3,3], [1] x 3."""
    rgb2cam = random_ccm(camera_type)
    cam2rgb = torch.inverse(rgb2cam)
    rgb_gain, red_gain, blue_gain = random_gains(camera_type) if lock_wb is False else torch.FloatTensor(np.array(lock_wb))
    return rgb2cam, cam2rgb, rgb_gain, red_gain, blue_gain


def _host_f32(v):
    return (v.detach().cpu() if torch.is_tensor(v) else torch.as_tensor(np.asarray(v))).to(torch.float32)


def unprocess_rows(rgb2cams, rgb_gains, red_gains, blue_gains, n, device='cuda'):
    """The parameter table of the kernel, f32 [n][UNP_NPARAM] on ``device``: rgb2cams [3,3] (shared) or [n,3,3]; the three gains [1]
    (shared) or [n] each.  The gains column is formed on the HOST with the reference's own float32 tensor ops
    (``torch.stack((1 / red, 1, 1 / blue)) / rgb_gain``, unprocess.py:111), so its bits are the reference's.  Device tensors are brought to
    the host first (a synchronisation): draw on the host, as ``unprocess_draw`` does."""
    m = _host_f32(rgb2cams).reshape(-1)
    g = [_host_f32(v).reshape(-1) for v in (rgb_gains, red_gains, blue_gains)]
    if m.numel() not in (9, 9 * n) or any(v.numel() not in (1, n) for v in g):
        raise _lib.PnnpError(f'unprocess rows: rgb2cams must hold 9 or {n}x9 entries and every gain 1 or {n}, got {m.numel()} and '
                             f'{[v.numel() for v in g]}')
    rgb_gain, red_gain, blue_gain = [v.expand(n) for v in g]
    gains = torch.stack((1.0 / red_gain, torch.ones(n), 1.0 / blue_gain)) / rgb_gain           # [3,n]
    rows = torch.zeros((n, UNP_NPARAM), dtype=torch.float32)
    rows[:, :9] = m.reshape(-1, 9)
    rows[:, 9:12] = gains.t()
    return rows.to(device, non_blocking=True)


def _check_batch(images, layout, packed):
    """-> (in_kind, B, H, W); raises before anything touches a device"""
    if layout not in ('hwc', 'chw'):
        raise _lib.PnnpError(f"unprocess: layout must be 'hwc' or 'chw', got {layout!r}")
    if packed not in (None, 'RGGB', 'GBRG'):
        raise _lib.PnnpError(f"unprocess: packed must be None, 'RGGB' or 'GBRG', got {packed!r}")
    if not torch.is_tensor(images) or images.dim() != 4 or images.shape[-1 if layout == 'hwc' else 1] != 3:
        want = '[B,H,W,3]' if layout == 'hwc' else '[B,3,H,W]'
        raise _lib.PnnpError(f'unprocess: expected a tensor {want}, got {tuple(images.shape) if hasattr(images, "shape") else type(images)}')
    if images.dtype == torch.uint8 and layout != 'hwc':
        raise _lib.PnnpError('unprocess: uint8 images are channel-last [B,H,W,3]')
    B, H, W = (images.shape[0], images.shape[1], images.shape[2]) if layout == 'hwc' else (images.shape[0], images.shape[2], images.shape[3])
    if B < 1 or H < 1 or W < 1:
        raise _lib.PnnpError(f'unprocess: empty batch {tuple(images.shape)}')
    if packed is not None and (H % 2 or W % 2):
        raise _lib.PnnpError(f'unprocess: a packed output needs even H and W, got {H}x{W}')
    kind = UNP_IN_HWC_U8 if images.dtype == torch.uint8 else (UNP_IN_HWC_F32 if layout == 'hwc' else UNP_IN_CHW_F32)
    return kind, B, H, W


def unprocess_batch(images, rows, layout='hwc', rgb=True, packed=None):
    """One launch of csrc/unprocess.hip over a batch on the device: images float32 [B,H,W,3] (``layout='hwc'``, the reference's) or
    [B,3,H,W] ('chw'), or uint8 [B,H,W,3] taken as v / 255 (an extension); rows from ``unprocess_rows``, one per image.
    -> (float32 RGB in the input's layout or None, packed raw float32 [B,4,H/2,W/2] or None): ``rgb`` asks for the first, ``packed`` =
    'RGGB' (``mosaic``: planes R, Gr, B, Gb, the order of ``isp_ops.raw2bayer``) or 'GBRG' (``mosaic_GBRG``: R, Gr, Gb, B) for the second.
    A non-contiguous input, or one of another float type, is copied first; the input is never written."""
    kind, B, H, W = _check_batch(images, layout, packed)
    if not rgb and packed is None:
        raise _lib.PnnpError('unprocess: no output asked for')
    _lib.require_cuda(images, rows)
    if not torch.is_tensor(rows) or rows.dtype != torch.float32 or tuple(rows.shape) != (B, UNP_NPARAM) or not rows.is_contiguous():
        raise _lib.PnnpError(f'unprocess: rows must be contiguous float32 [{B},{UNP_NPARAM}] (unprocess.unprocess_rows)')
    x = images.detach().contiguous()
    if kind != UNP_IN_HWC_U8:
        x = x.float()
    out_rgb = torch.empty(x.shape, dtype=torch.float32, device=x.device) if rgb else None
    out_packed = torch.empty((B, 4, H // 2, W // 2), dtype=torch.float32, device=x.device) if packed is not None else None
    try:
        entry = _lib.lib().pnnp_unprocess_f32
    except AttributeError:
        raise _lib.PnnpError(f'{_lib.LIB_PATH} has no pnnp_unprocess_f32: an older build of the library; rebuild it') from None
    flags = UNP_F_GBRG if packed == 'GBRG' else 0
    _lib.check(entry(_lib.ptr(x), kind, B, H, W, _lib.ptr(rows), C.c_uint(flags), _lib.ptr(out_rgb), _lib.ptr(out_packed), _lib.stream()), 'unprocess')
    return out_rgb, out_packed


def _check_image(image):
    if not torch.is_tensor(image) or image.dim() not in (3, 4, 5) or image.shape[-1] != 3:
        raise _lib.PnnpError(f'unprocess: expected a tensor [H,W,3], [N,H,W,3] or [crops,t,H,W,3], got '
                             f'{tuple(image.shape) if hasattr(image, "shape") else type(image)}')


def unprocess(image, lock_wb=False, use_gpu=False, camera_type='IMX686'):
    """unprocess.py:170-217: an sRGB image [H,W,3], or a stack [N,H,W,3] / [crops,t,H,W,3] that shares ONE draw (the reference's
    ``len(image.size()) >= 4`` branch), -> (the unprocessed image, float32, same shape; metadata), metadata = cam2rgb, rgb_gain, red_gain,
    blue_gain as in the reference.  ``lock_wb=([1.], [red], [blue])`` fixes the gains (no draw).  A CUDA tensor in gives a CUDA tensor
    out; a CPU tensor is moved to the device and back (as ``process.raw2rgb_v2`` stages numpy): there is no CPU path.  ``use_gpu`` puts
    the metadata on the device, as in the reference.  uint8 images are taken as v / 255 (an extension).  No mosaic: the reference leaves
    it to the caller (:209); ``unprocess_batch(packed=)`` does both in one launch."""
    _check_image(image)
    rgb2cam, cam2rgb, rgb_gain, red_gain, blue_gain = unprocess_draw(lock_wb, camera_type)
    x = image.detach()
    dev = x.device if x.is_cuda else torch.device('cuda')
    x = x.to(dev)
    flat = x.reshape((-1,) + tuple(x.shape[-3:]))
    rows = unprocess_rows(rgb2cam, rgb_gain, red_gain, blue_gain, 1, dev).expand(flat.shape[0], UNP_NPARAM).contiguous()
    out = unprocess_batch(flat, rows, layout='hwc', rgb=True)[0].reshape(image.shape)
    if not image.is_cuda:
        out = out.cpu()
    if use_gpu:
        cam2rgb, rgb_gain, red_gain, blue_gain = cam2rgb.to(dev), rgb_gain.to(dev), red_gain.to(dev), blue_gain.to(dev)
    return out, {'cam2rgb': cam2rgb, 'rgb_gain': rgb_gain, 'red_gain': red_gain, 'blue_gain': blue_gain}

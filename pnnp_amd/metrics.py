"""Eval-side epilogue on the device (reference: trainer_SID.py:230-248): IlluminanceCorrect and the
raw-domain PSNR / SSIM, without leaving the GPU; and the score of a noise model (trainer_NF_SID.py:163-174):
the integer-DN histogram KL divergence ``kl_div_norm`` (utils/kld_div.py:163-200) and the std mismatch."""
import ctypes as C

import numpy as np
import torch

from . import _lib


class IlluminanceCorrect(torch.nn.Module):
    """data_process/__init__.py:144-175 (ELD's brightness alignment): per image,
    out = <p,s>/<p,p> * p with p = clamp(predict,0,1), dots over source != 1."""

    def forward(self, predict, source):
        _lib.require_cuda(predict, source)
        if predict.numel() == 0:                         # (an empty batch would skip the loop below and return without a word)
            raise _lib.PnnpError(f'illuminance_correct: empty prediction {tuple(predict.shape)}')
        predict = predict.contiguous().float(); source = source.contiguous().float()
        out = torch.empty_like(predict)
        ws = torch.empty(512, dtype=torch.float64, device=predict.device)
        n_img = predict.shape[0]
        for i in range(n_img):
            s = source[i] if source.shape[0] != 1 else source[0]
            _lib.check(_lib.lib().pnnp_illuminance_correct_f32(_lib.ptr(predict[i]), _lib.ptr(s), _lib.ptr(out[i]),
                                                               C.c_int64(predict[i].numel()), _lib.ptr(ws), _lib.stream()),
                       'illuminance_correct')
        return out

    def correct(self, predict, source):
        assert predict.shape[0] == 1
        return self.forward(predict, source)


def quality_assess(output, target):
    """PSNR / SSIM of two [1,C,H,W] (or [C,H,W]) tensors in [0,1], as
    quality_assess(tensor2im(output), tensor2im(target), data_range=255) (utils/visualization.py:9-31).
    Returns a device tensor [psnr, ssim] (no sync)."""
    _lib.require_cuda(output, target)
    a = output[0] if output.dim() == 4 else output
    b = target[0] if target.dim() == 4 else target
    a = a.contiguous().float(); b = b.contiguous().float()
    Cc, H, W = a.shape
    ws = torch.empty(2 * Cc * ((H + 31) // 32) * ((W + 31) // 32), dtype=torch.float64, device=a.device)
    out = torch.empty(2, dtype=torch.float32, device=a.device)
    # the reference passes (Y=target, X=output): image_true = target
    _lib.check(_lib.lib().pnnp_psnr_ssim_f32(_lib.ptr(b), _lib.ptr(a), _lib.ptr(out), Cc, H, W, _lib.ptr(ws), _lib.stream()),
               'psnr_ssim')
    return out


# ---- score of a noise model (csrc/noise_score.hip)
MAX_WP = 16383                   # PNNP_NOISE_SCORE_MAX_WP
_SCORE_ROW = 8                   # PNNP_NOISE_SCORE_ROW
_lut_host, _lut_dev, _edges_dev = {}, {}, {}


def _kld_edges(wp):
    """kl_div_norm's bin edges (utils/kld_div.py:180-183 with left_edge = 0, right_edge = 1, n_bins = wp), float64."""
    bw = (1.0 - 0.0) / wp
    return np.arange(0.0, 1.0 + bw, bw)


def _kld_bin_lut(wp):
    """int32 [wp + 1]: the bin np.histogram(., _kld_edges(wp)) counts the clipped DN value k in, after the reference's
    ``norm`` (float32(k) / float32(wp), utils/kld_div.py:5-11); -1 where it counts it in no bin.  np.histogram's rule for given
    edges: half-open bins found with searchsorted, the last bin closed, a value beyond the last edge dropped.  This is not the
    identity: the float32 quotient and the float64 edge k / wp round differently (at wp = 16383, 8703 of 16384 values land in
    another bin than k; from k = 1024 upwards bins alternately receive two values and none).  It depends on wp alone."""
    wp = int(wp)
    if wp not in _lut_host:
        edges = _kld_edges(wp)
        v = (np.arange(wp + 1, dtype=np.float32) / np.float32(wp)).astype(np.float64)
        nb = len(edges) - 1
        b = np.searchsorted(edges, v, side='right') - 1
        b[v == edges[-1]] = nb - 1
        b[(v > edges[-1]) | (v < edges[0])] = -1
        _lut_host[wp] = b.astype(np.int32)
    return _lut_host[wp]


def _score_tables(wp, bl, device):
    key = (int(wp), device)
    if key not in _lut_dev:
        _lut_dev[key] = torch.from_numpy(_kld_bin_lut(wp)).to(device)
    ekey = (int(wp), float(bl), device)
    if ekey not in _edges_dev:
        _edges_dev[ekey] = torch.from_numpy(_kld_edges(int(wp)) * wp - bl).to(device)      # 'hist_p': (y_p, bin_edges*wp-bl)
    return _lut_dev[key], _edges_dev[ekey]


def _score_check(bl, wp, *tensors):
    if bl is None:
        raise _lib.PnnpError('kl_div_norm(bl=None) -- the reference\'s branch with data-dependent edges and no rounding -- is not provided '
                             '(the device score is the integer-DN one the trainers log)')
    _lib.require_cuda(*tensors)
    for t in tensors:
        if t.dtype != torch.float32:
            raise _lib.PnnpError(f'the noise-model score takes float32 tensors, got {t.dtype}')
    if int(wp) != wp or not 1 <= wp <= MAX_WP:
        raise _lib.PnnpError(f'kl_div_norm: wp = {wp}, this build counts integer white points 1 .. {MAX_WP}')


def _score_lib():
    L = _lib.lib()
    if L.pnnp_noise_score_ws_bytes.restype is not C.c_int64:
        L.pnnp_noise_score_ws_bytes.restype = C.c_int64
    return L


def _score_run(entry, arrays, B, n, extra, bl, wp):
    L = _score_lib()
    dev = arrays[0].device
    lut, edges = _score_tables(wp, bl, dev)
    nbins = edges.numel() - 1
    ws_bytes = int(L.pnnp_noise_score_ws_bytes(B, C.c_int64(n)))
    if ws_bytes < 0:
        _lib.check(ws_bytes, entry)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    hist = torch.empty(B, 2, nbins, dtype=torch.float64, device=dev)
    res = torch.empty(B, _SCORE_ROW, dtype=torch.float64, device=dev)
    _lib.check(getattr(L, entry)(*[_lib.ptr(a) for a in arrays], B, C.c_int64(n), *extra, C.c_float(bl), int(wp), _lib.ptr(lut), nbins,
                                 _lib.ptr(ws), _lib.ptr(hist), _lib.ptr(res), _lib.stream()), entry)
    return hist, res, edges.clone()                          # the caller's own copy: the cached tensor stays as it is


def _crops(t, per_crop):
    t = t.contiguous()
    return (t.shape[0], t.numel() // t.shape[0]) if per_crop else (1, t.numel())


def kl_div_norm(p_data, q_data, bl=512, wp=16383, per_crop=False):
    """utils/kld_div.py:163-200 on the device: forward, inverse and symmetric KL divergence of the integer-DN histograms of two
    float32 CUDA tensors of DN values.  Returns the reference's dict -- ``kl_fwd``, ``kl_inv``, ``kl_sym``, ``hist_p`` and
    ``hist_q`` = (y, bin_edges * wp - bl) -- as float64 device tensors: 0-dim and [nbins], or [B] and [B, nbins] with
    ``per_crop=True`` (one score per leading index of [B, ...] inputs).  No host synchronisation.

    The reference's quirks are kept: its float edges (``_kld_bin_lut``), the shift by ``bl`` only when ``min(p) < 0`` under numpy's
    NaN-propagating min, ``n`` counting NaNs.  One is dropped: the caller's tensors are not modified (the reference adds ``bl``
    into its arguments)."""
    _score_check(bl, wp, p_data, q_data)
    if p_data.shape != q_data.shape or p_data.numel() == 0 or (per_crop and p_data.dim() < 1):
        raise _lib.PnnpError(f'kl_div_norm: p {tuple(p_data.shape)} and q {tuple(q_data.shape)} must be equal, non-empty shapes')
    p, q = p_data.contiguous(), q_data.contiguous()
    B, n = _crops(p, per_crop)
    hist, res, edges = _score_run('pnnp_kl_div_norm_f32', (p, q), B, n, (), float(bl), int(wp))
    if not per_crop:
        hist, res = hist[0], res[0]
    return {'kl_fwd': res[..., 0], 'kl_inv': res[..., 1], 'kl_sym': res[..., 2],
            'hist_p': (hist[..., 0, :], edges), 'hist_q': (hist[..., 1, :], edges)}


def noise_model_score(clean, real, sampled_noise, bl, wp, per_crop=False):
    """trainer_NF_SID.py:165-172 in one call: ``clean`` (imgs_hr), ``real`` (imgs_lr) and ``sampled_noise`` (net.sample(...) * ratio),
    float32 CUDA tensors [B, C, H, W]; ``bl`` / ``wp``: the data set's black and white level (the DN scale wp - bl).  The histogram
    itself uses kl_div_norm's own defaults (512, 16383) whatever the camera, like the reference's call.  Scores crop 0 only, like the
    reference, unless ``per_crop=True``.  Returns float64 device tensors ``kl_int`` (= kl_fwd), ``kl_inv``, ``kl_sym``, ``gt_std``,
    ``out_std``, ``diff_p`` (0-dim, or [B]) and kl_div_norm's ``hist_p`` / ``hist_q``; no host synchronisation (``score_log_line`` is the one place that reads them)."""
    _score_check(512, 16383, clean, real, sampled_noise)
    if not (clean.shape == real.shape == sampled_noise.shape) or clean.dim() < 2 or clean.numel() == 0:
        raise _lib.PnnpError(f'noise_model_score: clean {tuple(clean.shape)}, real {tuple(real.shape)} and sampled_noise '
                             f'{tuple(sampled_noise.shape)} must be equal [B, ...] shapes')
    if not per_crop:
        clean, real, sampled_noise = clean[:1], real[:1], sampled_noise[:1]
    arrays = tuple(t.contiguous() for t in (clean, real, sampled_noise))
    B, n = _crops(arrays[0], True)
    s = float(np.float32(wp - bl))
    hist, res, edges = _score_run('pnnp_noise_score_f32', arrays, B, n, (C.c_float(s),), 512.0, 16383)
    if not per_crop:
        hist, res = hist[0], res[0]
    return {'kl_int': res[..., 0], 'kl_inv': res[..., 1], 'kl_sym': res[..., 2],
            'gt_std': res[..., 3], 'out_std': res[..., 4], 'diff_p': res[..., 5],
            'hist_p': (hist[..., 0, :], edges), 'hist_q': (hist[..., 1, :], edges)}


def score_log_line(res):
    """The reference's log text (trainer_NF_SID.py:173) of a ``noise_model_score`` result (crop 0 of a per-crop one).  Synchronises."""
    kl, out_std, gt_std, diff_p = (float(res[k].reshape(-1)[0]) for k in ('kl_int', 'out_std', 'gt_std', 'diff_p'))
    return f"kl_int:{kl:.6f}, std:{out_std:.3f} vs {gt_std:.3f} ({diff_p:.2f}%)"

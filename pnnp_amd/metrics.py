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


# ---- histogram KL over caller-given float edges (csrc/hist_kl.hip): the rest of utils/kld_div.py
MAX_BINS = 16384                 # PNNP_HIST_EDGES_MAX_BINS
_const_dev = {}


def _dev_const(arr, device):
    """A host array's device copy, cached per content (edges and bin centres are few and repeat from call to call; a data-dependent
    table such as kl_div_range's pushes the oldest entry out)."""
    key = (arr.dtype.str, arr.tobytes(), device)
    t = _const_dev.get(key)
    if t is None:
        if len(_const_dev) >= 64:
            _const_dev.pop(next(iter(_const_dev)))
        t = _const_dev[key] = torch.from_numpy(np.ascontiguousarray(arr)).to(device)
    return t


def noise_flow_edges():
    """The bin edges of the Noise Flow line of work's marginal KL: 100 bins of 0.002 on [-0.1, 0.1] and a catch-all bin on either side."""
    return np.concatenate(([-1000.0], np.arange(-0.1, 0.1 + 1e-9, 0.2 / 100), [1000.0]))


def _edges_of(bin_edges, left_edge, right_edge, n_bins):
    """(the caller's edges as given or the reference's arange, float64 edges [nb + 1], bin width, hint): validated on the host.  numpy raises
    ValueError for edges that decrease or hold a NaN; here every bad table is a PnnpError before any launch."""
    bw = (right_edge - left_edge) / n_bins                                  # get_histogram: from these three even when bin_edges is given
    hinted = bin_edges is None
    if hinted:
        bin_edges = np.arange(left_edge, right_edge + bw, bw)
    elif isinstance(bin_edges, torch.Tensor):
        bin_edges = bin_edges.detach().cpu().numpy()                        # (a tensor of edges costs one copy to the host: they are checked there)
    given = np.asarray(bin_edges)
    if given.ndim != 1 or given.size < 2 or given.dtype.kind not in 'fiu':
        raise _lib.PnnpError(f'bin_edges must be a 1-D array of at least 2 numbers, got shape {given.shape} {given.dtype}')
    e = np.ascontiguousarray(given, dtype=np.float64)
    if e.size - 1 > MAX_BINS:
        raise _lib.PnnpError(f'bin_edges: {e.size - 1} bins, this build counts at most {MAX_BINS}')
    if not np.isfinite(e).all():
        raise _lib.PnnpError('bin_edges must be finite (a NaN or an inf among them)')
    if (np.diff(e) < 0).any():
        raise _lib.PnnpError('bin_edges must increase monotonically (equal neighbours are allowed)')
    span = e[-1] - e[0]
    hint = (float(e[0]), float((e.size - 1) / span)) if hinted and span > 0 and np.isfinite(span) and np.isfinite((e.size - 1) / span) else (0.0, 0.0)
    return given, e, bw, hint


def _hist_lib():
    L = _lib.lib()
    if L.pnnp_hist_edges_ws_bytes.restype is not C.c_int64:
        L.pnnp_hist_edges_ws_bytes.restype = C.c_int64
    return L


def _sample_sets(what, per_crop, *tensors):
    _lib.require_cuda(*tensors)
    dt = tensors[0].dtype
    for t in tensors:
        if t.dtype not in (torch.float32, torch.float64) or t.dtype != dt:
            raise _lib.PnnpError(f'{what} takes float32 or float64 tensors of one dtype, got {[str(x.dtype) for x in tensors]}')
        if t.numel() == 0 or (per_crop and (t.dim() < 1 or t.shape[0] != tensors[0].shape[0])):
            raise _lib.PnnpError(f'{what}: non-empty sample sets, with per_crop of one leading size: got {[tuple(x.shape) for x in tensors]}')
    return [t.detach().contiguous() for t in tensors]


def _hist_run(what, p, q, e, hint, per_crop):
    """The count and finishing passes: (hist [B, 2, nb] and kl [B, 3]) of two sample sets, (hist [B, nb], None) of one."""
    L = _hist_lib()
    dev = p.device
    B = p.shape[0] if per_crop else 1
    nb = e.size - 1
    edges = _dev_const(e, dev)
    ws_bytes = int(L.pnnp_hist_edges_ws_bytes(B, nb))
    if ws_bytes < 0:
        _lib.check(ws_bytes, what)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    hist = torch.empty((B, nb) if q is None else (B, 2, nb), dtype=torch.float64, device=dev)
    kl = None if q is None else torch.empty(B, 3, dtype=torch.float64, device=dev)
    _lib.check(L.pnnp_hist_edges_f64(_lib.ptr(p), _lib.ptr(q), int(p.dtype == torch.float64), B, C.c_int64(p.numel() // B),
                                     C.c_int64(0 if q is None else q.numel() // B), _lib.ptr(edges), nb, C.c_double(hint[0]), C.c_double(hint[1]),
                                     _lib.ptr(ws), _lib.ptr(hist), _lib.ptr(kl), _lib.stream()), what)
    return hist, kl


def get_histogram(data, bin_edges=None, left_edge=0.0, right_edge=1.0, n_bins=1000, per_crop=False):
    """utils/kld_div.py:202-210 on the device: ``(hist, bin_centers)`` of a float32 or float64 CUDA tensor of any shape -- np.histogram's
    counts over ``bin_edges`` (a numpy array, a list or a tensor; by default ``np.arange(left_edge, right_edge + bw, bw)``, built on the host)
    divided by ``data.numel()``, and ``bin_edges[:-1] + bw / 2``, as float64 device tensors [nbins]; with ``per_crop=True`` one histogram per
    leading index, [B, nbins].  No host synchronisation (edges given as a tensor are copied to the host to be checked).

    np.histogram's rule holds sample by sample: half-open bins, the last one closed, float32 samples compared exactly with the float64
    edges; NaN and out-of-range samples are in no bin and count in n.  As in the reference ``bw = (right_edge - left_edge) / n_bins`` also when
    ``bin_edges`` is given.  Edges must be finite and non-decreasing, at most 16384 bins: PnnpError otherwise, before any launch."""
    given, e, bw, hint = _edges_of(bin_edges, left_edge, right_edge, n_bins)
    data, = _sample_sets('get_histogram', per_crop, data)
    hist, _ = _hist_run('get_histogram', data, None, e, hint, per_crop)
    centers = _dev_const(np.asarray(given[:-1] + (bw / 2.0), dtype=np.float64), data.device).clone()
    return (hist if per_crop else hist[0]), centers


def kl_div_3_data(p_data, q_data, bin_edges=None, left_edge=0.0, right_edge=1.0, n_bins=1000, per_crop=False, return_hist=False):
    """utils/kld_div.py:145-161 on the device -- the marginal KL of the Noise Flow line of work: ``(kl_fwd, kl_inv, kl_sym)`` between the
    histograms (``get_histogram``) of two float32 or float64 CUDA sample sets, which may differ in length (each is divided by its own n).
    float64 device tensors, 0-dim, or [B] with ``per_crop=True`` (one score per leading index; equal B).  ``return_hist=True`` appends
    ``(hist_p, hist_q)``.  No host synchronisation; the caller's tensors are not modified; bitwise reproducible.  The sums run over the bins
    where both histograms are positive, in the reference's ``p (log p - log q)`` form; all-empty histograms give exactly 0."""
    _, e, _, hint = _edges_of(bin_edges, left_edge, right_edge, n_bins)
    p, q = _sample_sets('kl_div_3_data', per_crop, p_data, q_data)
    hist, kl = _hist_run('kl_div_3_data', p, q, e, hint, per_crop)
    if not per_crop:
        hist, kl = hist[0], kl[0]
    out = (kl[..., 0], kl[..., 1], kl[..., 2])
    return out + ((hist[..., 0, :], hist[..., 1, :]),) if return_hist else out


def kl_div_range(p_data, q_data, wp=16383):
    """The reference's ``kl_div_norm(p_data, q_data, bl=None, wp=wp)`` (utils/kld_div.py:163-200, the branch :166-169): ``wp`` bins over the
    pooled range of the two sample sets, no rounding and no clipping.  Returns kl_div_norm's dict -- ``kl_fwd``, ``kl_inv``, ``kl_sym``,
    ``hist_p`` and ``hist_q`` = (y, bin_edges * wp) -- as float64 device tensors.

    SYNCHRONISES ONCE: a range pass on the device, then four scalars are read and the edges ``np.arange(l, r + bw, bw)`` are built on the
    host with numpy in the data's own dtype, as the reference builds them (for float32 data ``r - l``, ``bw`` and ``r + bw`` round in
    float32; there are wp + 1 or wp + 2 edges, depending on that rounding).  Pooled data only: a range per crop would give ragged results.
    ValueError where the reference raises it ('arange: cannot compute length'): a NaN or an inf in the data, or all values equal."""
    if int(wp) != wp or not 1 <= wp <= MAX_BINS - 1:
        raise _lib.PnnpError(f'kl_div_range: wp = {wp}, this build counts 1 .. {MAX_BINS - 1} bins over the range')
    wp = int(wp)
    p, q = _sample_sets('kl_div_range', False, p_data, q_data)
    L = _hist_lib()
    out = torch.empty(6, dtype=torch.float64, device=p.device)
    _lib.check(L.pnnp_minmax_f(_lib.ptr(p), _lib.ptr(q), int(p.dtype == torch.float64), C.c_int64(p.numel()), C.c_int64(q.numel()),
                               _lib.ptr(out), _lib.stream()), 'kl_div_range')
    v = out.cpu().numpy()                                                   # the one synchronisation
    if v[4] != 0.0:
        raise ValueError('arange: cannot compute length (kl_div_range: a NaN or an inf in the data)')
    T = np.float64 if p.dtype == torch.float64 else np.float32
    left_edge, right_edge = min(T(v[0]), T(v[2])), max(T(v[1]), T(v[3]))
    if left_edge == right_edge:
        raise ValueError('arange: cannot compute length (kl_div_range: all values are equal)')
    data_range = right_edge - left_edge                                     # utils/kld_div.py:181-183, in the data's dtype
    bin_width = data_range / wp
    bin_edges = np.arange(left_edge, right_edge + bin_width, bin_width)
    e = np.ascontiguousarray(bin_edges, dtype=np.float64)
    if e.size - 1 > MAX_BINS or e.size < 2 or (np.diff(e) < 0).any():
        raise _lib.PnnpError(f'kl_div_range: arange gave {e.size} edges')
    span = e[-1] - e[0]
    hist, kl = _hist_run('kl_div_range', p, q, e, (float(e[0]), float((e.size - 1) / span)), False)
    x = torch.from_numpy(np.asarray(bin_edges * wp - 0, dtype=np.float64)).to(p.device)
    return {'kl_fwd': kl[0, 0], 'kl_inv': kl[0, 1], 'kl_sym': kl[0, 2], 'hist_p': (hist[0, 0], x), 'hist_q': (hist[0, 1], x.clone())}


# The four functions below are torch ops on the device, not a kernel path: a histogram is a few thousand numbers, and these lines are the
# reference's own (utils/kld_div.py:100-128), in float64, with its masks (drop NaN and inf, keep p > 0 & q > 0) and its p log(p / q) form,
# which rounds differently from kl_div_3_data's p (log p - log q).  Masked terms are zeroed, not removed: no host synchronisation.
def _kl_terms(p, q):
    _lib.require_cuda(p, q)
    p, q = p.detach().double().reshape(-1), q.detach().double().reshape(-1)
    if p.shape != q.shape:
        raise _lib.PnnpError(f'histograms of {p.numel()} and {q.numel()} bins')
    keep = torch.isfinite(p) & torch.isfinite(q) & (p > 0) & (q > 0)
    one = torch.ones_like(p)
    return torch.where(keep, p, one), torch.where(keep, q, one), keep


def kl_div_forward(p, q):
    """utils/kld_div.py:100-107: sum p log(p / q) over the finite bins with p > 0 and q > 0; 0-dim float64 device tensor."""
    p, q, keep = _kl_terms(p, q)
    return torch.where(keep, p * torch.log(p / q), torch.zeros_like(p)).sum()


def kl_div_inverse(p, q):
    """utils/kld_div.py:110-117: sum q log(q / p) over the same bins."""
    p, q, keep = _kl_terms(p, q)
    return torch.where(keep, q * torch.log(q / p), torch.zeros_like(p)).sum()


def kl_div_sym(p, q):
    """utils/kld_div.py:120-121."""
    return (kl_div_forward(p, q) + kl_div_inverse(p, q)) / 2.0


def kl_div_3(p, q):
    """utils/kld_div.py:124-128: (kl_fwd, kl_inv, kl_sym) of two histograms."""
    kl_fwd = kl_div_forward(p, q)
    kl_inv = kl_div_inverse(p, q)
    return kl_fwd, kl_inv, (kl_inv + kl_fwd) / 2.0

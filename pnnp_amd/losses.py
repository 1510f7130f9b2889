"""Differentiable distribution losses on the device (reference: utils/kld_div.py:21-98; csrc/ddl.hip, csrc/quantile.hip): the linearly
interpolated empirical CDF of a sample set (``CDFPPF.get_cdf``), ``CDFLoss``, ``KLD``, ``cdf2pdf``, ``QuantileLoss`` (with ``quantile``,
the ``torch.quantile(..., dim=-1, interpolation='linear')`` it is built on) and the evaluation points ``get_x``, under the reference's
names and signatures.  Everything but ``get_x`` takes float32 CUDA tensors and is a ``torch.autograd.Function``:
``loss.backward()`` reaches whichever of ``output`` / ``gt`` requires grad.  The gradient stops at the samples and at the points
``x`` (the reference would also differentiate with respect to ``x``; nothing in it does).

Where the reference sorts every sample set, the kernels make two streaming passes (min / max, then a count, a minimum and a maximum
per gap between points) and a K-element finish.  The cdf is the reference's CPU float32 value bit for bit.  Among equal samples the
one with the LOWEST index brackets a point and receives its gradient (``torch.sort`` gives the upper neighbour's share to the
highest index of a run of equal values; the sums per distinct value agree).  NaN samples are not supported.  The caller's tensors
are never modified.  There is no CPU fallback: CPU tensors, another dtype or sizes outside 2 <= N < 2^31, 1 <= K <= MAX_K raise
``PnnpError``.

The kernels take ascending points.  ``assume_sorted=None`` (the default) checks that with one host read and, if ``x`` is not
ascending, sorts it with ``torch.sort`` and un-permutes the result (K elements of plumbing); ``assume_sorted=True`` skips the check
and the synchronisation it costs (``NoiseFlowFitStep.ddl`` does, its default points are ascending by construction).

``quantile`` / ``QuantileLoss`` compare in the value domain.  Where ``torch.quantile`` sorts every row, the kernels select the 2K order
statistics a row needs exactly in three streaming passes (range, a 2^15-bin census, a gather of the bins that hold a wanted rank) and a
finish per gathered bin.  Ranks and weights follow torch's float32 rule (``pos = q * float32(N - 1)``); the probabilities need not be
ascending, may repeat and are not read on the host.  The same tie rule, NaN and no-fallback terms as above apply, with
1 <= N < 2^31 per row and 1 <= K <= QUANTILE_MAX_K; rows are the flattened leading dimensions.

The denoiser's own loss family (losses/base_loss.py: ``Unet_Loss``, ``L1_Charbonnier_loss``, ``Pyramid_Sample``, ``Pyramid_Loss``, ``gradient``)
is at the end of the file, on csrc/unet_loss.hip."""
import ctypes as C

import torch

from . import _lib

MAX_K = 4096                     # PNNP_DDL_MAX_K
QUANTILE_MAX_K = 1024            # PNNP_QUANTILE_MAX_K


def _ddl_lib():
    L = _lib.lib()
    if L.pnnp_ddl_ws_bytes.restype is not C.c_int64:
        L.pnnp_ddl_ws_bytes.restype = C.c_int64
    return L


def _flat(t, what):
    """The reference's ``.view(-1)`` of a sample set, as a contiguous detached float32 CUDA tensor (a copy only if it has to be)."""
    if not isinstance(t, torch.Tensor):
        raise _lib.PnnpError(f'{what}: expected a tensor, got {type(t).__name__}')
    _lib.require_cuda(t)
    if t.dtype != torch.float32:
        raise _lib.PnnpError(f'{what}: the distribution losses take float32 tensors, got {t.dtype}')
    n = t.numel()
    if not 2 <= n < 2 ** 31:
        raise _lib.PnnpError(f'{what}: {n} samples, the kernels take 2 <= N < 2^31')
    return t.detach().reshape(-1).contiguous()


def _points(x, min_k, what, assume_sorted):
    """-> (ascending contiguous points, inverse permutation or None)"""
    if not isinstance(x, torch.Tensor):
        raise _lib.PnnpError(f'{what}: expected a tensor of points, got {type(x).__name__}')
    _lib.require_cuda(x)
    if x.dtype != torch.float32:
        raise _lib.PnnpError(f'{what}: the points must be float32, got {x.dtype}')
    k = x.numel()
    if not min_k <= k <= MAX_K:
        raise _lib.PnnpError(f'{what}: {k} points, the kernels take {min_k} <= K <= {MAX_K}')
    x = x.detach().reshape(-1).contiguous()
    if assume_sorted is None:
        assume_sorted = k < 2 or bool((x[1:] >= x[:-1]).all())                   # the one host read
    if assume_sorted:
        return x, None
    xs, perm = torch.sort(x)
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(k, device=x.device)
    return xs.contiguous(), inv


def _workspace(L, nops, k, device):
    nbytes = int(L.pnnp_ddl_ws_bytes(nops, k))
    if nbytes < 0:
        _lib.check(nbytes, 'pnnp_ddl_ws_bytes')
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def _backward(data, x, brackets, g, scale):
    """grad [N] of sum_k g[k] cdf[k] (g times the device scalar ``scale`` if given) with respect to the flat samples"""
    grad = torch.empty_like(data)
    _lib.check(_ddl_lib().pnnp_ecdf_bwd_f32(_lib.ptr(data), C.c_int64(data.numel()), _lib.ptr(x), x.numel(), _lib.ptr(brackets), _lib.ptr(g),
                                            _lib.ptr(scale), _lib.ptr(grad), _lib.stream()), 'pnnp_ecdf_bwd_f32')
    return grad


def ecdf_with_brackets(data, x):
    """The cdf [K] of the flattened ``data`` at the ASCENDING points ``x`` and the kernel's bracket indices, int32 [2K + 2]: arg hi [K]
    (the smallest sample >= the clamped point), arg lo [K] (the largest sample below it, -1 if none), arg min, arg max.  No autograd."""
    flat = _flat(data, 'CDFPPF')
    x, _ = _points(x, 1, 'CDFPPF', True)
    L = _ddl_lib()
    k = x.numel()
    cdf = torch.empty(k, dtype=torch.float32, device=flat.device)
    brackets = torch.empty(2 * k + 2, dtype=torch.int32, device=flat.device)
    ws = _workspace(L, 1, k, flat.device)
    _lib.check(L.pnnp_ecdf_f32(_lib.ptr(flat), C.c_int64(flat.numel()), _lib.ptr(x), k, _lib.ptr(ws), _lib.ptr(cdf), _lib.ptr(brackets),
                               _lib.stream()), 'pnnp_ecdf_f32')
    return cdf, brackets


class _ECDF(torch.autograd.Function):
    @staticmethod
    def forward(ctx, data, x):
        flat = _flat(data, 'CDFPPF')
        cdf, brackets = ecdf_with_brackets(flat, x)
        ctx.save_for_backward(flat, x, brackets)
        ctx.shape = data.shape
        return cdf

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None
        flat, x, brackets = ctx.saved_tensors
        g = g.to(torch.float32).contiguous()
        return _backward(flat, x, brackets, g, None).view(ctx.shape), None


class _Loss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, output, gt, x, kind):
        entry = {'cdf': 'pnnp_cdf_loss_f32', 'kld': 'pnnp_kld_loss_f32'}[kind]
        o, g = _flat(output, kind + ' loss: output'), _flat(gt, kind + ' loss: gt')
        if o.device != g.device or x.device != o.device:
            raise _lib.PnnpError(f'{kind} loss: output, gt and the points are on different devices')
        L = _ddl_lib()
        k = x.numel()
        dev = o.device
        cdf = torch.empty(2, k, dtype=torch.float32, device=dev)
        dcdf = torch.empty(2, k, dtype=torch.float32, device=dev)
        brackets = torch.empty(2, 2 * k + 2, dtype=torch.int32, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        ws = _workspace(L, 2, k, dev)
        _lib.check(getattr(L, entry)(_lib.ptr(o), C.c_int64(o.numel()), _lib.ptr(g), C.c_int64(g.numel()), _lib.ptr(x), k, _lib.ptr(ws),
                                     _lib.ptr(cdf), _lib.ptr(brackets), _lib.ptr(loss), _lib.ptr(dcdf), _lib.stream()), entry)
        ctx.save_for_backward(o, g, x, brackets, dcdf)
        ctx.shapes = (output.shape, gt.shape)
        return loss.view(())

    @staticmethod
    def backward(ctx, gup):
        o, g, x, brackets, dcdf = ctx.saved_tensors
        scale = gup.to(torch.float32).reshape(1).contiguous()
        grads = [None, None]
        for i, data in enumerate((o, g)):
            if ctx.needs_input_grad[i]:
                grads[i] = _backward(data, x, brackets[i], dcdf[i], scale).view(ctx.shapes[i])
        return grads[0], grads[1], None, None


class CDFPPF(torch.nn.Module):
    """utils/kld_div.py:21-46: the empirical CDF of ``data`` (1-D in the reference; any shape is flattened), linearly interpolated
    between order statistics.  Nothing is sorted or stored: ``get_cdf`` reads ``data`` when it is called."""

    def __init__(self, data, inf=None):
        super().__init__()
        if inf is not None:
            raise _lib.PnnpError('CDFPPF(inf=...): only the default padding (inf) is provided')
        _flat(data, 'CDFPPF')
        self.data = data

    def get_cdf(self, x, assume_sorted=None):
        xs, inv = _points(x, 1, 'CDFPPF.get_cdf', assume_sorted)
        if xs.device != self.data.device:
            raise _lib.PnnpError('CDFPPF.get_cdf: the points and the samples are on different devices')
        cdf = _ECDF.apply(self.data, xs)
        if inv is not None:
            cdf = cdf[inv]
        return cdf.view(x.shape)

    def forward(self, x):
        return self.get_cdf(x)


def cdf2pdf(data):
    """utils/kld_div.py:76-78: |data[k] - data[k+1]| (the reference's conv1d with the kernel [1, -1]); K elements, plain tensor ops."""
    _lib.require_cuda(data)
    d = data.reshape(-1)
    return torch.abs(d[:-1] - d[1:])


def CDFLoss(output, gt, x_cdf, assume_sorted=None):
    """utils/kld_div.py:56-60: mean_k |cdf_output(x_k) - cdf_gt(x_k)|, a 0-dim device tensor.  The mean does not depend on the order
    of the points, so points that are not ascending are simply sorted."""
    xs, _ = _points(x_cdf, 1, 'CDFLoss', assume_sorted)
    return _Loss.apply(output, gt, xs, 'cdf')


def KLD(output, gt, x_pdf, assume_sorted=None):
    """utils/kld_div.py:62-74: KL divergence of the two difference quotients of the interpolated CDFs (q from ``output``, p from ``gt``,
    clamped at 1e-9, divided by the detached larger sum), a 0-dim device tensor.  The differences depend on the order of the points:
    for points that are not ascending the loss is composed from ``get_cdf`` and K-element tensor ops in the given order."""
    xs, inv = _points(x_pdf, 2, 'KLD', assume_sorted)
    if inv is None:
        return _Loss.apply(output, gt, xs, 'kld')
    _flat(gt, 'kld loss: gt')
    q = cdf2pdf(_ECDF.apply(output, xs)[inv]).clamp_min(1e-9)
    p = cdf2pdf(_ECDF.apply(gt, xs)[inv]).clamp_min(1e-9)
    factor = torch.max(q.sum(), p.sum()).detach()
    q, p = q / factor, p / factor
    return torch.sum(p * (torch.log(p) - torch.log(q)))


def _quantile_lib():
    L = _lib.lib()
    if not hasattr(L, 'pnnp_quantile_loss_f32'):
        raise _lib.PnnpError('libpnnp_hip.so has no pnnp_quantile_* entries: it was built before they were added (rebuild with tools/build.py)')
    if L.pnnp_quantile_ws_bytes.restype is not C.c_int64:
        L.pnnp_quantile_ws_bytes.restype = C.c_int64
        L.pnnp_quantile_ws_bytes.argtypes = [C.c_int, C.c_int64, C.c_int64, C.c_int]
    return L


def _rows(t, what):
    """The samples as contiguous detached float32 rows [R, N] over the last dimension (a copy only if it has to be)."""
    if not isinstance(t, torch.Tensor):
        raise _lib.PnnpError(f'{what}: expected a tensor, got {type(t).__name__}')
    _lib.require_cuda(t)
    if t.dtype != torch.float32:
        raise _lib.PnnpError(f'{what}: the distribution losses take float32 tensors, got {t.dtype}')
    if t.dim() < 1:
        raise _lib.PnnpError(f'{what}: a 0-dim tensor has no last dimension')
    n = t.shape[-1]
    if not 1 <= n < 2 ** 31:
        raise _lib.PnnpError(f'{what}: {n} samples per row, the kernels take 1 <= N < 2^31')
    rows = t.numel() // n
    if not 1 <= rows <= 32767:
        raise _lib.PnnpError(f'{what}: {rows} rows, the kernels take 1 <= rows <= 32767')
    return t.detach().reshape(rows, n).contiguous()


def _probabilities(q, what, device):
    if not isinstance(q, torch.Tensor):
        raise _lib.PnnpError(f'{what}: expected a tensor of probabilities, got {type(q).__name__}')
    _lib.require_cuda(q)
    if q.dtype != torch.float32:
        raise _lib.PnnpError(f'{what}: the probabilities must be float32, got {q.dtype}')
    if q.dim() > 1:
        raise _lib.PnnpError(f'{what}: the probabilities must be 0-dim or 1-D, got {q.dim()} dimensions')
    k = q.numel()
    if not 1 <= k <= QUANTILE_MAX_K:
        raise _lib.PnnpError(f'{what}: {k} probabilities, the kernels take 1 <= K <= {QUANTILE_MAX_K}')
    if q.device != device:
        raise _lib.PnnpError(f'{what}: the probabilities and the samples are on different devices')
    return q.detach().reshape(-1).contiguous()


def _quantile_workspace(L, rows, n_a, n_b, k, device):
    nbytes = int(L.pnnp_quantile_ws_bytes(rows, n_a, n_b, k))
    if nbytes < 0:
        _lib.check(nbytes, 'pnnp_quantile_ws_bytes')
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def _quantile_backward(rows, n, arg, w, g, scale):
    """grad [R, N] of sum g[k, r] value[k, r] (g times the device scalar ``scale`` if given) with respect to the rows"""
    grad = torch.empty(rows, n, dtype=torch.float32, device=g.device)
    _lib.check(_quantile_lib().pnnp_quantile_bwd_f32(rows, C.c_int64(n), w.numel(), _lib.ptr(arg), _lib.ptr(w), _lib.ptr(g), _lib.ptr(scale),
                                                     _lib.ptr(grad), _lib.stream()), 'pnnp_quantile_bwd_f32')
    return grad


def quantile_with_state(data, q):
    """``torch.quantile(data, q, dim=-1, interpolation='linear')`` of float32 CUDA ``data`` as [K, R] (R: the flattened leading dimensions)
    and the kernel's state: arg int32 [2, R, K] (the element of its row that holds s[lo], then s[hi]: the lowest index among equal
    values) and the weights w [K].  No autograd."""
    rows = _rows(data, 'quantile')
    q = _probabilities(q, 'quantile', rows.device)
    L = _quantile_lib()
    r, n, k = rows.shape[0], rows.shape[1], q.numel()
    values = torch.empty(k, r, dtype=torch.float32, device=rows.device)
    arg = torch.empty(2, r, k, dtype=torch.int32, device=rows.device)
    w = torch.empty(k, dtype=torch.float32, device=rows.device)
    ws = _quantile_workspace(L, r, n, 0, k, rows.device)
    _lib.check(L.pnnp_quantile_f32(_lib.ptr(rows), r, C.c_int64(n), _lib.ptr(q), k, _lib.ptr(ws), _lib.ptr(values), _lib.ptr(arg), _lib.ptr(w),
                                   _lib.stream()), 'pnnp_quantile_f32')
    return values, arg, w


class _Quantile(torch.autograd.Function):
    @staticmethod
    def forward(ctx, data, q):
        values, arg, w = quantile_with_state(data, q)
        ctx.save_for_backward(arg, w)
        ctx.shape = data.shape
        out_shape = (() if q.dim() == 0 else (q.numel(),)) + tuple(data.shape[:-1])
        return values.view(out_shape)

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None
        arg, w = ctx.saved_tensors
        rows, n = arg.shape[1], ctx.shape[-1]
        g = g.to(torch.float32).reshape(w.numel(), rows).contiguous()
        return _quantile_backward(rows, n, arg, w, g, None).view(ctx.shape), None


def quantile(data, q):
    """``torch.quantile(data, q, dim=-1, keepdim=False, interpolation='linear')`` for float32 CUDA tensors: [K, *leading] (a 0-dim ``q``
    gives [*leading]).  Differentiable with respect to ``data`` only."""
    return _Quantile.apply(data, q)


class _QuantileLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, output, gt, q):
        o, g = _rows(output, 'QuantileLoss: output'), _rows(gt, 'QuantileLoss: gt')
        if o.device != g.device:
            raise _lib.PnnpError('QuantileLoss: output and gt are on different devices')
        q = _probabilities(q, 'QuantileLoss', o.device)
        if o.shape[0] != g.shape[0]:
            raise _lib.PnnpError(f'QuantileLoss: output has {o.shape[0]} rows and gt {g.shape[0]}')
        L = _quantile_lib()
        r, k, dev = o.shape[0], q.numel(), o.device
        values = torch.empty(2, k, r, dtype=torch.float32, device=dev)
        dq = torch.empty(2, k, r, dtype=torch.float32, device=dev)
        arg = torch.empty(2, 2, r, k, dtype=torch.int32, device=dev)
        w = torch.empty(2, k, dtype=torch.float32, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        ws = _quantile_workspace(L, r, o.shape[1], g.shape[1], k, dev)
        _lib.check(L.pnnp_quantile_loss_f32(_lib.ptr(o), C.c_int64(o.shape[1]), _lib.ptr(g), C.c_int64(g.shape[1]), r, _lib.ptr(q), k, _lib.ptr(ws),
                                            _lib.ptr(values), _lib.ptr(arg), _lib.ptr(w), _lib.ptr(loss), _lib.ptr(dq), _lib.stream()),
                   'pnnp_quantile_loss_f32')
        ctx.save_for_backward(arg, w, dq)
        ctx.shapes = (output.shape, gt.shape)
        ctx.ns = (o.shape[1], g.shape[1])
        return loss.view(())

    @staticmethod
    def backward(ctx, gup):
        arg, w, dq = ctx.saved_tensors
        scale = gup.to(torch.float32).reshape(1).contiguous()
        grads = [None, None]
        for i in range(2):
            if ctx.needs_input_grad[i]:
                grads[i] = _quantile_backward(arg.shape[2], ctx.ns[i], arg[i], w[i], dq[i], scale).view(ctx.shapes[i])
        return grads[0], grads[1], None


def QuantileLoss(output, gt, x_quant):
    """utils/kld_div.py:49-53: mean |quantile(output, x_quant, dim=-1) - quantile(gt, x_quant, dim=-1)|, a 0-dim device tensor.  1-D
    operands may differ in length; operands with leading dimensions are compared row by row (the same number of rows) and the mean
    runs over all K x R differences.  One fused call: both operands, the mean and dL/dquantile."""
    return _QuantileLoss.apply(output, gt, x_quant)


def get_x(sigma=4, size=1000, mode='uniform', random=True):
    """utils/kld_div.py:80-98: evaluation points in (0, 1) -- 'uniform': evenly spaced; 'cdf': the normal CDF of evenly spaced points
    over [-sigma, sigma], jittered by N(0, 10^-sigma) and clipped to [0, 1]; 'icdf': normal quantiles of evenly spaced probabilities
    jittered by N(0, (10^-sigma / 2)^2).  Host code on torch's global RNG: the same draws as the reference under ``torch.manual_seed``.
    Returns a CPU float32 tensor (ascending, except that the reference returns any other ``mode`` sorted too)."""
    tiny = 10 ** (-sigma)
    x = torch.linspace(tiny, 1 - tiny, size)
    if mode == 'uniform':
        return x
    normal = torch.distributions.Normal(loc=0, scale=1)
    if mode == 'cdf':
        x = normal.cdf(x * sigma * 2 - sigma)
        if random:
            x = torch.clamp(x + torch.randn(size) / 10 ** sigma, 0, 1)
    elif mode == 'icdf':
        if random:
            x = x + (torch.randn(size) / 2) / 10 ** sigma
        x = normal.icdf(x.clamp(tiny, 1 - tiny))
    return torch.sort(x)[0]


# ------------------------------------------------------------------------------------------------ Unet_Loss (losses/base_loss.py:15-107)
# The denoiser's own loss family under the reference's names.  ``Unet_Loss`` runs on csrc/unet_loss.hip (``ops.unet_loss``): forward and
# ``.backward()`` in streaming passes, gradient with respect to ``low`` only, no clamp inside (the trainers clamp before they call it:
# trainer_SID.py:99; ``HipTrainStep(loss=)`` folds that clamp into the kernel).  ``Pyramid_Sample``, ``Pyramid_Loss`` and ``gradient`` are plain
# tensor ops, not on the path: kept so that the reference's imports resolve, as ``apply_gains`` is in process.py.
# Not mirrored: ``Unet_dpsv_Loss``, ``Unet_dpsv_Loss_up`` and ``GAN_Loss`` (nothing in the reference instantiates them), the commented-out
# ``gamma`` term of ``loss()``, the pyramid of the edge term (never defined), odd sizes under the pyramid (the reference floors; here H and W
# must be multiples of 8 -- the networks need multiples of 16 anyway).

SOBEL = ((-1.0, -2.0, -1.0), (0.0, 0.0, 0.0), (1.0, 2.0, 1.0))
ROBERT = ((0.0, 0.0), (-1.0, 1.0))


def gradient(maps, direction, device='cuda', kernel='sobel'):
    """|first-derivative filter| of ``maps`` [B,C,H,W] (base_loss.py:15-31): the 3x3 Sobel (zero padding 1) or the 2x2 Robert kernel (one row of
    zero padding above and below), expanded to a [C,C,k,k] weight, so every output channel filters the channel SUM; 'y' transposes the kernel."""
    channels = maps.shape[1]
    if kernel == 'robert':
        k = torch.tensor(ROBERT).expand(channels, channels, 2, 2)
        maps = torch.nn.functional.pad(maps, (0, 0, 1, 1))
    elif kernel == 'sobel':
        k = torch.tensor(SOBEL).expand(channels, channels, 3, 3)
        maps = torch.nn.functional.pad(maps, (1, 1, 1, 1))
    else:
        raise ValueError(kernel)
    if direction == 'y':
        k = k.transpose(2, 3)
    elif direction != 'x':
        raise ValueError(direction)
    return torch.nn.functional.conv2d(maps, k.to(device=device, dtype=maps.dtype)).abs()


def Pyramid_Sample(img, max_scale=8):
    """[AvgPool2d(2,2)(img), AvgPool2d(2,2) of that, ...] down to 1 / max_scale (base_loss.py:38-46)."""
    out, scale = [], 2
    while scale <= max_scale:
        img = torch.nn.functional.avg_pool2d(img, 2, 2)
        out.append(img)
        scale *= 2
    return out


def Pyramid_Loss(lows, highs, loss_fn=torch.nn.functional.l1_loss, rate=1., norm=True):
    """sum_i rate^i loss_fn(lows[i], highs[i]), divided by sum_i rate^i when ``norm`` (base_loss.py:48-61)."""
    total, weights, lam = 0, 0, 1
    for low, high in zip(lows, highs):
        total = total + loss_fn(low, high) * lam
        weights += lam
        lam = lam * rate
    return total / weights if norm else total


def _image_pair(low, high, what):
    for name, t in (('low', low), ('high', high)):
        if not isinstance(t, torch.Tensor):
            raise _lib.PnnpError(f'{what}: {name}: expected a tensor, got {type(t).__name__}')
    _lib.require_cuda(low, high)
    if low.dtype != torch.float32 or high.dtype != torch.float32 or low.dim() != 4 or low.shape != high.shape or low.device != high.device:
        raise _lib.PnnpError(f'{what}: low and high must be float32 [B,C,H,W] of one shape on one device, got {tuple(low.shape)} ({low.dtype}) '
                             f'and {tuple(high.shape)} ({high.dtype})')
    if not 1 <= low.shape[1] <= 8:
        raise _lib.PnnpError(f'{what}: {low.shape[1]} channels, the kernel takes 1 .. 8')
    return low.detach().contiguous(), high.detach().contiguous()


class _UnetLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, low, high, charbonnier, pyramid, grad, recon):
        from . import ops
        lo, hi = _image_pair(low, high, 'Unet_Loss')
        B, dev = lo.shape[0], lo.device
        out = torch.empty(1 + B, dtype=torch.float32, device=dev)
        terms = torch.empty(ops.UNET_LOSS_TERMS, dtype=torch.float32, device=dev)
        ws = torch.empty(ops.unet_loss_workspace_floats(B), dtype=torch.float32, device=dev)
        g = torch.empty_like(lo) if ctx.needs_input_grad[0] else None
        ops.unet_loss(lo, hi, None, out, ws, clamp_pred=False, charbonnier=charbonnier, pyramid=pyramid, grad=grad, terms=terms, grad_nchw=g, recon=recon)
        ctx.save_for_backward(g)
        ctx.mark_non_differentiable(terms)
        return out[0], terms

    @staticmethod
    def backward(ctx, gup, _):
        g, = ctx.saved_tensors
        return (g * gup if g is not None else None), None, None, None, None, None


class L1_Charbonnier_loss(torch.nn.Module):
    """mean sqrt((low - high)^2 + 1e-6) (base_loss.py:63-73) on the device."""

    def __init__(self):
        super().__init__()
        self.eps = 1e-6

    def forward(self, low, high):
        return _UnetLoss.apply(low, high, True, False, 0.0, True)[0]


class Unet_Loss(torch.nn.Module):
    """base_loss.py:75-107.  ``forward(low, high, pyramid=False)``: the L1 (or, with ``charbonnier=True``, the Charbonnier) loss, plain or over the
    4-level average-pool pyramid; ``grad_loss``: the Sobel edge term the reference keeps out of ``loss()``.  float32 CUDA tensors [B,C,H,W] with
    C <= 8 (``PnnpError`` otherwise: no CPU path); differentiable with respect to ``low``.  ``terms`` holds the last call's terms before weighting
    (device tensor [5]: four level means, the edge term)."""

    def __init__(self, charbonnier=False):
        super().__init__()
        self.charbonnier = bool(charbonnier)
        self.l1_loss = L1_Charbonnier_loss() if charbonnier else torch.nn.functional.l1_loss      # the reference's attribute; forward() does not go through it
        self.terms = None

    def _run(self, low, high, pyramid, grad, recon):
        loss, self.terms = _UnetLoss.apply(low, high, self.charbonnier, bool(pyramid), float(grad), recon)
        return loss

    def grad_loss(self, low, high):
        return self._run(low, high, False, 1.0, False)

    def pyramid_loss(self, low, high):
        return self._run(low, high, True, 0.0, True)

    def loss(self, low, high):
        return self._run(low, high, False, 0.0, True)

    def forward(self, low, high, pyramid=False):
        return self.pyramid_loss(low, high) if pyramid else self.loss(low, high)

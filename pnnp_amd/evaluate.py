"""The eval step of the reference trainers as a product function, all on the device.

One iteration of `SID_Trainer.eval` (trainer_SID.py:208-248; trainer_LRID.py has the same body):

    if W % 16 != 0:  reflect-pad 4 px on every side, run the net, crop both back        (:221-228)
    if dst.ori:      imgs_lr *= ratio;  imgs_dn *= ratio                                 (:231-233)
    clamp both to [0, 1]                                                                 (:234-235)
    if brightness_correct and epoch < 0:  imgs_dn = IlluminanceCorrect(imgs_dn, imgs_hr) (:238-239)
    PSNR / SSIM of tensor2im(imgs_dn) and of tensor2im(imgs_lr) against tensor2im(imgs_hr), data_range 255  (:242-255)

and the bookkeeping around it: the `metrics` dict that goes to `metrics.pkl` (:247,314-315: name -> [PSNR, SSIM] of the
denoised frame, or (psnr_dn, ssim_dn) when plots are on) and the log line (:309-312).  With ``render=`` the three frames are also
rendered to sRGB by the pure-tensor ISP (process.raw2rgb_v2, csrc/isp.hip) and scored in the RGB domain, the figures of
plot_sample(res=None) (utils/visualization.py:55-63).  The rawpy renderer, matplotlib figures, file writing and checkpoint selection
stay outside (out of scope).  The IMX686 frame 4x1736x2312 takes the padded branch (2312 % 16 = 8 -> 4x1744x2320).
"""
import contextlib
import ctypes as C

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib
from ._lib import PnnpError
from .metrics import IlluminanceCorrect, quality_assess


# precision= -> the engine switches (ConvPolicy sub-switches, set_policy) a call forces; a switch not named stays as the call finds it
_PRECISION = {'fp32': dict(h1_eval=False), 'fp16': dict(h1_eval=True), 'fp16_all': dict(h1_eval=True, h1_pointwise=True)}
# ... and the precisions that also choose how activations are STORED.  A table of its own for one reason only: tests/test_host_h1pw_ref.py pins _PRECISION to
# exactly the three entries above, and existing tests stay as they are.  _precision() reads both; a later change that may touch that test can merge them.
_PRECISION_STORAGE = {'fp16_act': dict(h1_eval=True, h1_pointwise=True, h1_act16=True)}
# ... and fp16 storage for ResUnet as well (ConvPolicy.h1_act16_res).  A third table for the same reason: tests/test_host_act16_ref.py pins the one above.
_PRECISION_STORAGE_RES = {'fp16_act_res': dict(h1_eval=True, h1_pointwise=True, h1_act16=True, h1_act16_res=True)}


@contextlib.contextmanager
def _precision(net, precision):
    """``precision=`` of the functions below: None leaves the engine's policy alone; 'fp16' runs the eval forward's stride-1 3x3 layers with ONE fp16
    piece per operand (ConvPolicy.h1_eval, csrc/conv_h1s.hip), 'fp32' on the float32-accurate default path (fp16x2), for the duration of the call; the
    engine's previous setting comes back afterwards, also when the call raises.  Changing the switch invalidates the weight packs as set_policy does:
    alternating precisions per call re-packs each time -- to serve one precision, call ``net.engine.set_policy(h1_eval=True)`` once instead.
    'fp16_all' is 'fp16' with the ConvTranspose2d / 1x1 / stride-2 layers on one fp16 piece as well (ConvPolicy.h1_pointwise, csrc/gemm_h1s.hip): both
    switches are set for the call and both come back.  'fp16_act' is 'fp16_all' with every map a convolution writes and a convolution reads STORED as fp16
    (ConvPolicy.h1_act16; UNet plans whose layers all run on fp16x1 -- otherwise it is 'fp16_all'): three switches, set and restored alike.
    'fp16_act_res' is 'fp16_act' that reaches ResUnet too (ConvPolicy.h1_act16_res: its residual sums, stride-2 and 1x1 layers and both ends read and write
    fp16): four switches; on a UNet it is 'fp16_act' bit for bit."""
    if precision is None:
        yield
        return
    want = _PRECISION.get(precision) or _PRECISION_STORAGE.get(precision) or _PRECISION_STORAGE_RES.get(precision)
    if want is None:
        raise PnnpError(f"precision must be None, 'fp32', 'fp16', 'fp16_all', 'fp16_act' or 'fp16_act_res', got {precision!r}")
    eng = getattr(net, 'engine', None)
    if eng is None or not hasattr(eng, 'set_policy'):
        if precision != 'fp32':
            raise PnnpError(f"precision='{precision}' needs a network with a HIP engine")
        yield
        return
    if want['h1_eval'] and not eng.policy.h2:
        raise PnnpError(f"precision='{precision}' needs the fp16x2 family (set_policy(h2=True)): its amax slots are what the scale is made of")
    prev = {k: bool(getattr(eng.policy, k)) for k in want}
    if prev == want:
        yield
        return
    had = [k for k in want if k in eng._h2_sub]
    eng.set_policy(**want)
    try:
        yield
    finally:
        eng.set_policy(**prev)
        for k in want:
            if k not in had:
                eng._h2_sub.pop(k, None)


def forward_tiled(net, frame, patch_size, base=64, tile_batch=None, ratio=None, clamp=False, precision=None):
    """The network over one frame in overlapping tiles (the reference's eval_crop -> net per tile -> eval_merge, syn_datasets.py:109-159,
    trainer_SID.py:209-218,351-357): CUDA [1,C,h,w] -> [1,out_nc,h,w].  The frame need not be a multiple of 16 and may be larger than
    what one forward takes (engine.effective_policy); ``patch_size`` must be a multiple of 16 and ``h, w >= patch_size - base``.

    Per chunk of ``tile_batch`` tiles (None: all of them in one batch) there is one forward, whose layout pass gathers the tiles straight
    out of the frame (``engine.forward(tile_src=...)``: no padded frame, no NCHW tile batch), and one merge launch that writes what those
    tiles own, optionally with ``(. * ratio).clamp(0, 1)`` fused in (``ratio``: a float or a CUDA scalar; the eval tail).  Nothing synchronises.

    ``tile_batch`` only bounds the activation memory, which the engine keeps per batch shape: about ``40 * nf * patch_size^2`` bytes per
    tile for UNetSeeInDark (ten nf-channel full-resolution maps' worth over the five levels: 0.34 GB per tile at nf = 32, patch_size = 512)
    and about the same for ResUnet.  A last chunk of another size gets a buffer set of its own.  The result does not depend on the
    chunking beyond what the kernels' own choices by batch size (plan.py) change: float32 rounding.

    A ``net`` without a HIP engine runs as ``eval_merge(net(eval_crop(frame)))``, chunked the same way.

    ``precision``: None / 'fp32' / 'fp16' / 'fp16_all' for this call (``_precision``: 'fp16' = one fp16 rounding per operand in the stride-1 3x3 layers, float32
    accumulation, 'fp16_all' = in the ConvTranspose2d / 1x1 / stride-2 layers as well; the switch is restored afterwards, and alternating precisions per call re-packs the weights each time)."""
    with _precision(net, precision):
        return _forward_tiled(net, frame, patch_size, base, tile_batch, ratio, clamp)


def _forward_tiled(net, frame, patch_size, base, tile_batch, ratio, clamp):
    from . import ops
    from .tiles import TileGrid, _frame
    x = _frame(frame, 'forward_tiled')
    grid = TileGrid(x.shape[2], x.shape[3], patch_size, base, network=True)
    eng = getattr(net, 'engine', None)
    if not (eng is not None and hasattr(eng, 'forward')):
        eng = None
    elif x.shape[1] != eng.cin:
        raise PnnpError(f'forward_tiled: the network takes {eng.cin} channels, the frame has {x.shape[1]}')
    out = None
    with torch.no_grad():
        for t0, nt in grid.chunks(tile_batch):
            if eng is not None:
                y = eng.forward(None, False, tile_src=(x, grid, t0, nt))
            else:
                xt = torch.empty((nt, x.shape[1], grid.patch_size, grid.patch_size), dtype=torch.float32, device=x.device)
                ops.tile_crop(x, grid, t0, nt, nchw=xt)
                y = net(xt).contiguous().float()
            if out is None:
                out = torch.empty((1, y.shape[1], grid.h, grid.w), dtype=torch.float32, device=x.device)
            ops.tile_merge(y, out, grid, t0, nt, ratio=ratio, clamp=clamp)
    return out


def predict(net, raw, wp, bl, patch_size, base=64, bias=None, tile_batch=None, precision=None):
    """The reference's ``predict`` (trainer_SID.py:345-360, trainer_LRID.py:341-356): a Bayer frame [H,W] (uint16 / float32, numpy or CUDA)
    -> the denoised packed frame, a DEVICE tensor [C, H/2, W/2] (the reference saves it as .npy; writing files stays with the caller).
    The mosaic is packed by the raw2bayer kernel with the camera's ``wp`` / ``bl`` (the reference calls raw2bayer(raw + bl) with that
    function's defaults 1023 / 64), then ``forward_tiled`` without ratio or clamp (``precision``: as there)."""
    from . import isp_ops
    if not torch.is_tensor(raw):
        raw = torch.from_numpy(np.ascontiguousarray(raw))
    if raw.dim() != 2:
        raise PnnpError(f'predict expects one Bayer frame [H,W], got {tuple(raw.shape)}')
    packed = isp_ops.raw2bayer(raw.cuda(), wp=wp, bl=bl, norm=True, clip=False, bias=np.zeros(4) if bias is None else bias)
    return forward_tiled(net, packed[None], patch_size, base=base, tile_batch=tile_batch, precision=precision)[0]


def predict_rgb(net, raw, wp, bl, patch_size, wb, ccm, base=64, tile_batch=None, precision=None, bgr=False):
    """Raw file in, full-resolution picture out, without leaving the device: ``predict``, a clamp to [0,1], then the full-resolution
    render (process.fastisp_render) with the gains ``wb`` [4] and the matrix ``ccm`` [3,3] -> uint8 [H,W,3] device tensor, RGB or
    (``bgr``) BGR."""
    from . import process
    dn = predict(net, raw, wp, bl, patch_size, base=base, tile_batch=tile_batch, precision=precision)
    if dn.shape[0] != 4:
        raise PnnpError(f'predict_rgb needs a network that returns packed RGBG frames, got {tuple(dn.shape)}')
    rows = process.isp_rows(wb, ccm, 1, dn.device)
    return process.fastisp_render(dn.clamp(0, 1)[None], rows, f32=False, u8=True, bgr=bgr)[1][0]


def evaluate(net, imgs_lr, imgs_hr, ratio=None, ori=False, brightness_correct=True, epoch=-1, corrector=None, with_lr=True, render=None, tiles=None,
             precision=None, baseline=None):
    """-> dict(dn=<clamped (and corrected) prediction>, lr=<clamped input>, metrics=<device tensor [PSNR_dn, SSIM_dn, PSNR_lr, SSIM_lr]>).

    ``imgs_lr``, ``imgs_hr``: CUDA [1,C,H,W] (the eval loaders use batch_size 1); ``ratio``: scalar / [1] tensor, needed when
    ``ori``.  Nothing synchronises: read ``metrics`` (``.tolist()``) when the numbers are needed.

    ``render=dict(wb=<4 gains>, ccm=<3x3>, bgr=False)`` (C must be 4) adds ``rgb=dict(lr=, dn=, hr=)``, uint8 [H,W,3] device tensors of
    ``lr``, ``dn`` and ``imgs_hr`` through process.raw2rgb_v2's kernel, and ``metrics_rgb``, a device tensor [PSNR_dn, SSIM_dn, PSNR_lr,
    SSIM_lr] of ``quality_assess`` on the float renders.  ``rows=`` in the dictionary takes a table from process.isp_rows instead of
    wb / ccm.  Still nothing synchronises; without ``render`` nothing changes.  ``full=True`` in the dictionary renders at full resolution
    instead (process.fastisp_render, the reference's FastISP): ``rgb`` then holds uint8 [2H,2W,3] and ``metrics_rgb`` scores the
    full-resolution float renders, the resolution at which the reference's logs report them; without the key nothing changes.

    ``tiles=dict(patch_size=, base=64, tile_batch=None)``: the network runs over the frame in overlapping tiles (``forward_tiled``; the
    reference's strategy for frames that do not fit, trainer_SID.py:209-218) instead of in one forward: the reflect-pad-4 branch is not
    taken, the frame need not be a multiple of 16, and ``x ratio`` and the clamp of the prediction ride on the merge.  Everything behind
    that is the same; without ``tiles`` nothing changes.

    ``precision``: None / 'fp32' / 'fp16' / 'fp16_all' for the network forward of this call, as in ``forward_tiled``; the engine's previous setting is restored
    afterwards, also when the call raises.

    ``baseline=dict(gain=, sigma=, wp_bl=, d=7, eps=1.0)``: the input frame is also denoised by the non-learned baseline
    (isp_algos.vst_denoise: VST -> guided filter -> inverse VST; ``gain`` and ``sigma`` in DN, ``wp_bl`` = white point minus black level)
    at ``scale = float32(wp_bl) / float32(ratio)`` (one float32 division, however ``ratio`` is passed: a float, a host or a device tensor), or ``wp_bl`` with ``ori`` (the frame is then multiplied by ``ratio`` as the prediction is), clamped to
    [0, 1] like the prediction, and scored: the result gains ``base`` (the frame) and ``psnr_base`` / ``ssim_base`` (device scalars, its
    ``quality_assess`` against ``imgs_hr``).  None (the default): nothing changes."""
    with _precision(net, precision):
        res = _evaluate(net, imgs_lr, imgs_hr, ratio, ori, brightness_correct, epoch, corrector, with_lr, render, tiles)
    if baseline is not None:
        res.update(_baseline(baseline, imgs_lr, imgs_hr, ratio, ori))
    return res


def _baseline(baseline, imgs_lr, imgs_hr, ratio, ori):
    """the ``baseline=`` part of ``evaluate``: four launches of csrc/isp_algos.hip, one of the PSNR / SSIM kernel"""
    from . import isp_algos
    unknown = set(baseline) - {'gain', 'sigma', 'wp_bl', 'd', 'eps'}
    if unknown or not {'gain', 'sigma', 'wp_bl'} <= set(baseline):
        raise PnnpError(f'evaluate(baseline=...) takes gain, sigma, wp_bl and optionally d, eps; got {sorted(baseline)}')
    if ratio is None:
        raise PnnpError('evaluate(baseline=...) needs the ratio: the frame is brought back to DN with wp_bl / ratio')
    wp_bl = float(baseline['wp_bl'])
    with torch.no_grad():
        x = imgs_lr.contiguous().float()
        # one rule however the ratio arrives: a float32 value on the device, scale = float32(wp_bl) / float32(ratio) as a float32 division
        # (a device ratio stays on the device: nothing here synchronises)
        r = torch.as_tensor(ratio).detach().reshape(-1)[:1].to(device=x.device, dtype=torch.float32)
        scale = torch.full_like(r, wp_bl) if ori else torch.full_like(r, wp_bl) / r
        base = isp_algos.vst_denoise(x, baseline['gain'], baseline['sigma'], d=baseline.get('d', 7), eps=baseline.get('eps', 1.0), scale=scale, layout='chw')
        if ori:
            base = base * r
        base = base.clamp(0, 1)
        m = quality_assess(base, imgs_hr)
    return dict(base=base, psnr_base=m[0], ssim_base=m[1])


def _evaluate(net, imgs_lr, imgs_hr, ratio, ori, brightness_correct, epoch, corrector, with_lr, render, tiles):
    if not imgs_lr.is_cuda or not imgs_hr.is_cuda:
        raise PnnpError('evaluate needs CUDA tensors (pnnp_amd has no CPU path)')
    if imgs_lr.dim() != 4 or imgs_lr.shape[0] != 1:
        raise PnnpError('evaluate expects one frame per call: [1,C,H,W] (DataLoader batch_size 1, trainer_SID.py:52)')
    with torch.no_grad():
        lr_in = imgs_lr.contiguous().float()
        _, Cc, H, W = lr_in.shape
        pad = 4 if W % 16 != 0 else 0                         # :221 -- the reference tests the width only
        eng = getattr(net, 'engine', None)
        res = bool(getattr(net, 'res', False))
        if tiles is not None:
            if ori and ratio is None:
                raise PnnpError('ori=True needs the ratio (trainer_SID.py:231-233)')
            r_dev = ratio.reshape(-1)[:1].float().contiguous() if (ori and torch.is_tensor(ratio) and ratio.is_cuda) else None
            r = 1.0 if (not ori or r_dev is not None) else float(torch.as_tensor(ratio).reshape(-1)[0])
            dn = _forward_tiled(net, lr_in, ratio=r_dev if r_dev is not None else r, clamp=True,
                                **{'base': 64, 'tile_batch': None, **tiles})
            if dn.shape != lr_in.shape:
                raise PnnpError(f'evaluate: the network returns {tuple(dn.shape)} for a {tuple(lr_in.shape)} frame')
            # the clamped (x ratio) input frame: the tail kernel on the frame itself, its second output not asked for
            lr = torch.empty_like(lr_in)
            _lib.check(_lib.lib().pnnp_eval_post_f32(_lib.ptr(lr_in), _lib.ptr(lr_in), _lib.ptr(lr), _lib.ptr(None), Cc, H, W, H, W, 0,
                                                     C.c_float(r), _lib.ptr(r_dev), 0, _lib.stream()), 'eval_post')
            return _evaluate_tail(dn, lr, imgs_hr, brightness_correct, epoch, corrector, with_lr, render)
        if eng is not None and hasattr(eng, 'forward'):
            # the reflection is folded into the layout pass the input goes through anyway (no F.pad kernel, no padded copy); a `res` network
            # runs without its input residual, which the tail kernel adds after the crop
            out = eng.forward(lr_in, False, reflect_pad=pad, add_residual=not res)
            add_res = res
        else:
            out = net(F.pad(lr_in, (4, 4, 4, 4), mode='reflect')) if pad else net(lr_in)
            add_res = False
        if ori and ratio is None:
            raise PnnpError('ori=True needs the ratio (trainer_SID.py:231-233)')
        # (one frame per call: one scalar; a device tensor stays on the device -- nothing here synchronises)
        r_dev = ratio.reshape(-1)[:1].float().contiguous() if (ori and torch.is_tensor(ratio) and ratio.is_cuda) else None
        r = 1.0 if (not ori or r_dev is not None) else float(torch.as_tensor(ratio).reshape(-1)[0])
        # crop, residual, x ratio and both clamps (:226-235) in one pass
        out = out.contiguous()
        dn = torch.empty_like(lr_in); lr = torch.empty_like(lr_in)
        _lib.check(_lib.lib().pnnp_eval_post_f32(_lib.ptr(out), _lib.ptr(lr_in), _lib.ptr(dn), _lib.ptr(lr), Cc, H, W, out.shape[-2], out.shape[-1], pad,
                                                 C.c_float(r), _lib.ptr(r_dev), int(add_res), _lib.stream()), 'eval_post')
        return _evaluate_tail(dn, lr, imgs_hr, brightness_correct, epoch, corrector, with_lr, render)


def _evaluate_tail(dn, lr, imgs_hr, brightness_correct, epoch, corrector, with_lr, render):
    """what follows the clamps in one eval iteration (trainer_SID.py:238-255): IlluminanceCorrect, the metrics, ``render=``"""
    if brightness_correct and epoch < 0:
        dn = (corrector or IlluminanceCorrect())(dn.contiguous(), imgs_hr)
    m_dn = quality_assess(dn, imgs_hr)
    m_lr = quality_assess(lr, imgs_hr) if with_lr else torch.full((2,), float('nan'), device=dn.device)
    res = dict(dn=dn, lr=lr, metrics=torch.cat([m_dn, m_lr]))
    if render is not None:
        res.update(_render(render, lr, dn, imgs_hr))
    return res


def _render(render, lr, dn, hr):
    """the ``render=`` part of ``evaluate``: three launches of the render kernel, two of the PSNR / SSIM kernel"""
    from . import process
    if lr.shape[1] != 4:
        raise PnnpError('evaluate(render=...) needs packed RGBG frames [1,4,H,W]')
    rows = render.get('rows')
    if rows is None:
        rows = process.isp_rows(render['wb'], render['ccm'], 1, lr.device)
    bgr = bool(render.get('bgr', False))
    full = bool(render.get('full', False))                     # the full-resolution render (csrc/demosaic.hip) instead of the binned one
    f, b = {}, {}
    for k, t in (('lr', lr), ('dn', dn), ('hr', hr)):
        f[k], u8 = process.fastisp_render(t, rows, f32=True, u8=True, bgr=bgr) if full else process.isp_render(t, rows, f32=True, u8=True, bgr=bgr)
        b[k] = u8[0]
    return dict(rgb=b, metrics_rgb=torch.cat([quality_assess(f['dn'], f['hr']), quality_assess(f['lr'], f['hr'])]))


class AverageMeter:
    """utils/utils.py AverageMeter as far as the eval log needs it."""

    def __init__(self):
        self.sum, self.count = 0.0, 0

    def update(self, v):
        self.sum += float(v); self.count += 1

    @property
    def avg(self):
        return self.sum / self.count if self.count else 0.0


class EvalLoop:
    """Accumulates what `SID_Trainer.eval` reports over a dataset: `metrics` (name -> [PSNR, SSIM], the content of
    metrics.pkl) and the log line of trainer_SID.py:309-312."""

    def __init__(self, net, ori=False, brightness_correct=True, tiles=None, precision=None, baseline=None):
        """``tiles``: as in ``evaluate`` (every frame of the dataset runs in overlapping tiles); None: whole frames.  ``precision``: as in ``evaluate``,
        for every step (the switch is set and restored per step: with another precision than the engine's own, set it on the engine once instead).
        ``baseline``: as in ``evaluate``, for every step; the log then gains a line with the baseline's averages (None: the log is unchanged)"""
        self.net, self.ori, self.brightness_correct, self.tiles, self.precision = net, ori, brightness_correct, tiles, precision
        self.baseline = baseline
        self.corrector = IlluminanceCorrect()
        self.reset()

    def reset(self):
        self.metrics = {}
        self.psnr, self.ssim = AverageMeter(), AverageMeter()
        self.psnr_lr, self.ssim_lr = AverageMeter(), AverageMeter()
        self.rgb_psnr, self.rgb_ssim = AverageMeter(), AverageMeter()                # RGB-domain meters: only steps that rendered count
        self.rgb_psnr_lr, self.rgb_ssim_lr = AverageMeter(), AverageMeter()
        self.psnr_base, self.ssim_base = AverageMeter(), AverageMeter()              # the non-learned baseline: only with ``baseline``
        self._pending = []
        self._pending_rgb = []
        self._pending_base = []

    def step(self, name, imgs_lr, imgs_hr, ratio=None, epoch=-1, render=None):
        out = evaluate(self.net, imgs_lr, imgs_hr, ratio=ratio, ori=self.ori, brightness_correct=self.brightness_correct,
                       epoch=epoch, corrector=self.corrector, render=render, tiles=self.tiles, precision=self.precision,
                       **({} if self.baseline is None else dict(baseline=self.baseline)))
        self._pending.append((name, out['metrics']))          # device tensors: one host sync per dataset, in finish()
        if self.baseline is not None:
            self._pending_base.append(torch.stack([out['psnr_base'], out['ssim_base']]))
        if render is not None:
            self._pending_rgb.append(out['metrics_rgb'])
        return out

    def finish(self, epoch=-1):
        """-> (metrics dict, log text).  Reads the accumulated device metrics once."""
        if self._pending:
            vals = torch.stack([m for _, m in self._pending]).cpu().tolist()
            for (name, _), (p_dn, s_dn, p_lr, s_lr) in zip(self._pending, vals):
                self.metrics[name] = [p_dn, s_dn]
                self.psnr.update(p_dn); self.ssim.update(s_dn)
                self.psnr_lr.update(p_lr); self.ssim_lr.update(s_lr)
            self._pending = []
        if self._pending_rgb:
            for p_dn, s_dn, p_lr, s_lr in torch.stack(self._pending_rgb).cpu().tolist():
                self.rgb_psnr.update(p_dn); self.rgb_ssim.update(s_dn)
                self.rgb_psnr_lr.update(p_lr); self.rgb_ssim_lr.update(s_lr)
            self._pending_rgb = []
        if self._pending_base:
            for p_b, s_b in torch.stack(self._pending_base).cpu().tolist():
                self.psnr_base.update(p_b); self.ssim_base.update(s_b)
            self._pending_base = []
        text = (f"Epoch {epoch}: PSNR={self.psnr.avg:.2f}\n"
                f"psnrs_lr={self.psnr_lr.avg:.2f}, psnrs_dn={self.psnr.avg:.2f}"
                f"\nssims_lr={self.ssim_lr.avg:.4f}, ssims_dn={self.ssim.avg:.4f}")
        if self.rgb_psnr.count:
            text += (f"\nrgb: psnrs_lr={self.rgb_psnr_lr.avg:.2f}, psnrs_dn={self.rgb_psnr.avg:.2f}, "
                     f"ssims_lr={self.rgb_ssim_lr.avg:.4f}, ssims_dn={self.rgb_ssim.avg:.4f}")
        if self.psnr_base.count:
            text += f"\nbaseline (VST + guided filter): psnrs_base={self.psnr_base.avg:.2f}, ssims_base={self.ssim_base.avg:.4f}"
        return self.metrics, text

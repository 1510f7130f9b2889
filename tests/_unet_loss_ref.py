"""float64 restatement of Unet_Loss (losses/base_loss.py:33-107) and of what csrc/unet_loss.hip computes around it, written from the formulas.

    low  = clamp(pred * ratio_b, 0, 1) if clamp_pred else pred * ratio_b          (the product is the trainer's own float32 line, taken as the input)
    high = clamp(hr, 0, 1) if clamp_target else hr
    d_l  = pool^l(low) - pool^l(high),   pool = AvgPool2d(2, 2),   l = 0 .. 3 (only l = 0 without the pyramid)
    t_l  = mean f(d_l),   f = |.| or sqrt(.^2 + 1e-6)
    recon = sum_l lam_l t_l / sum_l lam_l,   lam = 1, 1/2, 1/4, 1/8
    edge  = mean over B, H, W of | |ux| - |vx| | + | |uy| - |vy| |,   u = Sobel * S_low, v = Sobel * S_high (zero padding 1), S = the channel sum
    total = recon + grad * edge

Two gradients of ``total`` with respect to pred, which tests/test_host_unet_loss.py compares:

    closed form:  inv_n ratio_b grad_weight [0 <= p <= 1] sum_l (lam_l / 1.875) f'(d_l[block_l(y, x)]),  inv_n = 1 / (B C H W), because three
                  AvgPool2d(2, 2) partition a plane into nested 2x2, 4x4, 8x8 blocks and the 1 / 4^l of the pooling cancels the level's element count;
                  edge: (grad / (B H W)) sum_k Sobel[k] r[q - k + 1], r = sign(|u| - |v|) sign(u), for every channel, through the same mask and factors
    autograd:     torch's own, over avg_pool2d / conv2d

For the L1 family the closed form is an integer times a coefficient; ``k`` (8 s0 + 4 s1 + 2 s2 + s3, or 15 s0 without the pyramid) and ``ks`` (the edge
term's integer in [-8, 8]) are returned so that a float32 result can be compared exactly, and ``fragile`` marks the elements where a float32 rounding may
flip a sign: some |d_l|, or (edge) some | |u| - |v| | or |u| within the 3x3 neighbourhood, below 1e-6."""
import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-6
LAM = (1.0, 0.5, 0.25, 0.125)
SOBEL = torch.tensor([[-1., -2., -1.], [0., 0., 0.], [1., 2., 1.]], dtype=torch.float64)
FRAGILE = 1e-6


def _f(d, charbonnier):
    return torch.sqrt(d * d + EPS) if charbonnier else d.abs()


def _df(d, charbonnier):
    return d / torch.sqrt(d * d + EPS) if charbonnier else torch.sign(d)


def _up(x, l):
    return x.repeat_interleave(2 ** l, dim=2).repeat_interleave(2 ** l, dim=3)


def _inputs(pred, hr, scale):
    pred, hr = torch.as_tensor(pred), torch.as_tensor(hr)
    p = pred.float()
    if scale is not None:
        p = p * torch.as_tensor(scale).float().view(-1, 1, 1, 1)          # float32, as `pred = pred * ratio` (trainer_SID.py:97-98)
    return p.double(), hr.double(), (torch.as_tensor(scale).double().view(-1, 1, 1, 1) if scale is not None else 1.0)


def _edges(S):
    k = SOBEL.view(1, 1, 3, 3)
    return F.conv2d(S, k, padding=1), F.conv2d(S, k.transpose(2, 3), padding=1)


def _forward(p, hr, charbonnier, pyramid, grad, clamp_pred, clamp_target, recon):
    """-> total, terms [5], with torch ops only (differentiable in p)"""
    low = p.clamp(0, 1) if clamp_pred else p
    high = hr.clamp(0, 1) if clamp_target else hr
    terms = [p.new_zeros(()) for _ in range(5)]
    total = p.new_zeros(())
    if recon:
        lo, hi = low, high
        for l in range(4 if pyramid else 1):
            if l:
                lo, hi = F.avg_pool2d(lo, 2, 2), F.avg_pool2d(hi, 2, 2)
            terms[l] = _f(lo - hi, charbonnier).mean()
        total = sum(LAM[l] * terms[l] for l in range(4)) / sum(LAM) if pyramid else terms[0]
    if grad > 0:
        (ux, uy), (vx, vy) = _edges(low.sum(1, keepdim=True)), _edges(high.sum(1, keepdim=True))
        terms[4] = ((ux.abs() - vx.abs()).abs() + (uy.abs() - vy.abs()).abs()).mean()
        total = total + grad * terms[4]
    return total, torch.stack(terms)


def autograd(pred, hr, charbonnier=False, pyramid=False, grad=0.0, scale=None, clamp_pred=True, clamp_target=False, grad_weight=1.0, recon=True):
    """-> dict(loss, terms, grad): torch's float64 autograd"""
    p, hr, sc = _inputs(pred, hr, scale)
    p.requires_grad_(True)
    total, terms = _forward(p, hr, charbonnier, pyramid, grad, clamp_pred, clamp_target, recon)
    total.backward()
    return dict(loss=float(total.detach()), terms=terms.detach().numpy(), grad=(p.grad * sc * grad_weight).numpy())


def closed_form(pred, hr, charbonnier=False, pyramid=False, grad=0.0, scale=None, clamp_pred=True, clamp_target=False, grad_weight=1.0, recon=True):
    """-> dict(loss, terms, sse [B], grad, k, ks, mask, fragile, coef [B], coef_edge [B]): the formulas of the module docstring"""
    p, hr, sc = _inputs(pred, hr, scale)
    B, C, H, W = p.shape
    with torch.no_grad():
        total, terms = _forward(p, hr, charbonnier, pyramid, grad, clamp_pred, clamp_target, recon)
        low = p.clamp(0, 1) if clamp_pred else p
        high = hr.clamp(0, 1) if clamp_target else hr
        mask = ((p >= 0) & (p <= 1)) if clamp_pred else torch.ones_like(p, dtype=torch.bool)
        sse = ((low.clamp(0, 1) - high.clamp(0, 1)) ** 2).sum(dim=(1, 2, 3))
        ones = torch.ones(B, 1, 1, 1, dtype=torch.float64)
        coef = ones * sc * grad_weight / (B * C * H * W)
        coef_edge = ones * sc * grad_weight * grad / (B * H * W)
        deriv = torch.zeros_like(p)
        k = torch.zeros_like(p)
        fragile = torch.zeros_like(p, dtype=torch.bool)
        if recon:
            lo, hi = low, high
            for l in range(4 if pyramid else 1):
                if l:
                    lo, hi = F.avg_pool2d(lo, 2, 2), F.avg_pool2d(hi, 2, 2)
                d = lo - hi
                w = LAM[l] / sum(LAM) if pyramid else 1.0
                deriv += w * _up(_df(d, charbonnier), l)
                k += (2 ** (3 - l) if pyramid else 15) * _up(torch.sign(d), l)
                fragile |= _up(d.abs() < FRAGILE, l)
        g = coef * deriv
        ks = torch.zeros(B, 1, H, W, dtype=torch.float64)
        if grad > 0:
            kx = SOBEL.view(1, 1, 3, 3)
            S_lo, S_hi = low.sum(1, keepdim=True), high.sum(1, keepdim=True)
            near = torch.zeros(B, 1, H, W, dtype=torch.bool)
            for kern, (u, v) in ((kx, (_edges(S_lo)[0], _edges(S_hi)[0])), (kx.transpose(2, 3), (_edges(S_lo)[1], _edges(S_hi)[1]))):
                e = u.abs() - v.abs()
                r = torch.sign(e) * torch.sign(u)
                ks += F.conv_transpose2d(r, kern, padding=1)           # dS[q] = sum_k K[k] r[q - k + 1]
                near |= (e.abs() < FRAGILE) | (u.abs() < FRAGILE)
            fragile |= F.max_pool2d(near.double(), 3, 1, 1).bool()
            g = g + coef_edge * ks
        g = g * mask
    return dict(loss=float(total), terms=terms.numpy(), sse=sse.numpy(), grad=g.numpy(), k=k.numpy().astype(np.int64), ks=ks.numpy().astype(np.int64),
                mask=mask.numpy(), fragile=fragile.numpy(), coef=coef.numpy().reshape(B), coef_edge=coef_edge.numpy().reshape(B))


def l1_family_expected(ref, grad_weight=1.0, scale=None, grad=0.0, pyramid=False):
    """The float32 gradient the kernel must produce for an L1-family case, from the restatement's integers and the kernel's documented float32
    coefficient chain: k * ((inv_n * ratio * grad_weight) [* (1 / 15) under the pyramid]) + ks * (inv_bhw * ratio * grad_weight * grad), masked."""
    B, C, H, W = ref['k'].shape
    f = np.float32
    sc = np.ones(B, f) if scale is None else np.asarray(scale, f).reshape(B)
    gsc = (f(1.0) / (f(B) * f(C) * f(H) * f(W))) * sc * f(grad_weight)
    if pyramid:
        main = ref['k'].astype(f) * (gsc * (f(1.0) / f(15.0))).reshape(B, 1, 1, 1)
    else:
        main = (ref['k'] // 15).astype(f) * gsc.reshape(B, 1, 1, 1)
    out = main
    if grad > 0:
        ce = (f(1.0) / (f(B) * f(H) * f(W))) * sc * f(grad_weight) * f(grad)
        out = main + ref['ks'].astype(f) * ce.reshape(B, 1, 1, 1)
    return np.where(ref['mask'], out, f(0)).astype(f)

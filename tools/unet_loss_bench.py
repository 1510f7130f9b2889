"""The Unet_Loss kernels (csrc/unet_loss.hip) against the L1 kernel they sit beside and against the torch-op composition they replace:

    python tools/unet_loss_bench.py [--out profiles/r7/unet_loss.txt] [--reps 25] [--inner 10] [--step-reps 7]

Workload: 16 crops of 4x512x512 (bench.py's step), gradient written NHWC with 8 channels as the step's backward takes it.  Part 1, the loss
pass alone, every form in ONE process, timed with device events around `inner` back-to-back calls, alternated round by round after warm-up
rounds; us per call, median [min .. max]:
  * l1_clamp:  ops.l1_clamp_loss, the parent's kernel + finish on the same tensors;
  * unet_loss: ops.unet_loss with every option off (the same arithmetic), Charbonnier, pyramid, Charbonnier + pyramid -- the same bytes as
    l1_clamp (read pred and hr once, write the gradient once), so the ratio is the cost of the in-block pooling and the arithmetic;
    then L1 + 0.5 x the Sobel edge term (two more launches that read pred and hr again and read-modify-write the gradient) and the edge
    term alone (recon = 0: a memset of the gradient instead of the main kernel);
  * the pyramid pass without a gradient store (n x 8 B), with the gradient as NCHW rows (n x 12 B) and as NHWC with 4 channels (n x 12 B):
    what the arithmetic and the exchange cost, and what the NHWC store pattern costs;
  * composition: the reference's lines (losses/base_loss.py) as torch ops + autograd on the device, pred.clamp(0, 1) in front, gradient
    with respect to pred in NCHW (the layout change to NHWC the step needs is NOT counted).
Traffic is counted from the shape: 8 B read per element, 4 B x 8 / 4 written per element for the padded NHWC gradient.
Part 2, the whole train step (UNet nf = 32, the bench.py configuration without its noise sampler: a fixed noisy batch) with loss=None and
with each option, alternated in one process, ms per step."""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch

from pnnp_amd import losses, ops


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / inner


def composition(pred, hr, charbonnier, pyramid, grad):
    """the reference's own lines as tensor ops: Unet_Loss(charbonnier)(pred.clamp(0, 1), hr, pyramid) [+ grad * grad_loss], then backward()"""
    p = pred.detach().requires_grad_(True)
    low = p.clamp(0, 1)
    f = (lambda a, b: torch.sqrt((a - b) * (a - b) + 1e-6).mean()) if charbonnier else torch.nn.functional.l1_loss
    if pyramid:
        loss = losses.Pyramid_Loss([low] + losses.Pyramid_Sample(low, 8), [hr] + losses.Pyramid_Sample(hr, 8), loss_fn=f, rate=0.5, norm=True)
    else:
        loss = f(low, hr)
    if grad > 0:
        loss = loss + grad * torch.mean(torch.abs(losses.gradient(low, 'x') - losses.gradient(hr, 'x')) + torch.abs(losses.gradient(low, 'y') - losses.gradient(hr, 'y')))
    loss.backward()
    return loss, p.grad


def alternate(forms, warmup, reps, inner):
    t = {n: [] for n, _ in forms}
    for r in range(warmup + reps):
        for n, fn in forms:
            us = timed(fn, inner)
            if r >= warmup:
                t[n].append(us)
    return {n: np.array(v) for n, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'r7', 'unet_loss.txt'))
    ap.add_argument('--reps', type=int, default=25)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--inner', type=int, default=10)
    ap.add_argument('--step-reps', type=int, default=7)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--nf', type=int, default=32)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'this benchmark needs the GPU'
    B, Cc, S, Cp = a.batch, 4, a.size, 8
    g = torch.Generator(device='cuda').manual_seed(0)
    pred = torch.rand(B, Cc, S, S, device='cuda', generator=g) * 1.4 - 0.2
    hr = torch.rand(B, Cc, S, S, device='cuda', generator=g)
    g8 = torch.empty(B, S, S, Cp, device='cuda')
    lo, tm = torch.empty(1 + B, device='cuda'), torch.empty(5, device='cuda')
    ws = torch.empty(ops.unet_loss_workspace_floats(B), device='cuda')
    n = pred.numel()
    nbytes = n * 8 + g8.numel() * 4
    lines = [f'Unet_Loss, {B} crops of {Cc}x{S}x{S}, gradient NHWC with {Cp} channels: {nbytes / 1e6:.1f} MB algorithmic for the one-pass forms; us per call, median '
             f'[min .. max] of {a.reps} alternated rounds of {a.inner} back-to-back calls after {a.warmup} warm-up rounds; device {torch.cuda.get_device_name(0)}']
    modes = [('unet_loss off', dict()), ('unet_loss charbonnier', dict(charbonnier=True)), ('unet_loss pyramid', dict(pyramid=True)),
             ('unet_loss charb+pyramid', dict(charbonnier=True, pyramid=True)), ('unet_loss L1+0.5 edge', dict(grad=0.5)),
             ('unet_loss edge alone', dict(grad=1.0, recon=False))]
    forms = [('l1_clamp (parent)', lambda: ops.l1_clamp_loss(pred, hr, g8, lo, ws))]
    for name, kw in modes:
        forms.append((name, (lambda kw: lambda: ops.unet_loss(pred, hr, g8, lo, ws, terms=tm, **kw))(kw)))
    # where the pyramid's time goes: the same pass without a gradient store, and with the gradient in NCHW (full-width rows) instead of NHWC
    gn = torch.empty(B, Cc, S, S, device='cuda')
    g4 = torch.empty(B, S, S, 4, device='cuda')
    for name, kw, nhwc, nchw in (('off, no gradient', dict(), None, None), ('pyramid, no gradient', dict(pyramid=True), None, None),
                                 ('pyramid, NCHW gradient', dict(pyramid=True), None, gn), ('pyramid, NHWC 4 channels', dict(pyramid=True), g4, None),
                                 ('charb+pyramid, no gradient', dict(charbonnier=True, pyramid=True), None, None)):
        forms.append((name, (lambda kw, nhwc, nchw: lambda: ops.unet_loss(pred, hr, nhwc, lo, ws, terms=tm, grad_nchw=nchw, **kw))(kw, nhwc, nchw)))
    comps = [('composition L1', (False, False, 0.0)), ('composition charb+pyramid', (True, True, 0.0)), ('composition L1+0.5 edge', (False, False, 0.5))]
    for name, args in comps:
        forms.append((name, (lambda args: lambda: composition(pred, hr, *args))(args)))
    t = alternate(forms, a.warmup, a.reps, a.inner)
    base = float(np.median(t['l1_clamp (parent)']))
    for name, _ in forms:
        v = t[name]
        rate = f'{nbytes / np.median(v) / 1e6:6.2f} TB/s of the one-pass bytes' if name.startswith(('l1_clamp', 'unet_loss')) and 'edge' not in name else ''
        lines.append(f'    {name:28s} {np.median(v):9.1f} [{v.min():9.1f} .. {v.max():9.1f}]   x {np.median(v) / base:5.2f} of l1_clamp   {rate}')
    # the kernel and the composition compute the same thing here
    ops.unet_loss(pred, hr, g8, lo, ws, terms=tm, charbonnier=True, pyramid=True)
    cl, cg = composition(pred, hr, True, True, 0.0)
    gk = g8[..., :Cc].permute(0, 3, 1, 2)
    lines.append(f'    charb+pyramid, kernel against composition on this data: loss {float(lo[0]):.8f} / {float(cl.detach()):.8f}, largest gradient difference '
                 f'{float((gk - cg).abs().max()):.3e} of a largest element {float(cg.abs().max()):.3e}')
    del cl, cg, gk
    torch.cuda.empty_cache()
    # ------------------------------------------------------------------ part 2: the whole step
    from pnnp_amd.archs import UNetSeeInDark, initialize_weights
    from pnnp_amd.trainer import HipTrainStep
    torch.manual_seed(0)
    net = UNetSeeInDark(dict(nframes=1, res=False, nf=a.nf, in_nc=4, out_nc=4))
    initialize_weights(net)
    net = net.cuda()
    noisy = (hr + 0.05 * torch.randn(hr.shape, device='cuda', generator=g)).clamp(0, 1)
    steps = [('step loss=None', None), ('step charbonnier', dict(charbonnier=True)), ('step pyramid', dict(pyramid=True)),
             ('step charb+pyramid', dict(charbonnier=True, pyramid=True)), ('step L1+0.5 edge', dict(grad=0.5))]
    sforms = []
    for name, kw in steps:
        ts = HipTrainStep(net, lr=0.0, clip=2, range_every=0, loss=kw)           # lr 0: every form steps on the same weights
        sforms.append((name, (lambda ts: lambda: ts.step(hr, noisy=noisy))(ts)))
    st = alternate(sforms, 2, a.step_reps, 2)
    sbase = float(np.median(st['step loss=None']))
    lines.append(f'whole train step, UNet nf = {a.nf}, {B} crops of {S}x{S}, fixed noisy batch, ms per step, median [min .. max] of {a.step_reps} alternated rounds of 2 '
                 f'steps after 2 warm-up rounds:')
    for name, _ in sforms:
        v = st[name] / 1e3
        lines.append(f'    {name:28s} {np.median(v):9.3f} [{v.min():9.3f} .. {v.max():9.3f}]   {(np.median(v) - sbase / 1e3) * 1e3:+8.1f} us against loss=None')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write(text)


if __name__ == '__main__':
    main()

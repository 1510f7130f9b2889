"""Restatements of the distribution losses the kernels of csrc/ddl.hip implement (reference: utils/kld_div.py:21-78), pinned to the
reference's own outputs by tests/test_host_ddl.py (tests/golden/ddl.npz).

``ecdf`` / ``cdf_loss`` / ``kld``: sort-based, torch, any device and dtype, differentiable by autograd -- the definition.
``ecdf_one_pass``: numpy float32, the formulation the kernels use (a count, a minimum and a maximum per gap between points, then
three scans); bit for bit the same cdf.  ``ecdf_grad_one_pass``: the gradient the backward kernel scatters."""
import numpy as np
import torch


def ecdf(data, x):
    """Empirical CDF of ``data`` at ``x``, linearly interpolated between neighbouring order statistics."""
    s, _ = torch.sort(data.reshape(-1))
    pad = torch.cat([s.new_full((1,), -float('inf')), s])
    xc = torch.clamp(x, s[0], s[-1])
    idx = torch.searchsorted(pad.detach(), xc.detach())       # first padded position whose value is >= the point
    # (the upper neighbour is gathered twice, as the reference does: autograd then accumulates its two shares in the reference's order)
    delta = (pad[idx] - xc) / (pad[idx] - pad[idx - 1])
    # (a 0-dim tensor, not a Python number: ATen's GPU kernels multiply by the reciprocal of a host scalar, which is not the CPU's quotient)
    return ((idx - delta) - 1) / s.new_tensor(float(s.numel() - 1))


def pdf_of(cdf):
    return torch.abs(cdf[:-1] - cdf[1:])


def cdf_loss(output, gt, x):
    return torch.mean(torch.abs(ecdf(output, x) - ecdf(gt, x)))


def kld(output, gt, x):
    q = pdf_of(ecdf(output, x)).clamp_min(1e-9)
    p = pdf_of(ecdf(gt, x)).clamp_min(1e-9)
    top = torch.maximum(q.sum(), p.sum()).detach()
    q, p = q / top, p / top
    return torch.sum(p * (torch.log(p) - torch.log(q)))


LOSSES = {'cdf': cdf_loss, 'kld': kld}


def loss_and_grads(kind, output, gt, x, dtype=torch.float32):
    """CPU autograd of the restatement in ``dtype``: (loss, d/d output, d/d gt) as float64 numpy"""
    o = torch.as_tensor(output).detach().cpu().to(dtype).reshape(-1).clone().requires_grad_(True)
    g = torch.as_tensor(gt).detach().cpu().to(dtype).reshape(-1).clone().requires_grad_(True)
    xx = torch.as_tensor(x).detach().cpu().to(dtype)
    loss = LOSSES[kind](o, g, xx)
    loss.backward()
    return float(loss.detach()), o.grad.double().numpy(), g.grad.double().numpy()


def one_pass_tables(d, x):
    """numpy float32: the clamped points and, per bin j(d) = #{k : xc[k] <= d}, the count and the LOWEST index of the minimum and of the
    maximum (-1: empty bin)"""
    d = np.ascontiguousarray(d, np.float32).reshape(-1)
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    K = x.size
    amin, amax = int(np.argmin(d)), int(np.argmax(d))         # first occurrences
    xc = np.clip(x, d[amin], d[amax])
    j = np.searchsorted(xc, d, side='right')
    cnt = np.bincount(j, minlength=K + 1)
    order = np.lexsort((np.arange(d.size), d, j))              # by bin, then value, then index
    first = np.full(K + 1, -1, np.int64); last = np.full(K + 1, -1, np.int64)
    starts = np.concatenate([[0], np.cumsum(cnt)])
    for b in range(K + 1):
        if cnt[b]:
            seg = order[starts[b]:starts[b + 1]]
            first[b] = seg[0]
            last[b] = seg[np.searchsorted(d[seg], d[seg[-1]], side='left')]       # lowest index among the bin's maxima
    return d, x, xc, cnt, first, last, amin, amax


def ecdf_one_pass(d, x):
    """-> cdf float32 [K], arg hi [K], arg lo [K] (-1: none), arg min, arg max"""
    d, x, xc, cnt, first, last, amin, amax = one_pass_tables(d, x)
    K = x.size
    inf = np.float32(np.inf)
    bmin = np.where(first >= 0, d[np.maximum(first, 0)], inf).astype(np.float32)
    bmax = np.where(last >= 0, d[np.maximum(last, 0)], -inf).astype(np.float32)
    c = np.cumsum(cnt)[:K]
    # running maximum from the left over bins <= k (ties: the earlier bin holds smaller values, so the later non-empty bin wins)
    arg_lo = np.full(K, -1, np.int64); arg_hi = np.full(K, -1, np.int64)
    run = -1
    for k in range(K):
        if last[k] >= 0:
            run = last[k]
        arg_lo[k] = run
    run = -1
    for k in range(K, 0, -1):                                  # running minimum from the right over bins > k - 1
        if first[k] >= 0:
            run = first[k]
        arg_hi[k - 1] = run
    lo = np.where(arg_lo >= 0, d[np.maximum(arg_lo, 0)], -inf).astype(np.float32)
    hi = d[arg_hi]
    with np.errstate(all='ignore'):
        w = (hi - xc).astype(np.float32)
        diff = (hi - lo).astype(np.float32)
        delta = (w / diff).astype(np.float32)
        cdf = (((c + 1).astype(np.float32) - delta).astype(np.float32) - np.float32(1)).astype(np.float32) / np.float32(d.size - 1)
    assert np.array_equal(np.maximum.accumulate(bmax)[:K], lo) and np.array_equal(np.minimum.accumulate(bmin[::-1])[::-1][1:], hi)
    return cdf.astype(np.float32), arg_hi, arg_lo, amin, amax


def ecdf_grad_one_pass(d, x, g):
    """float32 gradient of sum_k g[k] cdf[k] with respect to d, term by term like ATen (0 where lo = -inf)"""
    f = np.float32
    d = np.ascontiguousarray(d, f).reshape(-1)
    x = np.ascontiguousarray(x, f).reshape(-1)
    _, arg_hi, arg_lo, amin, amax = ecdf_one_pass(d, x)
    xc = np.clip(x, d[amin], d[amax])
    grad = np.zeros(d.size, np.float64)
    nm1 = f(d.size - 1)
    with np.errstate(all='ignore'):
        for k in range(x.size):
            hi = d[arg_hi[k]]
            lo = d[arg_lo[k]] if arg_lo[k] >= 0 else f(-np.inf)
            w, diff = f(hi - xc[k]), f(hi - lo)
            gd = f(-f(g[k]) / nm1)
            gw = f(gd / diff)
            gdiff = f(-gd * f(f(w / diff) / diff))
            grad[arg_hi[k]] += f(gw + gdiff)
            if arg_lo[k] >= 0:
                grad[arg_lo[k]] += -gdiff
            if x[k] < d[amin]:
                grad[amin] += -gw
            if x[k] > d[amax]:
                grad[amax] += -gw
    return grad.astype(f)

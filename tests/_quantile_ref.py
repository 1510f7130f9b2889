"""The sort-based restatement of ``torch.quantile(..., dim=-1, interpolation='linear')`` and of the reference's ``QuantileLoss``
(utils/kld_div.py:49-53) that the kernels of csrc/quantile.hip are tested against; tests/test_host_quantile.py pins it to the
reference's own outputs (tests/golden/quantile.npz).

    pos = q * float32(N - 1);  lo = floor(pos);  hi = ceil(pos);  w = pos - floor(pos)          (float32, lo / hi clamped into [0, N-1])
    value = w < 0.5 ? a + w (b - a) : b - (b - a) (1 - w)         a = s[lo], b = s[hi], s the row sorted ascending, unfused

``quantile`` / ``quantile_loss`` are torch code in any dtype (ranks and weights always by the float32 rule, then cast), so autograd
gives the float32 and the float64 gradients.  ``order_stats`` / ``grad_rule`` are numpy and apply the kernels' tie rule: among equal
values (-0.0 equals +0.0) the LOWEST index holds an order statistic and receives its gradient."""
import numpy as np
import torch


def ranks(q, n):
    """-> lo, hi (int64, clamped into [0, n-1]), w (float32): the float32 rank rule"""
    q = np.asarray(q, np.float32).reshape(-1)
    pos = q * np.float32(n - 1)
    fl = np.floor(pos)
    w = (pos - fl).astype(np.float32)
    lo = np.clip(np.nan_to_num(fl, nan=0.0), 0, n - 1).astype(np.int64)
    hi = np.clip(np.nan_to_num(np.ceil(pos), nan=0.0), 0, n - 1).astype(np.int64)
    return lo, hi, w


def quantile(data, q):
    """[K, *leading] like torch.quantile(data, q, dim=-1); ``data`` any float dtype, ``q`` float32"""
    n = data.shape[-1]
    lo, hi, w = ranks(q.detach().cpu().numpy(), n)
    s, _ = torch.sort(data, dim=-1)
    a, b = s[..., torch.from_numpy(lo).to(data.device)], s[..., torch.from_numpy(hi).to(data.device)]
    w = torch.from_numpy(w).to(device=data.device, dtype=data.dtype)
    d = b - a
    v = torch.where(w < 0.5, a + w * d, b - d * (1 - w))
    return v.movedim(-1, 0)


def quantile_loss(output, gt, q):
    return (quantile(output, q) - quantile(gt, q)).abs().mean()


def loss_and_grads(o, g, q, dtype):
    """(loss, grad_output, grad_gt) of the restatement in ``dtype`` on the CPU, as numpy"""
    a = torch.as_tensor(o).to(dtype).clone().requires_grad_(True)
    b = torch.as_tensor(g).to(dtype).clone().requires_grad_(True)
    loss = quantile_loss(a, b, torch.as_tensor(q))
    loss.backward()
    return loss.item(), a.grad.numpy(), b.grad.numpy()


def first_index_of_value(d):
    """for every element of a 1-D array: the lowest index that holds its value (-0.0 and +0.0 are one value)"""
    _, first, inv = np.unique(d + np.float32(0), return_index=True, return_inverse=True)
    return first[inv]


def order_stats(d, q):
    """-> s[lo], s[hi] (float32), arg lo, arg hi (int64, the lowest index of the value), w (float32) of a 1-D float32 array"""
    d = np.asarray(d, np.float32)
    lo, hi, w = ranks(q, d.size)
    order = np.argsort(d, kind='stable')
    first = first_index_of_value(d)
    return d[order[lo]], d[order[hi]], first[order[lo]], first[order[hi]], w


def value_from(a, b, w, dtype=np.float32):
    a, b, w = (np.asarray(t).astype(dtype) for t in (a, b, w))
    with np.errstate(invalid='ignore'):                        # infinite order statistics: NaN, as in the reference
        d = b - a
        return np.where(w < 0.5, a + w * d, b - d * (1 - w))


def grad_rule(d, q, g):
    """grad [N] of sum_k g[k] value[k] by the kernels' rule: g (1 - w) to arg lo, g w to arg hi (float32 products, summed in float64)"""
    _, _, alo, ahi, w = order_stats(d, q)
    g = np.asarray(g, np.float32)
    grad = np.zeros(np.asarray(d).size, np.float64)
    np.add.at(grad, alo, (g * (np.float32(1) - w)).astype(np.float64))
    np.add.at(grad, ahi, (g * w).astype(np.float64))
    return grad.astype(np.float32)

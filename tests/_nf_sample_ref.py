"""TEST INFRASTRUCTURE (CPU): ``NoiseFlow.sample`` restated with a dtype argument and a BatchNorm mode argument on the key layout of
``oracle/noiseflow_torch.py``, and differentiated with ``torch.autograd.grad`` -- the float64 reference of the sample backward
(tests/test_gpu_nf_sample_bwd.py).  Unlike the reference's ``Conv2d1x1`` inverse, which goes through ``.cpu()`` and cuts its own graph,
the 4x4 inverses here stay in the graph: the TRUE derivative.

BatchNorm modes:  'batch'    the statistics of the batch being sampled (``net.train()``), differentiated through;
                  'running'  the running buffers of the state dict (``net.eval()``);
                  a dict     {BatchNorm key prefix: (mean, biased var)}: those statistics as FIXED buffers (eval mode with matched buffers).
``batch_stats`` returns such a dict for an input, from a 'batch' run."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import noiseflow_torch as O


def _interp(table, iso):
    legal = np.asarray(O.LEGAL_ISO, np.float64)
    l = int(np.searchsorted(legal, iso, 'left')); r = int(np.searchsorted(legal, iso, 'right'))
    pl, pr = torch.exp(table[l]), torch.exp(table[r])
    if legal[r] - legal[l] != 0:
        return ((iso - legal[l]) * pr + (legal[r] - iso) * pl) / (legal[r] - legal[l])
    return pl


def _bn(x, sd, pre, mode, record):
    w, b = sd[pre + '.weight'], sd[pre + '.bias']
    if record is not None:
        record[pre] = (x.mean((0, 2, 3)).detach(), x.var((0, 2, 3), unbiased=False).detach())
    if mode == 'batch':
        return F.batch_norm(x, None, None, w, b, training=True, eps=O.BN_EPS)
    if mode == 'running':
        m, v = sd[pre + '.running_mean'], sd[pre + '.running_var']
    else:
        m, v = mode[pre]
    return F.batch_norm(x, m.to(x.dtype), v.to(x.dtype), w, b, training=False, eps=O.BN_EPS)


def _shift_and_log_scale(sd, k, z0, mode, record):
    p = f'model.{k}._shift_and_log_scale'
    h = F.relu(_bn(F.conv2d(z0, sd[p + '.conv2d_1.weight'], sd[p + '.conv2d_1.bias'], padding=1), sd, p + '.net.1', mode, record))
    h = F.relu(_bn(F.conv2d(h, sd[p + '.conv2d_2.weight'], sd[p + '.conv2d_2.bias']), sd, p + '.net.4', mode, record))
    h = F.pad(h, (1, 1, 1, 1, 0, 1), value=0.)
    ring = torch.ones(h.shape[-2:], dtype=h.dtype); ring[1:-1, 1:-1] = 0
    h = torch.cat([h[:, :4], (h[:, 4] + ring).unsqueeze(1)], 1)
    h = F.conv2d(h, sd[p + '.conv2d_3.weight'], sd[p + '.conv2d_3.bias'])
    h = h * torch.exp(sd[p + '.logs'] * 3)
    shift, ls = torch.split(h, 2, 1)
    return shift, sd[p + '.scale'] * torch.tanh(ls)


def _winv(sd, k, dt, like_oracle):
    m = torch.tril(torch.ones(4, 4, dtype=dt), -1)
    l = sd[f'model.{k}.l'] * m + torch.eye(4, dtype=dt)
    u = sd[f'model.{k}.u'] * m.t() + torch.diag(sd[f'model.{k}.sign_s'] * torch.exp(sd[f'model.{k}.log_s']))
    if like_oracle:                      # conv2d1x1.py:66-74: float64 inverses rounded to float32 (values only: this cuts the graph's precision, not the graph)
        return torch.matmul(torch.inverse(u.double()).to(dt), torch.matmul(torch.inverse(l.double()).to(dt), sd[f'model.{k}.p'].inverse()))
    return torch.inverse(u) @ torch.inverse(l) @ torch.inverse(sd[f'model.{k}.p'])


def sample(sd, clean, iso, z, mode='running', dtype=torch.float32, record=None):
    """The reversed chain on ``z`` (archs/noise_flow.py:173-188).  ``sd`` / ``clean`` / ``z`` are used in ``dtype`` as given."""
    iso = float(iso)
    x = z
    for k in range(17, -1, -1):
        if k in O.COUPLING_IDX:
            z0, z1 = x[:, :2], x[:, 2:]
            shift, ls = _shift_and_log_scale(sd, k, z0, mode, record)
            x = torch.cat([z0, (z1 - shift) * torch.exp(-ls)], 1)
        elif k in O.CONV_IDX:
            x = F.conv2d(x, _winv(sd, k, dtype, dtype == torch.float32).view(4, 4, 1, 1))
        elif k == 9:
            x = x * (torch.exp(_interp(sd['model.9.cam_param'], iso) * sd['model.9.gain_params']) * iso)
        else:
            cam = _interp(sd['model.0.cam_param'], iso)
            beta1 = torch.exp(sd['model.0.beta1'] * cam[0]); beta2 = torch.exp(sd['model.0.beta2'] * cam[1])
            gain = torch.exp(sd['model.0.gain'] * cam[2]) * iso
            x = x * torch.sqrt(beta1 * clean / gain + beta2)
    return x


def _cast(sd0, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd0.items()}


def batch_stats(sd0, clean, iso, z, dtype=torch.float64):
    """{BatchNorm prefix: (mean, biased variance)} of every coupling's two BatchNorm inputs for this very input, in ``dtype``."""
    record = {}
    with torch.no_grad():
        sample(_cast(sd0, dtype), clean.to(dtype), iso, z.to(dtype), 'batch', dtype, record)
    return record


def value_and_grads(sd0, clean, iso, z, cot, mode, dtype):
    """(sample, {key: d sum(sample * cot) / d key}) for every trainable key of ``oracle.noiseflow_torch.trainable`` and for 'z'.
    Runs on ONE thread: how torch splits a float32 convolution or sum over threads changes its roundings, a ReLU mask flips here and
    there, and the float32-vs-float64 error of a case (from which the tests take their bar) moved by up to 4x between 1 and 8 threads
    on one machine; on one thread it does not depend on how many cores the machine has (it still depends on the CPU's instruction set:
    (2,16,16) seed 2 gave 2.2e-5 on one machine and 1.8e-4 on another)."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return _value_and_grads(sd0, clean, iso, z, cot, mode, dtype)
    finally:
        torch.set_num_threads(threads)


def _value_and_grads(sd0, clean, iso, z, cot, mode, dtype):
    sd = _cast(sd0, dtype)
    leaves = {}
    for k in list(sd.keys()):
        if O.trainable(k):
            sd[k] = sd[k].clone().requires_grad_(True); leaves[k] = sd[k]
    zz = z.to(dtype).clone().requires_grad_(True)
    x = sample(sd, clean.to(dtype), iso, zz, mode, dtype)
    grads = torch.autograd.grad((x * cot.to(dtype)).sum(), list(leaves.values()) + [zz], allow_unused=True)
    out = {}
    for k, g in zip(list(leaves.keys()) + ['z'], grads):
        out[k] = torch.zeros_like(leaves[k] if k != 'z' else zz) if g is None else g
    return x.detach(), out


def layer_of(key):
    return key.split('.')[1] if key != 'z' else 'z'


def layer_max(ref):
    """{model.N (or 'z'): max |ref| over that layer's tensors}"""
    lay = {}
    for k, v in ref.items():
        lay[layer_of(k)] = max(lay.get(layer_of(k), 0.0), float(v.abs().max()))
    return lay


def worst_rel(got, ref):
    """Worst per-tensor max|got - ref| / max|ref| over the tensors that are not mathematically zero (max|ref| >= 1e-6 of their layer's)."""
    lay = layer_max(ref)
    worst = 0.0
    for k, r in ref.items():
        m = float(r.abs().max())
        if m < 1e-6 * lay[layer_of(k)]:
            continue
        worst = max(worst, float((got[k].double() - r.double()).abs().max()) / m)
    return worst


def check(got, ref64, r):
    """The bar: per tensor max|got - ref64| <= r max|ref64| + 1e-5 max|ref64 over the tensors of the same model.N|.  Returns the misses."""
    lay = layer_max(ref64)
    bad = []
    for k, ref in ref64.items():
        err = float((got[k].double() - ref).abs().max())
        tol = r * float(ref.abs().max()) + 1e-5 * lay[layer_of(k)]
        if not err <= tol:
            bad.append((k, err, tol))
    return bad

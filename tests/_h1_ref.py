"""Restatement of the fp16x1 ("h1") eval forward (csrc/conv_h1s.hip) in plain torch float64: what the kernels are checked against.

An operand tensor t with amax slot A is seen by the matrix cores as ``h1_round(t, A) = float16(t * 2^se) * 2^-se`` with
``se = h1_scale_exp(A)`` (csrc/h2.h pnnp_h2_scale_exp: the power of two that brings A into [2^14, 2^15)); products of two such values are
exact in the float32 accumulator, so a layer is the convolution of the ROUNDED operands, here summed in float64.  Everything is
device-agnostic torch (the host tests run it on the CPU; the GPU tests may hand it CUDA tensors: float64 matmuls, no library convolution).
Tensors are NCHW."""
import numpy as np
import torch


def h1_scale_exp(amax):
    """pnnp_h2_scale_exp on the float32 bit pattern of ``amax``: 0 for zero / subnormal / inf / NaN, else 141 - E, at most 127."""
    bits = int(np.array(amax, dtype=np.float64).astype(np.float32).view(np.uint32))
    E = (bits >> 23) & 0xff
    if E == 0 or E == 255:
        return 0
    return min(141 - E, 127)


def _amax(t):
    return float(t.detach().abs().max()) if t.numel() else 0.0


def h1_round(t, amax=None):
    """float64(float16(t * 2^se)) * 2^-se, se from ``amax`` (None: max |t|).  The scaled value passes through float32 first -- exact for the float32
    tensors the kernels read (a power-of-two scale), and what the engine's float32 activations are for a float64 emulation -- then rounds to
    fp16 once, to nearest even, subnormals kept."""
    se = h1_scale_exp(_amax(t) if amax is None else amax)
    return (t.double() * 2.0 ** se).float().half().double() * 2.0 ** -se


def conv64(x, w, bias=None, stride=1):
    """3x3 / pad 1 (or 1x1 / pad 0) convolution in float64 as one matmul per tap."""
    x, w = x.double(), w.double()
    k = w.shape[2]
    p = k // 2
    B, _, H, W = x.shape
    xp = torch.nn.functional.pad(x, (p, p, p, p))
    Ho, Wo = (H + stride - 1) // stride, (W + stride - 1) // stride
    out = torch.zeros((B, w.shape[0], Ho, Wo), dtype=torch.float64, device=x.device)
    for dy in range(k):
        for dx in range(k):
            out += torch.einsum('bchw,oc->bohw', xp[:, :, dy:dy + H:stride, dx:dx + W:stride], w[:, :, dy, dx])
    if bias is not None:
        out += bias.double().reshape(1, -1, 1, 1)
    return out


def act64(y, act):
    return torch.where(y > 0, y, 0.2 * y) if act == 1 else (y.clamp(min=0) if act == 2 else y)


def h1_conv(x1, x2, w, b, act, amax_x1=None, amax_x2=None, amax_w=None):
    """The float64 conv2d (3x3, pad 1) of the rounded operands + bias, activation 0 none / 1 LeakyReLU(0.2) / 2 ReLU.  Two input segments share ONE
    scale, taken from the larger of their slots."""
    a1 = _amax(x1) if amax_x1 is None else amax_x1
    x = x1
    if x2 is not None:
        a1 = max(a1, _amax(x2) if amax_x2 is None else amax_x2)
        x = torch.cat([x1, x2], 1)
    return act64(conv64(h1_round(x, a1), h1_round(w, amax_w), b), act)


def _convt64(x, w, b):
    """ConvTranspose2d(2, stride 2): y[b, o, 2 i + a, 2 j + c] = sum_k x[b, k, i, j] w[k, o, a, c] + bias"""
    B, _, H, W = x.shape
    y = torch.einsum('bkij,koac->boiajc', x.double(), w.double()).reshape(B, w.shape[1], 2 * H, 2 * W)
    return y + b.double().reshape(1, -1, 1, 1)


def _pool64(x):
    B, C, H, W = x.shape
    return x.reshape(B, C, H // 2, 2, W // 2, 2).amax(dim=(3, 5))


def h1_unet_forward(sd, x, h1_layers=(), res=False):
    """UNetSeeInDark in float64; the layers named in ``h1_layers`` (conv{i}_{j}: those an h1 eval plan marks 'h1*') round their operands as the
    kernels do, with amax taken from the activations computed HERE (a pooled map carries its full-resolution map's amax, as the engine's slot
    does); every other layer is exact.  ``h1_layers=()``: the exact float64 forward."""
    x = x.double()

    def c3(name, t, t2=None, amax=None):
        w, b = sd[name + '.weight'], sd[name + '.bias']
        if name in h1_layers:
            return h1_conv(t, t2, w, b, 1, amax_x1=amax)
        return act64(conv64(t if t2 is None else torch.cat([t, t2], 1), w, b), 1)

    def up(name, t):
        return _convt64(t, sd[name + '.weight'], sd[name + '.bias'])
    skips, cur, amax = [], x, None
    for i in range(1, 6):
        cur = c3(f'conv{i}_2', c3(f'conv{i}_1', cur, amax=amax))
        if i < 5:
            skips.append(cur)
            amax, cur = _amax(cur), _pool64(cur)
    for i in range(6, 10):
        cur = c3(f'conv{i}_2', c3(f'conv{i}_1', up(f'upv{i}', cur), skips[9 - i]))
    out = conv64(cur, sd['conv10_1.weight'], sd['conv10_1.bias'])
    return out + x if res else out


def h1_resunet_forward(sd, x, h1_layers=(), res=False):
    """ResUnet in float64 likewise; plan names conv_in, b{i}_0 / b{i}_1 (the two 3x3 convolutions of residual block conv{i}); the stride-2 pool
    layers, ConvTranspose2d, the 1x1 shortcuts and the head are never h1."""
    x = x.double()

    def c3(pname, wname, t, act):
        w = sd[wname]
        if pname in h1_layers:
            return h1_conv(t, None, w, sd.get(wname[:-6] + 'bias'), act)
        return act64(conv64(t, w, sd.get(wname[:-6] + 'bias')), act)

    def block(i, t):
        u = c3(f'b{i}_0', f'conv{i}.block.0.conv.conv.weight', t, 2)
        u = c3(f'b{i}_1', f'conv{i}.block.1.conv.conv.weight', u, 0)
        key = f'conv{i}.short_cut.0.conv.conv.weight'
        return u + (conv64(t, sd[key]) if key in sd else t)
    cur = c3('conv_in', 'conv_in.weight', x, 2)
    skips = []
    for i in range(1, 6):
        cur = block(i, cur)
        if i < 5:
            skips.append(cur)
            cur = conv64(cur, sd[f'pool{i}.conv.weight'], sd[f'pool{i}.conv.bias'], stride=2)
    for i in range(6, 10):
        cur = block(i, torch.cat([_convt64(cur, sd[f'upv{i}.weight'], sd[f'upv{i}.bias']), skips[9 - i]], 1))
    out = conv64(cur, sd['conv10.weight'], sd['conv10.bias'])
    return out + x if res else out

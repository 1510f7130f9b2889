"""Restatement of the fp16x1 ("h1") POINTWISE layers of an eval forward (csrc/gemm_h1s.hip) in plain torch float64, built on tests/_h1_ref.py:
ConvTranspose2d(k 2, s 2), the 1x1 convolution on one or two K segments and the stride-2 3x3 convolution see their operands as
``h1_round(t, amax)`` -- ONE fp16 rounding of the value scaled by its tensor's amax slot -- and sum exact products, here in float64.  The two K
segments of a 1x1 layer share ONE scale, taken from the LARGER of their slots (``scale_exps`` of the kernel).  ``rounded=False`` gives the plain
float64 layer.  The network forwards round at exactly the steps a plan marks 'h1*': the stride-1 3x3 layers (as tests/_h1_ref.py does) AND the
pointwise ones.  Tensors are NCHW; everything is device-agnostic torch."""
import torch

from _h1_ref import _amax, _convt64, _pool64, act64, conv64, h1_conv, h1_round


def h1_convt(x, w, b, amax_x=None, amax_w=None, rounded=True):
    """ConvTranspose2d(2, stride 2), w [Cin][Cout][2][2]: y[b, o, 2 i + a, 2 j + c] = sum_k x[b, k, i, j] w[k, o, a, c] + bias (no activation)."""
    if rounded:
        x, w = h1_round(x, amax_x), h1_round(w, amax_w)
    if b is None:
        b = torch.zeros(w.shape[1], dtype=torch.float64, device=w.device)
    return _convt64(x, w, b)


def h1_conv1x1(x1, x2, w, b, act, residual=None, amax_x1=None, amax_x2=None, amax_w=None, rounded=True):
    """1x1 convolution of cat([x1, x2]) (x2 may be None), w [Cout][C1 + C2][1][1]; + bias, + residual, then the activation."""
    x = x1 if x2 is None else torch.cat([x1, x2], 1)
    if rounded:
        a = _amax(x1) if amax_x1 is None else amax_x1
        if x2 is not None:
            a = max(a, _amax(x2) if amax_x2 is None else amax_x2)
        x, w = h1_round(x, a), h1_round(w, amax_w)
    y = conv64(x, w, b)
    if residual is not None:
        y = y + residual.double()
    return act64(y, act)


def h1_conv_s2(x, w, b, act, amax_x=None, amax_w=None, rounded=True):
    """3x3 / stride 2 / pad 1 convolution (even H and W), w [Cout][Cin][3][3]; + bias, activation."""
    if rounded:
        x, w = h1_round(x, amax_x), h1_round(w, amax_w)
    return act64(conv64(x, w, b, stride=2), act)


def h1pw_unet_forward(sd, x, h1_layers=(), res=False):
    """UNetSeeInDark in float64: conv{i}_{j} and upv{i} named in ``h1_layers`` round their operands as the kernels do (amax from the activations
    computed HERE; a pooled map carries its full-resolution map's amax, as the engine's slot does); every other layer is exact."""
    x = x.double()

    def c3(name, t, t2=None, amax=None):
        w, b = sd[name + '.weight'], sd[name + '.bias']
        if name in h1_layers:
            return h1_conv(t, t2, w, b, 1, amax_x1=amax)
        return act64(conv64(t if t2 is None else torch.cat([t, t2], 1), w, b), 1)

    def up(name, t):
        return h1_convt(t, sd[name + '.weight'], sd[name + '.bias'], rounded=name in h1_layers)
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


def h1pw_resunet_forward(sd, x, h1_layers=(), res=False):
    """ResUnet in float64 likewise; plan names conv_in, b{i}_0 / b{i}_1 (3x3), pool{i} (stride 2), upv{i} (ConvTranspose2d), sc{i} (the decoder
    blocks' 1x1 shortcut on cat([up, skip]): two K segments, one scale); the head is never h1."""
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
        if key not in sd:
            return u + t
        return u + h1_conv1x1(t, None, sd[key], None, 0, rounded=f'sc{i}' in h1_layers)          # (amax of the cat = the larger of the two slots)
    cur = c3('conv_in', 'conv_in.weight', x, 2)
    skips = []
    for i in range(1, 6):
        cur = block(i, cur)
        if i < 5:
            skips.append(cur)
            cur = h1_conv_s2(cur, sd[f'pool{i}.conv.weight'], sd[f'pool{i}.conv.bias'], 0, rounded=f'pool{i}' in h1_layers)
    for i in range(6, 10):
        up = h1_convt(cur, sd[f'upv{i}.weight'], sd[f'upv{i}.bias'], rounded=f'upv{i}' in h1_layers)
        cur = block(i, torch.cat([up, skips[9 - i]], 1))
    out = conv64(cur, sd['conv10.weight'], sd['conv10.bias'])
    return out + x if res else out

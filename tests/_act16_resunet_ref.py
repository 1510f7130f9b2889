"""Restatement of the fp16-STORAGE eval forward of ResUnet (ConvPolicy.h1_act16_res, Plan.act16) in plain torch float64, built on the layer emulations of
tests/_h1_ref.py and tests/_h1pw_ref.py: the fp16_all emulation (``h1pw_resunet_forward`` with every layer rounded) with ``store`` applied to every STORED
map -- t0, t1..t9, c1..c9, d1..d4, u6..u9, sc6..sc9: 31 maps.  A stored map is ``float16(float32(y))``: one round to nearest even, unscaled, subnormals kept,
not saturated.  Its consumer is the layer emulation, which rounds its input scaled by the tensor's own amax: for a tensor of fp16 values below 2^15 that
rounding is exact, which is how the kernels take the halves as they are.  A residual sum is made on the UNROUNDED conv result and rounded once:
c = store(conv(t) + shortcut).  The head (float64 here, float32 on the device) reads the stored c9; the output and a `res` network's input add are not stored.
``h1_first=False``: conv_in on the streaming float32 kernel (the default policy's choice) rounds neither its input nor its weights.
Tensors are NCHW; everything is device-agnostic torch."""
import torch

from _act16_ref import r16
from _h1_ref import act64, conv64, h1_conv
from _h1pw_ref import h1_conv1x1, h1_conv_s2, h1_convt

STORED = ['t0'] + [f't{i}' for i in range(1, 10)] + [f'c{i}' for i in range(1, 10)] + [f'd{i}' for i in range(1, 5)] + [f'u{i}' for i in range(6, 10)] + \
         [f'sc{i}' for i in range(6, 10)]


def identity(t):
    return t


def act16_resunet_forward(sd, x, res=False, store=r16, h1_first=True, maps=None):
    """``store``: the rounding of a stored map (``r16``; ``identity`` gives the fp16_all emulation: h1pw_resunet_forward with every layer rounded).
    ``maps``: a dict that receives every stored map by name (after ``store``)."""
    x = x.double()

    def keep(name, t):
        t = store(t)
        if maps is not None:
            maps[name] = t
        return t

    def block(i, t):
        u = keep(f't{i}', h1_conv(t, None, sd[f'conv{i}.block.0.conv.conv.weight'], None, 2))
        v = h1_conv(u, None, sd[f'conv{i}.block.1.conv.conv.weight'], None, 0)                  # not stored: the sum below is
        key = f'conv{i}.short_cut.0.conv.conv.weight'
        if key not in sd:
            return keep(f'c{i}', v + t)
        sc = keep(f'sc{i}', h1_conv1x1(t, None, sd[key], None, 0))                                # (amax of the cat = the larger of the two slots)
        return keep(f'c{i}', v + sc)
    w, b = sd['conv_in.weight'], sd['conv_in.bias']
    cur = keep('t0', h1_conv(x, None, w, b, 2) if h1_first else act64(conv64(x, w, b), 2))
    skips = []
    for i in range(1, 6):
        cur = block(i, cur)
        if i < 5:
            skips.append(cur)
            cur = keep(f'd{i}', h1_conv_s2(cur, sd[f'pool{i}.conv.weight'], sd[f'pool{i}.conv.bias'], 0))
    for i in range(6, 10):
        up = keep(f'u{i}', h1_convt(cur, sd[f'upv{i}.weight'], sd[f'upv{i}.bias']))
        cur = block(i, torch.cat([up, skips[9 - i]], 1))
    out = conv64(cur, sd['conv10.weight'], sd['conv10.bias'])
    return out + x if res else out

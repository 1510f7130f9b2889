"""Restatement of the fp16-STORAGE eval forward of UNetSeeInDark (ConvPolicy.h1_act16, Plan.act16) in plain torch float64, built on tests/_h1_ref.py and
tests/_h1pw_ref.py: the fp16_all emulation (``h1pw_unet_forward`` with every layer rounded) with ``float16`` rounding of every STORED map.  A stored map is
``float16(float32(y))`` -- one round to nearest even, unscaled, subnormals kept, not saturated; its consumer reads the halves as they are (no second rounding,
no scale), the weights keep their scaled one-piece rounding.  conv1_1 reads the float32 network input (scaled rounding, as before); conv9_2's map is never
stored (the head is in its epilogue).  Tensors are NCHW; everything is device-agnostic torch."""
import torch

from _h1_ref import _convt64, _pool64, act64, conv64, h1_round


def r16(t):
    """what an fp16 store keeps of a map: float64(float16(float32(t)))"""
    return t.float().half().double()


def act16_unet_forward(sd, x, res=False, store=r16):
    """``store``: the rounding of a stored map (``r16``; the identity gives the fp16_all emulation with exact float64 sums)"""
    x = x.double()

    def c3(name, t, t2=None, first=False, keep=True):
        w, b = h1_round(sd[name + '.weight']), sd[name + '.bias']
        t = t if t2 is None else torch.cat([t, t2], 1)
        y = act64(conv64(h1_round(t) if first else t, w, b), 1)
        return store(y) if keep else y

    def up(name, t):
        return store(_convt64(t, h1_round(sd[name + '.weight']), sd[name + '.bias']))
    skips, cur = [], x
    for i in range(1, 6):
        cur = c3(f'conv{i}_2', c3(f'conv{i}_1', cur, first=i == 1))
        if i < 5:
            skips.append(cur)
            cur = _pool64(cur)                                     # (the maximum of fp16 values is one of them)
    for i in range(6, 10):
        cur = c3(f'conv{i}_2', c3(f'conv{i}_1', up(f'upv{i}', cur), skips[9 - i]), keep=i < 9)
    out = conv64(cur, sd['conv10_1.weight'], sd['conv10_1.bias'])
    return out + x if res else out

"""ResUnet on hand-written HIP kernels (reference: archs/ResUnet.py:3-88, building blocks
archs/modules.py:130-153,176-197).

Same contract as UNetSeeInDark: the reference's constructor, attribute names and state_dict
keys (``conv_in``, ``conv{1..9}.block.{0,1}.conv.conv.weight``, ``conv{6..9}.short_cut.0.conv.conv
.weight``, ``pool{1..4}.conv.{weight,bias}``, ``upv{6..9}``, ``conv10``); children only own
parameters, forward/backward run through libpnnp_hip.so.

Reference quirks kept: ``conv3x3`` attaches its ReLU as a child of nn.Conv2d, which never runs
(the down-sampling convs are stride-2 conv + bias, NO activation); ResidualBlock is built with
``is_activate=False`` so the block output has no activation: out = conv(relu(conv(x))) + shortcut(x).
"""
from collections import OrderedDict

import torch
import torch.nn as nn

from .. import ops
from .._lib import PnnpError
from .engine import RELU, _EngineBase, _HipNet
from .plan import resolve_resunet


class _ConvHolder(nn.Module):      # modules.py:140-153 convWithBN(is_bn=False): .conv = Sequential(conv=Conv2d(bias=False))
    def __init__(self, ci, co, k):
        super().__init__()
        self.conv = nn.Sequential(OrderedDict([('conv', nn.Conv2d(ci, co, kernel_size=k, padding=k // 2, stride=1, bias=False))]))


class _ResBlockHolder(nn.Module):  # modules.py:176-197
    def __init__(self, ci, co):
        super().__init__()
        self.block = nn.Sequential(_ConvHolder(ci, co, 3), _ConvHolder(co, co, 3))
        self.short_cut = nn.Sequential(_ConvHolder(ci, co, 1)) if ci != co else nn.Sequential(OrderedDict([]))


class _DownHolder(nn.Module):      # modules.py:130-138 conv3x3(stride=2)
    def __init__(self, ci, co):
        super().__init__()
        self.conv = nn.Conv2d(ci, co, kernel_size=3, padding=1, stride=2)



class ResUnetEngine(_EngineBase):
    """Forward / backward schedule of ResUnet over the C-ABI layer kernels."""
    PACK_CAP = 512

    def __init__(self, module):
        self._init_net(module)

    def _resolve(self, pol, train, B, H, W):
        return resolve_resunet(self.ch, self.cin, self.cout, pol, train, B, H, W)

    @staticmethod
    def _pname(name):
        """the parameter names (weight, bias or None) of a layer of the plan"""
        if name[0] == 'b':
            return f'conv{name[1]}.block.{name[3]}.conv.conv.weight', None
        if name.startswith('sc'):
            return f'conv{name[2]}.short_cut.0.conv.conv.weight', None
        stem = name + '.conv' if name.startswith('pool') else name
        return stem + '.weight', stem + '.bias'

    def _layer(self, name):
        """(kind, padded input channels, padded output channels) of a layer of the plan (_EngineBase._build_pack_jobs)"""
        if name.startswith(('pool', 'upv')):
            return ('s2' if name[0] == 'p' else 'convt'), None, None
        if name.startswith('sc') or name == 'conv10':
            return '1x1', None, (self.cout_pad if name == 'conv10' else None)
        return '3x3', (self.cin_pad if name == 'conv_in' else None), None

    # ---------------------------------------------------------------- forward
    def forward(self, x, train, reflect_pad=0, add_residual=True, tile_src=None):
        """``reflect_pad`` > 0 (eval loop, trainer_SID.py:221-226): the network runs on the frame reflect-padded by that many pixels on
        every side -- the padding happens inside the NCHW -> NHWC layout pass, the result has the PADDED size (the caller crops).
        ``add_residual=False``: a `res` network returns f(x) without `+ x` (the caller adds the un-padded input after cropping:
        (f(pad x) + pad x)[crop] = f(pad x)[crop] + x; pnnp_eval_post_f32).
        ``tile_src=(frame [1,C,h,w], grid, t0, nt)`` (eval mode, ``x`` ignored; evaluate.forward_tiled): the batch is the tiles t0 .. t0 + nt of
        the frame (tiles.TileGrid), gathered by the layout pass itself; the result is [nt, out_nc, patch_size, patch_size]."""
        x, key, plan, bufs, P, T = self._forward_begin(x, train, reflect_pad, add_residual, tile_src)
        B, H, Wd, dev = key
        ch = self.ch
        g0 = lambda n, s: bufs.get(n, s, dev)
        # (Plan.act16: the 31 maps t, c, d, u, sc are fp16 buffers, keyed apart from the float32 ones; x8 and the output stay float32)
        g = (lambda n, s: bufs.get(n, s, dev, torch.float16)) if plan.act16 else g0
        hs = [H >> i for i in range(5)]; ws = [Wd >> i for i in range(5)]
        a = {}
        a['x8'], x = self._layout_in(x, g0('x8', (B, H, Wd, self.cin_pad)), reflect_pad, None, tile_src, bufs, dev)

        def cf(name, src, src2, out, cout, act, residual=None):
            return self._conv3_fwd(plan, name, T, a, src, src2, None, out, cout, act, residual=residual)

        # (the zero-padded network input: a kernel of its own fills its slot)
        xin = a['t0'] = self._first_fwd(plan, 'conv_in', T, a, a['x8'], P['conv_in.weight'], P['conv_in.bias'], g('t0', (B, H, Wd, ch[0])), ch[0], RELU,
                                        fill='in:conv_in')
        for l in range(1, 6):
            lv = l - 1
            shp = (B, hs[lv], ws[lv], ch[lv])
            a[f't{l}'] = cf(f'b{l}_0', xin, None, g(f't{l}', shp), ch[lv], RELU)
            a[f'c{l}'] = cf(f'b{l}_1', a[f't{l}'], None, g(f'c{l}', shp), ch[lv], 0, residual=xin)
            if l < 5:
                xin = a[f'd{l}'] = self._s2_fwd(plan, f'pool{l}', T, a[f'c{l}'], P[f'pool{l}.conv.bias'], g(f'd{l}', (B, hs[l], ws[l], ch[l])), ch[l])
        cur = a['c5']
        for i in range(6, 10):
            lv = 9 - i
            shp = (B, hs[lv], ws[lv], ch[lv])
            u = a[f'u{i}'] = self._convt_fwd(plan, f'upv{i}', T, cur, P[f'upv{i}.bias'], g(f'u{i}', shp), ch[lv])
            skip = a[f'c{lv + 1}']
            a[f't{i}'] = cf(f'b{i}_0', u, skip, g(f't{i}', shp), ch[lv], RELU)
            sc = self._conv1_fwd(plan, f'sc{i}', T, u, skip, None, g(f'sc{i}', shp), ch[lv], 0)
            a[f'c{i}'] = cur = cf(f'b{i}_1', a[f't{i}'], None, g(f'c{i}', shp), ch[lv], 0, residual=sc)
        out = torch.empty((B, self.cout, H, Wd), dtype=torch.float32, device=dev)
        self._head_fwd(plan, 'conv10', T, a['c9'], P['conv10.weight'], P['conv10.bias'], out, x if (self.m.res and add_residual) else None)
        self._forward_end(a, key, plan, T)
        return out

    # ---------------------------------------------------------------- backward
    def backward(self, g_out8, need_dx=False, accumulate=False, on_ready=None):
        a, (B, H, Wd, dev), plan, bufs, P, G, wsf, F, T = self._backward_begin()
        ch = self.ch
        gb = lambda n, like: bufs.get('g_' + n, like.shape, dev)
        acc = 1 if accumulate else 0

        def done(name):
            if on_ready is not None:
                on_ready(self.params.slices[self._pname(name)[0]][0])

        dg = lambda name, gsrc, dx1, **kw: self._conv3_dgrad(plan, name, a, F, T, gsrc, dx1, **kw)

        def wgrad(name, gpre, cout, x1, c1, x2=None):
            pw, pb = self._pname(name)
            self._wgrad(plan[name].wgrad, F, T, gpre, cout, x1, c1, x2, G(pw), G(pb), wsf, acc, P[pw].shape[-1] ** 2)

        # head
        g = self._head_bwd(plan, 'conv10', F, T, g_out8, a['c9'], P['conv10.weight'], gb('c9', a['c9']), G('conv10.weight'), G('conv10.bias'), wsf, acc, 0)
        done('conv10')
        for i in range(9, 5, -1):                    # decoder blocks, top-down
            lv = 9 - i
            u, skip, t = a[f'u{i}'], a[f'c{lv + 1}'], a[f't{i}']
            wgrad(f'sc{i}', g, ch[lv], u, ch[lv], x2=skip)
            wgrad(f'b{i}_1', g, ch[lv], t, ch[lv])
            g_t = gb(f't{i}', t)
            dg(f'b{i}_1', g, g_t, mask1=t, mode1=RELU)
            wgrad(f'b{i}_0', g_t, ch[lv], u, ch[lv], x2=skip)
            done(f'b{i}_0')
            g_u, g_skip = gb(f'u{i}', u), gb(f'c{lv + 1}', skip)
            dg(f'b{i}_0', g_t, g_u, dx2=g_skip)
            self._conv1_dgrad_acc(plan, f'sc{i}', T, g, g_u, g_skip, f'gu{i}')
            below = a['c5'] if i == 6 else a[f'c{i - 1}']
            name = f'upv{i}'
            self._convt_wgrad(plan, name, F, T, below, g_u, G(name + '.weight'), G(name + '.bias'), wsf, acc)
            done(name)
            g = self._convt_dgrad(plan, name, T, g_u, gb('c5' if i == 6 else f'c{i - 1}', below))
        for l in range(5, 0, -1):                    # encoder blocks, bottom-up; g = dL/d c_l
            lv = l - 1
            t = a[f't{l}']
            xin = a['t0'] if l == 1 else a[f'd{l - 1}']
            wgrad(f'b{l}_1', g, ch[lv], t, ch[lv])
            g_t = gb(f't{l}', t)
            dg(f'b{l}_1', g, g_t, mask1=t, mode1=RELU)
            wgrad(f'b{l}_0', g_t, ch[lv], xin, ch[lv])
            done(f'b{l}_0')
            g_x = gb('t0' if l == 1 else f'd{l - 1}', xin)
            # identity shortcut: d/d(xin) = dgrad(block) + g ; xin = t0 is a ReLU output (mask), d_l is not.  (The stride-2 layer's fp16x2
            # backward kernels split g_x next.)
            self._conv3_dgrad_res(plan, f'b{l}_0', T, g_t, g_x, g, xin if l == 1 else None, RELU, f'gx{l}')
            if l > 1:
                name, c_prev = f'pool{l - 1}', a[f'c{l - 1}']
                self._s2_wgrad(plan, name, F, T, g_x, c_prev, G(name + '.conv.weight'), G(name + '.conv.bias'), wsf, acc, f'gx{l}')
                done(name)
                g = self._s2_dgrad_acc(plan, name, T, g_x, gb(f'c{l - 1}', c_prev), f'gx{l}')      # (c{l-1}'s gradient already holds the skip gradient)
            else:
                wgrad('conv_in', g_x, ch[0], a['x8'], self.cin)
                done('conv_in')
        if need_dx:
            raise PnnpError('gradient w.r.t. the network input is not implemented on the HIP path')
        return None


class ResUnet(_HipNet):
    """Drop-in for archs/ResUnet.py:3-88 (``args`` keys: nframes, res, nf, in_nc, out_nc)."""
    _engine_cls = ResUnetEngine

    def __init__(self, args=None):
        super().__init__(args)
        nf = self.nf
        c = [nf, nf * 2, nf * 4, nf * 8, nf * 16]
        self.conv_in = nn.Conv2d(self.in_nc * self.nframes, nf, kernel_size=3, stride=1, padding=1)
        for l in range(1, 6):
            setattr(self, f'conv{l}', _ResBlockHolder(c[l - 1], c[l - 1]))
            if l < 5:
                setattr(self, f'pool{l}', _DownHolder(c[l - 1], c[l]))
        for i in range(6, 10):
            lv = 9 - i
            setattr(self, f'upv{i}', nn.ConvTranspose2d(c[lv + 1], c[lv], 2, stride=2))
            setattr(self, f'conv{i}', _ResBlockHolder(c[lv + 1], c[lv]))
        self.conv10 = nn.Conv2d(nf, self.out_nc, kernel_size=1, stride=1)

    def forward(self, x, noise_map=None):
        return super().forward(x)

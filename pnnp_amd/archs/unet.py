"""UNetSeeInDark on hand-written HIP kernels (reference: archs/Unet.py:4-99).

The module keeps the reference's constructor (``args`` dict), attribute names and
``state_dict`` layout (46 tensors, ``conv{1..9}_{1,2}``, ``upv{6..9}``, ``conv10_1``) so
released checkpoints load unchanged and ``initialize_weights`` / ``load_weights`` work on
it.  The nn.Conv2d / nn.ConvTranspose2d children only own parameters: ``forward`` runs the
whole network through libpnnp_hip.so (NHWC fp32 activations, fp32 MFMA) and backward is a
hand-sequenced pass over the same kernels, exposed to autograd as one Function so
``loss.backward(); optimizer.step()`` of the reference trainer works as is.
"""
import torch
import torch.nn as nn

from .. import ops
from .._lib import PnnpError
from .engine import LRELU, _EngineBase, _HipNet
from .plan import DEFAULT_POLICY, ConvPolicy, resolve_unet  # noqa: F401  (ConvPolicy, DEFAULT_POLICY: re-exported)


class UNetEngine(_EngineBase):
    """Forward / backward schedule of UNetSeeInDark over the C-ABI layer kernels."""

    def __init__(self, module):
        self._init_net(module)

    # ------------------------------------------------------------------ weights
    def _resolve(self, pol, train, B, H, W):
        return resolve_unet(self.ch, self.cin, self.cout, pol, train, B, H, W)

    @staticmethod
    def _pname(name):
        """the parameter names (weight, bias) of a layer of the plan"""
        return name + '.weight', name + '.bias'

    def _layer(self, name):
        """(kind, padded input channels, padded output channels) of a layer of the plan (_EngineBase._build_pack_jobs)"""
        if name.startswith('upv'):
            return 'convt', None, None
        return ('1x1' if name == 'conv10_1' else '3x3'), (self.cin_pad if name == 'conv1_1' else None), (self.cout_pad if name == 'conv10_1' else None)

    def _pack_order(self, plan):
        """every Conv2d, then the ConvTranspose2d layers"""
        return [n for n in plan.steps if not n.startswith('upv')] + [n for n in plan.steps if n.startswith('upv')]

    def _head_fusable(self):
        """conv10_1 inside conv9_2's epilogue (the plan's 'h2+head'): nf = 32, 4 output planes, conv9_2 on the fp16x2 kernel."""
        return self._plan['conv10_1'].fwd == 'fused'

    # ------------------------------------------------------------------ forward
    def forward(self, x, train, reflect_pad=0, add_residual=True, tile_src=None):
        """``reflect_pad`` > 0 (eval loop, trainer_SID.py:221-226): the network runs on the frame reflect-padded by that many pixels on
        every side -- the padding happens inside the NCHW -> NHWC layout pass, the result has the PADDED size (the caller crops).
        ``add_residual=False``: a `res` network returns f(x) without `+ x` (the caller adds the un-padded input after cropping:
        (f(pad x) + pad x)[crop] = f(pad x)[crop] + x; pnnp_eval_post_f32).
        ``tile_src=(frame [1,C,h,w], grid, t0, nt)`` (eval mode, ``x`` ignored; evaluate.forward_tiled): the batch is the tiles t0 .. t0 + nt of
        the frame (tiles.TileGrid), gathered by the layout pass itself; the result is [nt, out_nc, patch_size, patch_size]."""
        x, key, plan, bufs, P, T = self._forward_begin(x, train, reflect_pad, add_residual, tile_src)
        B, H, W, dev = key
        ch = self.ch
        g = lambda n, s: bufs.get(n, s, dev)
        a = {}
        # (Plan.act16: conv, pooled and up-sampled maps are fp16 buffers, keyed apart from the float32 ones; x8, the split-K slabs and the output stay float32)
        gm = (lambda n, s: bufs.get(n, s, dev, torch.float16)) if plan.act16 else g
        # the zero-padded NHWC copy of the network input; its amax rides on the layout pass when conv1_1 runs on the fp16x2 kernel.  (A pooled
        # map shares its full-resolution map's amax slot.)
        x8, x = self._layout_in(x, g('x8', (B, H, W, self.cin_pad)), reflect_pad, self._in_amax(plan, 'conv1_1', T), tile_src, bufs, dev)
        a['x8'] = T.put(x8, 'x8', True)

        def conv(name, src, src2, h, w, cout):
            return self._conv3_fwd(plan, name, T, a, src, src2, P[name + '.bias'], gm(name, (B, h, w, cout)), cout, LRELU)

        hs = [H >> i for i in range(5)]
        ws = [W >> i for i in range(5)]
        cur = a['c1a'] = self._first_fwd(plan, 'conv1_1', T, a, a['x8'], P['conv1_1.weight'], P['conv1_1.bias'], gm('conv1_1', (B, H, W, ch[0])), ch[0], LRELU)
        for lvl in range(5):               # encoder: conv{l}_1, conv{l}_2, pool
            i = lvl + 1
            if i > 1:
                a[f'c{i}a'] = conv(f'conv{i}_1', cur, None, hs[lvl], ws[lvl], ch[lvl])
            name = f'conv{i}_2'
            if lvl == 4:
                a[f'c{i}'] = conv(name, a[f'c{i}a'], None, hs[lvl], ws[lvl], ch[lvl])
                continue
            shp = (B, hs[lvl + 1], ws[lvl + 1], ch[lvl])
            codes = None
            if plan[name].codes:                   # argmax + sign codes: the backward pass then does not re-read the full-resolution map
                codes = bufs.t.get(f'pc{i}')
                if codes is None or tuple(codes.shape) != shp or codes.device != dev:
                    codes = bufs.t[f'pc{i}'] = torch.empty(shp, dtype=torch.uint8, device=dev)
                a[f'pc{i}'] = codes
            pooled = gm(f'p{i}', shp)
            a[f'c{i}'] = self._conv3_pool_fwd(plan, name, T, a, a[f'c{i}a'], P[name + '.bias'], gm(name, (B, hs[lvl], ws[lvl], ch[lvl])), pooled, codes, ch[lvl], LRELU)
            a[f'p{i}'] = cur = T.put(pooled, name, fused=True)        # max |pooled| <= max |full-resolution map|
        cur = a['c5']
        for i in range(6, 10):             # decoder: upv{i}, conv{i}_1 on [up, skip], conv{i}_2 (conv9_2: with the head, below)
            lvl = 9 - i
            u = a[f'u{i}'] = self._convt_fwd(plan, f'upv{i}', T, cur, P[f'upv{i}.bias'], gm(f'u{i}', (B, hs[lvl], ws[lvl], ch[lvl])), ch[lvl])
            a[f'c{i}a'] = conv(f'conv{i}_1', u, a[f'c{lvl + 1}'], hs[lvl], ws[lvl], ch[lvl])
            if i < 9:
                a[f'c{i}'] = cur = conv(f'conv{i}_2', a[f'c{i}a'], None, hs[lvl], ws[lvl], ch[lvl])
        out = torch.empty((B, self.cout, H, W), dtype=torch.float32, device=dev)
        a['c9'] = self._conv3_head_fwd(plan, 'conv9_2', 'conv10_1', T, a, a['c9a'], P['conv9_2.bias'], (B, H, W, ch[0]), LRELU,
                                       P['conv10_1.weight'], P['conv10_1.bias'], out, x if (self.m.res and add_residual) else None)
        self._forward_end(a, key, plan, T)
        return out

    # ------------------------------------------------------------------ backward
    def backward(self, g_out8, need_dx=False, accumulate=False, on_ready=None):
        """g_out8: dL/d(out) as NHWC [B,H,W,cout_pad] (zero padded).  Fills the flat gradient
        buffer.  ``on_ready(offset)`` is called as soon as flat_grad[offset:] is final (layers
        finish in exactly the reverse of the flat parameter order) so a data-parallel reducer
        can start all-reducing the tail while the rest of the backward pass still runs."""
        a, (B, H, W, dev), plan, bufs, P, G, wsf, F, T = self._backward_begin()
        ch = self.ch
        gb = lambda n, s: bufs.get('g_' + n, s, dev)
        acc = 1 if accumulate else 0

        dgrad = lambda name, gsrc, dx1, **kw: self._conv3_dgrad(plan, name, a, F, T, gsrc, dx1, **kw)

        def done(name):
            if on_ready is not None:
                on_ready(self.params.slices[name + '.weight'][0])

        def wgrad(name, gpre, cout, x1, c1, x2=None):
            self._wgrad(plan[name].wgrad, F, T, gpre, cout, x1, c1, x2, G(name + '.weight'), G(name + '.bias'), wsf, acc)
            done(name)

        # conv10_1 (1x1, no activation); its input c9 is a LeakyReLU output
        g_cur = self._head_bwd(plan, 'conv10_1', F, T, g_out8, a['c9'], P['conv10_1.weight'], gb('c9', a['c9'].shape),
                               G('conv10_1.weight'), G('conv10_1.bias'), wsf, acc, LRELU)
        done('conv10_1')
        skip_later = {}                    # encoder level -> (decoder layer, its output gradient): skip-gradient launches deferred to the pool's backward
        for i in range(9, 5, -1):          # decoder, top-down
            lvl = 9 - i
            wgrad(f'conv{i}_2', g_cur, ch[lvl], a[f'c{i}a'], ch[lvl])
            g_a = gb(f'c{i}a', a[f'c{i}a'].shape)
            dgrad(f'conv{i}_2', g_cur, g_a, mask1=a[f'c{i}a'], mode1=LRELU)
            skip = a[f'c{lvl + 1}']
            wgrad(f'conv{i}_1', g_a, ch[lvl], a[f'u{i}'], ch[lvl], x2=skip)
            g_u = gb(f'u{i}', a[f'u{i}'].shape)
            g_skip = gb(f'c{lvl + 1}', skip.shape)
            if plan[f'conv{i}_1'].unpool:
                # only g_u is needed now: columns [0, c) of the pack (no mask: the plain forward epilogue).  The skip half -- columns [c, 2 c) -- is launched in
                # the encoder loop, where the pooled map's gradient exists, and adds MaxPool2d's backward before it stores; g_a stays untouched until then
                self._conv3_dgrad_cols(f'conv{i}_1', T, g_a, 0, g_u, f'd1:conv{i}_1')
                skip_later[lvl + 1] = (f'conv{i}_1', g_a)
            else:
                dgrad(f'conv{i}_1', g_a, g_u, dx2=g_skip, mask2=skip, mode2=LRELU)
            below = a['c5'] if i == 6 else a[f'c{i - 1}']
            name = f'upv{i}'
            self._convt_wgrad(plan, name, F, T, below, g_u, G(name + '.weight'), G(name + '.bias'), wsf, acc)
            done(name)
            # the act' mask as the sign bits conv{i-1}_2's forward kernel stored (the float32 activation is not read: 503 MB per step over the four layers)
            bits = a.get('bits:' + F.names.get(id(below), '?')) if plan.pol.convt_bits and below.shape[3] % 32 == 0 else None
            g_cur = self._convt_dgrad(plan, name, T, g_u, gb('c5' if i == 6 else f'c{i - 1}', below.shape), mask=below, mode=LRELU, bits=bits)
        for i in range(5, 0, -1):          # encoder, bottom-up
            lvl = i - 1
            wgrad(f'conv{i}_2', g_cur, ch[lvl], a[f'c{i}a'], ch[lvl])
            g_a = gb(f'c{i}a', a[f'c{i}a'].shape)
            dgrad(f'conv{i}_2', g_cur, g_a, mask1=a[f'c{i}a'], mode1=LRELU)
            if i > 1:
                src = a[f'p{i - 1}']
                wgrad(f'conv{i}_1', g_a, ch[lvl], src, ch[lvl - 1])
                g_p = gb(f'p{i - 1}', src.shape)
                dgrad(f'conv{i}_1', g_a, g_p)
                g_cur = gb(f'c{i - 1}', a[f'c{i - 1}'].shape)      # already holds the skip gradient
                # (the skip gradient + the scattered pooled gradient: a new tensor, a new amax slot)
                if (i - 1) in skip_later:
                    # the deferred skip half of conv{11-i}_1's backward-data: act'(c{i-1}) x dgrad + unpool(g_p) stored once
                    dname, g_dec = skip_later.pop(i - 1)
                    self._conv3_dgrad_cols(dname, T, g_dec, ch[lvl - 1], g_cur, f'pool{i - 1}', bits=a[f'bits:conv{i - 1}_2'], mode=LRELU,
                                           gp=g_p, codes=a[f'pc{i - 1}'])
                else:
                    ops.maxpool_bwd(a[f'c{i - 1}'], g_p, g_cur, LRELU, 1, codes=a.get(f'pc{i - 1}'), amax_gx=T.slot(f'pool{i - 1}') if plan.h2 else None)
                T.put(g_cur, f'pool{i - 1}', fused=True)
            else:
                wgrad('conv1_1', g_a, ch[0], a['x8'], self.cin)
                if need_dx:
                    raise PnnpError('gradient w.r.t. the network input is not implemented on the HIP path')
        return None


class UNetSeeInDark(_HipNet):
    """Drop-in for archs/Unet.py:4-99 (same ``args`` keys: nframes, res, nf, in_nc, out_nc)."""
    _engine_cls = UNetEngine

    def __init__(self, args=None):
        super().__init__(args)
        nf = self.nf
        c = [nf, nf * 2, nf * 4, nf * 8, nf * 16]
        prev = self.in_nc * self.nframes
        for lvl in range(5):
            setattr(self, f'conv{lvl + 1}_1', nn.Conv2d(prev, c[lvl], kernel_size=3, stride=1, padding=1))
            setattr(self, f'conv{lvl + 1}_2', nn.Conv2d(c[lvl], c[lvl], kernel_size=3, stride=1, padding=1))
            prev = c[lvl]
        for i in range(6, 10):
            lvl = 9 - i
            setattr(self, f'upv{i}', nn.ConvTranspose2d(c[lvl + 1], c[lvl], 2, stride=2))
            setattr(self, f'conv{i}_1', nn.Conv2d(c[lvl + 1], c[lvl], kernel_size=3, stride=1, padding=1))
            setattr(self, f'conv{i}_2', nn.Conv2d(c[lvl], c[lvl], kernel_size=3, stride=1, padding=1))
        self.conv10_1 = nn.Conv2d(nf, self.out_nc, kernel_size=1, stride=1)

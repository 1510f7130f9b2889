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
from .plan import resolve_resunet
from .unet import FlatParams, _Bufs, _EngineBase, _Slots, RELU


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
    def __init__(self, module):
        self._init_base()
        self.m = module
        self.params = FlatParams(module)
        self.bufs = {}
        self.packed = {}
        nf = module.nf
        if nf % 8:
            raise PnnpError('ResUnet on HIP needs nf % 8 == 0')
        self.ch = [nf, nf * 2, nf * 4, nf * 8, nf * 16]
        self.cin = module.in_nc * module.nframes
        self.cin_pad = (self.cin + 7) // 8 * 8
        self.cout = module.out_nc
        self.cout_pad = (self.cout + 7) // 8 * 8

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

    # ---------------------------------------------------------------- weights
    def _buf(self, key, n, dev, dtype=torch.float32):
        k = (key, dev)
        if k not in self.packed or self.packed[k].numel() != n:
            self.packed[k] = torch.empty(n, dtype=dtype, device=dev)
        return self.packed[k]

    def grad_out_channels(self, B, H, W):
        """channels of the NHWC loss gradient backward() wants (UNetEngine.grad_out_channels)"""
        return 4 if (self.cout == 4 and self._pol.use_thin_head(self.ch[0], self.cout, B * H * W)) else self.cout_pad

    def _build_pack_jobs(self, train, dev, P, plan):
        """One record per layer, in the plan's families: self._wp[name] = (forward pack, backward-data pack, the weight's amax slot)."""
        jobs = ops.PackJobs(cap=512)
        self._wp = {}
        u8 = torch.uint8
        for name, s in plan.steps.items():
            w = P[self._pname(name)[0]]
            pf, pd = s.pack
            b = lambda kind, n, dt=u8: self._buf(name + kind, n, dev, dt)
            kind = 's2' if name.startswith('pool') else 'convt' if name.startswith('upv') else '1x1' if w.shape[-1] == 1 else None
            co, ci = (w.shape[1], w.shape[0]) if kind == 'convt' else (w.shape[0], w.shape[1])
            if kind and pf in ('h2', 'x3'):    # 3x3 stride 2, ConvTranspose2d 2x2 stride 2, 1x1: the pointwise fp16x2 / bf16x3 GEMM kernels
                mat = ops.h2mat_bytes if pf == 'h2' else ops.x3mat_bytes
                fn, dn = dict(s2=(mat(9 * ci, co), 9 * mat(co, ci)), convt=(mat(ci, 4 * co), mat(4 * co, ci)), **{'1x1': (mat(ci, co), mat(co, ci))})[kind]
                f, d = b(':h2mf' if pf == 'h2' else ':x3f', fn), b(':h2md' if pf == 'h2' else ':x3d', dn) if pd else None
                self._wp[name] = (f, d, getattr(jobs, f'add_{pf}_{kind}')(w, f, d))
                continue
            if kind in ('s2', 'convt'):        # the direct kernels (their own weight layouts)
                f, d = b(':f', w.numel(), torch.float32), b(':d', w.numel(), torch.float32) if pd else None
                if kind == 'convt':
                    jobs.add_convt(w, f, d)
                else:
                    jobs.add_conv(w, f, None)
                    if pd:
                        jobs.add_s2_dgrad(w, d)
                self._wp[name] = (f, d, None)
                continue
            kh, kw = w.shape[2], w.shape[3]
            cip = self.cin_pad if name == 'conv_in' else ci
            got, slot = {}, None
            if 'h2' in (pf, pd):                               # the fp16x2 kernel takes what bf16x3 would have taken
                got['h2'] = (b(':h2f', ops.h2_weight_bytes(cip, co)) if pf == 'h2' else None, b(':h2d', ops.h2_weight_bytes(co, ci)) if pd == 'h2' else None)
                slot = jobs.add_h2(w, *got['h2'], cin_pad=(cip + 15) // 16 * 16)
            if 'direct' in (pf, pd):
                got['direct'] = (b(':f', kh * kw * cip * co, torch.float32) if pf == 'direct' else None,
                                 b(':d', kh * kw * (self.cout_pad if name == 'conv10' else co) * ci, torch.float32) if pd == 'direct' else None)
                jobs.add_conv(w, *got['direct'], cin_pad=cip, cout_pad=self.cout_pad if name == 'conv10' else co)
            if 'wino' in (pf, pd):
                got['wino'] = (b(':uf', 16 * co * ci, torch.float32) if pf == 'wino' else None, b(':ud', 16 * co * ci, torch.float32) if pd == 'wino' else None)
                jobs.add_wino(w, *got['wino'])
            if 'x3' in (pf, pd):
                got['x3'] = (b(':x3f', ops.x3_weight_bytes(cip, co)) if pf == 'x3' else None, b(':x3d', ops.x3_weight_bytes(co, ci)) if pd == 'x3' else None)
                jobs.add_x3(w, *got['x3'], cin_pad=(cip + 15) // 16 * 16)
            self._wp[name] = (got[pf][0], got[pd][1] if pd else None, slot)
        return jobs

    # ---------------------------------------------------------------- forward
    def forward(self, x, train, reflect_pad=0, add_residual=True):
        """``reflect_pad`` > 0 (eval loop, trainer_SID.py:221-226): the network runs on the frame reflect-padded by that many pixels on
        every side -- the padding happens inside the NCHW -> NHWC layout pass, the result has the PADDED size (the caller crops).
        ``add_residual=False``: a `res` network returns f(x) without `+ x` (the caller adds the un-padded input after cropping:
        (f(pad x) + pad x)[crop] = f(pad x)[crop] + x; pnnp_eval_post_f32)."""
        if not x.is_cuda:
            raise PnnpError('ResUnet.forward: input must be a CUDA tensor (pnnp_amd has no CPU path)')
        x = x.contiguous().float()
        B, Cin, H, Wd = x.shape
        if reflect_pad:
            if train or (self.m.res and add_residual):
                raise PnnpError('reflect_pad is an eval-mode option; a `res` network needs add_residual=False (the caller adds the input after cropping)')
            H, Wd = H + 2 * reflect_pad, Wd + 2 * reflect_pad
        if Cin != self.cin or H % 16 or Wd % 16:
            raise PnnpError(f'input must be [B,{self.cin},H,W] with H,W multiples of 16, got {tuple(x.shape)}')
        dev = x.device
        self.params.ensure(dev)
        # packed weights are re-used while no parameter changed (eval loops); in-place torch updates bump
        # tensor._version, the fused Adam kernel goes through mark_dirty()
        self._pol = self.effective_policy(H, Wd, max(self.ch[0], self.cin_pad, self.cout_pad))
        plan = self._plan = self._plan_for(B, H, Wd, train)
        self._packs_ready(train, dev, plan)
        gen = self._begin_forward((B, H, Wd, dev), train)
        bufs = self.bufs.setdefault((B, H, Wd, dev), _Bufs())
        P = dict(self.m.named_parameters())
        ch = self.ch
        g = lambda n, s: bufs.get(n, s, dev)
        hs = [H >> i for i in range(5)]; ws = [Wd >> i for i in range(5)]
        a = {}
        a['x8'] = ops.nchw_to_nhwc(x, g('x8', (B, H, Wd, self.cin_pad)), self.cin_pad, reflect_pad=reflect_pad)
        # fp16x2 family (csrc/h2.h): amax slots of the activations, keyed by the layer that wrote the tensor; sign bits of the ReLU outputs
        # that backward-data will need as masks
        split = {} if train else None                                 # (range census) what the fp16x2 kernels split in this step
        T = _Slots(bufs, 'f', dev, plan.h2, log=split)
        sl = T.slot

        def cf(name, src, src2, bias, out, cout, act, residual=None):
            bits = None
            if plan[name].fwd == 'h2':
                if train and act != 0 and residual is None:
                    bits = a['bits:' + name] = bufs.bits(name, B, out.shape[1], out.shape[2], cout, dev)
                if src is a['x8']:                              # (the zero-padded network input: a kernel of its own fills its slot)
                    T.put(src, 'in:' + name, fused=False)
            return self._conv3_fwd(plan, name, T, src, src2, bias, out, cout, act, bits=bits, residual=residual)

        if plan['conv_in'].fwd == 'thin':
            a['t0'] = T.put(ops.first_fwd(a['x8'], P['conv_in.weight'], P['conv_in.bias'], g('t0', (B, H, Wd, ch[0])), RELU,
                                          amax_y=sl('conv_in') if plan.h2 else None), 'conv_in', fused=True)
        else:
            a['t0'] = cf('conv_in', a['x8'], None, P['conv_in.bias'], g('t0', (B, H, Wd, ch[0])), ch[0], RELU)
        xin = a['t0']
        for l in range(1, 6):
            lv = l - 1
            shp = (B, hs[lv], ws[lv], ch[lv])
            a[f't{l}'] = cf(f'b{l}_0', xin, None, None, g(f't{l}', shp), ch[lv], RELU)
            a[f'c{l}'] = cf(f'b{l}_1', a[f't{l}'], None, None, g(f'c{l}', shp), ch[lv], 0, residual=xin)
            if l < 5:
                name, c = f'pool{l}', a[f'c{l}']
                f, _, wslot = self._wp[name]
                y = g(f'd{l}', (B, hs[l], ws[l], ch[l]))
                if plan[name].fwd == 'h2':
                    ops.conv_s2_h2_fwd(c, T.of(c), f, wslot, P[name + '.conv.bias'], y, ch[l], 0, amax_y=sl(name))
                elif plan[name].fwd == 'x3':
                    ops.conv_s2_x3_fwd(c, f, P[name + '.conv.bias'], y, ch[l], amax_y=sl(name) if plan.h2 else None)
                else:
                    ops.conv_s2_fwd(c, f, P[name + '.conv.bias'], y, ch[l])
                xin = a[f'd{l}'] = T.put(y, name, fused=plan[name].fwd != 'direct')
        cur = a['c5']
        for i in range(6, 10):
            lv = 9 - i
            shp = (B, hs[lv], ws[lv], ch[lv])
            u = a[f'u{i}'] = self._convt_fwd(plan, f'upv{i}', T, cur, P[f'upv{i}.bias'], g(f'u{i}', shp), ch[lv])
            skip = a[f'c{lv + 1}']
            a[f't{i}'] = cf(f'b{i}_0', u, skip, None, g(f't{i}', shp), ch[lv], RELU)
            f, _, wslot = self._wp[f'sc{i}']
            sc = g(f'sc{i}', shp)
            if plan[f'sc{i}'].fwd == 'h2':
                ops.conv1x1_h2_fwd(u, T.of(u), skip, T.of(skip), f, wslot, None, sc, ch[lv], 0)
            elif plan[f'sc{i}'].fwd == 'x3':
                ops.conv1x1_x3_fwd(u, skip, f, None, sc, ch[lv], 0)
            else:
                ops.conv_fwd(u, skip, f, None, sc, ch[lv], 1, 0)
            a[f'c{i}'] = cur = cf(f'b{i}_1', a[f't{i}'], None, None, g(f'c{i}', shp), ch[lv], 0, residual=sc)
        out = torch.empty((B, self.cout, H, Wd), dtype=torch.float32, device=dev)
        res = x if (self.m.res and add_residual) else None
        if plan['conv10'].fwd == 'thin':
            ops.head_fwd(a['c9'], P['conv10.weight'], P['conv10.bias'], out, residual=res)
        else:
            o = ops.conv_fwd(a['c9'], None, self._wp['conv10'][0], P['conv10.bias'], g('o', (B, H, Wd, self.cout)), self.cout, 1, 0)
            ops.nhwc_to_nchw(o, out, residual=res)
        if train:
            a['_plan'] = plan
            a['_src_name'] = T.names
            a['_split'] = split
            self.saved = (a, (B, H, Wd, dev), gen)
        return out

    # ---------------------------------------------------------------- backward
    def backward(self, g_out8, need_dx=False, accumulate=False, on_ready=None):
        a, (B, H, Wd, dev), _ = self.saved
        plan = self._plan = a['_plan']     # the kernel families this forward ran on
        self._pol = plan.pol
        bufs = self.bufs[(B, H, Wd, dev)]
        ch = self.ch
        gb = lambda n, like: bufs.get('g_' + n, like.shape, dev)
        P = dict(self.m.named_parameters())
        G = lambda pname: self.params.grad_view(pname, P[pname].shape) if pname else None
        acc = 1 if accumulate else 0
        wsf = bufs.get('wgrad_ws', (plan.ws,), dev)

        def done(name):
            if on_ready is not None:
                on_ready(self.params.slices[self._pname(name)[0]][0])

        # fp16x2 family: amax slots of the gradients (zeroed per backward), the activations' slots are the forward's
        F = _Slots(bufs, 'f', dev, False, names=a['_src_name'], log=a['_split'])
        T = _Slots(bufs, 'b', dev, plan.h2, log=a['_split'])
        bslot = lambda n: T.slot(n) if plan.h2 else None

        dg = lambda name, gsrc, dx1, **kw: self._conv3_dgrad(plan, name, a, F, T, gsrc, dx1, **kw)

        def wgrad(name, gpre, cout, x1, c1, x2=None):
            pw, pb = self._pname(name)
            self._wgrad(plan[name].wgrad, F, T, gpre, cout, x1, c1, x2, G(pw), G(pb), wsf, acc, P[pw].shape[-1] ** 2)

        # head
        g = gb('c9', a['c9'])
        if plan['conv10'].dgrad == 'thin':
            ops.head_bwd(g_out8, a['c9'], P['conv10.weight'], g, G('conv10.weight'), G('conv10.bias'), wsf, mode=0, accumulate=acc, amax_gx=bslot('head'))
        else:
            wgrad('conv10', g_out8, self.cout, a['c9'], ch[0])
            ops.conv_bwd_data(g_out8, self._wp['conv10'][1], g, taps=1)
        T.put(g, 'head', fused=plan['conv10'].dgrad == 'thin')
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
            # the shortcut's gradient is ACCUMULATED into g_u and g_skip next: their slots are stale from here on.  An fp16x2 shortcut
            # reports max |block + shortcut gradient| of g_u (the plan runs ConvTranspose2d's backward on fp16x2 only then); g_skip's stays stale
            T.names.pop(id(g_u), None); T.names.pop(id(g_skip), None)
            _, d, wslot = self._wp[f'sc{i}']
            if plan[f'sc{i}'].dgrad == 'h2':
                ops.conv1x1_h2_bwd_data(g, T.of(g), d, wslot, g_u, accum1=1, amax_dx1=bslot(f'gu{i}'), dx2=g_skip, accum2=1)
                T.put(g_u, f'gu{i}', fused=True)
            elif plan[f'sc{i}'].dgrad == 'x3':
                ops.conv1x1_x3_bwd_data(g, d, g_u, accum1=1, dx2=g_skip, accum2=1)
            else:
                ops.conv_bwd_data(g, d, g_u, accum1=1, dx2=g_skip, accum2=1, taps=1)
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
            # identity shortcut: d/d(xin) = dgrad(block) + g ; xin = t0 is a ReLU output (mask), d_l is not
            _, d, wslot = self._wp[f'b{l}_0']
            fam, mask = plan[f'b{l}_0'].dgrad, xin if l == 1 else None
            if fam == 'h2+res':                          # (the stride-2 layer's fp16x2 backward kernels split g_x next)
                ops.conv_h2_bwd_data_res(g_t, T.of(g_t), d, wslot, g_x, addsrc=g, mask=mask, mode=RELU, amax_dx=bslot(f'gx{l}'))
                T.put(g_x, f'gx{l}', fused=True)
            elif fam == 'x3+res':
                ops.conv_x3_bwd_data_res(g_t, d, g_x, addsrc=g, mask=mask, mode=RELU)
            elif fam == 'wino+res':
                ops.conv_wino_bwd_data_res(g_t, d, g_x, addsrc=g, mask=mask, mode=RELU)
            else:
                ops.conv_bwd_data_res(g_t, d, g_x, addsrc=g, mask=mask, mode=RELU)
            if l > 1:
                name, c_prev = f'pool{l - 1}', a[f'c{l - 1}']
                s = plan[name]
                # without a fused amax in g_x, a launch of its own fills its slot before the first fp16x2 kernel that splits it
                fill = fam != 'h2+res'
                if s.wgrad == 'h2':
                    if fill:
                        T.put(g_x, f'gx{l}', fused=False)
                    ops.conv_s2_h2_bwd_weight(g_x, T.of(g_x), c_prev, F.of(c_prev), G(name + '.conv.weight'), G(name + '.conv.bias'), wsf, accumulate=acc)
                elif s.wgrad == 'x3':       # (the fp16x2 kernel also has a tile for Cout = 64: pool1, which bf16x3 leaves to the fp32-MFMA kernel)
                    ops.conv_s2_x3_bwd_weight(g_x, c_prev, G(name + '.conv.weight'), G(name + '.conv.bias'), wsf, accumulate=acc)
                else:
                    ops.conv_s2_bwd_weight(g_x, c_prev, G(name + '.conv.weight'), G(name + '.conv.bias'), wsf, accumulate=acc)
                done(name)
                g = gb(f'c{l - 1}', c_prev)                          # already holds the skip gradient
                _, d, wslot = self._wp[name]
                if s.dgrad == 'h2':
                    if fill and s.wgrad != 'h2':
                        T.put(g_x, f'gx{l}', fused=False)
                    ops.conv_s2_h2_bwd_data(g_x, T.of(g_x), d, wslot, g, accum=1, amax_dx=bslot(name))
                elif s.dgrad == 'x3':
                    ops.conv_s2_x3_bwd_data(g_x, d, g, accum=1, amax_dx=bslot(name))   # (the sums it stored: skip gradient + this layer's)
                else:
                    ops.conv_s2_bwd_data(g_x, d, g, accum=1)
                T.put(g, name, fused=s.dgrad != 'direct')
            else:
                wgrad('conv_in', g_x, ch[0], a['x8'], self.cin)
                done('conv_in')
        if need_dx:
            raise PnnpError('gradient w.r.t. the network input is not implemented on the HIP path')
        return None


class _ResUnetFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, engine, train, *params):
        ctx.engine = engine
        ctx.x_needs = x.requires_grad
        out = engine.forward(x, train)
        ctx.gen = engine.gen
        return out

    @staticmethod
    def backward(ctx, grad_out):
        e = ctx.engine
        e.check_saved(ctx.gen)
        B, _, H, W = grad_out.shape
        bufs = e.bufs[(B, H, W, grad_out.device)]
        g8 = ops.nchw_to_nhwc(grad_out.contiguous().float(), bufs.get('g_out8', (B, H, W, e.cout_pad), grad_out.device), e.cout_pad)
        e.backward(g8, need_dx=ctx.x_needs)
        grads = [e.params.grad_view(n, p.shape).clone() if p.requires_grad else None for n, p in e.m.named_parameters()]
        return (None, None, None) + tuple(grads)


class ResUnet(nn.Module):
    """Drop-in for archs/ResUnet.py:3-88 (``args`` keys: nframes, res, nf, in_nc, out_nc)."""

    def __init__(self, args=None):
        super().__init__()
        self.args = args
        self.nframes = args['nframes']
        self.cf = args['nframes'] // 2
        self.res = args['res']
        nf = self.nf = args['nf']
        self.in_nc = args['in_nc']
        self.out_nc = args['out_nc']
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
        self._engine = None

    @property
    def engine(self):
        if self._engine is None:
            object.__setattr__(self, '_engine', ResUnetEngine(self))
        return self._engine

    def forward(self, x, noise_map=None):
        params = list(self.parameters())
        train = torch.is_grad_enabled() and any(p.requires_grad for p in params)
        return _ResUnetFn.apply(x, self.engine, train, *params)

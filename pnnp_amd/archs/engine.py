"""What the two network engines (unet.py, resunet.py) share: the kernel-family policy, the weight packs, the start and end of a forward and
a backward pass, one method per layer kind and direction that calls the layer's kernel in the family the plan chose (plan.py) and keeps
the fp16x2 amax slots by that family's rule, the activation / gradient buffers, the flat parameter buffers, and the autograd Function
and nn.Module base both networks use.  An engine adds its schedule -- the order of the layers and the names of the buffers."""
import torch
import torch.nn as nn

from .. import ops
from .._lib import PnnpError
from .plan import DEFAULT_POLICY, ConvPolicy

LRELU, RELU = 1, 2


class _EngineBase:
    """What the two network engines share: the kernel-family policy and the bookkeeping that ties an autograd backward to
    the training forward whose activations it needs."""

    def _init_base(self):
        self.policy = ConvPolicy(*DEFAULT_POLICY.key()[:7])
        self._h2_sub = {}            # explicit set_policy(h2_wgrad= / h2_pointwise=) overrides: they survive later set_policy calls
        self._pol = self.policy      # the effective policy of the current forward (effective_policy)
        self.saved = None
        self.gen = 0                 # bumped by every forward that (re)writes an activation buffer set
        self._pack_key = None
        self._jobs_key = None
        self._dirty_epoch = 0
        self._plans = {}

    def _plan_for(self, B, H, W, train):
        """The per-layer plan of a forward on [B,.,H,W] (plan.py), cached per shape, mode and policy."""
        key = (B, H, W, train, self._pol.plan_key())
        if key not in self._plans:
            self._plans[key] = self._resolve(self._pol, train, B, H, W)
        return self._plans[key]

    def _pack_state_key(self, train, dev):
        return (train, dev, self._dirty_epoch, self._pol.key()) + tuple(p._version for p in self.m.parameters())

    def _packs_ready(self, train, dev, plan):
        """Start of a forward: (re-)pack the weights if the packs are not the ones this forward needs (mode, policy, parameter versions)."""
        key = self._pack_state_key(train, dev)
        if key != self._pack_key:
            self.pack_weights(train, plan)
            self._pack_key = key

    def pack_weights(self, need_dgrad, plan):
        """Re-pack every layer's weights into the kernels' K-major order in the families of ``plan``; called once per forward because the
        optimiser has moved them.  The table of pack jobs is built once per device / mode / packs / parameter storage and runs in two or
        three launches (ops.PackJobs) instead of ~70."""
        dev = self.params.flat.device
        P = dict(self.m.named_parameters())
        key = (dev, need_dgrad, plan.packs, tuple(p.data_ptr() for p in P.values()))
        if self._jobs_key != key:
            self._jobs, self._jobs_key = self._build_pack_jobs(need_dgrad, dev, P, plan), key
        self._jobs.run()

    def set_policy(self, policy=None, **kw):
        """``set_policy(x3=False)`` etc.: fields not named keep their current value."""
        if policy is None:
            cur = dict(wino=self.policy.wino, wino_wgrad=self.policy.wino_wgrad, wino_mink=self.policy.wino_mink, x3=self.policy.x3,
                       thin=self.policy.thin, pool_fused=self.policy.pool_fused, h2=self.policy.h2)
            for k in ('h2_wgrad', 'h2_pointwise', 'head_fused', 'splitk', 'convt_bits', 'unpool_fused', 'h1_eval', 'h1_pointwise', 'h1_act16', 'h1_act16_res'):   # sub-switches of h2 (host-side A/B): not constructor arguments, kept as overrides
                if k in kw:
                    self._h2_sub[k] = bool(kw.pop(k))
            if 'unpool_levels' in kw:                              # which encoder levels unpool_fused applies to (plan.py)
                self._unpool_levels = tuple(sorted(int(l) for l in kw.pop('unpool_levels')))
            cur.update(kw)
            policy = ConvPolicy(**cur)                             # (defaults of the sub-switches: environment, as at construction)
            for k, v in self._h2_sub.items():
                setattr(policy, k, v and policy.h2)
            if getattr(self, '_unpool_levels', None) is not None:
                policy.unpool_levels = self._unpool_levels
        self.policy = self._pol = policy
        self._pack_key = None        # re-pack for the other kernel family
        self._jobs_key = None

    def effective_policy(self, H, W, cs_max):
        """The policy a forward on [.,.,H,W] inputs runs with (also what its backward uses, whatever set_policy does in between).
        Every convolution kernel of the library -- bf16x3 and fp32-MFMA families alike -- addresses ONE image of a map through a
        buffer resource with 32-bit byte offsets, so the largest map of the network ([H][W][cs_max] floats) must stay below 2 GB
        per image (pnnp_x3_image_fits; ~16.7 M pixels at nf = 32).  A larger frame is refused HERE, before anything is packed or
        launched, instead of failing with PNNP_E_UNSUPPORTED somewhere inside the network: tile the frame.  (The batch-wide limit of
        the bf16x3 backward-weight kernel is different: past it the layer falls back to the fp32 kernels: plan.py.)"""
        self._needs_act16 = False
        if not ops.x3_image_fits(H, W, cs_max):
            # fp16 storage (Plan.act16): the conv / pooled / up-sampled maps are 2-byte tensors, so THEIR bound doubles (~33 M pixels at nf = 32); x8 and the
            # padded output keep the 4-byte one.  Whether this forward's plan has fp16 storage is known once it is resolved: _forward_begin refuses then.
            pol = self.policy
            if (pol.h1_eval and pol.h1_pointwise and pol.h1_act16 and ops.image_fits(H, W, cs_max, 2)
                    and ops.image_fits(H, W, max(self.cin_pad, self.cout_pad), 4)):
                self._needs_act16 = True
                return pol
            raise PnnpError(f'frame {H} x {W} is too large for the HIP convolution kernels: one image of a {cs_max}-channel map must stay '
                            f'below 2 GB ((H + 4) * W * {cs_max} * 4 bytes); run the frame in tiles: evaluate(..., tiles=dict(patch_size=...)) / '
                            f'forward_tiled (pnnp_amd/evaluate.py)')
        return self.policy

    def h2_range_report(self, sample=1 << 22):
        """Debug aid for the fp16x2 family's ONE precision caveat (csrc/h2.h): the scale is per TENSOR, so elements below
        2^-18 of a tensor's largest magnitude keep only absolute accuracy (2^-40 of that maximum).  After a training forward + backward this walks the
        tensors the kernels split on the fly -- the saved activations and the gradient buffers of that step -- and returns, per tensor,
        ``dict(name, kind, amax, median, log2_ratio = log2(amax / median |x|), frac_small, l2_small)``: ``median`` over the non-zero elements
        of a strided sample, ``frac_small`` the share of non-zero elements below 2^-18 amax, ``l2_small`` the share of the tensor's sum of squares they
        carry (what an output that depends on them alone would lose).  Plain torch ops: for tools and tests (tools/soak.py), never on the hot path."""
        if self.saved is None:
            raise PnnpError('h2_range_report: no saved training forward')
        a, key, _ = self.saved
        rows = []

        def add(name, kind, t):
            if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != 4:
                return
            v = t.reshape(-1)
            amax = float(v.abs().max())
            step = max(1, v.numel() // sample)
            sv = v[::step].abs()
            nz = sv[sv > 0]
            if amax == 0.0 or nz.numel() == 0 or not torch.isfinite(sv).all():
                rows.append(dict(name=name, kind=kind, amax=amax, median=0.0, log2_ratio=float('nan'), frac_small=0.0, l2_small=0.0))
                return
            med = float(nz.median())
            small = nz < amax * 2.0 ** -18
            rows.append(dict(name=name, kind=kind, amax=amax, median=med, log2_ratio=float(torch.log2(torch.tensor(amax / med))),
                             frac_small=float(small.float().mean()), l2_small=float((nz[small] ** 2).sum() / (nz ** 2).sum())))

        for k, t in a.items():
            if isinstance(k, str) and not k.startswith(('bits:', 'pc', '_')):
                add(k, 'act', t)
        for k, t in self.bufs[key].t.items():
            if isinstance(k, str) and k.startswith('g_') and k not in ('g_out8', 'g_out4'):
                add(k, 'grad', t)
        return rows

    def census_pairs(self):
        """(name, kind, tensor, amax slot) of every tensor an fp16x2 kernel split in the saved training step: what _Slots.of handed to the h2
        kernels of the forward and backward (kind 'act': table 'f', named as in the saved activations; 'grad': table 'b', named by buffer) and
        the weights the fp16x2 packs split against their PackJobs slots ('weight').  Empty under a policy without fp16x2 kernels."""
        if self.saved is None:
            raise PnnpError('range census: no saved training forward (run it after a training forward and backward)')
        a, key, _ = self.saved
        bufs, dev = self.bufs[key], key[3]
        act = {id(t): k for k, t in a.items() if torch.is_tensor(t) and not k.startswith(('bits:', 'pc', '_'))}
        grad = {id(t): k for k, t in bufs.t.items() if torch.is_tensor(t)}
        out, seen = [], set()
        for (which, _, sname), t in (a.get('_split') or {}).items():
            name = (act if which == 'f' else grad).get(id(t), sname)
            if (which, name) in seen:                            # one buffer under two slots (the census would show it as `over`)
                name = f'{name}@{sname}'
            seen.add((which, name))
            out.append((name, 'act' if which == 'f' else 'grad', t, bufs.slot(which, sname, dev)))
        if a['_plan'].h2:
            pname = {p.data_ptr(): n for n, p in self.m.named_parameters()}
            for w, slot in self._jobs.split_weights:
                out.append((pname.get(w.data_ptr(), '?'), 'weight', w, slot))
        return out

    def range_census(self, census=None, step=0):
        """Count the saved training step's split tensors into ``census`` (an ops.RangeCensus; None: one the engine keeps) on the current
        stream, without synchronising; returns the census.  Call it after a training forward and backward and before the optimiser moves
        the weights (HipTrainStep does, every ``range_every`` steps).  Under a policy without fp16x2 kernels nothing is counted."""
        pairs = self.census_pairs()
        if census is None:
            if getattr(self, '_census', None) is None or self._census.device != self.saved[1][3]:
                self._census = ops.RangeCensus(self.saved[1][3])
            census = self._census
        census.run(pairs, step)
        return census

    def mark_dirty(self):
        """Parameters were modified behind torch's back (fused Adam on the flat buffer)."""
        self._dirty_epoch += 1

    def _begin_forward(self, key, train):
        """Activation buffers are per input shape and reused: a later forward on the same shape overwrites what an earlier
        training forward saved for its backward.  Every forward gets a generation number; `saved` remembers the one it
        belongs to and is dropped when its buffers are about to be overwritten by a forward that does not replace it."""
        self.gen += 1
        if self.saved is not None and self.saved[1] == key and not train:
            self.saved = None
        return self.gen

    def check_saved(self, gen):
        if self.saved is None or self.saved[2] != gen:
            raise PnnpError('backward: the activations of this forward were overwritten by a later forward on the same input shape '
                            '(the HIP engine keeps ONE saved forward per shape: run backward before the next forward, '
                            'or accumulate gradients step by step)')

    # ------------------------------------------------------------------ construction, weights
    def _init_net(self, module):
        self._init_base()
        self.m = module
        self.params = FlatParams(module)
        self.bufs = {}
        self.packed = {}
        nf = module.nf
        if nf % 8:
            raise PnnpError(f'{type(module).__name__} on HIP needs nf % 8 == 0')
        self.ch = [nf, nf * 2, nf * 4, nf * 8, nf * 16]
        self.cin = module.in_nc * module.nframes
        self.cin_pad = (self.cin + 7) // 8 * 8
        self.cout = module.out_nc
        self.cout_pad = (self.cout + 7) // 8 * 8

    def grad_out_channels(self, B, H, W):
        """channels of the NHWC loss gradient backward() wants: the streaming head kernel takes the 4 real ones (half the bytes of the zero-padded copy)"""
        return 4 if (self.cout == 4 and self._pol.use_thin_head(self.ch[0], self.cout, B * H * W)) else self.cout_pad

    def _buf(self, key, n, dev, dtype):
        k = (key, dev)
        if k not in self.packed or self.packed[k].numel() != n:
            self.packed[k] = torch.empty(n, dtype=dtype, device=dev)
        return self.packed[k]

    PACK_CAP = 256                   # rows of the pack-job table (ops.PackJobs)

    def _pack_order(self, plan):
        return plan.steps

    def _build_pack_jobs(self, train, dev, P, plan):
        """One record per layer, in the plan's families: self._wp[name] = (forward pack, backward-data pack, the weight's amax slot).  The engine
        describes a layer (_pname: its parameters; _layer: kind '3x3' / '1x1' / 's2' / 'convt' and the padded input / output channels, None = the
        weight's own) and gives the order of the jobs (_pack_order); whether a backward-data pack exists is the plan's word (an eval plan has none)."""
        jobs = ops.PackJobs(cap=self.PACK_CAP)
        self._wp = {}
        u8, f32 = torch.uint8, torch.float32
        for name in self._pack_order(plan):
            w = P[self._pname(name)[0]]
            pf, pd = plan[name].pack
            kind, cip, cop = self._layer(name)
            b = lambda sfx, n, dt=u8: self._buf(name + sfx, n, dev, dt)
            co, ci = (w.shape[1], w.shape[0]) if kind == 'convt' else (w.shape[0], w.shape[1])
            if kind != '3x3' and pf in ('h2', 'x3', 'h1'):   # 3x3 stride 2, ConvTranspose2d 2x2 stride 2, 1x1: the pointwise fp16x2 / bf16x3 / fp16x1 GEMM kernels
                # pack size, buffer suffix of the forward and of the backward-data pack ('h1': eval plans under h1_pointwise, the one-piece forward pack alone)
                mat, sf, sd = {'h2': (ops.h2mat_bytes, ':h2mf', ':h2md'), 'x3': (ops.x3mat_bytes, ':x3f', ':x3d'), 'h1': (ops.h1_pointwise_weight_bytes, ':h1mf', None)}[pf]
                if kind == 's2':                       # (K, N) of the forward GEMM, of the backward-data GEMM, and how many of those
                    fkn, dkn, nd = (9 * ci, co), (co, ci), 9
                elif kind == 'convt':
                    fkn, dkn, nd = (ci, 4 * co), (4 * co, ci), 1
                else:
                    fkn, dkn, nd = (ci, co), (co, ci), 1
                f, d = b(sf, mat(*fkn)), b(sd, nd * mat(*dkn)) if pd and sd else None
                self._wp[name] = (f, d, getattr(jobs, f'add_{pf}_{kind}')(*((w, f) if sd is None else (w, f, d))))
                continue
            if kind in ('s2', 'convt'):                # the direct kernels (their own weight layouts)
                f, d = b(':f', w.numel(), f32), b(':d', w.numel(), f32) if pd else None
                if kind == 'convt':
                    jobs.add_convt(w, f, d)
                else:
                    jobs.add_conv(w, f, None)
                    if pd:
                        jobs.add_s2_dgrad(w, d)
                self._wp[name] = (f, d, None)
                continue
            taps = w.shape[2] * w.shape[3]
            cip, cop = cip or ci, cop or co
            got, slot = {}, None
            if pf == 'h1':                             # (eval plans under h1_eval) the one-piece forward pack; no backward-data pack exists
                got['h1'] = (b(':h1f', ops.h1_weight_bytes(cip, co)), None)
                slot = jobs.add_h1(w, got['h1'][0], cin_pad=(cip + 15) // 16 * 16)
            if 'h2' in (pf, pd):                       # the fp16x2 kernel takes what bf16x3 would have taken
                got['h2'] = (b(':h2f', ops.h2_weight_bytes(cip, co)) if pf == 'h2' else None, b(':h2d', ops.h2_weight_bytes(co, ci)) if pd == 'h2' else None)
                slot = jobs.add_h2(w, *got['h2'], cin_pad=(cip + 15) // 16 * 16)
            if 'direct' in (pf, pd):
                got['direct'] = (b(':f', taps * cip * co, f32) if pf == 'direct' else None, b(':d', taps * cop * ci, f32) if pd == 'direct' else None)
                jobs.add_conv(w, *got['direct'], cin_pad=cip, cout_pad=cop)
            if 'x3' in (pf, pd):
                got['x3'] = (b(':x3f', ops.x3_weight_bytes(cip, co)) if pf == 'x3' else None, b(':x3d', ops.x3_weight_bytes(co, ci)) if pd == 'x3' else None)
                jobs.add_x3(w, *got['x3'], cin_pad=(cip + 15) // 16 * 16)
            if 'wino' in (pf, pd):
                got['wino'] = (b(':uf', 16 * co * ci, f32) if pf == 'wino' else None, b(':ud', 16 * co * ci, f32) if pd == 'wino' else None)
                jobs.add_wino(w, *got['wino'])
            self._wp[name] = (got[pf][0], got[pd][1] if pd else None, slot)
        return jobs

    # ------------------------------------------------------------------ the start and end of a pass
    def _forward_begin(self, x, train, reflect_pad, add_residual, tile_src=None):
        """Input checks, the plan and the packs of this forward, its buffers and the activations' amax slots: (x, (B, H, W, dev), plan, bufs,
        parameters, T).  H, W are the size the network runs on (the frame + 2 reflect_pad).  With ``tile_src`` = (frame [1,C,h,w], grid, t0, nt)
        the batch is the tiles t0 .. t0 + nt of the frame (tiles.TileGrid): B = nt, H = W = patch_size, and ``x`` comes back as the frame."""
        if tile_src is not None:
            x, grid, t0, nt = tile_src
            if train or reflect_pad:
                raise PnnpError('tile_src is an eval-mode option and excludes reflect_pad (a tile carries its own border)')
        if not torch.is_tensor(x) or not x.is_cuda:
            raise PnnpError(f'{type(self.m).__name__}.forward: input must be a CUDA tensor (pnnp_amd has no CPU path)')
        x = x.contiguous().float()
        B, Cin, H, W = x.shape
        if tile_src is not None:
            if B != 1 or (H, W) != (grid.h, grid.w) or t0 < 0 or nt < 1 or t0 + nt > grid.T:
                raise PnnpError(f'tile_src: frame {tuple(x.shape)} / tiles [{t0}, {t0 + nt}) do not match the {grid.h} x {grid.w} grid of {grid.T} tiles')
            B, H, W = nt, grid.patch_size, grid.patch_size
        if reflect_pad:
            if train or (self.m.res and add_residual):
                raise PnnpError('reflect_pad is an eval-mode option; a `res` network needs add_residual=False (the caller adds the input after cropping)')
            H, W = H + 2 * reflect_pad, W + 2 * reflect_pad
        # (a frame past the kernels' size limit is told so, and where to go, whatever else is wrong with it: such a frame is rarely a multiple of 16)
        self._pol = self.effective_policy(H, W, max(self.ch[0], self.cin_pad, self.cout_pad))
        if Cin != self.cin or H % 16 or W % 16:
            raise PnnpError(f'input must be [B,{self.cin},H,W] with H,W multiples of 16, got {tuple(x.shape)}')
        dev = x.device
        self.params.ensure(dev)
        # packed weights are re-used while no parameter changed (eval loops); in-place torch updates bump
        # tensor._version, the fused Adam kernel goes through mark_dirty()
        plan = self._plan = self._plan_for(B, H, W, train)
        if self._needs_act16 and not plan.act16:
            raise PnnpError(f'frame {H} x {W} is too large for float32 activation maps (one image of a map must stay below 2 GB) and this forward has no fp16 '
                            f'storage (ConvPolicy.h1_act16 -- for ResUnet with ConvPolicy.h1_act16_res -- takes effect in eval plans whose layers all run on fp16x1): '
                            f'run the frame in tiles (forward_tiled)')
        self._packs_ready(train, dev, plan)
        key = (B, H, W, dev)
        self._begin_forward(key, train)
        bufs = self.bufs.setdefault(key, _Bufs())
        # fp16x2 family (csrc/h2.h): amax slots of the activations (keyed by the name of the layer that wrote the tensor) and, in a training
        # forward, the sign bits of every activation output that backward-data will need as a mask; the log: what the fp16x2 kernels split in
        # this step (range census)
        T = _Slots(bufs, 'f', dev, plan.h2, log={} if train else None)
        return x, key, plan, bufs, dict(self.m.named_parameters()), T

    def _layout_in(self, x, x8, reflect_pad, amax, tile_src, bufs, dev):
        """The network input's layout pass into ``x8`` (zero-padded-channel NHWC): -> (x8, the NCHW input a `res` head adds).  With ``tile_src``
        the tile-crop kernel gathers the batch straight out of the frame ``x``; the NCHW tiles are written (same launch) only for a `res` network."""
        if tile_src is None:
            return ops.nchw_to_nhwc(x, x8, self.cin_pad, reflect_pad=reflect_pad, amax=amax), x
        _, grid, t0, nt = tile_src
        P = grid.patch_size
        xt = bufs.get('x_tiles', (nt, self.cin, P, P), dev) if self.m.res else None
        ops.tile_crop(x, grid, t0, nt, nchw=xt, nhwc=x8, amax=amax)
        return x8, xt

    def act16_range(self):
        """Debug aid for the ONE caveat of fp16 activation storage (Plan.act16): a stored map is float16(y), unscaled and not saturated, so
        |y| > 65504 becomes inf.  Per stored map of the last eval forward that ran with fp16 storage: ``dict(name, amax, overflow)``, amax = max |y| of the
        float32 values BEFORE the rounding (the layers' amax slots), overflow = 65504 < amax < inf: THIS layer computed finite values that fp16 cannot hold;
        ``inherited`` = amax is inf (a map downstream of an overflow: it read the inf).  Synchronises; never on the forward path."""
        if getattr(self, '_act16_last', None) is None:
            raise PnnpError('act16_range: no eval forward with fp16 activation storage has run (ConvPolicy.h1_act16, Plan.act16)')
        names, slots = self._act16_last
        vals = torch.stack([s.reshape(()) for s in slots]).cpu().view(torch.float32).tolist()
        return [dict(name=n, amax=v, overflow=65504.0 < v < float('inf'), inherited=v == float('inf')) for n, v in zip(names, vals)]

    def _forward_end(self, a, key, plan, T):
        if plan.act16:                         # the stored fp16 maps' slots, by layer (conv9_2's map is never stored: the head is in its epilogue; ResUnet's head writes float32)
            names = [n for n in plan.steps if n not in ('conv9_2', 'conv10_1', 'conv10')]
            self._act16_last = (names, [T.slot(n) for n in names])
        if plan.train:
            a['_plan'] = plan
            a['_src_name'] = T.names
            a['_split'] = T.log
            self.saved = (a, key, self.gen)

    def _backward_begin(self):
        """The saved forward's (activations, (B, H, W, dev), plan, buffers, parameters, G, backward-weight workspace, F, T): a backward runs on the
        kernel families of its own forward; G: FlatParams.grad_of; F: the forward's amax slots, T: the gradients' (keyed by buffer name, zeroed
        per backward)."""
        a, key, _ = self.saved
        plan = self._plan = a['_plan']
        self._pol = plan.pol
        bufs, dev = self.bufs[key], key[3]
        P = dict(self.m.named_parameters())
        G = self.params.grad_of
        F = _Slots(bufs, 'f', dev, False, names=a['_src_name'], log=a['_split'])
        T = _Slots(bufs, 'b', dev, plan.h2, log=a['_split'])
        return a, key, plan, bufs, P, G, bufs.get('wgrad_ws', (plan.ws,), dev), F, T

    # ---- one call per layer kind and direction, in the family the plan chose (self._wp: the layer's packs and weight amax slot; T / F: the _Slots
    # of the pass / of the forward's activations; a: the forward's activations, where the sign-bit images live as 'bits:' + layer)
    def _in_amax(self, plan, name, T):
        """the slot the input's layout pass fills: only an fp16x2 first layer splits the network input"""
        return T.slot('x8') if plan[name].fwd in ('h2', 'h1') else None

    def _bits(self, plan, name, T, a, y, cout, act):
        """the sign-bit image an fp16x2 forward writes beside an activation output in a training forward"""
        if not (plan.train and act):
            return None
        B, h, w, _ = y.shape
        bits = a['bits:' + name] = T.bufs.bits(name, B, h, w, cout, T.dev)
        return bits

    @staticmethod
    def _op(name):
        """The ops wrapper of a layer in one of the two fp16 families, by its per-family name ('conv_h1_fwd_pool'): one arm serves 'h2' and 'h1'.  Looked up
        per call and under that name, so that whatever wraps ``ops.conv_h2_fwd`` & co. to record their operands (tests/test_gpu_range_census.py) sees the call."""
        return getattr(ops, name)

    @staticmethod
    def _fam(fwd):
        """a forward's family string (plan.py) as (family, variant): 'h1+splitk' -> ('h1', 'splitk'), 'x3' -> ('x3', '')"""
        fam, _, var = fwd.partition('+')
        return fam, var

    def _conv3_fwd(self, plan, name, T, a, x1, x2, bias, y, cout, act, residual=None, fill=None):
        """``fill``: x1 has no amax yet (no producer with a fused one): an fp16 layer fills slot ``fill`` with a launch of its own first"""
        s, (f, _, wslot) = plan[name], self._wp[name]
        fam, var = self._fam(s.fwd)
        f16 = fam in ('h2', 'h1')                            # both fp16 families: one arm, the family picks the ops wrapper (h1: eval plans only)
        if plan.act16:                                       # fp16 storage: every layer is 'h1...'; the element types are the tensors' dtypes (x8 alone is float32)
            if fill is not None and x1.dtype == torch.float32:      # (ResUnet's x8 on the matrix-core first layer: a launch of its own fills the slot)
                T.put(x1, fill, fused=False)
            ax1 = T.of(x1) if x1.dtype == torch.float32 else None
            if residual is not None:                         # (ResUnet: an fp16 shortcut added to the float32 sum before the one rounding)
                assert var == '', 'a residual layer is a plain launch'
                ops.conv_h1a_fwd(x1, x2, f, wslot, bias, y, cout, act, amax_x1=ax1, amax_y=T.slot(name), residual=residual)
            elif var == 'splitk':
                ops.conv_h1a_fwd_splitk(x1, x2, f, wslot, bias, y, cout, act, s.ks, T.bufs.scratch('splitk_ws', s.ks * y.numel(), T.dev), amax_x1=ax1, amax_y=T.slot(name))
            else:
                ops.conv_h1a_fwd(x1, x2, f, wslot, bias, y, cout, act, amax_x1=ax1, amax_y=T.slot(name))
            return T.put(y, name, fused=True)
        if f16:
            bits = self._bits(plan, name, T, a, y, cout, act) if fam == 'h2' and residual is None else None      # sign bits: fp16x2 only
            if fill is not None:
                T.put(x1, fill, fused=False)
            ax1, ax2 = T.of(x1), T.of(x2) if x2 is not None else None
            if var == 'splitk':                              # a small grid: K in slices, one reduce (bias, activation, amax, sign bits)
                self._op(f'conv_{fam}_fwd_splitk')(x1, x2, f, wslot, bias, y, cout, act, ax1, s.ks, T.bufs.scratch('splitk_ws', s.ks * y.numel(), T.dev),
                                                   amax_x2=ax2, amax_y=T.slot(name), bits_y=bits)
            else:
                self._op(f'conv_{fam}_fwd')(x1, x2, f, wslot, bias, y, cout, act, ax1, ax2, amax_y=T.slot(name), bits_y=bits, residual=residual)
        elif s.fwd == 'x3':
            ops.conv_x3_fwd(x1, x2, f, bias, y, cout, act, residual=residual)
        elif s.fwd == 'wino':
            ops.conv_wino_fwd(x1, x2, f, bias, y, cout, act, residual=residual)
        else:
            ops.conv_fwd(x1, x2, f, bias, y, cout, 9, act, residual=residual)
        return T.put(y, name, fused=f16)

    def _first_fwd(self, plan, name, T, a, x, w, bias, y, cout, act, fill=None):
        if plan[name].fwd != 'thin':
            return self._conv3_fwd(plan, name, T, a, x, None, bias, y, cout, act, fill=fill)
        # the first layer on the streaming kernel: its 4 input channels are not worth a (padded) GEMM chunk.  (With the fp16x2 family the
        # matrix-core kernel is as fast -- a padded chunk is 14 instructions, not 27 -- and writes the sign bits that make the next layer's
        # backward-data read 1/32 of the bytes: the streaming kernel keeps the first layer's weight gradient only.)
        if plan.act16:                         # (fp16 storage: float16(y) out of the streaming kernel, max |y| of the float32 value into the slot)
            ops.first_fwd_et(x, w, bias, y, act, amax_y=T.slot(name))
            return T.put(y, name, fused=True)
        ops.first_fwd(x, w, bias, y, act, amax_y=T.slot(name) if plan.h2 else None)
        return T.put(y, name, fused=True)

    def _conv3_pool_fwd(self, plan, name, T, a, x, bias, y, pooled, codes, cout, act):
        """a 3x3 layer and the MaxPool2d(2) behind it: y, pooled and (if not None) the argmax + sign codes"""
        s, (f, _, wslot) = plan[name], self._wp[name]
        fam, var = self._fam(s.fwd)
        if plan.act16:
            if var == 'pool':
                ops.conv_h1a_fwd_pool(x, None, f, wslot, bias, y, pooled, codes, cout, act, amax_y=T.slot(name))
                T.put(y, name, fused=True)
            else:                              # (a split-K launch has no pool in its epilogue)
                self._conv3_fwd(plan, name, T, a, x, None, bias, y, cout, act)
                ops.maxpool_fwd_f16(y, pooled)
            return y
        if var == 'pool' and fam in ('h2', 'h1'):
            # the layer writes the pooled map, the codes, its amax (the pooled map is a subset) and (fp16x2) the sign bits from its own epilogue
            self._op(f'conv_{fam}_fwd_pool')(x, None, f, wslot, bias, y, pooled, codes, cout, act, T.of(x), amax_y=T.slot(name),
                                             bits_y=self._bits(plan, name, T, a, y, cout, act) if fam == 'h2' else None)
            T.put(y, name, fused=True)
        elif s.fwd == 'x3+pool':
            # the layer writes the pooled map and the codes from its own epilogue (csrc/conv_x3s.hip)
            ops.conv_x3_fwd_pool(x, None, f, bias, y, pooled, codes, cout, act)
            T.put(y, name, fused=False)
        else:                                  # (also a split-K launch: it has no fused pool)
            self._conv3_fwd(plan, name, T, a, x, None, bias, y, cout, act)
            ops.maxpool_fwd(y, pooled, codes=codes)
        return y

    def _conv3_head_fwd(self, plan, name, hname, T, a, x, bias, yshape, act, hw, hb, out, res):
        """The last 3x3 layer (its output: buffer ``name``, yshape) and the 1x1 head behind it, into ``out`` (NCHW, + res).  Returns the 3x3
        layer's output, or None where it was never stored."""
        if plan[hname].fwd != 'fused':
            y = self._conv3_fwd(plan, name, T, a, x, None, bias, T.bufs.get(name, yshape, T.dev), yshape[3], act)
            self._head_fwd(plan, hname, T, y, hw, hb, out, res)
            return y
        # both layers in one kernel (csrc/conv_s.h EK_HEAD; fp16x2 or, in eval plans, fp16x1): the output planes come straight from the accumulators; the
        # 3x3 layer's map is stored (with its sign bits and amax) only for a backward pass -- an eval forward neither writes nor re-reads it
        f, _, wslot = self._wp[name]
        fam = self._fam(plan[name].fwd)[0]
        if plan.act16:                         # fp16 source, float32 NCHW out, nothing else stored
            ops.conv_h1a_fwd_head(x, None, f, wslot, bias, yshape[3], act, hw, hb, out, residual=res)
            return None
        y = T.bufs.get(name, yshape, T.dev) if plan.train else None
        self._op(f'conv_{fam}_fwd_head')(x, None, f, wslot, bias, y, yshape[3], act, T.of(x), hw, hb, out, amax_y=T.slot(name) if plan.train else None,
                                         bits_y=self._bits(plan, name, T, a, y, yshape[3], act) if fam == 'h2' else None, residual=res)
        return T.put(y, name, fused=True) if plan.train else None

    def _head_fwd(self, plan, name, T, x, w, bias, out, res):
        """the 1x1 head on its own: x (NHWC) -> out (NCHW, + res)"""
        if plan.act16 and x.dtype == torch.float16:      # (ResUnet's fp16 c9: the streaming head widens it, or the 1x1 GEMM below would need a float32 copy)
            assert plan[name].fwd == 'thin', 'an fp16-storage plan has its head on the streaming kernel'
            ops.head_fwd_et(x, w, bias, out, residual=res)
        elif plan[name].fwd == 'thin':
            ops.head_fwd(x, w, bias, out, residual=res)
        else:
            o = ops.conv_fwd(x, None, self._wp[name][0], bias, T.bufs.get('o', tuple(x.shape[:3]) + (self.cout,), T.dev), self.cout, 1, 0)
            ops.nhwc_to_nchw(o, out, residual=res)

    def _head_bwd(self, plan, name, F, T, g, x, w, gx, dW, db, ws, acc, mode):
        """backward of the 1x1 head: dW, db and gx (slot 'head'); ``mode``: x is that activation's output (0: none)"""
        if plan[name].dgrad == 'thin':
            ops.head_bwd(g, x, w, gx, dW, db, ws, mode=mode, accumulate=acc, amax_gx=T.slot('head') if plan.h2 else None)
            return T.put(gx, 'head', fused=True)
        self._wgrad(plan[name].wgrad, F, T, g, self.cout, x, self.ch[0], None, dW, db, ws, acc, taps=1)
        ops.conv_bwd_data(g, self._wp[name][1], gx, mask1=x if mode else None, mode1=mode, taps=1)
        return T.put(gx, 'head', fused=False)

    def _conv3_dgrad(self, plan, name, a, F, T, gsrc, dx1, **kw):
        _, d, wslot = self._wp[name]
        dx2, fam = kw.get('dx2'), plan[name].dgrad
        if fam == 'h2':
            # the act' masks as the forward kernels' sign bits where the masking activation came out of an fp16x2 layer
            for k_mask, k_bits in (('mask1', 'bits1'), ('mask2', 'bits2')):
                m = kw.get(k_mask)
                if m is not None and ('bits:' + F.names.get(id(m), '?')) in a:
                    kw[k_bits], kw[k_mask] = a['bits:' + F.names[id(m)]], None
            T.names[id(dx1)] = 'd1:' + name
            if dx2 is not None:
                T.names[id(dx2)] = 'd2:' + name
            ops.conv_h2_bwd_data(gsrc, T.of(gsrc), d, wslot, dx1, amax_dx1=T.slot('d1:' + name), amax_dx2=T.slot('d2:' + name) if dx2 is not None else None, **kw)
            return
        if fam == 'x3':
            ops.conv_x3_bwd_data(gsrc, d, dx1, **kw)
        elif fam == 'wino':
            ops.conv_wino_bwd_data(gsrc, d, dx1, **kw)
        else:
            ops.conv_bwd_data(gsrc, d, dx1, **kw)
        T.put(dx1, 'd1:' + name, fused=False)
        if dx2 is not None:
            T.put(dx2, 'd2:' + name, fused=False)

    def _conv3_dgrad_res(self, plan, name, T, gsrc, dx, addsrc, mask, mode, slot):
        """backward-data through an identity shortcut: dx = (dgrad(gsrc) + addsrc) * act'(mask).  Only the fp16x2 kernel leaves dx's amax (``slot``);
        after the others the first fp16x2 kernel that splits dx fills it (_Slots.of)."""
        _, d, wslot = self._wp[name]
        fam = plan[name].dgrad
        if fam == 'h2+res':
            ops.conv_h2_bwd_data_res(gsrc, T.of(gsrc), d, wslot, dx, addsrc=addsrc, mask=mask, mode=mode, amax_dx=T.slot(slot))
            T.put(dx, slot, fused=True)
        elif fam == 'x3+res':
            ops.conv_x3_bwd_data_res(gsrc, d, dx, addsrc=addsrc, mask=mask, mode=mode)
        elif fam == 'wino+res':
            ops.conv_wino_bwd_data_res(gsrc, d, dx, addsrc=addsrc, mask=mask, mode=mode)
        else:
            ops.conv_bwd_data_res(gsrc, d, dx, addsrc=addsrc, mask=mask, mode=mode)

    def _conv3_dgrad_cols(self, name, T, gsrc, col0, dx, slot, **kw):
        """One half of a two-input layer's fp16x2 backward-data (Step.unpool): columns [col0, col0 + C) of its pack into dx [.., C], dx's amax into
        ``slot``; with gp / codes it adds MaxPool2d's backward before it stores (csrc/conv_h2s.hip EK_BWDU)."""
        _, d, wslot = self._wp[name]
        T.names[id(dx)] = slot
        ops.conv_h2_bwd_data_unpool(gsrc, T.of(gsrc), d, wslot, col0, 2 * dx.shape[3], dx, amax_dx=T.slot(slot), **kw)

    @staticmethod
    def _wgrad(fam, F, T, gpre, cout, x1, c1, x2, dW, db, ws, acc, taps=9):
        """backward-weight of a 3x3 (taps 9) or 1x1 (taps 1) layer"""
        if fam == 'h2':
            (ops.conv1x1_h2_bwd_weight if taps == 1 else ops.conv_h2_bwd_weight)(gpre, T.of(gpre), cout, x1, F.of(x1), c1, x2, F.of(x2) if x2 is not None else None,
                                                                                  dW, db, ws, accumulate=acc)
        elif fam == 'x3':
            (ops.conv1x1_x3_bwd_weight if taps == 1 else ops.conv_x3_bwd_weight)(gpre, cout, x1, c1, x2, dW, db, ws, accumulate=acc)
        elif fam == 'wino':
            ops.conv_wino_bwd_weight(gpre, cout, x1, c1, x2, dW, db, ws, accumulate=acc)
        elif fam == 'thin':
            ops.first_bwd_weight(gpre, cout, x1, c1, dW, db, ws, accumulate=acc)
        else:
            ops.conv_bwd_weight(gpre, cout, x1, c1, x2, dW, db, taps, ws, accumulate=acc)

    def _s2_fwd(self, plan, name, T, x, bias, y, cout):
        f, _, wslot = self._wp[name]
        fam = plan[name].fwd
        if plan.act16:
            ops.conv_s2_h1a_fwd(x, f, wslot, bias, y, cout, 0, amax_y=T.slot(name))
            return T.put(y, name, fused=True)
        if fam in ('h2', 'h1'):                              # ('h1': eval plans only, ConvPolicy.h1_pointwise)
            self._op(f'conv_s2_{fam}_fwd')(x, T.of(x), f, wslot, bias, y, cout, 0, amax_y=T.slot(name))
        elif fam == 'x3':
            ops.conv_s2_x3_fwd(x, f, bias, y, cout, amax_y=T.slot(name) if plan.h2 else None)
        else:
            ops.conv_s2_fwd(x, f, bias, y, cout)
        return T.put(y, name, fused=fam != 'direct')

    def _s2_wgrad(self, plan, name, F, T, g, x, dW, db, ws, acc, fill):
        """``fill``: g's slot, should no kernel have left g's amax yet (_conv3_dgrad_res)"""
        fam = plan[name].wgrad
        if fam == 'h2':
            ops.conv_s2_h2_bwd_weight(g, T.of(g, fill), x, F.of(x), dW, db, ws, accumulate=acc)
        elif fam == 'x3':       # (the fp16x2 kernel also has a tile for Cout = 64: pool1, which bf16x3 leaves to the fp32-MFMA kernel)
            ops.conv_s2_x3_bwd_weight(g, x, dW, db, ws, accumulate=acc)
        else:
            ops.conv_s2_bwd_weight(g, x, dW, db, ws, accumulate=acc)

    def _s2_dgrad_acc(self, plan, name, T, g, dx, fill):
        """dx += backward-data of a stride-2 layer (dx already holds the skip gradient); ``fill`` as in _s2_wgrad"""
        _, d, wslot = self._wp[name]
        fam = plan[name].dgrad
        if fam == 'h2':
            ops.conv_s2_h2_bwd_data(g, T.of(g, fill), d, wslot, dx, accum=1, amax_dx=T.slot(name))
        elif fam == 'x3':
            ops.conv_s2_x3_bwd_data(g, d, dx, accum=1, amax_dx=T.slot(name) if plan.h2 else None)   # (the sums it stored: skip gradient + this layer's)
        else:
            ops.conv_s2_bwd_data(g, d, dx, accum=1)
        return T.put(dx, name, fused=fam != 'direct')

    def _conv1_fwd(self, plan, name, T, x1, x2, bias, y, cout, act):
        f, _, wslot = self._wp[name]
        fam = plan[name].fwd
        if plan.act16:                         # (its amax slot: what act16_range reports for the shortcut map)
            ops.conv1x1_h1a_fwd(x1, x2, f, wslot, bias, y, cout, act, amax_y=T.slot(name))
            return T.put(y, name, fused=True)
        if fam in ('h2', 'h1'):
            self._op(f'conv1x1_{fam}_fwd')(x1, T.of(x1), x2, T.of(x2), f, wslot, bias, y, cout, act)
        elif fam == 'x3':
            ops.conv1x1_x3_fwd(x1, x2, f, bias, y, cout, act)
        else:
            ops.conv_fwd(x1, x2, f, bias, y, cout, 1, act)
        return y

    def _conv1_dgrad_acc(self, plan, name, T, g, dx1, dx2, slot):
        """dx1, dx2 += backward-data of a 1x1 layer on cat([x1, x2]).  The gradient is ACCUMULATED into dx1 and dx2: their slots are stale from here
        on.  An fp16x2 layer reports max |sum| of dx1 in ``slot`` (the plan runs ConvTranspose2d's backward on fp16x2 only then); dx2's stays stale."""
        T.names.pop(id(dx1), None)
        T.names.pop(id(dx2), None)
        _, d, wslot = self._wp[name]
        fam = plan[name].dgrad
        if fam == 'h2':
            ops.conv1x1_h2_bwd_data(g, T.of(g), d, wslot, dx1, accum1=1, amax_dx1=T.slot(slot), dx2=dx2, accum2=1)
            T.put(dx1, slot, fused=True)
        elif fam == 'x3':
            ops.conv1x1_x3_bwd_data(g, d, dx1, accum1=1, dx2=dx2, accum2=1)
        else:
            ops.conv_bwd_data(g, d, dx1, accum1=1, dx2=dx2, accum2=1, taps=1)

    def _convt_fwd(self, plan, name, T, x, bias, y, cout):
        f, _, wslot = self._wp[name]
        fam = plan[name].fwd
        if plan.act16:
            ops.convt_h1a_fwd(x, f, wslot, bias, y, cout, amax_y=T.slot(name))
            return T.put(y, name, fused=True)
        if fam in ('h2', 'h1'):
            self._op(f'convt_{fam}_fwd')(x, T.of(x), f, wslot, bias, y, cout, amax_y=T.slot(name))
        elif fam == 'x3':
            ops.convt_x3_fwd(x, f, bias, y, cout, amax_y=T.slot(name) if plan.h2 else None)
        else:
            ops.convt_fwd(x, f, bias, y, cout)
        return T.put(y, name, fused=fam != 'direct')

    def _convt_wgrad(self, plan, name, F, T, x, g, dW, db, ws, acc):
        fam = plan[name].wgrad
        if fam == 'h2':
            ops.convt_h2_bwd_weight(x, F.of(x), g, T.of(g), dW, ws, accumulate=acc, dbias=db)
        elif fam == 'x3':
            ops.convt_x3_bwd_weight(x, g, dW, ws, accumulate=acc, dbias=db)
        else:
            ops.convt_bwd_weight(x, g, dW, ws, accumulate=acc, dbias=db)

    def _convt_dgrad(self, plan, name, T, g, dx, mask=None, mode=0, bits=None):
        _, d, wslot = self._wp[name]
        fam = plan[name].dgrad
        if fam == 'h2':
            ops.convt_h2_bwd_data(g, T.of(g), d, wslot, dx, mask=mask, mode=mode, amax_dx=T.slot(name), bits=bits)
        elif fam == 'x3':
            ops.convt_x3_bwd_data(g, d, dx, mask=mask, mode=mode, amax_dx=T.slot(name) if plan.h2 else None)
        else:
            ops.convt_bwd_data(g, d, dx, mask=mask, mode=mode)
        return T.put(dx, name, fused=fam != 'direct')


class _Slots:
    """fp16x2 amax-slot bookkeeping of one pass (csrc/h2.h): table 'f' (activations, zeroed when a forward starts) or 'b' (gradients,
    zeroed when a backward starts).  ``put`` records which slot a tensor's amax is in -- its producer wrote it (fused) or, when ``on``
    (some layer of the plan runs on an fp16x2 kernel), a standalone amax launch fills it here."""

    def __init__(self, bufs, which, dev, on, names=None, log=None):
        self.bufs, self.which, self.dev, self.on = bufs, which, dev, on
        self.names = {} if names is None else names          # id(tensor) -> slot name
        self.log = log                                       # a training step's split operands for the range census (None: not recorded)
        if on:
            bufs.slots(which, dev).zero_()

    def slot(self, name):
        return self.bufs.slot(self.which, name, self.dev)

    def put(self, t, name, fused):
        self.names[id(t)] = name
        if self.on and not fused:
            ops.amax(t, self.slot(name))
        return t

    def of(self, t, fill=None):
        """The slot of ``t`` for an fp16x2 kernel that splits ``t`` (every caller hands it to one as an operand's amax); recorded for the range
        census (_EngineBase.census_pairs).  ``fill``: where no kernel has left ``t``'s amax yet, a launch of its own fills slot ``fill`` first."""
        if fill is not None and id(t) not in self.names:
            self.put(t, fill, fused=False)
        name = self.names[id(t)]
        if self.log is not None:
            self.log[(self.which, id(t), name)] = t
        return self.slot(name)


class FlatParams:
    """All parameters (and their gradients) of a module as views of two flat fp32 buffers,
    16-byte aligned per tensor: one fused Adam launch and one (bucketed) all-reduce."""

    def __init__(self, module):
        self.module = module
        self.flat = None
        self.grad = None
        self.slices = {}
        self._grad_of = {None: None}     # grad_of's views of the current flat gradient buffer

    def ensure(self, device):
        ps = list(self.module.named_parameters())
        ok = self.flat is not None and self.flat.device == device and all(
            p.data_ptr() == self.flat.data_ptr() + 4 * self.slices[n][0] for n, p in ps)
        if ok:
            return
        off = 0
        self.slices = {}
        for n, p in ps:
            self.slices[n] = (off, p.numel())
            off += (p.numel() + 3) // 4 * 4
        flat = torch.zeros(off, dtype=torch.float32, device=device)
        grad = torch.zeros(off, dtype=torch.float32, device=device)
        for n, p in ps:
            o, k = self.slices[n]
            flat[o:o + k].copy_(p.data.reshape(-1).to(device=device, dtype=torch.float32))
            p.data = flat[o:o + k].view(p.shape)
            p.grad = None
        self.flat, self.grad = flat, grad
        self._grad_of = {None: None}

    def grad_view(self, name, shape):
        o, k = self.slices[name]
        return self.grad[o:o + k].view(shape)

    def grad_of(self, name):
        """the gradient of parameter ``name`` in the parameter's shape: a view of the flat buffer, made once (None for None)"""
        if name not in self._grad_of:
            self._grad_of[name] = self.grad_view(name, dict(self.module.named_parameters())[name].shape)
        return self._grad_of[name]


class _Bufs:
    """Activation / gradient buffers for one input shape, allocated once and reused."""

    def __init__(self):
        self.t = {}

    def get(self, name, shape, device, dtype=torch.float32):
        """(an fp16 map of an fp16-storage eval forward -- Plan.act16 -- is keyed apart from the float32 buffer of the same layer)"""
        if dtype != torch.float32:
            name = f'{name}:{str(dtype).split(".")[-1]}'
        b = self.t.get(name)
        if b is None or tuple(b.shape) != tuple(shape) or b.device != device:
            b = torch.empty(shape, dtype=dtype, device=device)
            self.t[name] = b
        return b

    def scratch(self, name, n, device):
        """a 1-D float32 scratch buffer of at least n elements (grows, never shrinks)"""
        b = self.t.get(name)
        if b is None or b.numel() < n or b.device != device:
            b = self.t[name] = torch.empty(int(n), dtype=torch.float32, device=device)
        return b

    # ---- fp16x2 family (csrc/h2.h): one 4-byte amax slot per tensor the kernels split, in two tables -- 'f' (activations, zeroed when a
    # forward starts) and 'b' (gradients, zeroed when a backward starts) -- and the sign-bit images of the activations that serve as act' masks
    NSLOTS = 64

    def slots(self, which, device):
        key = 'slots_' + which
        t = self.t.get(key)
        if t is None or t.device != device:
            t = self.t[key] = torch.zeros(self.NSLOTS, dtype=torch.int32, device=device)
            self.t[key + '_idx'] = {}
        return t

    def slot(self, which, name, device):
        t = self.slots(which, device)
        idx = self.t['slots_' + which + '_idx']
        if name not in idx:
            if len(idx) >= self.NSLOTS:
                raise PnnpError('amax slot table full')
            idx[name] = len(idx)
        i = idx[name]
        return t[i:i + 1]

    def bits(self, name, B, H, W, C_, device):
        n = ops.h2_bits_words(B, H, W, C_)
        key = 'bits_' + name
        b = self.t.get(key)
        if b is None or b.numel() != n or b.device != device:
            b = self.t[key] = torch.empty(n, dtype=torch.int32, device=device)
        return b


class _EngineFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, engine, train, *params):
        # autograd.Function.forward runs with grad mode off: `train` is decided by the caller
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
        # autograd may keep (or accumulate in place into) what we return, and the flat buffer
        # is overwritten by the next backward: hand out copies on this compatibility path
        grads = [e.params.grad_view(n, p.shape).clone() if p.requires_grad else None for n, p in e.m.named_parameters()]
        return (None, None, None) + tuple(grads)


class _HipNet(nn.Module):
    """A network whose children only own parameters: ``forward`` runs its engine (``_engine_cls``, made on first use) as one autograd Function."""
    _engine_cls = None

    def __init__(self, args):
        super().__init__()
        self.args = args
        self.nframes = args['nframes']
        self.cf = args['nframes'] // 2
        self.res = args['res']
        self.nf = args['nf']
        self.in_nc = args['in_nc']
        self.out_nc = args['out_nc']
        self._engine = None

    @property
    def engine(self):
        if self._engine is None:
            object.__setattr__(self, '_engine', self._engine_cls(self))
        return self._engine

    def forward(self, x):
        params = list(self.parameters())
        train = torch.is_grad_enabled() and any(p.requires_grad for p in params)
        return _EngineFn.apply(x, self.engine, train, *params)

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
from .plan import DEFAULT_POLICY, ConvPolicy, resolve_unet  # noqa: F401  (ConvPolicy: re-exported)

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
            for k in ('h2_wgrad', 'h2_pointwise', 'head_fused', 'splitk', 'convt_bits', 'unpool_fused'):   # sub-switches of h2 (host-side A/B): not constructor arguments, kept as overrides
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
        if not ops.x3_image_fits(H, W, cs_max):
            raise PnnpError(f'frame {H} x {W} is too large for the HIP convolution kernels: one image of a {cs_max}-channel map must stay '
                            f'below 2 GB ((H + 4) * W * {cs_max} * 4 bytes); run the frame in tiles')
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

    # ---- one call per layer and direction, in the family the plan chose (self._wp: the layer's packs and weight amax slot; T / F: the _Slots
    # of the pass / of the forward's activations)
    def _conv3_fwd(self, plan, name, T, x1, x2, bias, y, cout, act, bits=None, residual=None, splitk_ws=None):
        s, (f, _, wslot) = plan[name], self._wp[name]
        if s.fwd == 'h2+splitk':                             # a small grid: K in slices, one reduce (bias, activation, amax, sign bits)
            ops.conv_h2_fwd_splitk(x1, x2, f, wslot, bias, y, cout, act, T.of(x1), s.ks, splitk_ws(s.ks * y.numel()),
                                   amax_x2=T.of(x2) if x2 is not None else None, amax_y=T.slot(name), bits_y=bits)
        elif s.fwd == 'h2':
            ops.conv_h2_fwd(x1, x2, f, wslot, bias, y, cout, act, T.of(x1), T.of(x2) if x2 is not None else None, amax_y=T.slot(name),
                            bits_y=bits, residual=residual)
        elif s.fwd == 'x3':
            ops.conv_x3_fwd(x1, x2, f, bias, y, cout, act, residual=residual)
        elif s.fwd == 'wino':
            ops.conv_wino_fwd(x1, x2, f, bias, y, cout, act, residual=residual)
        else:
            ops.conv_fwd(x1, x2, f, bias, y, cout, 9, act, residual=residual)
        return T.put(y, name, fused=s.fwd.startswith('h2'))

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

    def _convt_fwd(self, plan, name, T, x, bias, y, cout):
        f, _, wslot = self._wp[name]
        fam = plan[name].fwd
        if fam == 'h2':
            ops.convt_h2_fwd(x, T.of(x), f, wslot, bias, y, cout, amax_y=T.slot(name))
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

    def of(self, t):
        """The slot of ``t`` for an fp16x2 kernel that splits ``t`` (every caller hands it to one as an operand's amax); recorded for the range
        census (_EngineBase.census_pairs)."""
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

    def grad_view(self, name, shape):
        o, k = self.slices[name]
        return self.grad[o:o + k].view(shape)


class _Bufs:
    """Activation / gradient buffers for one input shape, allocated once and reused."""

    def __init__(self):
        self.t = {}

    def get(self, name, shape, device):
        b = self.t.get(name)
        if b is None or tuple(b.shape) != tuple(shape) or b.device != device:
            b = torch.empty(shape, dtype=torch.float32, device=device)
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


class UNetEngine(_EngineBase):
    """Forward / backward schedule of UNetSeeInDark over the C-ABI layer kernels."""

    def __init__(self, module):
        self._init_base()
        self.m = module
        self.params = FlatParams(module)
        self.bufs = {}
        self.packed = {}
        nf = module.nf
        self.ch = [nf, nf * 2, nf * 4, nf * 8, nf * 16]
        if nf % 8:
            raise PnnpError('UNetSeeInDark on HIP needs nf % 8 == 0')
        self.cin = module.in_nc * module.nframes
        self.cin_pad = (self.cin + 7) // 8 * 8
        self.cout = module.out_nc
        self.cout_pad = (self.cout + 7) // 8 * 8

    # ------------------------------------------------------------------ weights
    def _resolve(self, pol, train, B, H, W):
        return resolve_unet(self.ch, self.cin, self.cout, pol, train, B, H, W)

    def _conv_names(self):
        return ['conv%d_%d' % (i, j) for i in range(1, 10) for j in (1, 2)] + ['conv10_1']

    def _build_pack_jobs(self, need_dgrad, dev, P, plan):
        """One record per layer, in the plan's families: self._wp[name] = (forward pack, backward-data pack, the weight's amax slot)."""
        jobs = ops.PackJobs()
        self._wp = {}
        def buf(key, n, dt=torch.float32):
            if key not in self.packed:
                self.packed[key] = torch.empty(n, dtype=dt, device=dev)
            return self.packed[key]
        for name in self._conv_names():
            w = P[name + '.weight']
            co, ci, kh, kw = w.shape
            taps = kh * kw
            cip = self.cin_pad if name == 'conv1_1' else ci
            cop = self.cout_pad if name == 'conv10_1' else co
            pf, pd = plan[name].pack
            got, slot = {}, None
            if 'h2' in (pf, pd):
                got['h2'] = (buf((name, dev, 'h2f'), ops.h2_weight_bytes(cip, co), torch.uint8) if pf == 'h2' else None,
                             buf((name, dev, 'h2d'), ops.h2_weight_bytes(co, ci), torch.uint8) if pd == 'h2' else None)
                slot = jobs.add_h2(w, *got['h2'], cin_pad=(cip + 15) // 16 * 16)
            if 'direct' in (pf, pd):
                got['direct'] = (buf((name, dev, 'f'), taps * cip * co) if pf == 'direct' else None, buf((name, dev, 'd'), taps * cop * ci) if pd == 'direct' else None)
                jobs.add_conv(w, *got['direct'], cin_pad=cip, cout_pad=cop)
            if 'x3' in (pf, pd):
                got['x3'] = (buf((name, dev, 'x3f'), ops.x3_weight_bytes(cip, co), torch.uint8) if pf == 'x3' else None,
                             buf((name, dev, 'x3d'), ops.x3_weight_bytes(co, ci), torch.uint8) if pd == 'x3' else None)
                jobs.add_x3(w, *got['x3'], cin_pad=(cip + 15) // 16 * 16)
            if 'wino' in (pf, pd):
                got['wino'] = (buf((name, dev, 'uf'), 16 * co * ci) if pf == 'wino' else None, buf((name, dev, 'ud'), 16 * co * ci) if pd == 'wino' else None)
                jobs.add_wino(w, *got['wino'])
            self._wp[name] = (got[pf][0], got[pd][1] if pd else None, slot)
        for name in ('upv6', 'upv7', 'upv8', 'upv9'):
            w = P[name + '.weight']
            ci, co = w.shape[0], w.shape[1]
            pf = plan[name].fwd
            if pf == 'h2':                 # ConvTranspose2d on the pointwise fp16x2 GEMM kernel (csrc/gemm_h2s.hip)
                f, d = (buf((name, dev, 'h2mf'), ops.h2mat_bytes(ci, 4 * co), torch.uint8),
                        buf((name, dev, 'h2md'), ops.h2mat_bytes(4 * co, ci), torch.uint8) if need_dgrad else None)
                self._wp[name] = (f, d, jobs.add_h2_convt(w, f, d))
            elif pf == 'x3':               # ConvTranspose2d on the pointwise bf16x3 GEMM kernel
                f, d = (buf((name, dev, 'x3f'), ops.x3mat_bytes(ci, 4 * co), torch.uint8),
                        buf((name, dev, 'x3d'), ops.x3mat_bytes(4 * co, ci), torch.uint8) if need_dgrad else None)
                jobs.add_x3_convt(w, f, d)
                self._wp[name] = (f, d, None)
            else:
                if (name, dev) not in self.packed:
                    self.packed[(name, dev)] = (torch.empty(w.numel(), dtype=torch.float32, device=dev),
                                                torch.empty(w.numel(), dtype=torch.float32, device=dev))
                f, d = self.packed[(name, dev)]
                jobs.add_convt(w, f, d if need_dgrad else None)
                self._wp[name] = (f, d, None)
        return jobs

    def _head_fusable(self):
        """conv10_1 inside conv9_2's epilogue (the plan's 'h2+head'): nf = 32, 4 output planes, conv9_2 on the fp16x2 kernel."""
        return self._plan['conv10_1'].fwd == 'fused'

    def grad_out_channels(self, B, H, W):
        """channels of the NHWC loss gradient backward() wants: the streaming head kernel takes the 4 real ones (half the bytes of the zero-padded copy)"""
        return 4 if (self.cout == 4 and self._pol.use_thin_head(self.ch[0], self.cout, B * H * W)) else self.cout_pad

    # ------------------------------------------------------------------ forward
    def forward(self, x, train, reflect_pad=0, add_residual=True):
        """``reflect_pad`` > 0 (eval loop, trainer_SID.py:221-226): the network runs on the frame reflect-padded by that many pixels on
        every side -- the padding happens inside the NCHW -> NHWC layout pass, the result has the PADDED size (the caller crops).
        ``add_residual=False``: a `res` network returns f(x) without `+ x` (the caller adds the un-padded input after cropping:
        (f(pad x) + pad x)[crop] = f(pad x)[crop] + x; pnnp_eval_post_f32)."""
        if not x.is_cuda:
            raise PnnpError('UNetSeeInDark.forward: input must be a CUDA tensor (pnnp_amd has no CPU path)')
        x = x.contiguous().float()
        B, Cin, H, W = x.shape
        if reflect_pad:
            if train or (self.m.res and add_residual):
                raise PnnpError('reflect_pad is an eval-mode option; a `res` network needs add_residual=False (the caller adds the input after cropping)')
            H, W = H + 2 * reflect_pad, W + 2 * reflect_pad
        if Cin != self.cin or H % 16 or W % 16:
            raise PnnpError(f'input must be [B,{self.cin},H,W] with H,W multiples of 16, got {tuple(x.shape)}')
        dev = x.device
        self.params.ensure(dev)
        # packed weights are re-used while no parameter changed (eval loops); in-place torch updates bump
        # tensor._version, the fused Adam kernel goes through mark_dirty()
        self._pol = self.effective_policy(H, W, max(self.ch[0], self.cin_pad, self.cout_pad))
        plan = self._plan = self._plan_for(B, H, W, train)
        self._packs_ready(train, dev, plan)
        gen = self._begin_forward((B, H, W, dev), train)
        bufs = self.bufs.setdefault((B, H, W, dev), _Bufs())
        P = dict(self.m.named_parameters())
        ch = self.ch
        g = lambda n, s: bufs.get(n, s, dev)
        a = {}
        # fp16x2 family: amax slots of the activations (keyed by the name of the layer that wrote the tensor; a pooled map shares its
        # full-resolution map's slot) and, in a training forward, the sign bits of every LeakyReLU output that backward-data will need
        split = {} if train else None                                 # (range census) what the fp16x2 kernels split in this step
        T = _Slots(bufs, 'f', dev, plan.h2, log=split)
        sl = T.slot
        # the zero-padded NHWC copy of the network input; its amax rides on the layout pass when conv1_1 runs on the fp16x2 kernel
        first_h2 = plan['conv1_1'].fwd == 'h2'
        a['x8'] = T.put(ops.nchw_to_nhwc(x, g('x8', (B, H, W, self.cin_pad)), self.cin_pad, reflect_pad=reflect_pad, amax=sl('x8') if first_h2 else None), 'x8', True)

        def bits_of(name, h, w, cout, act=LRELU):
            if train and act == LRELU:
                a['bits:' + name] = bufs.bits(name, B, h, w, cout, dev)
                return a['bits:' + name]
            return None

        def conv(name, src, src2, h, w, cout):
            bits = bits_of(name, h, w, cout) if plan[name].fwd.startswith('h2') else None
            return self._conv3_fwd(plan, name, T, src, src2, P[name + '.bias'], g(name, (B, h, w, cout)), cout, LRELU, bits=bits,
                                   splitk_ws=lambda n: bufs.scratch('splitk_ws', n, dev))

        hs = [H >> i for i in range(5)]
        ws = [W >> i for i in range(5)]
        cur = a['x8']
        for lvl in range(5):               # encoder: conv{l}_1, conv{l}_2, pool
            i = lvl + 1
            if plan[f'conv{i}_1'].fwd == 'thin':
                # conv1_1 on the streaming kernel: its 4 input channels are not worth a (padded) GEMM chunk.  (With the fp16x2 family the
                # matrix-core kernel is as fast -- a padded chunk is 14 instructions, not 27 -- and writes the sign bits that make conv1_2's
                # backward-data read 1/32 of the bytes: the streaming kernel keeps conv1_1's weight gradient only.)
                a['c1a'] = T.put(ops.first_fwd(cur, P['conv1_1.weight'], P['conv1_1.bias'], g('conv1_1', (B, H, W, ch[0])), LRELU,
                                               amax_y=sl('conv1_1') if plan.h2 else None), 'conv1_1', fused=True)
            else:
                a[f'c{i}a'] = conv(f'conv{i}_1', cur, None, hs[lvl], ws[lvl], ch[lvl])
            name = f'conv{i}_2'
            s = plan[name]
            if lvl == 4:
                a[f'c{i}'] = conv(name, a[f'c{i}a'], None, hs[lvl], ws[lvl], ch[lvl])
                continue
            codes = None
            if s.codes:                            # argmax + sign codes: the backward pass then does not re-read the full-resolution map
                codes = bufs.t.get(f'pc{i}')
                shp = (B, hs[lvl + 1], ws[lvl + 1], ch[lvl])
                if codes is None or tuple(codes.shape) != shp or codes.device != dev:
                    codes = bufs.t[f'pc{i}'] = torch.empty(shp, dtype=torch.uint8, device=dev)
                a[f'pc{i}'] = codes
            pooled = g(f'p{i}', (B, hs[lvl + 1], ws[lvl + 1], ch[lvl]))
            if s.fwd == 'h2+pool':
                # conv{i}_2 writes the pooled map, the codes, its amax (the pooled map is a subset) and the sign bits from its own epilogue
                a[f'c{i}'] = T.put(ops.conv_h2_fwd_pool(a[f'c{i}a'], None, self._wp[name][0], self._wp[name][2], P[name + '.bias'],
                                                        g(name, (B, hs[lvl], ws[lvl], ch[lvl])), pooled, codes, ch[lvl], LRELU, T.of(a[f'c{i}a']),
                                                        amax_y=sl(name), bits_y=bits_of(name, hs[lvl], ws[lvl], ch[lvl])), name, fused=True)
                a[f'p{i}'] = pooled
            elif s.fwd == 'x3+pool':
                # conv{i}_2 writes the pooled map and the codes from its own epilogue (csrc/conv_x3s.hip)
                a[f'c{i}'] = T.put(ops.conv_x3_fwd_pool(a[f'c{i}a'], None, self._wp[name][0], P[name + '.bias'],
                                                        g(name, (B, hs[lvl], ws[lvl], ch[lvl])), pooled, codes, ch[lvl], LRELU), name, fused=False)
                a[f'p{i}'] = pooled
            else:                                  # (also a split-K launch: it has no fused pool)
                a[f'c{i}'] = conv(name, a[f'c{i}a'], None, hs[lvl], ws[lvl], ch[lvl])
                a[f'p{i}'] = ops.maxpool_fwd(a[f'c{i}'], pooled, codes=codes)
            cur = T.put(a[f'p{i}'], name, fused=True)                 # max |pooled| <= max |full-resolution map|
        cur = a['c5']
        for i in range(6, 10):             # decoder: upv{i}, conv{i}_1 on [up, skip], conv{i}_2
            lvl = 9 - i
            u = a[f'u{i}'] = self._convt_fwd(plan, f'upv{i}', T, cur, P[f'upv{i}.bias'], g(f'u{i}', (B, hs[lvl], ws[lvl], ch[lvl])), ch[lvl])
            a[f'c{i}a'] = conv(f'conv{i}_1', u, a[f'c{lvl + 1}'], hs[lvl], ws[lvl], ch[lvl])
            if i == 9 and plan['conv9_2'].fwd == 'h2+head':
                break
            a[f'c{i}'] = cur = conv(f'conv{i}_2', a[f'c{i}a'], None, hs[lvl], ws[lvl], ch[lvl])
        out = torch.empty((B, self.cout, H, W), dtype=torch.float32, device=dev)
        res = x if (self.m.res and add_residual) else None
        if plan['conv10_1'].fwd == 'fused':
            # conv9_2 + LeakyReLU + conv10_1 in one kernel (csrc/conv_h2s.hip EK_HEAD): the 4 output planes come straight from the accumulators; the
            # 32-channel map c9 is stored (with its sign bits and amax) only for a backward pass -- an eval forward neither writes nor re-reads it
            name = 'conv9_2'
            y = g(name, (B, H, W, ch[0])) if train else None
            ops.conv_h2_fwd_head(a['c9a'], None, self._wp[name][0], self._wp[name][2], P[name + '.bias'], y, ch[0], LRELU, T.of(a['c9a']),
                                 P['conv10_1.weight'], P['conv10_1.bias'], out, amax_y=sl(name) if train else None,
                                 bits_y=bits_of(name, H, W, ch[0]), residual=res)
            if train:
                a['c9'] = T.put(y, name, fused=True)
        elif plan['conv10_1'].fwd == 'thin':
            ops.head_fwd(a['c9'], P['conv10_1.weight'], P['conv10_1.bias'], out, residual=res)
        else:
            o = ops.conv_fwd(a['c9'], None, self._wp['conv10_1'][0], P['conv10_1.bias'], g('o', (B, H, W, self.cout)), self.cout, 1, 0)
            ops.nhwc_to_nchw(o, out, residual=res)
        if train:
            a['_plan'] = plan
            a['_src_name'] = T.names
            a['_split'] = split
            self.saved = (a, (B, H, W, dev), gen)
        return out

    # ------------------------------------------------------------------ backward
    def backward(self, g_out8, need_dx=False, accumulate=False, on_ready=None):
        """g_out8: dL/d(out) as NHWC [B,H,W,cout_pad] (zero padded).  Fills the flat gradient
        buffer.  ``on_ready(offset)`` is called as soon as flat_grad[offset:] is final (layers
        finish in exactly the reverse of the flat parameter order) so a data-parallel reducer
        can start all-reducing the tail while the rest of the backward pass still runs."""
        a, (B, H, W, dev), _ = self.saved
        plan = self._plan = a['_plan']     # the kernel families this forward ran on
        self._pol = plan.pol
        bufs = self.bufs[(B, H, W, dev)]
        ch = self.ch
        gb = lambda n, s: bufs.get('g_' + n, s, dev)
        G = self.params.grad_view
        P = dict(self.m.named_parameters())
        acc = 1 if accumulate else 0
        wsf = bufs.get('wgrad_ws', (plan.ws,), dev)
        # fp16x2 family: amax slots of the gradients (keyed by the buffer name), zeroed per backward; the activations' slots are the forward's
        F = _Slots(bufs, 'f', dev, False, names=a['_src_name'], log=a['_split'])
        T = _Slots(bufs, 'b', dev, plan.h2, log=a['_split'])

        dgrad = lambda name, gsrc, dx1, **kw: self._conv3_dgrad(plan, name, a, F, T, gsrc, dx1, **kw)

        def done(name):
            if on_ready is not None:
                on_ready(self.params.slices[name + '.weight'][0])

        def wgrad(name, gpre, cout, x1, c1, x2=None, taps=9):
            self._wgrad(plan[name].wgrad, F, T, gpre, cout, x1, c1, x2, G(name + '.weight', P[name + '.weight'].shape), G(name + '.bias', (cout,)),
                        wsf, acc, taps)
            done(name)

        # conv10_1 (1x1, no activation); its input c9 is a LeakyReLU output
        g_cur = gb('c9', a['c9'].shape)
        if plan['conv10_1'].dgrad == 'thin':
            ops.head_bwd(g_out8, a['c9'], P['conv10_1.weight'], g_cur, G('conv10_1.weight', P['conv10_1.weight'].shape),
                         G('conv10_1.bias', (self.cout,)), wsf, mode=LRELU, accumulate=acc, amax_gx=T.slot('head') if plan.h2 else None)
            done('conv10_1')
            T.put(g_cur, 'head', fused=True)
        else:
            wgrad('conv10_1', g_out8, self.cout, a['c9'], ch[0], taps=1)
            ops.conv_bwd_data(g_out8, self._wp['conv10_1'][1], g_cur, mask1=a['c9'], mode1=LRELU, taps=1)
            T.put(g_cur, 'head', fused=False)
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
                _, d, wslot = self._wp[f'conv{i}_1']
                T.names[id(g_u)] = f'd1:conv{i}_1'
                ops.conv_h2_bwd_data_unpool(g_a, T.of(g_a), d, wslot, 0, 2 * ch[lvl], g_u, amax_dx=T.slot(f'd1:conv{i}_1'))
                skip_later[lvl + 1] = (f'conv{i}_1', g_a)
            else:
                dgrad(f'conv{i}_1', g_a, g_u, dx2=g_skip, mask2=skip, mode2=LRELU)
            below = a['c5'] if i == 6 else a[f'c{i - 1}']
            name = f'upv{i}'
            self._convt_wgrad(plan, name, F, T, below, g_u, G(name + '.weight', P[name + '.weight'].shape), G(name + '.bias', (ch[lvl],)), wsf, acc)
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
                    # the deferred skip half of conv{11-i}_1's backward-data: act'(c{i-1}) x dgrad + unpool(g_p) stored once (csrc/conv_h2s.hip EK_BWDU)
                    dname, g_dec = skip_later.pop(i - 1)
                    _, d, wslot = self._wp[dname]
                    ops.conv_h2_bwd_data_unpool(g_dec, T.of(g_dec), d, wslot, ch[lvl - 1], 2 * ch[lvl - 1], g_cur, bits=a[f'bits:conv{i - 1}_2'], mode=LRELU,
                                                amax_dx=T.slot(f'pool{i - 1}'), gp=g_p, codes=a[f'pc{i - 1}'])
                else:
                    ops.maxpool_bwd(a[f'c{i - 1}'], g_p, g_cur, LRELU, 1, codes=a.get(f'pc{i - 1}'), amax_gx=T.slot(f'pool{i - 1}') if plan.h2 else None)
                T.put(g_cur, f'pool{i - 1}', fused=True)
            else:
                wgrad('conv1_1', g_a, ch[0], a['x8'], self.cin)
                if need_dx:
                    raise PnnpError('gradient w.r.t. the network input is not implemented on the HIP path')
        return None


class _UNetFn(torch.autograd.Function):
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
        grads = []
        for n, p in e.m.named_parameters():
            grads.append(e.params.grad_view(n, p.shape).clone() if p.requires_grad else None)
        return (None, None, None) + tuple(grads)


class UNetSeeInDark(nn.Module):
    """Drop-in for archs/Unet.py:4-99 (same ``args`` keys: nframes, res, nf, in_nc, out_nc)."""

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
        self._engine = None

    @property
    def engine(self):
        if self._engine is None:
            object.__setattr__(self, '_engine', UNetEngine(self))
        return self._engine

    def forward(self, x):
        params = list(self.parameters())
        train = torch.is_grad_enabled() and any(p.requires_grad for p in params)
        return _UNetFn.apply(x, self.engine, train, *params)

"""One place that decides which kernel family every parameterised layer of a network runs on.

``resolve_unet`` / ``resolve_resunet`` are pure host functions of (network shape, policy, train / eval, B, H, W): they allocate nothing
and launch nothing (the shape predicates they ask are host functions of libpnnp_hip.so), so the whole per-layer choice can be tested
without a GPU.  The engines build their weight packs and issue their launches from the returned Plan; a backward pass uses the plan of
its own forward.  Families: 'h2' (fp16x2), 'x3' (bf16x3), 'wino' (Winograd), 'direct' (fp32 implicit GEMM), 'thin' (the streaming
4-channel ends); a forward may carry a fused variant ('h2+pool', 'x3+pool', 'h2+splitk', 'h2+head'; conv10_1 is then 'fused'), and
ResUnet's identity-shortcut backward-data 'FAMILY+res'.  None: the pass does not run (eval, or no gradient w.r.t. the input).
'h1' (fp16x1, csrc/conv_h1s.hip) exists in EVAL plans only, under ``ConvPolicy.h1_eval``: the stride-1 3x3 layers whose forward would
be 'h2' / 'h2+pool' / 'h2+splitk' / 'h2+head' take the same variant of 'h1'; everything else in the plan stays as it is -- unless
``ConvPolicy.h1_pointwise`` is on as well: then the ConvTranspose2d / 1x1 / stride-2 steps whose forward is 'h2' become 'h1' too
(csrc/gemm_h1s.hip)."""
import os

from .. import ops


class ConvPolicy:
    """Which kernel family a 3x3 layer runs on.
    ``x3``: forward / backward-data on the bf16 matrix cores with float32 operands split into three bf16 pieces
    (csrc/conv_x3s.hip: float32-accurate, 6/16 of the fp32-MFMA time) wherever the layer qualifies (reduction % 8 == 0,
    channels written % 32 == 0) -- the default;
    ``wino``: Winograd F(2x2,3x3) on the fp32 matrix cores for forward / backward-data where x3 is off and the layer
    qualifies (channels written % 64 == 0, reduction >= ``wino_mink`` channels), ``wino_wgrad``: the Winograd
    backward-weight kernel likewise; everything else (and everything when all are off) uses the direct fp32 implicit-GEMM
    kernels.  ``thin``: the 4-channel ends -- the 1x1 head and the first layer's backward-weight -- on the streaming vector-ALU
    kernels of csrc/thin.hip instead of the channel-padded GEMM kernels.  An engine takes DEFAULT_POLICY at construction; ``engine.set_policy(...)`` switches it (tests compare the
    families against each other at full size)."""

    def __init__(self, wino=True, wino_wgrad=True, wino_mink=32, x3=True, thin=True, pool_fused=True, h2=True):
        self.wino, self.wino_wgrad, self.wino_mink, self.x3, self.thin = bool(wino), bool(wino_wgrad), int(wino_mink), bool(x3), bool(thin)
        self.pool_fused = bool(pool_fused)         # training forward: MaxPool2d(2) in the epilogue of the bf16x3 / fp16x2 conv in front of it
        # ``h2``: the 3x3 layers that qualify for x3 run on the fp16 matrix cores instead, float32 operands split into TWO scaled fp16 pieces
        # (csrc/conv_h2s.hip, csrc/h2.h: half the matrix instructions of bf16x3; amax slots travel beside the tensors, the act' masks of the
        # backward pass are the forward kernels' sign bits).  The default since round 5: every float64 yardstick and reference-golden test of the
        # bf16x3 family passes at the same bars (tests/test_gpu_h2.py, tests/test_gpu_fullsize.py); ``set_policy(h2=False)`` = the bf16x3 family.
        self.h2 = bool(h2)
        self.h2_wgrad = bool(h2) and os.environ.get('PNNP_H2_WGRAD', '1') != '0'      # (host-side A/B switch: backward-weight stays on bf16x3 with 0)
        self.h2_pointwise = bool(h2) and os.environ.get('PNNP_H2_POINTWISE', '1') != '0'      # (A/B switch: ConvTranspose2d stays on bf16x3 with 0)
        self.head_fused = bool(h2) and os.environ.get('PNNP_HEAD_FUSED', '1') != '0'          # (A/B switch) conv10_1 inside conv9_2's epilogue (round 6)
        self.splitk = bool(h2) and os.environ.get('PNNP_SPLITK', '1') != '0'                  # (A/B switch) split-K forward launches for small grids (round 6)
        self.convt_bits = bool(h2) and os.environ.get('PNNP_CONVT_BITS', '1') != '0'          # (A/B switch) ConvTranspose2d backward-data masks with sign bits (round 6)
        # (A/B switch, round 7) MaxPool2d backward inside the epilogue of the decoder's skip-gradient launch (csrc/conv_h2s.hip EK_BWDU) instead of a pass of
        # its own; ``unpool_levels``: the encoder levels (1 = the full-resolution one .. 4) it applies to -- PNNP_UNPOOL_LEVELS=234 keeps level 1 on the pass
        self.unpool_fused = bool(h2) and os.environ.get('PNNP_UNPOOL_FUSED', '1') != '0'
        self.unpool_levels = tuple(sorted({int(c) for c in os.environ.get('PNNP_UNPOOL_LEVELS', '1234') if c in '1234'}))
        # (opt-in, off by default) EVAL forwards run the stride-1 3x3 layers that are on fp16x2 with ONE fp16 piece per operand instead (csrc/conv_h1s.hip:
        # one rounding per operand, float32 accumulation, ~1e-3 of the activations' scale; 5 matrix instructions per chunk where fp16x2 issues 14).  Only
        # meaningful with ``h2``; a training plan ignores it.  Not part of key(): the packs are keyed by the plan's pack families ('h1')
        self.h1_eval = bool(h2) and os.environ.get('PNNP_H1_EVAL', '0') != '0'
        # (opt-in, off by default) ... and, with ``h1_eval``, the ConvTranspose2d / 1x1 / stride-2 layers that are on the pointwise fp16x2 kernel as well
        # (csrc/gemm_h1s.hip: one matrix instruction per 32 channels where fp16x2 issues three).  Without ``h2`` and ``h1_eval`` it changes nothing.
        self.h1_pointwise = bool(h2) and os.environ.get('PNNP_H1_POINTWISE', '0') != '0'
        # (opt-in, off by default) ... and, with BOTH, every map a convolution writes and a convolution reads is STORED as fp16 in a UNet eval forward whose
        # layers all resolved to 'h1...' / 'fused' (Plan.act16; csrc/conv_h1s.hip H1a, csrc/gemm_h1s.hip H1ga): float16(y) of the float32 value, unscaled, not
        # saturated.  In every other case -- ResUnet, a layer held on another family, a training plan -- it changes nothing.
        self.h1_act16 = bool(h2) and os.environ.get('PNNP_H1_ACT16', '0') != '0'
        # (opt-in, off by default) ... and, with ALL THREE, the same storage in a ResUnet eval forward (residual sums, stride-2 and 1x1 layers and the two streaming
        # layers at the ends included: 31 maps).  A switch of its own because ``h1_act16`` is pinned to leave ResUnet on the fp16_all plan.  UNet plans never read it.
        self.h1_act16_res = bool(h2) and os.environ.get('PNNP_H1_ACT16_RES', '0') != '0'

    def key(self):
        return (self.wino, self.wino_wgrad, self.wino_mink, self.x3, self.thin, self.pool_fused, self.h2, self.h2_wgrad, self.h2_pointwise, self.head_fused, self.splitk, self.convt_bits)

    def plan_key(self):
        """What a cached Plan depends on: key() (the families and packs) + the switches that only change the launch sequence."""
        return self.key() + (self.unpool_fused, self.unpool_levels, self.h1_eval, self.h1_pointwise, self.h1_act16, self.h1_act16_res)

    def use_thin_head(self, cin, cout, npix):
        return self.thin and ops.head_supported(cin, cout, npix)

    def use_thin_first(self, cin, cout, h, w, x_cs):
        return self.thin and x_cs >= 4 and ops.first_wgrad_supported(cin, cout, h, w)

    def use_x3(self, co, ci, taps=9, c1=None):
        """(forward, backward-data) of a 3x3 Conv2d(ci -> co) on the bf16x3 kernel?  ``c1``: channels of the first of two
        concatenated inputs (its gradient is a separate destination: the split must fall on a 32-column block)."""
        if taps != 9 or not self.x3:
            return False, False
        return (ops.x3_supported(ci, co) and (c1 is None or c1 % 16 == 0),
                ops.x3_supported(co, ci) and (c1 is None or c1 % 32 == 0))

    def use_h2(self, co, ci, taps=9, c1=None):
        """(forward, backward-data) of a 3x3 Conv2d(ci -> co) on the fp16x2 kernel?  Same shape rules as use_x3 (+ at most 1024 channels written)."""
        if taps != 9 or not (self.h2 and self.x3):
            return False, False
        return (ops.h2_supported(ci, co) and (c1 is None or c1 % 16 == 0),
                ops.h2_supported(co, ci) and (c1 is None or c1 % 32 == 0))

    def use_wino(self, co, ci, taps=9):
        """(forward, backward-data) of a Conv2d(ci -> co, taps) on the Winograd kernel?"""
        if taps != 9 or not self.wino:
            return False, False
        return (ops.wino_supported(ci, co) and ci >= self.wino_mink, ops.wino_supported(co, ci) and co >= self.wino_mink)

    def use_x3_pointwise(self, K, N):
        """a one-tap-per-segment layer (ConvTranspose2d, 1x1, stride-2 3x3) on the pointwise bf16x3 GEMM kernel (csrc/gemm_x3.hip)?"""
        return self.x3 and ops.gemm_x3_supported(K, N)

    def use_x3_wgrad(self, h, w, cout, c1, c2, batch=None, cs=None):
        """backward-weight of a 3x3 layer on the bf16x3 kernel (csrc/wgrad_x3.hip)?  ``batch`` / ``cs`` (largest channel stride of
        the tensors involved): the kernel addresses a whole [B][H][W][cs] map with 32-bit byte offsets; past that the layer falls
        back to the Winograd / direct fp32 kernels instead of failing inside backward."""
        if not (self.x3 and ops.x3_wgrad_supported(h, w, cout, c1, c2)):
            return False
        return batch is None or ops.x3_wgrad_fits(batch, h, w, cs if cs is not None else max(cout, c1, c2))

    def use_x3g_wgrad(self, kind, M, N, batch, uh, uw, sh, sw, cs):
        """backward-weight of a ConvTranspose2d / stride-2 3x3 / 1x1 layer on the bf16x3 kernel of csrc/wgrad_x3g.hip?  (M, N) must have a
        tile configuration and both whole maps must fit 32-bit byte offsets; otherwise the fp32-MFMA kernel of csrc/wgrad.hip takes it."""
        if not (self.x3 and ops.x3g_wgrad_supported(kind, M, N)):
            return False
        return ops.x3_wgrad_fits(batch, uh, uw, cs) and ops.x3_wgrad_fits(batch, sh, sw, cs)

    def use_wino_wgrad(self, h, w, cout, c1, c2, g_cs, x_cs):
        return self.wino and self.wino_wgrad and g_cs == cout and x_cs == c1 and ops.wino_wgrad_supported(h, w, cout, c1, c2)


DEFAULT_POLICY = ConvPolicy(wino=os.environ.get('PNNP_WINO', '1') != '0', x3=os.environ.get('PNNP_X3', '1') != '0', h2=os.environ.get('PNNP_H2', '1') != '0')      # host-side defaults only; the library reads no environment


class Step:
    """What one layer runs: ``fwd`` / ``dgrad`` / ``wgrad`` families (see the module docstring) and ``pack`` = the (forward, backward-data)
    weight packs it needs; ``ks``: K slices of a split-K forward; ``codes``: a pooled layer keeps argmax / sign codes for its backward;
    ``unpool`` (decoder conv{6..9}_1): its backward-data runs as two column-range launches, the skip half deferred to where the pooled map's
    gradient exists and carrying MaxPool2d's backward in its epilogue (not a family: ``families()`` does not show it)."""

    def __init__(self, fwd, dgrad=None, wgrad=None, pack=None, ks=1, codes=False):
        self.fwd, self.dgrad, self.wgrad, self.ks, self.codes = fwd, dgrad, wgrad, ks, codes
        self.unpool = False
        self.pack = pack if pack is not None else (fwd, dgrad)

    def families(self):
        return (self.fwd, self.dgrad, self.wgrad)


class Plan:
    """Per-layer Steps of one (network, policy, mode, B, H, W); ``h2`` = some layer runs on an fp16x2 kernel (the amax slots are kept up);
    ``ws`` = the backward-weight workspace (floats) every family's kernels are given."""

    def __init__(self, steps, pol, train, ws):
        self.steps, self.pol, self.train, self.ws = steps, pol, train, ws
        self.h2 = any(p == 'h2' for s in steps.values() for p in s.pack)
        self.act16 = False                  # (eval plans under ConvPolicy.h1_act16 / h1_act16_res) the maps convolutions write and read are stored as fp16: mark_act16()
        # the weight packs the engines build; they depend on the policy and the mode only, never on B, H, W
        self.packs = tuple(s.pack for s in steps.values())

    def __getitem__(self, name):
        return self.steps[name]

    def table(self):
        return {n: s.families() for n, s in self.steps.items()}

    def to_h1(self, names):
        """(eval plans, ConvPolicy.h1_eval) the layers ``names`` whose forward is an fp16x2 3x3 launch take the fp16x1 kernel: same variant, pack family
        'h1'.  ``h2`` stays as it was: the amax slots are what the scale is made of, and the pointwise layers stay on fp16x2."""
        for n in names:
            s = self.steps[n]
            if s.fwd in ('h2', 'h2+pool', 'h2+splitk', 'h2+head'):
                s.fwd, s.pack = 'h1' + s.fwd[2:], ('h1', s.pack[1])
        self.packs = tuple(s.pack for s in self.steps.values())
        return self

    def mark_act16(self):
        """(eval plans, ConvPolicy.h1_eval + h1_pointwise + h1_act16) fp16 storage of the activations, if EVERY layer's forward is an fp16x1 launch ('h1...', or
        'fused' into one): a map has one element type, so one layer on another family keeps the whole plan on float32 storage -- the fp16_all plan, unchanged.
        The launch sequence is the same either way: families, variants and K slices stay."""
        self.act16 = not self.train and all(s.fwd == 'fused' or s.fwd.split('+')[0] == 'h1' for s in self.steps.values())
        return self

    def mark_act16_res(self, ends):
        """(ResUnet eval plans, ConvPolicy.h1_eval + h1_pointwise + h1_act16 + h1_act16_res) the same, where the layers ``ends`` (the first layer and the head)
        may also run on the streaming kernels ('thin': they have an fp16 side of their own, csrc/thin.hip).  A head on 'direct', or any layer on another
        family, keeps the fp16_all plan."""
        self.act16 = not self.train and all(s.fwd == 'h1' or (n in ends and s.fwd == 'thin') for n, s in self.steps.items())
        return self

    # (kind, K, N) of a pointwise forward GEMM that stays on fp16x2 under h1_pointwise because one piece measured SLOWER there (none so far)
    H1_POINTWISE_KEEP_H2 = frozenset()

    def to_h1_pointwise(self, layers):
        """(eval plans, ConvPolicy.h1_eval and h1_pointwise) ``layers``: name -> (kind, K, N) of the ConvTranspose2d / 1x1 / stride-2 steps' forward GEMMs; those
        whose forward is the pointwise fp16x2 launch take the fp16x1 kernel, pack family 'h1'.  ``h2`` stays as it was (the amax slots are still kept up)."""
        for n, knd in layers.items():
            s = self.steps[n]
            if s.fwd == 'h2' and s.pack[0] == 'h2' and knd not in self.H1_POINTWISE_KEEP_H2 and ops.h1_pointwise_supported(knd[1], knd[2]):
                s.fwd, s.pack = 'h1', ('h1', s.pack[1])
        self.packs = tuple(s.pack for s in self.steps.values())
        return self


def _pad8(c):
    return (c + 7) // 8 * 8


def _conv3_packs(pol, co, cip, ci, c1, bwd):
    """(forward, backward-data) family of a 3x3 Conv2d: fp16x2 takes what bf16x3 would take, then Winograd, then the direct kernels."""
    xf, xd = pol.use_x3(co, cip, 9, c1)
    hf, hd = pol.use_h2(co, cip, 9, c1)
    wf, wd = pol.use_wino(co, ci, 9)
    f = 'h2' if hf and xf else 'x3' if xf else 'wino' if wf else 'direct'
    d = None if not bwd else 'h2' if hd and xd else 'x3' if xd else 'wino' if wd else 'direct'
    return f, d


def _wgrad3(pol, h2, B, h, w, cout, c1, c2, gcs, xcs, slots=True):
    """backward-weight of a 3x3 layer; ``slots``: the amax slots of both operands are valid (the fp16x2 kernel reads them)."""
    if pol.use_x3_wgrad(h, w, cout, c1, c2, batch=B, cs=max(gcs, xcs)):
        return 'h2' if (h2 and pol.h2_wgrad and slots) else 'x3'
    return 'wino' if pol.use_wino_wgrad(h, w, cout, c1, c2, gcs, xcs) else 'direct'


def _convt_wgrad(pol, h2, B, ci, co, H, W, lvl, slots=True):
    hs, ws = H >> lvl, W >> lvl
    if not pol.use_x3g_wgrad(ops.X3G_CT, ci, co, B, hs >> 1, ws >> 1, hs, ws, max(ci, co)):
        return 'direct'
    return 'h2' if (h2 and pol.h2_pointwise and slots) else 'x3'


def _pointwise_family(pol, kf, nf, kd, nd, h2=True):
    """A ConvTranspose2d or stride-2 3x3 layer on the pointwise GEMM kernels: its forward is a GEMM with K = kf, N = nf, its backward-data one with
    K = kd, N = nd.  bf16x3 where both have a tile, fp16x2 (``h2``: the layer's operands carry amax slots) where it would take what bf16x3 takes,
    else the direct kernels."""
    if not (pol.use_x3_pointwise(kf, nf) and pol.use_x3_pointwise(kd, nd)):
        return 'direct'
    return 'h2' if (h2 and pol.h2 and pol.h2_pointwise and ops.gemm_h2_supported(kf, nf) and ops.gemm_h2_supported(kd, nd)) else 'x3'


def resolve_unet(ch, cin, cout, pol, train, B, H, W):
    """UNetSeeInDark: conv{1..9}_{1,2} (3x3), upv{6..9} (ConvTranspose2d 2x2 s2), conv10_1 (1x1 head)."""
    cin_pad = _pad8(cin)
    st = {}
    for i in range(1, 10):
        lvl = i - 1 if i <= 5 else 9 - i
        for j in (1, 2):
            name = f'conv{i}_{j}'
            ci = ch[lvl] if j == 2 else (cin if i == 1 else ch[lvl - 1] if i <= 5 else 2 * ch[lvl])
            cip = cin_pad if name == 'conv1_1' else ci
            c1 = ch[lvl] if (j == 1 and i >= 6) else None                  # decoder conv{6..9}_1 read cat([up, skip])
            st[name] = Step(*_conv3_packs(pol, ch[lvl], cip, ci, c1, train and name != 'conv1_1'))
        if i >= 6:
            ci, co = ch[lvl + 1], ch[lvl]
            f = _pointwise_family(pol, ci, 4 * co, co, ci)
            st[f'upv{i}'] = Step(f, f if train else None)
    thin_head = pol.use_thin_head(ch[0], cout, B * H * W)
    st['conv10_1'] = Step('thin' if thin_head else 'direct', ('thin' if thin_head else 'direct') if train else None, pack=('direct', 'direct' if train else None))
    plan = Plan(st, pol, train, ws_floats_unet(ch, cin, cout, B, H, W))
    h2 = plan.h2
    s = st['conv1_1']
    if s.fwd != 'h2' and pol.use_thin_first(cin, ch[0], H, W, cin_pad):
        s.fwd = 'thin'
    for i in range(1, 10):                 # fused / split forwards of the fp16x2 and bf16x3 3x3 layers
        lvl = i - 1 if i <= 5 else 9 - i
        for j in (1, 2):
            s = st[f'conv{i}_{j}']
            src_cs = cin_pad if (i, j) == (1, 1) else ch[lvl - 1] if (j == 1 and i <= 5) else ch[lvl]
            if s.fwd == 'h2' and pol.splitk and not train:
                s.ks = ops.h2_splitk(B, H >> lvl, W >> lvl, (2 if (j == 1 and i >= 6) else 1) * ((src_cs + 15) // 16), ch[lvl])
            if j == 2 and i <= 4:
                s.codes = train or (pol.pool_fused and s.fwd in ('h2', 'x3'))
                if pol.pool_fused and s.fwd in ('h2', 'x3') and s.ks == 1:
                    s.fwd += '+pool'
            if s.ks > 1:
                s.fwd = 'h2+splitk'
    if pol.head_fused and ch[0] == 32 and cout == 4 and st['conv9_2'].fwd.startswith('h2'):
        st['conv9_2'].fwd, st['conv9_2'].ks, st['conv10_1'].fwd = 'h2+head', 1, 'fused'
    if not train and pol.h1_eval and pol.h2:
        plan.to_h1([f'conv{i}_{j}' for i in range(1, 10) for j in (1, 2)])
        if pol.h1_pointwise:
            plan.to_h1_pointwise({f'upv{i}': ('convt', ch[10 - i], 4 * ch[9 - i]) for i in range(6, 10)})
            if pol.h1_act16:
                plan.mark_act16()
    if train:
        for i in range(6, 10):             # the skip gradient of conv{i}_1 + MaxPool2d backward in one epilogue: needs the skip tensor's sign bits and codes
            skip = st[f'conv{10 - i}_2']
            st[f'conv{i}_1'].unpool = bool(pol.unpool_fused and (10 - i) in pol.unpool_levels and st[f'conv{i}_1'].dgrad == 'h2'
                                           and skip.fwd in ('h2', 'h2+pool') and skip.codes)
        for i in range(1, 10):
            lvl = i - 1 if i <= 5 else 9 - i
            c = ch[lvl]
            h, w = H >> lvl, W >> lvl
            st[f'conv{i}_2'].wgrad = _wgrad3(pol, h2, B, h, w, c, c, 0, c, c)
            if i >= 6:
                st[f'conv{i}_1'].wgrad = _wgrad3(pol, h2, B, h, w, c, c, c, c, c)
                st[f'upv{i}'].wgrad = _convt_wgrad(pol, h2, B, ch[lvl + 1], c, H, W, lvl)
            elif i > 1:
                st[f'conv{i}_1'].wgrad = _wgrad3(pol, h2, B, h, w, c, ch[lvl - 1], 0, c, ch[lvl - 1])
        st['conv1_1'].wgrad = ('thin' if pol.use_thin_first(cin, ch[0], H, W, cin_pad) else
                               _wgrad3(pol, h2, B, H, W, ch[0], cin, 0, ch[0], cin_pad))
        st['conv10_1'].wgrad = 'thin' if thin_head else 'direct'
    return plan


def _pointwise_packs(pol, ci, co, c1, train):
    """ResUnet's 1x1 shortcut (Conv2d(ci -> co) on cat([up, skip])): the pointwise fp16x2 / bf16x3 GEMM kernels, else direct."""
    if not (pol.use_x3_pointwise(ci, co) and pol.use_x3_pointwise(co, ci) and (c1 is None or c1 % 32 == 0)):
        return None
    h2 = pol.h2 and pol.h2_pointwise and ops.gemm_h2_supported(c1 if c1 else ci, co) and ops.gemm_h2_supported(co, ci)
    f = 'h2' if h2 else 'x3'
    return f, f if train else None


def resolve_resunet(ch, cin, cout, pol, train, B, H, W):
    """ResUnet: conv_in (3x3), b{l}_{0,1} (the residual blocks' 3x3 convs), pool{1..4} (3x3 stride 2), upv{6..9} (ConvTranspose2d),
    sc{6..9} (the decoder blocks' 1x1 shortcuts on cat([up, skip])), conv10 (1x1 head)."""
    cin_pad, cout_pad = _pad8(cin), _pad8(cout)
    st = {'conv_in': Step(*_conv3_packs(pol, ch[0], cin_pad, cin, None, False))}
    for i in range(1, 10):
        lv = i - 1 if i <= 5 else 9 - i
        c = ch[lv]
        st[f'b{i}_0'] = Step(*_conv3_packs(pol, c, 2 * c if i >= 6 else c, 2 * c if i >= 6 else c, c if i >= 6 else None, train))
        st[f'b{i}_1'] = Step(*_conv3_packs(pol, c, c, c, None, train))
        if i >= 6:
            st[f'sc{i}'] = Step(*(_pointwise_packs(pol, 2 * c, c, c, train) or ('direct', 'direct' if train else None)))
    for i in range(1, 5):                  # (the engine packs in the order of the steps)
        f = _pointwise_family(pol, ch[i - 1], ch[i], ch[i], ch[i - 1])
        st[f'pool{i}'] = Step(f, f if train else None)
    for i in range(6, 10):
        lv = 9 - i
        ci, co = ch[lv + 1], ch[lv]
        # (only beside an fp16x2 shortcut: its backward-data leaves the amax slot of the summed gradient this layer's backward splits)
        f = _pointwise_family(pol, ci, 4 * co, co, ci, h2=st[f'sc{i}'].fwd == 'h2')
        st[f'upv{i}'] = Step(f, f if train else None)
    head = _pointwise_packs(pol, ch[0], cout, None, train) or ('direct', 'direct' if train else None)
    thin_head = pol.use_thin_head(ch[0], cout, B * H * W)
    st['conv10'] = Step('thin' if thin_head else 'direct', ('thin' if thin_head else 'direct') if train else None, pack=head)
    plan = Plan(st, pol, train, ws_floats_resunet(ch, cin, cout, B, H, W))
    h2 = plan.h2
    thin_first = pol.use_thin_first(cin, ch[0], H, W, cin_pad)
    if thin_first:
        st['conv_in'].fwd = 'thin'
    if not train:
        if pol.h1_eval and pol.h2:
            plan.to_h1(['conv_in'] + [f'b{i}_{j}' for i in range(1, 10) for j in (0, 1)])
            if pol.h1_pointwise:
                pw = {f'upv{i}': ('convt', ch[10 - i], 4 * ch[9 - i]) for i in range(6, 10)}
                pw.update({f'sc{i}': ('1x1', ch[9 - i], ch[9 - i]) for i in range(6, 10)})          # (K per segment of cat([up, skip]))
                pw.update({f'pool{i}': ('s2', ch[i - 1], ch[i]) for i in range(1, 5)})             # (K per tap segment)
                plan.to_h1_pointwise(pw)
                if pol.h1_act16 and pol.h1_act16_res:
                    plan.mark_act16_res(('conv_in', 'conv10'))
        return plan
    for l in range(1, 6):
        st[f'b{l}_0'].dgrad += '+res'                  # identity shortcut: d/d(input) = dgrad(block) + g in one kernel
    for i in range(1, 10):
        lv = i - 1 if i <= 5 else 9 - i
        c, h, w = ch[lv], H >> lv, W >> lv
        st[f'b{i}_1'].wgrad = _wgrad3(pol, h2, B, h, w, c, c, 0, c, c)
        st[f'b{i}_0'].wgrad = _wgrad3(pol, h2, B, h, w, c, c, c if i >= 6 else 0, c, c)
        if i >= 6:
            sc_h2 = st[f'sc{i}'].fwd == 'h2'
            # the upv's gradient carries a valid amax slot only after an fp16x2 shortcut's backward-data rewrote it
            st[f'upv{i}'].wgrad = _convt_wgrad(pol, h2, B, ch[lv + 1], c, H, W, lv, slots=sc_h2)
            x3g = pol.use_x3g_wgrad(ops.X3G_PW, c, 2 * c, B, h, w, h, w, c)
            if (h2 and pol.h2_pointwise and pol.x3 and not x3g and ops.h2g_wgrad_supported(ops.X3G_PW, c, 2 * c) and ops.x3_wgrad_fits(B, h, w, c)
                    and plan.ws >= ops.h2g_wgrad_workspace_floats(ops.X3G_PW, B, h, w, c, 2 * c)):
                st[f'sc{i}'].wgrad = 'h2'                 # a shape only the fp16x2 kernel has a tile for (sc9: 32 x 64)
            else:
                st[f'sc{i}'].wgrad = ('h2' if h2 and pol.h2_pointwise else 'x3') if x3g else 'direct'
        if 2 <= i <= 5:                                    # pool{i-1}: stride-2 3x3 from c{i-1} to d{i-1}
            co, ci, hs, ws, cs = c, ch[lv - 1], h, w, max(c, ch[lv - 1])
            if (h2 and pol.h2_pointwise and pol.x3 and ops.h2g_wgrad_supported(ops.X3G_S2, co, ci)
                    and ops.x3_wgrad_fits(B, hs, ws, cs) and ops.x3_wgrad_fits(B, 2 * hs, 2 * ws, cs)):
                f = 'h2'
            else:
                f = 'x3' if pol.use_x3g_wgrad(ops.X3G_S2, co, ci, B, hs, ws, 2 * hs, 2 * ws, cs) else 'direct'
            st[f'pool{i - 1}'].wgrad = f
    st['conv_in'].wgrad = ('thin' if thin_first else
                           _wgrad3(pol, h2, B, H, W, ch[0], cin, 0, ch[0], cin_pad, slots=st['conv_in'].fwd == 'h2' and st['b1_0'].dgrad == 'h2+res'))
    if thin_head:
        st['conv10'].wgrad = 'thin'
    else:
        st['conv10'].wgrad = 'x3' if pol.use_x3g_wgrad(ops.X3G_PW, cout, ch[0], B, H, W, H, W, max(cout_pad, ch[0])) else 'direct'
    return plan


def ws_floats_unet(ch, cin, cout, B, H, W):
    need = 1024 * max(ch)
    for lvl in range(5):
        h, w = H >> lvl, W >> lvl
        c = ch[lvl]
        ci = cin if lvl == 0 else ch[lvl - 1]
        need = max(need, ops.x3_wgrad_workspace_floats(B, h, w, c, c), ops.x3_wgrad_workspace_floats(B, h, w, c, 2 * c),
                   ops.x3_wgrad_workspace_floats(B, h, w, c, ci) if ci % 32 == 0 else 0)
        need = max(need, ops.wgrad_workspace_floats(B, h, w, c, c, 9), ops.wgrad_workspace_floats(B, h, w, c, ci, 9),
                   ops.wgrad_workspace_floats(B, h, w, c, 2 * c, 9), ops.wino_wgrad_workspace_floats(B, h, w, c, c),
                   ops.wino_wgrad_workspace_floats(B, h, w, c, ci), ops.wino_wgrad_workspace_floats(B, h, w, c, 2 * c))
        if lvl < 4:
            need = max(need, ops.wgrad_workspace_floats(B, h >> 1, w >> 1, ch[lvl + 1], c, 4),
                       ops.x3g_wgrad_workspace_floats(ops.X3G_CT, B, h >> 1, w >> 1, ch[lvl + 1], c))
    need = max(need, ops.wgrad_workspace_floats(B, H, W, cout, ch[0], 1))
    return max(need, ops.head_bwd_workspace_floats(ch[0]), ops.first_wgrad_workspace_floats(ch[0]))


def ws_floats_resunet(ch, cin, cout, B, H, W):
    need = 1024 * max(ch)
    for lv in range(5):
        h, w, c = H >> lv, W >> lv, ch[lv]
        need = max(need, ops.wino_wgrad_workspace_floats(B, h, w, c, c), ops.wino_wgrad_workspace_floats(B, h, w, c, 2 * c),
                   ops.x3_wgrad_workspace_floats(B, h, w, c, c), ops.x3_wgrad_workspace_floats(B, h, w, c, 2 * c))
        need = max(need, ops.wgrad_workspace_floats(B, h, w, c, c, 9), ops.wgrad_workspace_floats(B, h, w, c, 2 * c, 9),
                   ops.wgrad_workspace_floats(B, h, w, c, 2 * c, 1), ops.wgrad_workspace_floats(B, h, w, c, cin, 9))
        need = max(need, ops.x3g_wgrad_workspace_floats(ops.X3G_PW, B, h, w, c, 2 * c))
        if lv < 4:
            need = max(need, ops.wgrad_workspace_floats(B, h >> 1, w >> 1, ch[lv + 1], c, 4),
                       ops.wgrad_workspace_floats(B, h >> 1, w >> 1, ch[lv + 1], c, 18),
                       ops.x3g_wgrad_workspace_floats(ops.X3G_CT, B, h >> 1, w >> 1, ch[lv + 1], c),
                       ops.x3g_wgrad_workspace_floats(ops.X3G_S2, B, h >> 1, w >> 1, ch[lv + 1], c),
                       ops.h2g_wgrad_workspace_floats(ops.X3G_S2, B, h >> 1, w >> 1, ch[lv + 1], c))
    need = max(need, ops.head_bwd_workspace_floats(ch[0]), ops.first_wgrad_workspace_floats(ch[0]))
    return max(need, ops.wgrad_workspace_floats(B, H, W, cout, ch[0], 1))

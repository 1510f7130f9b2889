"""Float64 references, a derived per-element error bound and a mirror of the launch rules for the fp32 "direct" kernels (csrc/conv_igemm.hip, csrc/wgrad.hip
behind ops.conv_fwd / conv_bwd_data / conv_bwd_data_res / conv_bwd_weight / convt_* / conv_s2_*).  No GPU: torch on the CPU in float64.

The bound.  v_mfma_f32_32x32x2_f32 is a k-ordered chain of float32 fma, one rounding per product and no wider internal sum, so an output that sums n products
in ANY order and then takes e rounded epilogue operations (bias, residual / addsrc, activation slope, mask slope, accumulate) obeys the standard bound

    |got - ref64| <= (n + e) * 2^-24 * S * 1.01,

S being the same operation in float64 on |x|, |w|, |bias|, |residual|, |previous contents| (the factor 1.01 absorbs the second-order terms gamma_k - k u for
the k <= 3e5 met here; it is not a tuned margin).  What counts as a rounded operation: an addition; a multiplication by the slope 0.2.  Multiplications by 1 or 0
(ReLU, ReLU', the positive side of LeakyReLU) are exact.  The slope of the operation is float32(0.2) -- what LeakyReLU(0.2) multiplies by in float32, in
torch as in the kernels -- so the float64 references use that value, and the slope costs one rounding, not two.  A slope <= 1 never enlarges an error that
is already bounded by S, so S is taken before the activation.

A weight gradient sums B*H*W products per element in pieces (pixel tiles of a workgroup, the waves that split a tile, then Z slabs), n = B*H*W + Z; a bias
gradient sums `terms` values (B*H*W of g for a Conv2d, 4*B*H*W for a ConvTranspose2d) the same way, n = terms + Z.  That n is the SIZE of the sum; the
rounding error of a summation tree is bounded by its DEPTH (the most additions one term passes), which for these kernels is hundreds of times smaller, so the
tests assert the bound with both (wgrad_depth below): only the second can see a pixel tile that went missing from a large map.

Tensors here are NCHW, float32 on the way in, float64 on the way out."""
import collections

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
SLOPE = float(np.float32(0.2))

Ref = collections.namedtuple('Ref', 'ref S n e')        # n: a number, or a tensor that broadcasts against ref (stride-2 backward-data)


def bound(r):
    return (r.n + r.e) * U * r.S * 1.01


def d(t):
    return None if t is None else t.detach().double()


def _act(z, act):
    return torch.where(z > 0, z, SLOPE * z) if act == 1 else (F.relu(z) if act == 2 else z)


def _dact(mask, mode):
    """act'(mask) as the kernels take it: mode 1 LeakyReLU', 2 ReLU', 0 / no mask: 1."""
    if mask is None or not mode:
        return 1.0
    return torch.where(d(mask) > 0, 1.0, SLOPE if mode == 1 else 0.0)


def _epilogue(z, Sz, n, e, mask, mode, base):
    """(z * act'(mask)) + base, with the count of rounded operations."""
    m = _dact(mask, mode)
    e += 1 if (mask is not None and mode == 1) else 0
    z, Sz = z * m, Sz * m
    if base is not None:
        z, Sz, e = z + d(base), Sz + d(base).abs(), e + 1
    return Ref(z, Sz, n, e)


def conv_fwd(x, w, b=None, residual=None, act=0, stride=1):
    """act(conv(x, w) + b + residual): Conv2d 3x3 pad 1 or 1x1, stride 1 or (3x3 only) 2."""
    k = w.shape[2]
    run = lambda x, w, b, r: F.conv2d(x, w, b, stride=stride, padding=k // 2) + (0 if r is None else r)
    z = run(d(x), d(w), d(b), d(residual))
    S = run(d(x).abs(), d(w).abs(), None if b is None else d(b).abs(), None if residual is None else d(residual).abs())
    e = (b is not None) + (residual is not None) + (act == 1)
    return Ref(_act(z, act), S, w.shape[1] * k * k, e)


def conv_bwd_data(g, w, c0=0, c1=None, mask=None, mode=0, base=None, addsrc=None, stride=1):
    """Channels [c0, c1) of dL/dx of conv(x, w) given g = dL/dy: (dgrad(g) [+ addsrc]) * act'(mask) [+ base].  Stride 2 (3x3): each input pixel is reached by
    (1 + y % 2) * (1 + x % 2) taps (csrc/conv_api.hip s2_bwd_args: one GEMM per parity class over 1 / 2 / 2 / 4 taps), so n varies per pixel."""
    k = w.shape[2]
    ws = d(w)[:, c0:c1]
    run = lambda g, w: F.conv_transpose2d(g, w, stride=stride, padding=k // 2, output_padding=stride - 1)
    z, S = run(d(g), ws), run(d(g).abs(), ws.abs())
    if stride == 2:
        H, W = z.shape[2:]
        n = ((1 + torch.arange(H) % 2)[:, None] * (1 + torch.arange(W) % 2)[None, :]).double() * w.shape[0]
    else:
        n = w.shape[0] * k * k
    e = 0
    if addsrc is not None:
        z, S, e = z + d(addsrc), S + d(addsrc).abs(), 1
    return _epilogue(z, S, n, e, mask, mode, base)


def convt_fwd(x, w, b=None):
    """ConvTranspose2d(2, stride 2): every output pixel sums Cin products."""
    z = F.conv_transpose2d(d(x), d(w), d(b), stride=2)
    S = F.conv_transpose2d(d(x).abs(), d(w).abs(), None if b is None else d(b).abs(), stride=2)
    return Ref(z, S, w.shape[0], int(b is not None))


def convt_bwd_data(g, w, mask=None, mode=0):
    """dL/dx of the layer above: a stride-2 2x2 correlation of g with w [Cin][Cout][2][2], 4 Cout products."""
    z, S = F.conv2d(d(g), d(w), stride=2), F.conv2d(d(g).abs(), d(w).abs(), stride=2)
    return _epilogue(z, S, 4 * w.shape[1], 0, mask, mode, None)


def _wgrad(fn, wshape, nb, x, g):
    w = torch.zeros(wshape, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(nb, dtype=torch.float64, requires_grad=True)
    fn(x, w, b).backward(g)
    return w.grad, b.grad


def _wgrad_refs(fn, wshape, nb, x, g, pixels, bias_terms, Z):
    dW, db = _wgrad(fn, wshape, nb, d(x), d(g))
    SW, Sb = _wgrad(fn, wshape, nb, d(x).abs(), d(g).abs())
    return Ref(dW, SW, pixels + Z, 0), Ref(db, Sb, bias_terms + Z, 0)


def conv_bwd_weight(g, x, k, Z, stride=1):
    """dW [Cout][Cin][k][k] and dbias of Conv2d(k, pad k // 2, stride) on x (the cat of a two-tensor input), by autograd.  Z: the slab count."""
    B, Co, h, w_ = g.shape
    fn = lambda x, w, b: F.conv2d(x, w, b, stride=stride, padding=k // 2)
    return _wgrad_refs(fn, (Co, x.shape[1], k, k), Co, x, g, B * h * w_, B * h * w_, Z)


def convt_bwd_weight(x, g, Z):
    """dW [Cin][Cout][2][2] and dbias (the sum of g: four g pixels per x pixel) of ConvTranspose2d(2, stride 2)."""
    B, Ci, H, W = x.shape
    fn = lambda x, w, b: F.conv_transpose2d(x, w, b, stride=2)
    return _wgrad_refs(fn, (Ci, g.shape[1], 2, 2), g.shape[1], x, g, B * H * W, 4 * B * H * W, Z)


def accumulated(r, base):
    """`accumulate = 1`: the gradient is added to what the destination held -- one more rounded addition."""
    return Ref(r.ref + d(base), r.S + d(base).abs(), r.n, r.e + 1)


# ---------------------------------------------------------------- the launch rules, restated

def pick_bn(ntot):
    """csrc/conv_igemm.hip: int pick_bn(int ntot) { return ntot >= 128 ? 128 : (ntot >= 64 ? 64 : 32); }"""
    return 128 if ntot >= 128 else (64 if ntot >= 64 else 32)


def pick_kc(bn, chan, taps=9):
    """csrc/conv_igemm.hip pick_kc:
        if (taps == 1) { int kc = 16; while (kc > 8 && (chan % kc)) kc >>= 1; return kc; }
        int kc = 1024 / bn; if (kc > 16) kc = 16; while (kc > 8 && (chan % kc)) kc >>= 1; return kc;"""
    kc = 16 if taps == 1 else min(1024 // bn, 16)
    while kc > 8 and chan % kc:
        kc >>= 1
    return kc


# launch_taps<TAPS>: (KC, BN) -> launch_cfg<TAPS, KC, BN, MT, NT, WM, WN>.  The three `kc == 32` arms of launch_taps<1> are not listed: pick_kc never returns 32.
_MNW = {32: (2, 1, 4, 1), 64: (2, 2, 4, 1), 128: (2, 2, 2, 2)}
IGEMM_INSTANCES = ({(9, kc, bn) for kc, bn in ((16, 32), (8, 32), (16, 64), (8, 64), (8, 128))} |
                   {(1, kc, bn) for kc, bn in ((16, 32), (8, 32), (16, 64), (8, 64), (16, 128), (8, 128))})


def igemm_inst(taps, ntot, chan):
    """launch_taps: bn = pick_bn(a.Ntot), kc = pick_kc(bn, kc_chan, TAPS); `if (kc_chan % kc) return PNNP_E_UNSUPPORTED`.  -> (TAPS, KC, BN)."""
    bn = pick_bn(ntot)
    kc = pick_kc(bn, chan, taps)
    assert chan % kc == 0 and kc in (8, 16), (taps, ntot, chan, kc)
    if taps == 9:
        assert (kc, bn) != (16, 128)         # 1024 / 128 = 8
    return (taps, kc, bn)


def igemm_th(bn):
    """IgemmCfg: TH = WM * MT."""
    mt, _, wm, _ = _MNW[bn]
    return wm * mt


def igemm_tiles(B, DH, DW, ntot):
    """launch_cfg: tiles = ((a.DW + 31) / 32) * ((a.DH + Cfg::TH - 1) / Cfg::TH) * a.B * ((a.Ntot + BN - 1) / BN); the grid is min(tiles, per_cu * cus) workgroups and
    workgroup i of G walks tiles i', i' + G, ... (i' = xcd_remap(i, G), a bijection), so the shares are ceil or floor of tiles / G."""
    bn = pick_bn(ntot)
    th = igemm_th(bn)
    return ((DW + 31) // 32) * ((DH + th - 1) // th) * B * ((ntot + bn - 1) // bn)


def igemm_class(tiles, cus):
    """'one': a tile per workgroup whatever the occupancy query says (tiles <= cus: the grid is at least cus);  'many': more tiles than 8 x cus -- 8 is the most
    256-thread workgroups a CU holds (32 wave slots / 4 waves) -- and no k x cus (k = 1..4; __launch_bounds__(256, 2) and ~40 KB of LDS allow 2-4) divides
    them, so some workgroup takes two or more and the shares are uneven;  else 'between'."""
    if tiles <= cus:
        return 'one'
    if tiles > 8 * cus and all(tiles % (k * cus) for k in (1, 2, 3, 4)):
        return 'many'
    return 'between'


def pick_shape(M, N):
    """csrc/wgrad.hip: int pick_shape(int M, int N) { return (M > 32 ? 1 : 0) + (N > 32 ? 2 : 0); }"""
    return (1 if M > 32 else 0) + (2 if N > 32 else 0)


def tile_rows(taps, shape):
    """csrc/wgrad.hip tile_rows (taps == 18: the stride-2 3x3 layer):
        if (taps == 18) return shape == 0 ? 4 : (shape == 3 ? 1 : 2);
        return taps == 4 ? 2 : (shape == 0 ? 4 : 2);"""
    if taps == 18:
        return 4 if shape == 0 else (1 if shape == 3 else 2)
    return 2 if taps == 4 else (4 if shape == 0 else 2)


def wgrad_tiles(B, H, W, M, N, taps):
    th = tile_rows(taps, pick_shape(M, N))
    return ((W + 31) // 32) * ((H + th - 1) // th) * B


def wgrad_splits(B, H, W, M, N, taps):
    """csrc/wgrad.hip pnnp_wgrad_splits (H, W: the U map -- the OUTPUT of a stride-2 layer, the INPUT of a ConvTranspose2d):
        const int bmo = (shape & 1) ? 64 : 32, bno = (shape & 2) ? 64 : 32;
        const int tiles = ((W + 31) / 32) * ((H + th - 1) / th) * B;
        const int out_tiles = ((M + bmo - 1) / bmo) * ((N + bno - 1) / bno);
        int z = (2 * 256 + out_tiles - 1) / out_tiles;  if (z > tiles) z = tiles;  if (z < 1) z = 1;"""
    shape = pick_shape(M, N)
    bmo, bno = (64 if shape & 1 else 32), (64 if shape & 2 else 32)
    out_tiles = ((M + bmo - 1) // bmo) * ((N + bno - 1) // bno)
    return max(1, min((512 + out_tiles - 1) // out_tiles, wgrad_tiles(B, H, W, M, N, taps)))


def wgrad_depth(B, H, W, M, N, taps, bias=False):
    """The most rounded additions any one product passes on its way into a weight gradient (bias: any one value into a bias gradient) -- the n of a summation
    tree is its depth, not its size, and B*H*W + Z above is the size.  As csrc/wgrad.hip sums:
      wgrad_kernel: a wave owns rows r = wk, wk + WK, ... < TH of a pixel tile (launch_shape / launch_s2: WK = 4 / 2 / 2 / 1 by pick_shape) and chains 32
        products per row and tap into one accumulator, over the ceil(tiles / Z) pixel tiles of its workgroup; then the WK waves are added in order.
        (bsum takes 16 values per row and half-wave, then one __shfl_xor addition; a ConvTranspose2d's bsn 4 taps x 16.)
      slab_reduce_kernel: thread row ty adds slabs ty, ty + 8, ... in four interleaved partial sums (<= ceil(Z / 32) each, then <= 3 more into the first),
        two additions join the four, eight join the thread rows."""
    shape = pick_shape(M, N)
    wk = (4, 2, 2, 1)[shape]
    th = tile_rows(taps, shape)
    tiles, z = wgrad_tiles(B, H, W, M, N, taps), wgrad_splits(B, H, W, M, N, taps)
    per_row = ((64 if taps == 4 else 16) + 1) if bias else 32
    return ((tiles + z - 1) // z) * ((th + wk - 1) // wk) * per_row + wk + (z + 31) // 32 + 3 + 2 + 8


def wgrad_class(B, H, W, M, N, taps):
    """wgrad_kernel: split z walks pixel tiles z, z + Z, ...  'one': none walks two;  'many': some walk two or more and the shares are uneven."""
    t, z = wgrad_tiles(B, H, W, M, N, taps), wgrad_splits(B, H, W, M, N, taps)
    return 'one' if t <= z else ('many' if t % z else 'even')

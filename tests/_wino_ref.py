"""Float64 references, a derived per-element error bound, a float32 emulation and a mirror of the launch rules for the Winograd F(2x2,3x3) kernels
(csrc/wino.hip, csrc/wino_wgrad.hip and the filter transform wino_job of csrc/pack_jobs.hip behind ops.conv_wino_fwd / conv_wino_bwd_data /
conv_wino_bwd_data_res / conv_wino_bwd_weight / pack_conv_weight_wino).  No GPU: torch on the CPU.  Ref, bound, U, SLOPE, _act, _dact and the epilogue
counting come from tests/_direct_ref.py.

The bound.  `ref` is the plain operation in float64 (F.conv2d / F.conv_transpose2d / autograd).  Winograd subtracts before it multiplies, so its error is NOT
bounded by the direct form's S = conv(|x|, |w|); it is bounded by the same algorithm run on absolute values with the absolute values of the transform
matrices, every term of which passes a counted number of float32 roundings:

    S_w  = |A|^T [ sum_k (|G| |g_k| |G|^T) (.) (|B|^T |d_k| |B|) ] |A|        (+ |bias|, |residual|, |addsrc|, |base| as in _direct_ref)
    |got - ref64| <= (K + 10 + e) 2^-24 S_w 1.01

  K   the k-ordered fma chain of v_mfma_f32_32x32x2_f32: wino_kernel keeps ONE accumulator acc[xi] per transformed position over all K / 8 chunks.
  10  = 4 in U = G g G^T as wino_job computes it (gg[1] = 0.5f * (g0 + g1 + g2): two additions, the halving is exact; the same again along the row)
      + 2 in B^T d B (input_transform / WINO_STEP: t = fma(db, +-1, da), one rounding; then one t - t' or t + t')
      + 4 in A^T M A (s[j] = acc[j] + acc[4 + j] + acc[8 + j]: two additions; o = s[0] + s[1] + s[2]: two more).
  e   the epilogue as _direct_ref counts it: bias, residual / addsrc, the slope 0.2 of an activation or of a mask, accumulation; multiplications by 1 or 0
      are exact (the kernel's `v + bias4` with a zero bias4 and `fmaxf(v, 1.f * v)` round nothing).

The weight gradient  dg = G^T [ sum_tiles (A dY A^T) (.) (B^T d B) ] G  likewise, with

    S_wg = |G|^T [ sum_tiles (|A| |dY| |A|^T) (.) (|B|^T |d| |B|) ] |G|

  by size   n = tiles + 8 + Z, tiles = B H W / 4;  8 = 2 (z_write: r = za * y0 + zb * y1 with za, zb in {0, +-1}, then r + r' or r - r')
            + 2 (v_write: one fma, one add / sub) + 4 (h = u0 + 0.5f * (u1 + u2): two additions, and again for w0..w2);  Z slabs.
  by depth  n = 8 per + 8 + ceil(Z / 8) + 8: a workgroup chains the 8 tiles of a chunk (k of four 32x32x2 MFMAs) over its `per` chunks into one accumulator,
            the 8 transform roundings, then ww_reduce_kernel: thread row ty adds slabs ty, ty + 8, ... (ceil(Z / 8)), then `t += red[k]` over the 8 rows.
  bias      S = sum |g|.  By size n = B H W + Z.  By depth n = 1 + 3 + 2 per + ceil(Z / 8) + 8: r = y0 + y1 (wave 1: za = zb = 1), the tree
            ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)) of depth 3, one addition into bsum per z_write call, two calls per chunk, then the reduce.
  `accumulate = 1` adds one rounded addition (e = 1, _direct_ref.accumulated).

emulate_* below run the same operations with every float32 rounding the kernels make, in their order; tests/test_host_wino_ref.py holds them to these bounds
(the proof that the reference and the bound agree without a GPU) and prints what Winograd costs against the direct form's S.

Tensors are NCHW, float32 on the way in, float64 on the way out."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import _direct_ref as R
from _direct_ref import Ref, U, SLOPE, bound, d, _act, _dact, _epilogue, accumulated  # noqa: F401  (re-exported)

BT = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=torch.float64)
G = torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=torch.float64)
AT = torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=torch.float64)

TRANSFORM_ROUNDINGS = 4 + 2 + 4        # U, V, A^T M A (docstring)
WG_TRANSFORM_ROUNDINGS = 2 + 2 + 4     # Z, V, G^T dU G


def _mats(absolute):
    return (BT.abs(), G.abs(), AT.abs()) if absolute else (BT, G, AT)


def _patches(x):
    """The 4x4 input patches of the 2x2 output tiles of x [B, C, H, W] (pad 1, tiles from pixel (0, 0), the map padded with zeros to whole tiles)
    -> [B, C, 4, 4, L], ty, tx."""
    B, C, H, W = x.shape
    ty, tx = (H + 1) // 2, (W + 1) // 2
    xp = F.pad(x, (1, 2 * tx - W + 1, 1, 2 * ty - H + 1))
    return F.unfold(xp, 4, stride=2).view(B, C, 4, 4, ty * tx), ty, tx


def _untile(y, ty, tx, H, W):
    """[B, N, 2, 2, L] -> [B, N, H, W]"""
    B, N = y.shape[:2]
    return y.view(B, N, 2, 2, ty, tx).permute(0, 1, 4, 2, 5, 3).reshape(B, N, 2 * ty, 2 * tx)[:, :, :H, :W]


def wino_conv(x, w, absolute=False):
    """conv3x3(x, w), pad 1, through F(2x2,3x3) in float64; absolute: |x|, |w| and the absolute values of the three matrices (S_w)."""
    x, w = d(x), d(w)
    bt, g, at = _mats(absolute)
    if absolute:
        x, w = x.abs(), w.abs()
    B, C, H, W = x.shape
    p, ty, tx = _patches(x)
    V = torch.einsum('ia,bcajl,kj->bcikl', bt, p, bt)
    Uw = torch.einsum('ia,ncaj,kj->ncik', g, w, g)
    M = torch.einsum('ncik,bcikl->bnikl', Uw, V)
    Y = torch.einsum('ia,bnajl,kj->bnikl', at, M, at)
    return _untile(Y, ty, tx, H, W)


def dgrad_filter(w):
    """The filter of the backward-data convolution: w2[n][k][a][b] = w[k][n][2 - a][2 - b] (wino_job: `g[r][c] = dgrad ? w[(k * Cin + n) * 9 + (2 - r) * 3 + (2 - c)]`)."""
    return w.flip(2, 3).transpose(0, 1).contiguous()


def conv_fwd(x, w, b=None, residual=None, act=0):
    """act(conv3x3(x, w) + b + residual): ref by F.conv2d, S = S_w + |b| + |residual|, n = K + 10."""
    r = R.conv_fwd(x, w, b, residual, act)
    S = wino_conv(x, w, True) + (0 if b is None else d(b).abs().view(1, -1, 1, 1)) + (0 if residual is None else d(residual).abs())
    return Ref(r.ref, S, w.shape[1] + TRANSFORM_ROUNDINGS, r.e)


def conv_bwd_data(g, w, c0=0, c1=None, mask=None, mode=0, base=None, addsrc=None):
    """_direct_ref.conv_bwd_data (channels [c0, c1) of (dgrad(g) [+ addsrc]) * act'(mask) [+ base]) with S_w in place of S and n = Cout + 10."""
    r = R.conv_bwd_data(g, w, c0, c1, mask, mode, base, addsrc)
    S = wino_conv(g, dgrad_filter(w)[c0:c1], True)
    if addsrc is not None:
        S = S + d(addsrc).abs()
    S = S * _dact(mask, mode)
    if base is not None:
        S = S + d(base).abs()
    return Ref(r.ref, S, w.shape[0] + TRANSFORM_ROUNDINGS, r.e)


def filter_transform(w, dgrad=False):
    """U = G g G^T [N][K][4][4] in float64 and |G| |g| |G|^T; forward: g = w[n][k], backward-data: g = w[k][n] flipped."""
    g = d(dgrad_filter(w) if dgrad else w)
    return torch.einsum('ia,ncaj,kj->ncik', G, g, G), torch.einsum('ia,ncaj,kj->ncik', G.abs(), g.abs(), G.abs())


def unpack_u(u, K, N):
    """A pack [N/64][K/8][16][2][64][4] (wino_job: `o = u + (nb * (K / 8) + kc) * US_STAGE + (kg * 64 + nn) * 4 + e`, element xi at `+ xi * 2 * UPLANE`)
    -> [N][K][4][4]."""
    t = u.view(N // 64, K // 8, 16, 2, 64, 4)                  # nb kc xi kg nn e
    return t.permute(0, 4, 1, 3, 5, 2).reshape(N, K, 4, 4)     # (nb nn) (kc kg e) xi


def wino_wgrad(g, x, absolute=False):
    """dW [Cout][Cin][3][3] of conv3x3(x, w), pad 1, given g = dL/dy, through F(2x2,3x3) in float64 (H, W even); absolute: S_wg."""
    zp, x = d(g), d(x)
    bt, gm, at = _mats(absolute)
    if absolute:
        zp, x = zp.abs(), x.abs()
    B, M, H, W = zp.shape
    ty, tx = H // 2, W // 2
    dy = zp.view(B, M, ty, 2, tx, 2).permute(0, 1, 3, 5, 2, 4).reshape(B, M, 2, 2, ty * tx)
    a = at.t()
    Z = torch.einsum('ia,bmajl,kj->ikbml', a, dy, a)
    p, _, _ = _patches(x)
    V = torch.einsum('ia,bnajl,kj->ikbnl', bt, p, bt)
    L = Z.shape[-1]
    dU = torch.matmul(Z.permute(0, 1, 3, 2, 4).reshape(4, 4, M, B * L), V.permute(0, 1, 2, 4, 3).reshape(4, 4, B * L, -1))      # [4][4][M][N]
    return torch.einsum('ia,ajmn,jk->mnik', gm.t(), dU, gm)


def conv_bwd_weight(g, x, Z, per):
    """dW, dbias of conv3x3 on x (the cat of a two-tensor input) by autograd in float64 -> (Ref dW, depth dW, Ref dbias, depth dbias); the Refs carry the n by size."""
    B, Co, H, W = g.shape
    fn = lambda x, w, b: F.conv2d(x, w, b, padding=1)
    dW, db = R._wgrad(fn, (Co, x.shape[1], 3, 3), Co, d(x), d(g))
    zr = (Z + 7) // 8
    return (Ref(dW, wino_wgrad(g, x, True), B * H * W // 4 + WG_TRANSFORM_ROUNDINGS + Z, 0), 8 * per + WG_TRANSFORM_ROUNDINGS + zr + 8,
            Ref(db, d(g).abs().sum((0, 2, 3)), B * H * W + Z, 0), 1 + 3 + 2 * per + zr + 8)


# ---------------------------------------------------------------- the kernels' arithmetic in float32, rounding by rounding

def _f(t):
    return t.float()


def _fma(a, b, c):
    """float32 fma: the product of two float32 is exact in float64; the sum is rounded to float64 and then to float32 (a double rounding 2^-29 below the
    float32 one: it makes the emulation no more exact than the hardware)."""
    return (a.double() * b.double() + c.double()).float()


def emulate_filter(w, dgrad=False):
    """wino_job: gg[1] = 0.5f * (g0 + g1 + g2), gg[2] = 0.5f * (g0 - g1 + g2) per column, then the same per row.  -> [N][K][4][4] float32"""
    g = _f(dgrad_filter(w) if dgrad else w)
    def pass_(t, dim):
        a, b, c = t.unbind(dim)
        return torch.stack([a, 0.5 * ((a + b) + c), 0.5 * ((a - b) + c), c], dim)
    return pass_(pass_(g, 2), 3)


def _emulate_v(p):
    """input_transform on patches [..., 4, 4, L] float32: rows t_i = fma(d_rb, sg, d_ra) (d0 - d2, d1 + d2, d2 - d1, d1 - d3), then t0 - t2, t1 + t2, t2 - t1, t1 - t3."""
    r0, r1, r2, r3 = p.unbind(-3)
    t = torch.stack([r0 - r2, r1 + r2, r2 - r1, r1 - r3], -3)
    c0, c1, c2, c3 = t.unbind(-2)
    return torch.stack([c0 - c2, c1 + c2, c2 - c1, c1 - c3], -2)


def emulate_core(x, w, dgrad=False):
    """wino_kernel on x [B, K, H, W] up to A^T M A (dgrad: x is g and w the layer's weight).  -> NCHW float32"""
    x = _f(x)
    Uw = emulate_filter(w, dgrad)                              # [N][K][4][4]
    B, K, H, W = x.shape
    p, ty, tx = _patches(x)
    V = _emulate_v(p)                                          # [B][K][4][4][L]
    acc = torch.zeros(B, Uw.shape[0], 4, 4, V.shape[-1])
    for k in range(K):                                         # the MFMA chain, k ascending over all chunks
        acc = _fma(V[:, None, k], Uw[None, :, k, :, :, None], acc)
    m0, m1, m2, m3 = acc.unbind(2)
    s, t = (m0 + m1) + m2, (m1 - m2) - m3                      # over the first index, then over the second
    def cols(r):
        c0, c1, c2, c3 = r.unbind(2)
        return torch.stack([(c0 + c1) + c2, (c1 - c2) - c3], 2)
    return _untile(torch.stack([cols(s), cols(t)], 2), ty, tx, H, W)


def emulate_epilogue(v, b=None, residual=None, act=0, mask=None, mode=0, base=None):
    """wino_kernel's epilogue on emulate_core's result: + bias, + residual / addsrc, max(v, slope * v), * act'(mask), + what the destination held."""
    if b is not None:
        v = v + _f(b).view(1, -1, 1, 1)
    if residual is not None:
        v = v + _f(residual)
    if act:
        v = torch.maximum(v, v * (np.float32(0.2) if act == 1 else np.float32(0.0)))
    if mask is not None and mode:
        v = v * torch.where(_f(mask) > 0, 1.0, 0.2 if mode == 1 else 0.0).float()
    if base is not None:
        v = v + _f(base)
    return v


def emulate_bwd_weight(g, x, Z, per, m_keep=4, n_keep=4):
    """wino_wgrad_kernel + ww_reduce_kernel for the first m_keep output and n_keep input channels (every element sums alone): split z chains the 8 tiles of
    each of its chunks [z * per, min(chunks, (z + 1) * per)) into one accumulator, transforms, and the reduce adds the Z slabs as 8 thread rows.  The bias sum
    takes all channels.  -> dW [m_keep][n_keep][3][3], db [Cout], float32."""
    g, x = _f(g), _f(x)
    B, M, H, W = g.shape
    m_keep, n_keep = min(m_keep, M), min(n_keep, x.shape[1])
    cy, cx = H // 4, W // 8
    chunks = B * cy * cx
    # tiles in chunk order: chunk = (b, cy, cx), tile in chunk = (tq, 4 tiles)
    def by_chunk(t):                                           # [B][C][r][s][ty*tx] -> [chunks][8][C][r][s]
        C, r, s = t.shape[1:4]
        t = t.view(B, C, r, s, cy, 2, cx, 4).permute(0, 4, 6, 5, 7, 1, 2, 3)
        return t.reshape(chunks, 8, C, r, s)
    dy = g.view(B, M, H // 2, 2, W // 2, 2).permute(0, 1, 3, 5, 2, 4).reshape(B, M, 2, 2, -1)
    y0, y1 = dy[:, :, 0], dy[:, :, 1]                          # [B][M][2 cols][L]
    rows = torch.stack([y0, y0 + y1, y0 - y1, -y1], 2)         # r = za * y0 + zb * y1, [B][M][4][2][L]
    e, o = rows[:, :, :, 0], rows[:, :, :, 1]
    e, o = e[:, :m_keep], o[:, :m_keep]
    Zt = by_chunk(torch.stack([e, e + o, e - o, -o], 3))
    p, _, _ = _patches(x[:, :n_keep])
    Vt = by_chunk(_emulate_v(p))
    pad = Z * per - chunks
    Zt = torch.cat([Zt, torch.zeros(pad, *Zt.shape[1:])]).view(Z, per * 8, m_keep, 4, 4)
    Vt = torch.cat([Vt, torch.zeros(pad, *Vt.shape[1:])]).view(Z, per * 8, n_keep, 4, 4)
    acc = torch.zeros(Z, m_keep, n_keep, 4, 4)
    for k in range(per * 8):                                   # (a padded chunk adds exact zeros)
        acc = _fma(Zt[:, k, :, None], Vt[:, k, None, :], acc)
    def gt(u, dim):
        u0, u1, u2, u3 = u.unbind(dim)
        return torch.stack([_fma(torch.tensor(0.5), u1 + u2, u0), 0.5 * (u1 - u2), _fma(torch.tensor(0.5), u1 + u2, u3)], dim)
    slab = gt(gt(acc, 3), 4)
    # bias: wave 1 sums r = y0 + y1 over the 8 columns of a chunk's tile-row pair as a depth-3 tree, one fma into bsum per tile row
    r = (y0 + y1).view(B, M, cy, 2, cx, 8).permute(0, 2, 4, 3, 1, 5).reshape(chunks, 2, M, 8)
    s8 = ((r[..., 0] + r[..., 1]) + (r[..., 2] + r[..., 3])) + ((r[..., 4] + r[..., 5]) + (r[..., 6] + r[..., 7]))
    s8 = torch.cat([s8, torch.zeros(pad, 2, M)]).view(Z, per * 2, M)
    bs = torch.zeros(Z, M)
    for k in range(per * 2):
        bs = bs + s8[:, k]
    def reduce(sl):
        rows_ = []
        for ty in range(8):
            s = torch.zeros(sl.shape[1:])
            for zz in range(ty, Z, 8):
                s = s + sl[zz]
            rows_.append(s)
        t = torch.zeros(sl.shape[1:])
        for s in rows_:
            t = t + s
        return t
    return reduce(slab), reduce(bs)


# ---------------------------------------------------------------- the launch rules, restated

def wino_supported(K, N):
    """csrc/wino.hip: int pnnp_wino_supported(int K, int N) { return (K % KC == 0 && N % BN == 0) ? 1 : 0; }   (KC = 8, BN = 64)"""
    return K % 8 == 0 and N % 64 == 0


def wino_grid(B, H, W, K, N):
    """wino_launch: a.tiles_x = (a.W + 15) / 16; a.tiles_y = (a.H + 15) / 16;  grid((a.tiles_x * a.tiles_y * a.B), (a.N / BN));
    wino_kernel: const int nchunks = a.K / KC;    -> (tiles_x, tiles_y, (grid x, grid y), nchunks)"""
    tx, ty = (W + 15) // 16, (H + 15) // 16
    return tx, ty, (tx * ty * B, N // 64), K // 8


def wino_switch_chunk(C1, C2):
    """gload_raw: `const bool s = k0 >= a.C1;` with k0 = c * KC: the first chunk read from src[1], or None with one source."""
    return C1 // 8 if C2 else None


def depth_class(nchunks):
    """The prologue stages chunks 0, 1, 2 (`if (nchunks > 1)`, `if (nchunks > 2)`), iteration c prefetches min(c + 3, nchunks - 1): 1, 2, 3, 4 or '5+' chunks."""
    return nchunks if nchunks < 5 else '5+'


def switch_class(C1, C2):
    s = wino_switch_chunk(C1, C2)
    return None if s is None else (s if s < 4 else '4+')


def wino_wgrad_supported(H, W, Cout, C1, C2=0):
    """csrc/wino_wgrad.hip: return (H > 0 && W > 0 && H % 4 == 0 && W % 8 == 0 && Cout % BM == 0 && C1 % BN == 0 && C2 % BN == 0) ? 1 : 0;"""
    return H > 0 and W > 0 and H % 4 == 0 and W % 8 == 0 and Cout % 64 == 0 and C1 % 64 == 0 and C2 % 64 == 0


def ww_chunks(B, H, W):
    """ww_splits: const int chunks = B * (H / 4) * (W / 8);"""
    return B * (H // 4) * (W // 8)


def ww_splits(B, H, W, M, N, cus=256):
    """ww_splits: const int blocks = (M / BM) * (N / BN);  int z = (cus + blocks - 1) / blocks;  if (z > chunks) z = chunks;  if (z < 1) z = 1;
        const int per = (chunks + z - 1) / z;  return (chunks + per - 1) / per;"""
    chunks, blocks = ww_chunks(B, H, W), (M // 64) * (N // 64)
    z = max(1, min((cus + blocks - 1) // blocks, chunks))
    per = (chunks + z - 1) // z
    return (chunks + per - 1) // per


def ww_per(B, H, W, M, N, cus=256):
    """wino_wgrad_kernel: const int per = (a.nchunks + a.Z - 1) / a.Z;"""
    return (ww_chunks(B, H, W) + ww_splits(B, H, W, M, N, cus) - 1) // ww_splits(B, H, W, M, N, cus)


def ww_nloc(B, H, W, M, N, cus=256):
    """wino_wgrad_kernel: c_begin = z * per, c_end = min(a.nchunks, c_begin + per), nloc = c_end - c_begin   -> the list over z"""
    chunks, Z, per = ww_chunks(B, H, W), ww_splits(B, H, W, M, N, cus), ww_per(B, H, W, M, N, cus)
    return [min(chunks, (z + 1) * per) - z * per for z in range(Z)]


def ww_crosses_image(B, H, W, M, N, cus=256):
    """chunk_pos: `b = c / a.chunks_y` after `c /= a.chunks_x`: a split whose first and last chunk lie in different images."""
    chunks, per, img = ww_chunks(B, H, W), ww_per(B, H, W, M, N, cus), (H // 4) * (W // 8)
    return any(z * per // img != (min(chunks, (z + 1) * per) - 1) // img for z in range(ww_splits(B, H, W, M, N, cus)))


def ww_workspace_floats(B, H, W, Cout, Cin, cus=256):
    """pnnp_wino_wgrad_workspace_floats: if (!pnnp_wino_wgrad_supported(H, W, Cout, Cin, 0)) return 0;  return z * ((int64_t)9 * Cout * Cin + Cout);"""
    if not wino_wgrad_supported(H, W, Cout, Cin):
        return 0
    return ww_splits(B, H, W, Cout, Cin, cus) * (9 * Cout * Cin + Cout)


def ww_class(B, H, W, M, N, cus=256):
    """'one' / 'two' / 'three': per = 1 / 2 / 3;  'many': per >= 4 and a shorter last split (the chunk loop runs past its three staged chunks and parks
    on a last chunk that comes early);  'even': per >= 4, all splits alike."""
    per, nloc = ww_per(B, H, W, M, N, cus), ww_nloc(B, H, W, M, N, cus)
    assert all(n >= 1 for n in nloc) and sum(nloc) == ww_chunks(B, H, W)
    return {1: 'one', 2: 'two', 3: 'three'}.get(per, 'many' if nloc[-1] < per else 'even')


def ww_map(cus, blocks, per, rem, cross=False):
    """The smallest (B, H, W) whose chunks make splits of `per` chunks with `rem` in the last one (rem < per; rem = 0: any) on a device with `cus` compute units and
    `blocks` 64 x 64 output blocks; cross: some split crosses an image boundary."""
    z = (cus + blocks - 1) // blocks
    for chunks in range((per - 1) * z + 1, per * z + 1):
        if per > 1 and rem and chunks % per != rem:
            continue
        for B in ((3, 2) if cross else (1, 2, 3)):
            if chunks % B:
                continue
            hw = chunks // B
            for h in range(int(math.isqrt(hw)), 0, -1):
                if hw % h == 0 and hw // h <= 4 * h + 8:
                    m = (B, 4 * h, 8 * (hw // h))
                    if ww_per(*m, 64, 64 * blocks, cus) == per and (not cross or ww_crosses_image(*m, 64, 64 * blocks, cus)):
                        return m
                    break
    raise AssertionError(('no map', cus, blocks, per, rem, cross))

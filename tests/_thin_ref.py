"""Float64 references, summation depths and a mirror of the launch rules for the thin ends of the networks (csrc/thin.hip behind ops.head_fwd / head_bwd /
first_fwd / first_bwd_weight).  No GPU: torch on the CPU in float64.  The bound and its vocabulary (U, SLOPE, Ref, bound, accumulated, d) are those of
tests/_direct_ref.py:  |got - ref64| <= (n + e) * 2^-24 * S * 1.01  per element, n products summed, e rounded epilogue operations, S the same operation on
absolute values.  These kernels are float32 on the vector ALUs: a product and the addition that takes it in are two roundings or (contracted to an fma) one,
so "n products and n additions" costs at most n + 1 roundings on any path and the n of the forward kernels below (the products of an element) covers it: the
forward of the head chains 4 products in a lane and joins LPP = cin / 4 lanes in log2(LPP) additions, the first layer chains 18 packed products into two
partial sums and joins them.

A weight or bias gradient sums B*H*W terms per element.  That is the SIZE of the sum; what bounds its rounding error is its DEPTH, the most rounded operations
one term passes on its way into the element (head_bwd_depth, first_wgrad_depth: a few hundred where the size is several hundred thousand).  The tests assert
the bound with both; only the second can see a 64-pixel group or a pixel tile that went missing from a large map.  (With n = B*H*W beyond 3e5 the factor 1.01
no longer covers the second-order terms of the size bound; the depth bound, which is asserted beside it and is the smaller of the two, is the rigorous one.)

Tensors here are NCHW, float32 on the way in, float64 on the way out; the tests lay them out as the kernels want them."""
import math

import torch
import torch.nn.functional as F

from _direct_ref import SLOPE, U, Ref, accumulated, bound, d  # noqa: F401  (re-exported: the tests take them from here)


def _act(z, act):
    return torch.where(z > 0, z, SLOPE * z) if act == 1 else (F.relu(z) if act == 2 else z)


# ---------------------------------------------------------------- references

def head_fwd(x, w, b, residual=None):
    """conv1x1(x [B,cin,H,W]; w [cout,cin,1,1]) + b (+ residual [B,cout,H,W]): n = cin products, e = 1 (bias) + (residual is not None)."""
    run = lambda x, w, b, r: F.conv2d(x, w, b) + (0 if r is None else r)
    z = run(d(x), d(w), d(b), d(residual))
    S = run(d(x).abs(), d(w).abs(), d(b).abs(), None if residual is None else d(residual).abs())
    return Ref(z, S, w.shape[1], 1 + (residual is not None))


def _sum_pix(g, x):
    """sum over b, h, w of g[b][o] x[b][i] -> [o][i], in float64, as a plain einsum."""
    return torch.einsum('bohw,bihw->oi', g, x)


def head_bwd(g, x, w, mode):
    """The head's one-pass backward given g = dL/dout [B,cout,H,W], its input x [B,cin,H,W] and w [cout,cin,1,1] -> (gx, dW, db).
    gx [B,cin,H,W] = (sum_co g w) * act'(x): n = 4 products (the kernel always multiplies four, the rows past cout being zeros), e = (mode == 1): the mask is
    x > 0 on the float32 x, the slope float32(0.2), one rounded multiplication.  dW [cout,cin,1,1] = sum_pix g (x) x and db [cout] = sum_pix g: size
    n = B*H*W, no epilogue."""
    B, Co, H, W = g.shape
    gd, xd, wd = d(g), d(x), d(w).reshape(Co, -1)
    m = 1.0 if mode == 0 else torch.where(x > 0, 1.0, SLOPE if mode == 1 else 0.0).double()
    gx = torch.einsum('bohw,oi->bihw', gd, wd) * m
    Sx = torch.einsum('bohw,oi->bihw', gd.abs(), wd.abs()) * m
    npix = B * H * W
    return (Ref(gx, Sx, 4, int(mode == 1)),
            Ref(_sum_pix(gd, xd)[:, :, None, None], _sum_pix(gd.abs(), xd.abs())[:, :, None, None], npix, 0),
            Ref(gd.sum((0, 2, 3)), gd.abs().sum((0, 2, 3)), npix, 0))


def first_fwd(x, w, b=None, act=0):
    """act(conv3x3(x [B,cin,H,W]; w [cout,cin,3,3], pad 1) + b): n = 36 (the kernel multiplies four channels per tap whatever cin is; the zeros it adds are
    exact), e = (b is not None) + (act == 1)."""
    z = F.conv2d(d(x), d(w), d(b), padding=1)
    S = F.conv2d(d(x).abs(), d(w).abs(), None if b is None else d(b).abs(), padding=1)
    return Ref(_act(z, act), S, 36, (b is not None) + (act == 1))


def _first_dw(g, x):
    """dW[o][i][kh][kw] = sum_pix g[pix][o] x[pix + (kh - 1, kw - 1)][i] over the pixels whose tap lies inside the image: float64 einsums over shifted views,
    not autograd through a padded convolution, so that a padding zero never meets an inf of g."""
    B, Co, H, W = g.shape
    dW = torch.zeros(Co, x.shape[1], 3, 3, dtype=torch.float64)
    for kh in range(3):
        for kw in range(3):
            h0, h1, w0, w1 = max(0, 1 - kh), min(H, H + 1 - kh), max(0, 1 - kw), min(W, W + 1 - kw)
            dW[:, :, kh, kw] = _sum_pix(g[:, :, h0:h1, w0:w1], x[:, :, h0 + kh - 1:h1 + kh - 1, w0 + kw - 1:w1 + kw - 1])
    return dW


def first_bwd_weight(g, x):
    """dW [cout,cin,3,3] and db [cout] of Conv2d(3, pad 1) on x [B,cin,H,W] given g [B,cout,H,W]: size n = B*H*W each, no epilogue."""
    B, Co, H, W = g.shape
    gd, xd = d(g), d(x)
    npix = B * H * W
    return (Ref(_first_dw(gd, xd), _first_dw(gd.abs(), xd.abs()), npix, 0),
            Ref(gd.sum((0, 2, 3)), gd.abs().sum((0, 2, 3)), npix, 0))


# ---------------------------------------------------------------- the launch rules, restated

HEAD_FWD_PER_CU, HEAD_BWD_PER_CU, FW_PER_CU, FW_TW = 8, 4, 6, 48


def head_lpp(cin):
    """csrc/thin.hip: int head_lpp(int cin) { return (cin == 16 || cin == 32 || cin == 64) ? cin / 4 : 0; }"""
    return cin // 4 if cin in (16, 32, 64) else 0


def thin_blocks(units, per_cu, cus):
    """csrc/thin.hip thin_blocks:
        const int64_t cap = (int64_t)pnnp_device_cus() * per_cu;
        return (int)(units < cap ? (units < 1 ? 1 : units) : cap);"""
    cap = cus * per_cu
    return (1 if units < 1 else units) if units < cap else cap


def head_launch(npix, per_cu, cus):
    """pnnp_head_fwd_et: `const dim3 grid(thin_blocks((npix >> 6) / 4, 8))`; pnnp_head_bwd_amax_f32: `const int blocks = thin_blocks((npix >> 6) / 4, 4)`;
    both kernels: `const int64_t ngroups = a.npix >> 6; wave0 = blockIdx.x * 4 + wave; nwaves = gridDim.x * 4; for (grp = wave0; grp < ngroups; grp += nwaves)`.
    -> dict(ngroups, blocks, waves, trips: the most groups any wave takes, cls).  Classes:
      'one'     no wave takes two groups (ngroups <= waves)
      'second'  the grid is not capped, ngroups % 4 != 0 and ngroups > 4: units = ngroups / 4 rounds down, so waves 0 .. r - 1 (r = ngroups % 4, all in the
                first block) take a second group and no wave a third
      'capped'  blocks == per_cu * CUs and ngroups is no multiple of 4 * blocks: the shares are uneven and some wave makes two or more trips
      'even'    capped with equal shares (no case uses it)"""
    assert npix > 0 and npix % 64 == 0, npix
    ngroups = npix >> 6
    units = ngroups // 4
    blocks = thin_blocks(units, per_cu, cus)
    waves = 4 * blocks
    trips = -(-ngroups // waves)
    if ngroups <= waves:
        cls = 'one'
    elif units < per_cu * cus:
        assert ngroups > 4 and ngroups % 4 and trips == 2
        cls = 'second'
    else:
        cls = 'capped' if ngroups % waves else 'even'
    return dict(ngroups=ngroups, blocks=blocks, waves=waves, trips=trips, cls=cls)


def head_bwd_workspace(npix, cin, cus):
    """pnnp_head_bwd_amax_f32: `const int np = 4 * cin + 4; if (ws_floats < (int64_t)blocks * np) return PNNP_E_WORKSPACE;`"""
    return head_launch(npix, HEAD_BWD_PER_CU, cus)['blocks'] * (4 * cin + 4)


def first_launch(B, H, W, cout, cus):
    """pnnp_first_fwd_amax_et / pnnp_first_bwd_weight_f32: `const int tr = 512 / cout; tiles_w = ceil_div(W, FW_TW); a.ntiles = B * (H / tr) * a.tiles_w;
    blocks = thin_blocks(a.ntiles, FW_PER_CU)` (FW_TW = 48, FW_PER_CU = 6); both kernels: `for (tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x)` with
    `tw = tile % tiles_w, th = (tile / tiles_w) % tiles_h, b = tile / (tiles_w * tiles_h)` and `nw = min(FW_TW, a.W - w0)`.
    -> dict(tr, tiles_w, tiles_h, ntiles, blocks, per_wg: the most tiles any workgroup takes, nws: the set of nw met, cls).  Classes:
      'one'   ntiles <= 6 * CUs: a tile per workgroup
      'many'  ntiles > 6 * CUs and no multiple of it: some workgroup takes two or more and the shares are uneven
      'even'  more tiles than workgroups in equal shares (no case uses it)"""
    assert cout in (32, 64) and H % (512 // cout) == 0 and W % 16 == 0, (H, W, cout)
    tr = 512 // cout
    tiles_w, tiles_h = -(-W // FW_TW), H // tr
    ntiles = B * tiles_h * tiles_w
    blocks = thin_blocks(ntiles, FW_PER_CU, cus)
    cap = FW_PER_CU * cus
    cls = 'one' if ntiles <= cap else ('many' if ntiles % cap else 'even')
    nws = {min(FW_TW, W - tw * FW_TW) for tw in range(tiles_w)}
    return dict(tr=tr, tiles_w=tiles_w, tiles_h=tiles_h, ntiles=ntiles, blocks=blocks, per_wg=-(-ntiles // blocks), nws=nws, cls=cls)


def first_wgrad_workspace(B, H, W, cout, cus):
    """pnnp_first_bwd_weight_f32: `const int np = 37 * cout; if (ws_floats < (int64_t)blocks * np) return PNNP_E_WORKSPACE;`"""
    return first_launch(B, H, W, cout, cus)['blocks'] * 37 * cout


# ---------------------------------------------------------------- summation depth of the gradients

def head_bwd_depth(npix, cin, cus, bias=False):
    """The most rounded operations one product g x passes on its way into an element of the head's dW (bias: one value of g into db).  As csrc/thin.hip sums:
      head_bwd_kernel: a lane owns four channels of 64 / LPP pixels per group and adds them one after the other into one accumulator, over every group of its
        wave (`acc[co] += xv[k] * g4[co]; db += g4;` for k < LPP, inside the group loop): trips * LPP additions;
        `for (m = LPP; m < 64; m <<= 1) acc += __shfl_xor(acc, m)`: log2(64 / LPP) additions join the lanes of one channel quad;
        `(red[0] + red[1]) + (red[2] + red[3])`: 2 join the four waves.
      thin_reduce_kernel: thread slice s adds workgroups s, s + 16, ... into one sum, ceil(blocks / 16) additions; `v = red[0]; for (i = 1; i < 16; ++i)
        v += red[i]`: 15 join the slices.
      One more for the product itself (none for db, which sums g)."""
    L = head_launch(npix, HEAD_BWD_PER_CU, cus)
    lpp = head_lpp(cin)
    return L['trips'] * lpp + int(math.log2(64 // lpp)) + 2 + -(-L['blocks'] // 16) + 15 + (0 if bias else 1)


def first_wgrad_depth(B, H, W, cout, cus, bias=False):
    """The same for the first layer's dW (bias: db).  As csrc/thin.hip sums:
      first_wgrad_kernel: a lane (one output channel of one stream) walks its row pair through all 48 columns of a tile, `acc[..] += x * g2; db += gval`
        once per column and row -- the columns past nw too, with g made zero -- so 96 additions per tile into one accumulator, over every tile of its
        workgroup; `s = red[0]; for (i = 1; i < NS; ++i) s += red[i]`: NS - 1 = 256 / cout - 1 join the streams.
      thin_reduce_kernel: ceil(blocks / 16) + 15 as for the head.
      One more for the product itself (none for db)."""
    L = first_launch(B, H, W, cout, cus)
    return L['per_wg'] * 96 + 256 // cout - 1 + -(-L['blocks'] // 16) + 15 + (0 if bias else 1)


# ---------------------------------------------------------------- shapes of the capped and many-tile classes, by CU count

WINDOW = (1.02, 1.25)       # a capped / many-tile case has this many times the groups / tiles its grid takes in one trip; never a multiple


def head_capped_shape(cus, per_cu, straddle):
    """(B, H, W) with about 1.1 x (4 * per_cu * cus) groups of 64 pixels.  straddle: B = 4 images of H x 80, 5 H groups, H % 4 != 0 so that H * W % 64 != 0 and
    groups cross from one image into the next; else B = 2 images of H x 64."""
    t = 4 * per_cu * cus
    if straddle:
        H = -(-11 * t // 50)
        while H % 4 == 0:
            H += 1
        return (4, H, 80)
    return (2, -(-11 * t // 20), 64)


def first_many_shape(cus, cout, W):
    """(B, H, W) with B = 2 and about 1.1 x (6 * cus) tiles: W = 64 or 80 gives two column tiles, the second of 16 or 32 columns."""
    tiles_w = -(-W // FW_TW)
    tiles_h = -(-11 * FW_PER_CU * cus // (10 * 2 * tiles_w))
    return (2, tiles_h * (512 // cout), W)

// 3x3 convolution (forward / backward-data) on the fp16 matrix cores, float32 operands split into TWO scaled fp16 pieces (csrc/h2.h: the
// scheme, its error, the amax slots) -- the workgroup of csrc/conv_x3s.hip (8 MFMA-only consumer waves, 2 pixel rows x BN channels each, + 4
// producer waves; 16-row x 32-px tiles; persistent, XCD-aware tile order) with HALF the matrix instructions:
//
//   per 16-channel chunk and (16 px x 16 ch) block the nine taps need  hi hi' + lo hi'  (one v_mfma_f32_16x16x32_f16 per tap: pixels
//   [hi | lo] concatenated along K against weights [hi' | hi']) and  hi lo'  (half an instruction per tap: TWO TAPS share one, pixels
//   [hi @ tap t | hi @ tap t'] against [lo' @ t | lo' @ t'] -- the K halves of an instruction are fetched per lane anyway, so the second half
//   simply reads the halo image at the other tap's offset): 9 + 5 = 14 instructions where the bf16x3 kernel issues 27.
//
// Everything a chunk needs is resident at once -- halo image 2 pieces x 2 octets x 624 px x 16 B = 39 KB, weights 18 KB per 32-channel block
// -- so the work item is a whole CHUNK (one s_barrier per chunk instead of three), the weights ring has two chunk stages (LDS-DMA, one chunk
// ahead) and the halo tile two images.  Producers: fp32 NHWC global -> registers (one chunk ahead) -> x 2^se, hi / lo by v_fma_mix*_f16 (4
// vector instructions per pixel pair where the 3-way bf16 split took 11) -> LDS.  Consumers: ds_read_b128 + MFMA only inside the K loop; the
// epilogue works on the accumulators (x 2^-(se_x + se_w) by v_ldexp_f32, bias, activation, act' mask, residual, accumulate) and additionally
//   * tracks max|stored value| per destination (one atomicMax per wave at the end of the launch: the next layer's scale),
//   * forward: writes the SIGN BITS of the activated output, 32 per lane, in a tile-private layout; backward-data reads them back as the
//     LeakyReLU' / ReLU' mask -- 4 bytes per lane and 32-channel block where the float32 activation cost 8 x 16.
#include "conv_s.h"

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

namespace {

constexpr int WPLANE = 9 * 2 * 32 * 16;                            // the hi' piece of one 32-channel block of one chunk: [tap 9][octet 2][32][16 B] = 9216

// The 14 matrix instructions of a (chunk, 16 x 16 block): kind 0 = tap t0, pixels [hi | lo] x weights [hi' | hi'];  kind 1 / 2 = taps (t0, t0 + 1),
// pixels [hi @ t0 | hi @ t0 + 1] x weights [lo' @ t0 | lo' @ t0 + 1] (the second tap's halo offset is + 1 pixel, or + 32 from tap 2 to tap 3);
// tap 8 has no partner: its pair is (8, "9"), where the pack holds a tenth lo' tap of zeros (the pixel half reads one pixel on: finite x 0).
constexpr int NGRP = 14;
__device__ constexpr int grp_t0(int g) { constexpr int t[NGRP] = {0, 1, 0, 2, 3, 2, 4, 5, 4, 6, 7, 6, 8, 8}; return t[g]; }
__device__ constexpr int grp_kind(int g) { constexpr int k[NGRP] = {0, 0, 1, 0, 0, 2, 0, 0, 1, 0, 0, 1, 0, 1}; return k[g]; }

struct H2s {
    // halo image: 2 pieces x 2 octets x 624 px x 16 B = 39 KB; the 12 padding words of the hi planes are ZERO (the unpaired ninth tap reads one of them)
    static constexpr int PIECES = 2;
    static constexpr bool ZERO_PAD = true;
    static __device__ __forceinline__ void split(float a0, float a1, float s, unsigned (&p)[2]) { split_h2(a0, a1, s, p[0], p[1]); }
    // weights of one 32-channel block of one chunk: [hi' 9 taps][lo' 9 taps + one tap of ZEROS: the unpaired ninth tap's partner] = 19456 bytes (19 pieces)
    static constexpr int WBLK = 2 * WPLANE + 1024;
    // Everything a chunk needs is resident at once, so the work item is a whole CHUNK: two chunk stages, one chunk ahead, every staging slot in the one item
    static constexpr int ITEMS = 1, SLOTS = NSLOT;
    static constexpr int nstage(int) { return 2; }
    static constexpr int ahead(int) { return 1; }
    // producer register sets for the halo tile: 1 = a chunk's halo is requested at the END of the period before the one that splits it (round 5),
    // 2 / 3 = at the START of that period / a period earlier still (profiles/r6/ab_producer_sets.txt)
    static constexpr int NSETS = 2;
    static constexpr bool SCALED = true, BITS = true;
    static constexpr bool has(int EK, int BN) { return EK != EK_HEAD || BN == 32; }
    static __device__ __forceinline__ void scale_exps(const H2Args& ha, int& se_x, int& se_w) {
        unsigned ax = ha.amax_in[0] ? ha.amax_in[0][0] : 0u;
        if (ha.amax_in[1]) { const unsigned a2 = ha.amax_in[1][0]; ax = a2 > ax ? a2 : ax; }
        se_x = __builtin_amdgcn_readfirstlane(pnnp_h2_scale_exp(ax));
        se_w = __builtin_amdgcn_readfirstlane(ha.amax_w ? pnnp_h2_scale_exp(ha.amax_w[0]) : 0);
    }
    // MFMAs of one chunk (halo image img, weight stage st): group by group (grp_*), per group pass j (16 output channels) x pixel block mb.
    // The 4 pixel words of the NEXT group and the weight word of the NEXT pass are read between the MFMAs into the other register set.
    template <int BN>
    static __device__ __forceinline__ void mfma_item(f32x4 (&acc)[2 * MT][BN / 16], const u32x4* xs, const char* wsb, int wave, int lane, int, int st, int img) {
        constexpr int MB = 2 * MT, NB = BN / 16, WS_STAGE = (BN / 32) * WBLK, XS_F4 = PIECES * 2 * NPIXP;
        // lane bases (16-byte words of an image / bytes of a weight block); k-block q16 of an instruction = (octet q16 & 1, K half q16 >> 1).
        // Derived from an OPAQUE copy of the lane number per chunk: five registers that would otherwise live (spilled, in the 64-column forward
        // kernel) across the epilogue
        int lane_m = lane;
        asm volatile("" : "+v"(lane_m));
        const int r16 = lane_m & 15, q16 = lane_m >> 4, oct16 = q16 & 1, ps16 = q16 >> 1;
        const int rowbase = wave * MT * HC + r16;
        const int a_main = XS_PLANE(ps16, oct16) + rowbase;          // [hi | lo]
        const int a_hi = XS_PLANE(0, oct16) + rowbase;
        const int a_p1 = a_hi + ps16, a_p32 = a_hi + 32 * ps16;      // [hi @ t | hi @ t + 1]: the second tap is one pixel (taps 2 -> 3: 32 pixels) on
        const int b_main = (oct16 * 32 + r16) * 16, b_p1 = b_main + ps16 * 1024;
        const char* wst = wsb + st * WS_STAGE;
        const u32x4* xim = xs + img * XS_F4;
        u32x4 A[2][MB], Bv[2];
        auto a_read = [&](auto gtag, int mb) {
            constexpr int gg = decltype(gtag)::value, t0 = grp_t0(gg), kind = grp_kind(gg);
            const int off = ((mb >> 1) + t0 / 3) * HC + t0 % 3 + 16 * (mb & 1);
            A[gg & 1][mb] = xim[(kind == 0 ? a_main : (kind == 1 ? a_p1 : a_p32)) + off];
        };
        auto b_read = [&](auto ptag) {
            constexpr int pp = decltype(ptag)::value, gg = pp / NB, j = pp % NB, t0 = grp_t0(gg), kind = grp_kind(gg);
            const int base = kind == 0 ? b_main : b_p1;
            Bv[pp & 1] = *reinterpret_cast<const u32x4*>(wst + base + (kind == 0 ? 0 : WPLANE) + (j >> 1) * WBLK + t0 * 1024 + (j & 1) * 256);
        };
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) a_read(std::integral_constant<int, 0>{}, mb);
        b_read(std::integral_constant<int, 0>{});
        __builtin_amdgcn_sched_barrier(0);
        constexpr int GM = NB * MB;                                  // MFMAs per group
        static_for<0, NGRP * GM>([&](auto Gc) {
            constexpr int gi = decltype(Gc)::value;
            constexpr int gg = gi / GM, m = gi % GM, j = m / MB, mb = m % MB, pass = gg * NB + j;
            acc[mb][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, Bv[pass & 1]), __builtin_bit_cast(f16x8, A[gg & 1][mb]), acc[mb][j], 0, 0, 0);
            if constexpr (mb == 0 && pass + 1 < NGRP * NB) b_read(std::integral_constant<int, pass + 1>{});
            if constexpr (gg + 1 < NGRP) {
                // the next group's pixel words: NB = 4: one per pass (behind its second MFMA); NB = 2: two per pass
                if constexpr (NB >= MB) { if constexpr (mb == 1 && j < MB) a_read(std::integral_constant<int, gg + 1>{}, j); }
                else { if constexpr (mb == 1 || mb == 2) a_read(std::integral_constant<int, gg + 1>{}, j * 2 + mb - 1); }
            }
            __builtin_amdgcn_sched_barrier(0);
        });
    }
};

template <int BN, int EK>
__global__ void __launch_bounds__(NTHR, 1)
igemm_h2s_kernel(const H2Args ha) {
    using Scheme = std::enable_if_t<BN != 0, H2s>;                       // (a dependent name: the body's `if constexpr (Scheme::...)` then discards)
#include "conv_s_body.h"
}

// ---- split-K reduce: y = act(sum_s slab[s] + bias) in a fixed order (s = 0, 1, ...), one float4 per thread (coalesced), max |y| into the amax slot and -- a
// training forward -- the sign bits OR-ed into the tile-private words of csrc/h2.h (zeroed by the launcher; 8 threads share a word, no two the same bits)
__global__ void __launch_bounds__(256)
h2_splitk_reduce_kernel(const float* __restrict__ slab, int S, const float* __restrict__ bias, float* __restrict__ y, unsigned* __restrict__ bits,
                        unsigned* __restrict__ amax, int B, int H, int W, int N, int act) {
    const int tiles_x = (W + 31) >> 5, tiles_y = (H + TH - 1) / TH, nblk = N >> 5, nq = N >> 2;
    const int64_t img = (int64_t)B * H * W * N, total = img >> 2;     // floats per slab; float4 elements
    const float slope = act == 1 ? 0.2f : (act == 2 ? 0.f : 1.f);
    float am = 0.f;
    for (int64_t e4 = (int64_t)blockIdx.x * 256 + threadIdx.x; e4 < total; e4 += (int64_t)gridDim.x * 256) {
        const f32x4* p = reinterpret_cast<const f32x4*>(slab) + e4;
        const int64_t st4 = img >> 2;
        f32x4 o = p[0];
        int sidx = 1;
        for (; sidx + 3 < S; sidx += 4) {                           // (four independent loads in flight; the ORDER of the additions stays s = 0, 1, 2, ...)
            const f32x4 v0 = p[sidx * st4], v1 = p[(sidx + 1) * st4], v2 = p[(sidx + 2) * st4], v3 = p[(sidx + 3) * st4];
            o += v0; o += v1; o += v2; o += v3;
        }
        for (; sidx < S; ++sidx) o += p[sidx * st4];
        const int cq = (int)(e4 % nq), ch = cq * 4;
        if (bias) o += *reinterpret_cast<const f32x4*>(bias + ch);
#pragma unroll
        for (int c = 0; c < 4; ++c) o[c] = o[c] > 0.f ? o[c] : o[c] * slope;
        reinterpret_cast<f32x4*>(y)[e4] = o;
        am = fmaxf(fmaxf(am, fmaxf(fabsf(o.x), fabsf(o.y))), fmaxf(fabsf(o.z), fabsf(o.w)));
        if (bits) {
            int64_t px = e4 / nq;
            const int xx = (int)(px % W); px /= W;
            const int yy = (int)(px % H); const int b = (int)(px / H);
            const int ty = yy / TH, wv = (yy % TH) >> 1, i = yy & 1, tx = xx >> 5, h = (xx >> 4) & 1, p16 = xx & 15;
            const int cb = ch >> 5, jj = (ch >> 4) & 1, q = (ch >> 2) & 3;
            const int64_t word = ((((int64_t)(b * tiles_y + ty) * tiles_x + tx) * nblk + cb) * NCW + wv) * 64 + q * 16 + p16;
            const unsigned nib = (o.x > 0.f ? 8u : 0u) | (o.y > 0.f ? 4u : 0u) | (o.z > 0.f ? 2u : 0u) | (o.w > 0.f ? 1u : 0u);
            atomicOr(bits + word, nib << (28 - ((i * 2 + h) * 2 + jj) * 4));
        }
    }
    if (amax) pnnp_amax_commit_block(am, amax);
}

template <int BN, int EK>
int launch_h2s(const H2Args& a, hipStream_t s) { return conv_s_launch<H2s, BN, EK, igemm_h2s_kernel<BN, EK>>(a, s); }

}  // namespace

// words of the tile-private sign-bit image of a [B][H][W][C] tensor (csrc/h2.h), C a multiple of 32
extern "C" int64_t pnnp_h2_bits_words(int B, int H, int W, int C) {
    return (int64_t)B * ((H + TH - 1) / TH) * ((W + 31) / 32) * ((C + 31) / 32) * NCW * 64;
}

// tile width of a launch (the rule itself: pnnp_conv3_tile_columns, csrc/igemm.h -- shared with csrc/conv_x3s.hip)
static_assert(TH == 16, "pnnp_conv3_tile_columns counts 16-row tiles");
extern "C" int pnnp_h2_tile_columns(int B, int H, int W, int N, int pool) { return pnnp_conv3_tile_columns(B, H, W, N, pool); }

// split-K policy: how many K slices a [B][H][W] layer with `chunks` 16-channel chunks of K and N channels written should be cut into so that the grid fills
// the chip (1 = no split): the smallest divisor of `chunks` that brings 32-column tiles x slices to 3/4 of the CUs, at least 2 chunks per slice
extern "C" int pnnp_h2_splitk(int B, int H, int W, int chunks, int N) {
    int cus = pnnp_device_cus();
    if (cus < 1) cus = 256;
    const int64_t tiles32 = (int64_t)((W + 31) / 32) * ((H + TH - 1) / TH) * B * ((N + 31) / 32);
    if (tiles32 * 4 >= (int64_t)cus * 3 || chunks < 4) return 1;
    int best = 1;
    for (int sp = 2; sp * 2 <= chunks; ++sp) {
        if (chunks % sp) continue;
        best = sp;
        if (tiles32 * sp * 4 >= (int64_t)cus * 3) break;
    }
    return best;
}
int pnnp_h2_splitk_reduce_launch(const float* slab, int S, const float* bias, float* y, unsigned* bits, unsigned* amax, int B, int H, int W, int N, int act, hipStream_t st) {
    const int64_t total = (int64_t)B * H * W * N / 4;
    if (total <= 0) return PNNP_OK;
    if (bits && hipMemsetAsync(bits, 0, (size_t)pnnp_h2_bits_words(B, H, W, N) * 4, st) != hipSuccess) return PNNP_E_LAUNCH;
    const int64_t blocks = (total + 255) / 256;
    // (at most one block per CU: every block ends with ONE atomicMax on the amax slot, and blocks that finish together serialise on it -- ~15 ns each)
    hipLaunchKernelGGL(h2_splitk_reduce_kernel, dim3((unsigned)(blocks > 256 ? 256 : blocks)), dim3(256), 0, st, slab, S, bias, y, bits, amax, B, H, W, N, act);
    return pnnp_launch_status();
}

// Validation shared with pnnp_igemm_x3_launch (csrc/conv_s.h); a.g.w: the h2 pack of csrc/pack_jobs.hip (kind 4).  Below it: which epilogue a launch takes.
int pnnp_igemm_h2s_launch(const H2Args& ha, int chan_per_seg, hipStream_t s) {
    const IgemmArgs& a = ha.g;
    H2Args b = ha;
    if (!ha.amax_in[0] || !ha.amax_w || (a.nseg > 1 && !ha.amax_in[1])) return PNNP_E_INVALID;
    if (const int rc = conv_s_validate(a, chan_per_seg, H2s::ITEMS * H2s::WBLK, b.g); rc != PNNP_OK) return rc;
    if (b.ksplit < 1) b.ksplit = 1;
    if (b.ksplit > 1) {
        // split-K: raw partial sums into a slab tensor of ksplit x B images -- nothing but the sums themselves (the reduce kernel adds bias, activation, amax)
        if ((b.g.nseg * b.g.chunks_per_seg) % b.ksplit || a.dst[1] || a.bias || a.act || a.mask_mode[0] || a.accum[0] || a.addsrc || a.pool_dst || a.pool_codes ||
            ha.bits_out || ha.bits_in[0] || ha.bits_in[1] || ha.head_out || ha.amax_out[0]) return PNNP_E_UNSUPPORTED;
        if ((int64_t)a.OH * a.OW * a.dst_cs[0] * 4 >= (1ll << 31)) return PNNP_E_UNSUPPORTED;
        return pnnp_h2_tile_columns(a.B * b.ksplit, a.DH, a.DW, a.Ntot, 0) == 64 ? launch_h2s<64, EK_GEN>(b, s) : launch_h2s<32, EK_GEN>(b, s);
    }
    const bool two = a.dst[1] != nullptr;
    for (int d = 0; d < 2; ++d) {                                  // the bit images must fit a buffer resource
        const unsigned* p = d ? ha.bits_in[1] : (ha.bits_in[0] ? ha.bits_in[0] : ha.bits_out);
        if (p && (ha.bits_nblk[d] <= 0 || pnnp_h2_bits_words(a.B, a.DH, a.DW, 32 * ha.bits_nblk[d]) * 4 >= (1ll << 31))) return PNNP_E_UNSUPPORTED;
    }
    if (ha.head_out) {
        // forward + 1x1 head (EK_HEAD): one 32-column block holds every channel of a pixel; plain single-destination forward layers only
        if (!ha.head_w || a.Ntot != 32 || two || a.mask_mode[0] || a.accum[0] || a.addsrc || a.pool_dst || a.pool_codes || ha.bits_in[0] || ha.bits_in[1] ||
            a.OH != a.DH || a.OW != a.DW || (((uintptr_t)ha.head_w | (uintptr_t)ha.head_out | (uintptr_t)ha.head_res | (uintptr_t)ha.head_b) & 3))
            return PNNP_E_UNSUPPORTED;
        if (!a.dst[0] && (ha.bits_out || ha.amax_out[0])) return PNNP_E_INVALID;     // (nothing stored: nothing to describe)
        return launch_h2s<32, EK_HEAD>(b, s);
    }
    if (!a.dst[0]) return PNNP_E_INVALID;
    if (ha.unpool_g || ha.unpool_codes) {
        // bit-masked backward-data + the un-pooled gradient of the destination's pooled map (EK_BWDU): one destination, mask bits, nothing else; even sizes
        if (conv_s_validate_pool(a, ha.unpool_g, ha.unpool_codes) != PNNP_OK || !a.mask_mode[0] || !ha.bits_in[0] || a.bias || a.act || a.pool_dst || a.pool_codes || ha.bits_out)
            return PNNP_E_UNSUPPORTED;
        return pnnp_h2_tile_columns(a.B, a.DH, a.DW, a.Ntot, 0) == 64 ? launch_h2s<64, EK_BWDU>(b, s) : launch_h2s<32, EK_BWDU>(b, s);
    }
    if (a.pool_dst || a.pool_codes) {
        // fused MaxPool2d(2): plain forward layers only (one destination, no mask / residual / accumulate), even sizes
        if (conv_s_validate_pool(a, a.pool_dst, a.pool_codes) != PNNP_OK || a.mask_mode[0] || ha.bits_in[0] || ha.bits_in[1]) return PNNP_E_UNSUPPORTED;
        return pnnp_h2_tile_columns(a.B, a.DH, a.DW, a.Ntot, 1) == 64 ? launch_h2s<64, EK_POOL>(b, s) : launch_h2s<32, EK_POOL>(b, s);
    }
    const bool wide = pnnp_h2_tile_columns(a.B, a.DH, a.DW, a.Ntot, 0) == 64;
    const bool plain = !a.addsrc && !a.accum[0] && !(two && a.accum[1]);
    const bool m0 = a.mask_mode[0] != 0, m1 = two && a.mask_mode[1] != 0;
    const bool f0 = m0 && !ha.bits_in[0], f1 = m1 && !ha.bits_in[1];           // float32 masks
    const bool b0 = m0 && ha.bits_in[0], b1 = m1 && ha.bits_in[1];             // bit masks
    if ((f0 || f1) && (b0 || b1)) return PNNP_E_UNSUPPORTED;                   // one kind per launch
    if ((b0 || b1) && (!plain || a.act || a.bias)) return PNNP_E_UNSUPPORTED;  // bit masks: the masked backward-data epilogue only
    if (ha.bits_out && (m0 || m1 || !plain || two)) return PNNP_E_UNSUPPORTED; // sign bits: plain single-destination forward layers
    if (a.addsrc && !two && !a.accum[0] && !a.act && !m0 && !ha.bits_out) return wide ? launch_h2s<64, EK_RES>(b, s) : launch_h2s<32, EK_RES>(b, s);
    // an unmasked backward-data column range (H2Args::dgrad_plain) runs the EK_BWDB epilogue, not EK_FWD (profiles/r7/ab_unpool_fused.txt)
    if (ha.dgrad_plain && plain && !two && !m0 && !a.bias && !a.act && !ha.bits_out && !ha.bits_in[0])
        return wide ? launch_h2s<64, EK_BWDB>(b, s) : launch_h2s<32, EK_BWDB>(b, s);
    if (plain && !m0 && !m1) return wide ? launch_h2s<64, EK_FWD>(b, s) : launch_h2s<32, EK_FWD>(b, s);
    if (plain && !a.act && !a.bias) {
        if (b0 || b1) return wide ? launch_h2s<64, EK_BWDB>(b, s) : launch_h2s<32, EK_BWDB>(b, s);
        return wide ? launch_h2s<64, EK_BWD>(b, s) : launch_h2s<32, EK_BWD>(b, s);
    }
    return wide ? launch_h2s<64, EK_GEN>(b, s) : launch_h2s<32, EK_GEN>(b, s);
}

// 3x3 convolution, EVAL FORWARD ONLY, on the fp16 matrix cores with ONE scaled fp16 piece per float32 operand ("h1", fp16x1): the kernel text of
// csrc/conv_s_body.h on a third scheme.  An operand a becomes hi = f16(a 2^se) (the `hi` of csrc/h2.h: round to nearest even, subnormals kept; se from the
// tensor's amax slot exactly as in the fp16x2 family), a product is ONE fp16 x fp16 product, exact in the float32 accumulator: one rounding per operand
// (relative 2^-11 each), float32 accumulation.  Opt-in (ConvPolicy.h1_eval); training and the default eval forward stay on csrc/conv_h2s.hip.
//
//   per 16-channel chunk and (16 px x 16 ch) block the nine taps are FIVE v_mfma_f32_16x16x32_f16: two taps share an instruction, pixels
//   [hi @ t | hi @ t + 1] against weights [hi' @ t | hi' @ t + 1] -- the "kind 1 / 2" groups of csrc/conv_h2s.hip with hi' in place of lo'.  The second
//   tap's halo offset is + 1 pixel (taps 2 -> 3: + 32); tap 8 pairs with a tenth tap of ZEROS in the pack, and its pixel half reads tap 8's OWN pixel
//   again (finite x 0 wherever tap 8 itself is finite: no pixel outside the 3x3 window and no padding word of the image is ever read, so a NaN or inf
//   input reaches exactly the 3x3 outputs around it and Scheme::ZERO_PAD stays off).  csrc/conv_h2s.hip issues fourteen.
//
// Halo image 1 piece x 2 octets x 624 px x 16 B = 20 KB, weights 10 KB per 32-channel block and chunk; work item = a whole chunk, two weight stages, two
// producer register sets (as fp16x2).  The epilogues are the forward ones of the body: EK_FWD, EK_POOL, EK_HEAD, EK_RES and EK_GEN for split-K partial
// sums (reduced by h2_splitk_reduce_kernel); no sign bits, no masks, no accumulation -- the launcher refuses the rest.
#include "conv_s.h"

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

namespace {

struct H1s {
    // halo image: 1 piece x 2 octets x 624 px x 16 B = 20 KB; the 12 padding words of a plane are never read (mfma_item: the last group)
    static constexpr int PIECES = 1;
    static constexpr bool ZERO_PAD = false;
    static __device__ __forceinline__ void split(float a0, float a1, float s, unsigned (&p)[1]) { p[0] = h2_hi(a0, a1, s); }
    // weights of one 32-channel block of one chunk: hi' [tap 10][octet 2][32][16 B], the tenth tap ZERO = 10240 bytes (10 pieces)
    static constexpr int WBLK = 10 * 1024;
    static constexpr int ITEMS = 1, SLOTS = NSLOT;
    static constexpr int nstage(int) { return 2; }
    static constexpr int ahead(int) { return 1; }
    static constexpr int NSETS = 2;
    // (BITS false: an eval forward stores no sign bits -- the activation is max(o, slope o), nothing is shifted or written)
    static constexpr bool SCALED = true, BITS = false;
    static constexpr bool has(int EK, int BN) { return EK == EK_FWD || EK == EK_POOL || EK == EK_RES || EK == EK_GEN || (EK == EK_HEAD && BN == 32); }
    static __device__ __forceinline__ void scale_exps(const H2Args& ha, int& se_x, int& se_w) {
        unsigned ax = ha.amax_in[0] ? ha.amax_in[0][0] : 0u;
        if (ha.amax_in[1]) { const unsigned a2 = ha.amax_in[1][0]; ax = a2 > ax ? a2 : ax; }
        se_x = __builtin_amdgcn_readfirstlane(pnnp_h2_scale_exp(ax));
        se_w = __builtin_amdgcn_readfirstlane(ha.amax_w ? pnnp_h2_scale_exp(ha.amax_w[0]) : 0);
    }
    // MFMAs of one chunk (halo image img, weight stage st): group g = taps (2 g, 2 g + 1), per group pass j (16 output channels) x pixel block mb.
    // The pixel words of the NEXT group and the weight word of the NEXT pass are read between the MFMAs into the other register set: MB + NB
    // ds_read_b128 per NB MB MFMAs, the ratio of csrc/conv_h2s.hip.
    static constexpr int NGRP = 5;
    template <int BN>
    static __device__ __forceinline__ void mfma_item(f32x4 (&acc)[2 * MT][BN / 16], const u32x4* xs, const char* wsb, int wave, int lane, int, int st, int img) {
        constexpr int MB = 2 * MT, NB = BN / 16, WS_STAGE = (BN / 32) * WBLK, XS_F4 = PIECES * 2 * NPIXP;
        // lane bases from an OPAQUE copy of the lane number per chunk (csrc/conv_h2s.hip: registers that would otherwise live across the epilogue);
        // k-block q16 of an instruction = (octet q16 & 1, K half q16 >> 1 = the pair's first / second tap)
        int lane_m = lane;
        asm volatile("" : "+v"(lane_m));
        const int r16 = lane_m & 15, q16 = lane_m >> 4, oct16 = q16 & 1, ps16 = q16 >> 1;
        const int a_hi = XS_PLANE(0, oct16) + wave * MT * HC + r16;
        // the second tap is one pixel (taps 2 -> 3: 32 pixels) on; the zero tap behind tap 8 reads tap 8's pixel again
        const int a_p1 = a_hi + ps16, a_p32 = a_hi + 32 * ps16;
        const int b_p1 = (oct16 * 32 + r16) * 16 + ps16 * 1024;
        const char* wst = wsb + st * WS_STAGE;
        const u32x4* xim = xs + img * XS_F4;
        u32x4 A[2][MB], Bv[2];
        auto a_read = [&](auto gtag, int mb) {
            constexpr int gg = decltype(gtag)::value, t0 = 2 * gg;
            const int off = ((mb >> 1) + t0 / 3) * HC + t0 % 3 + 16 * (mb & 1);
            A[gg & 1][mb] = xim[(t0 == 8 ? a_hi : (t0 == 2 ? a_p32 : a_p1)) + off];
        };
        auto b_read = [&](auto ptag) {
            constexpr int pp = decltype(ptag)::value, gg = pp / NB, j = pp % NB, t0 = 2 * gg;
            Bv[pp & 1] = *reinterpret_cast<const u32x4*>(wst + b_p1 + (j >> 1) * WBLK + t0 * 1024 + (j & 1) * 256);
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
igemm_h1s_kernel(const H2Args ha) {
    using Scheme = std::enable_if_t<BN != 0, H1s>;                       // (a dependent name: the body's `if constexpr (Scheme::...)` then discards)
#include "conv_s_body.h"
}

template <int BN, int EK>
int launch_h1s(const H2Args& a, hipStream_t s) { return conv_s_launch<H1s, BN, EK, igemm_h1s_kernel<BN, EK>>(a, s); }

// ---- the same scheme with fp16 ACTIVATIONS on one or both sides ("h1a": csrc/conv_s.h SElem, csrc/conv_s_body.h SRC16 / DST16).  An fp16 source is unscaled
// (se_x = 0: its halves are the halo image's words, dexp = -se_w) and has no amax slot; an fp16 destination is float16(y) of the float32 value H1s stores, and
// its amax slot still records max |y| BEFORE the rounding.  Same pack (kind 7), same mfma_item: fed x16 and x16.float() the two schemes add the same products
// times the same power of two in the same order.  Split-K slabs (EK_GEN) stay float32; the residual epilogue (EK_RES) exists with fp16 on all three sides only.
template <bool S16, bool D16>
struct H1a : H1s {
    static constexpr bool SRC16 = S16, DST16 = D16;
    static constexpr bool has(int EK, int BN) { return D16 ? (EK == EK_FWD || EK == EK_POOL || (S16 && EK == EK_RES)) : (EK == EK_FWD || EK == EK_GEN || (EK == EK_HEAD && BN == 32)); }
    static __device__ __forceinline__ void scale_exps(const H2Args& ha, int& se_x, int& se_w) {
        if constexpr (S16) { se_x = 0; se_w = __builtin_amdgcn_readfirstlane(ha.amax_w ? pnnp_h2_scale_exp(ha.amax_w[0]) : 0); }
        else H1s::scale_exps(ha, se_x, se_w);
    }
};

template <int BN, int EK, bool S16, bool D16>
__global__ void __launch_bounds__(NTHR, 1)
igemm_h1a_kernel(const H2Args ha) {
    using Scheme = std::enable_if_t<BN != 0, H1a<S16, D16>>;
#include "conv_s_body.h"
}

template <int BN, int EK, bool S16, bool D16>
int launch_h1a(const H2Args& a, hipStream_t s) { return conv_s_launch<H1a<S16, D16>, BN, EK, igemm_h1a_kernel<BN, EK, S16, D16>>(a, s); }

// h2_splitk_reduce_kernel (csrc/conv_h2s.hip) with an fp16 destination: the same float32 sums in the same order, bias, activation, max |.| of the float32
// value, then one rounding; 4 channels = 8 bytes per thread.  No sign bits (an eval forward).
__global__ void __launch_bounds__(256)
h1_splitk_reduce_f16_kernel(const float* __restrict__ slab, int S, const float* __restrict__ bias, _Float16* __restrict__ y, unsigned* __restrict__ amax, int64_t img, int N, int act) {
    typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
    const int nq = N >> 2;
    const int64_t total = img >> 2, st4 = img >> 2;
    const float slope = act == 1 ? 0.2f : (act == 2 ? 0.f : 1.f);
    float am = 0.f;
    for (int64_t e4 = (int64_t)blockIdx.x * 256 + threadIdx.x; e4 < total; e4 += (int64_t)gridDim.x * 256) {
        const f32x4* p = reinterpret_cast<const f32x4*>(slab) + e4;
        f32x4 o = p[0];
        int sidx = 1;
        for (; sidx + 3 < S; sidx += 4) {
            const f32x4 v0 = p[sidx * st4], v1 = p[(sidx + 1) * st4], v2 = p[(sidx + 2) * st4], v3 = p[(sidx + 3) * st4];
            o += v0; o += v1; o += v2; o += v3;
        }
        for (; sidx < S; ++sidx) o += p[sidx * st4];
        const int ch = (int)(e4 % nq) * 4;
        if (bias) o += *reinterpret_cast<const f32x4*>(bias + ch);
#pragma unroll
        for (int c = 0; c < 4; ++c) o[c] = o[c] > 0.f ? o[c] : o[c] * slope;
        reinterpret_cast<f16x4*>(y)[e4] = f16x4{(_Float16)o.x, (_Float16)o.y, (_Float16)o.z, (_Float16)o.w};
        am = fmaxf(fmaxf(am, fmaxf(fabsf(o.x), fabsf(o.y))), fmaxf(fabsf(o.z), fabsf(o.w)));
    }
    if (amax) pnnp_amax_commit_block(am, amax);
}

}  // namespace

int pnnp_h1_splitk_reduce_f16_launch(const float* slab, int S, const float* bias, void* y, unsigned* amax, int B, int H, int W, int N, int act, hipStream_t st) {
    const int64_t img = (int64_t)B * H * W * N, total = img / 4;
    if (total <= 0) return PNNP_OK;
    const int64_t blocks = (total + 255) / 256;
    hipLaunchKernelGGL(h1_splitk_reduce_f16_kernel, dim3((unsigned)(blocks > 256 ? 256 : blocks)), dim3(256), 0, st, slab, S, bias, static_cast<_Float16*>(y), amax, img, N, act);
    return pnnp_launch_status();
}

// pnnp_igemm_h1s_launch with element types: src_f16: every K segment is an fp16 NHWC tensor (a.seg[i].ptr points at halves; cstride and coff in multiples of 8,
// no amax slot read); dst_f16: dst[0] and the pooled map are fp16 (channel strides in multiples of 8).  Refuses what pnnp_igemm_h1s_launch refuses, and: a
// residual unless all three sides are fp16, an fp16 split-K slab, a stored map beside the head.  Both zero: pnnp_igemm_h1s_launch itself.
int pnnp_igemm_h1a_launch(const H2Args& ha, int chan_per_seg, int src_f16, int dst_f16, hipStream_t s) {
    if (!src_f16 && !dst_f16) return pnnp_igemm_h1s_launch(ha, chan_per_seg, s);
    const IgemmArgs& a = ha.g;
    H2Args b = ha;
    if (!ha.amax_w || (!src_f16 && (!ha.amax_in[0] || (a.nseg > 1 && !ha.amax_in[1])))) return PNNP_E_INVALID;
    if (src_f16) { b.amax_in[0] = nullptr; b.amax_in[1] = nullptr; }
    if ((((uintptr_t)b.amax_in[0]) | ((uintptr_t)b.amax_in[1]) | ((uintptr_t)ha.amax_w) | ((uintptr_t)ha.amax_out[0]) | ((uintptr_t)ha.amax_out[1])) & 3) return PNNP_E_INVALID;
    if (a.mask[0] || a.mask[1] || a.mask_mode[0] || a.mask_mode[1] || a.accum[0] || a.accum[1] || ha.bits_out || ha.bits_in[0] || ha.bits_in[1] ||
        ha.unpool_g || ha.unpool_codes || ha.dgrad_plain || a.dst[1]) return PNNP_E_UNSUPPORTED;
    // a residual (a.addsrc: an fp16 tensor of dst[0]'s geometry, read through the destination's offsets): fp16 on all three sides, the plain layer, no activation
    if (a.addsrc && (!src_f16 || !dst_f16 || a.act || ha.ksplit > 1 || ha.head_out || a.pool_dst || a.pool_codes)) return PNNP_E_UNSUPPORTED;
    if (const int rc = conv_s_validate(a, chan_per_seg, H1s::ITEMS * H1s::WBLK, b.g, src_f16 ? 2 : 4, dst_f16 ? 2 : 4); rc != PNNP_OK) return rc;
    if (b.ksplit < 1) b.ksplit = 1;
    if (b.ksplit > 1) {
        if (!src_f16 || dst_f16) return PNNP_E_UNSUPPORTED;           // (slabs are float32; a float32 source takes pnnp_igemm_h1s_launch)
        if ((b.g.nseg * b.g.chunks_per_seg) % b.ksplit || a.bias || a.act || a.pool_dst || a.pool_codes || ha.head_out || ha.amax_out[0] || !a.dst[0])
            return PNNP_E_UNSUPPORTED;
        return pnnp_conv3_tile_columns(a.B * b.ksplit, a.DH, a.DW, a.Ntot, 0) == 64 ? launch_h1a<64, EK_GEN, true, false>(b, s) : launch_h1a<32, EK_GEN, true, false>(b, s);
    }
    if (ha.head_out) {
        if (!src_f16 || dst_f16 || a.dst[0] || ha.amax_out[0]) return PNNP_E_UNSUPPORTED;      // (fp16 source, float32 NCHW head_out, nothing else stored)
        if (!ha.head_w || a.Ntot != 32 || a.pool_dst || a.pool_codes || a.OH != a.DH || a.OW != a.DW ||
            (((uintptr_t)ha.head_w | (uintptr_t)ha.head_out | (uintptr_t)ha.head_res | (uintptr_t)ha.head_b) & 3)) return PNNP_E_UNSUPPORTED;
        return launch_h1a<32, EK_HEAD, true, false>(b, s);
    }
    if (!a.dst[0]) return PNNP_E_INVALID;
    if (a.pool_dst || a.pool_codes) {
        if (!src_f16 || !dst_f16) return PNNP_E_UNSUPPORTED;          // (the pooled layers of an fp16-storage forward read and write fp16)
        if (conv_s_validate_pool(a, a.pool_dst, a.pool_codes, 2) != PNNP_OK) return PNNP_E_UNSUPPORTED;
        return pnnp_conv3_tile_columns(a.B, a.DH, a.DW, a.Ntot, 1) == 64 ? launch_h1a<64, EK_POOL, true, true>(b, s) : launch_h1a<32, EK_POOL, true, true>(b, s);
    }
    const bool wide = pnnp_conv3_tile_columns(a.B, a.DH, a.DW, a.Ntot, 0) == 64;
    if (a.addsrc) return wide ? launch_h1a<64, EK_RES, true, true>(b, s) : launch_h1a<32, EK_RES, true, true>(b, s);
    if (src_f16 && dst_f16) return wide ? launch_h1a<64, EK_FWD, true, true>(b, s) : launch_h1a<32, EK_FWD, true, true>(b, s);
    if (src_f16) return wide ? launch_h1a<64, EK_FWD, true, false>(b, s) : launch_h1a<32, EK_FWD, true, false>(b, s);
    return wide ? launch_h1a<64, EK_FWD, false, true>(b, s) : launch_h1a<32, EK_FWD, false, true>(b, s);
}

// pnnp_igemm_h2s_launch restricted to what an eval forward launches.  a.g.w: the one-piece pack of csrc/pack_jobs.hip (kind 7).  Anything with a mask, a bit
// image, an accumulating destination, an un-pool term or the plain backward-data switch: PNNP_E_UNSUPPORTED.
int pnnp_igemm_h1s_launch(const H2Args& ha, int chan_per_seg, hipStream_t s) {
    const IgemmArgs& a = ha.g;
    H2Args b = ha;
    if (!ha.amax_in[0] || !ha.amax_w || (a.nseg > 1 && !ha.amax_in[1])) return PNNP_E_INVALID;
    if ((((uintptr_t)ha.amax_in[0]) | ((uintptr_t)ha.amax_in[1]) | ((uintptr_t)ha.amax_w) | ((uintptr_t)ha.amax_out[0]) | ((uintptr_t)ha.amax_out[1])) & 3) return PNNP_E_INVALID;
    if (a.mask[0] || a.mask[1] || a.mask_mode[0] || a.mask_mode[1] || a.accum[0] || a.accum[1] || ha.bits_out || ha.bits_in[0] || ha.bits_in[1] ||
        ha.unpool_g || ha.unpool_codes || ha.dgrad_plain) return PNNP_E_UNSUPPORTED;
    if (const int rc = conv_s_validate(a, chan_per_seg, H1s::ITEMS * H1s::WBLK, b.g); rc != PNNP_OK) return rc;
    if (b.ksplit < 1) b.ksplit = 1;
    if (b.ksplit > 1) {
        // split-K: raw partial sums into a slab tensor of ksplit x B images (the reduce kernel adds bias, activation, amax)
        if ((b.g.nseg * b.g.chunks_per_seg) % b.ksplit || a.dst[1] || a.bias || a.act || a.addsrc || a.pool_dst || a.pool_codes || ha.head_out || ha.amax_out[0] || !a.dst[0])
            return PNNP_E_UNSUPPORTED;
        if ((int64_t)a.OH * a.OW * a.dst_cs[0] * 4 >= (1ll << 31)) return PNNP_E_UNSUPPORTED;
        return pnnp_conv3_tile_columns(a.B * b.ksplit, a.DH, a.DW, a.Ntot, 0) == 64 ? launch_h1s<64, EK_GEN>(b, s) : launch_h1s<32, EK_GEN>(b, s);
    }
    if (a.dst[1]) return PNNP_E_UNSUPPORTED;                       // (a forward layer has one destination)
    if (ha.head_out) {
        if (!ha.head_w || a.Ntot != 32 || a.addsrc || a.pool_dst || a.pool_codes || a.OH != a.DH || a.OW != a.DW ||
            (((uintptr_t)ha.head_w | (uintptr_t)ha.head_out | (uintptr_t)ha.head_res | (uintptr_t)ha.head_b) & 3)) return PNNP_E_UNSUPPORTED;
        if (!a.dst[0] && ha.amax_out[0]) return PNNP_E_INVALID;       // (nothing stored: nothing to describe)
        return launch_h1s<32, EK_HEAD>(b, s);
    }
    if (!a.dst[0]) return PNNP_E_INVALID;
    if (a.pool_dst || a.pool_codes) {
        if (conv_s_validate_pool(a, a.pool_dst, a.pool_codes) != PNNP_OK) return PNNP_E_UNSUPPORTED;
        return pnnp_conv3_tile_columns(a.B, a.DH, a.DW, a.Ntot, 1) == 64 ? launch_h1s<64, EK_POOL>(b, s) : launch_h1s<32, EK_POOL>(b, s);
    }
    const bool wide = pnnp_conv3_tile_columns(a.B, a.DH, a.DW, a.Ntot, 0) == 64;
    if (a.addsrc) {
        if (a.act) return PNNP_E_UNSUPPORTED;                       // (EK_RES: conv + bias + shortcut, no activation)
        return wide ? launch_h1s<64, EK_RES>(b, s) : launch_h1s<32, EK_RES>(b, s);
    }
    return wide ? launch_h1s<64, EK_FWD>(b, s) : launch_h1s<32, EK_FWD>(b, s);
}

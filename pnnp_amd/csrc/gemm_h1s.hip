// Pointwise convolutions, EVAL FORWARD ONLY, on the fp16 matrix cores with ONE scaled fp16 piece per float32 operand ("h1", fp16x1): the kernel of
// csrc/gemm_s.h on a third scheme, as csrc/conv_h1s.hip is a third scheme on csrc/conv_s_body.h.  ConvTranspose2d(k2, s2), the 1x1 shortcuts and the
// stride-2 3x3 convolution of an eval forward under ConvPolicy.h1_pointwise; training and the default eval forward stay on csrc/gemm_h2s.hip.
//   * an operand a becomes hi = f16(a 2^se) (h2_hi of csrc/h2.h: round to nearest even, subnormals kept; se from the tensor's amax slot exactly as in
//     the fp16x2 family), a product is ONE fp16 x fp16 product, exact in the float32 accumulator: one rounding per operand (relative 2^-11 each);
//   * an ITEM is 32 channels (octets 0 .. 3), ONE v_mfma_f32_16x16x32_f16 per item and 16 x 16 block:
//       pixels [hi h0 | hi h1] x weights [hi' h0 | hi' h1]        (K group q16 of the instruction = octet q16 of the item on both sides)
//     where fp16x2 issues three;
//   * images [piece 1][octet 4][pixel] 16-byte words = 16 KB per 256-pixel image, weights [octet 4][32][8] fp16 = 2048 bytes per item and 32-column block
//     (csrc/pack_jobs.hip kind 8: the hi' plane of the kind-6 pack), scaled with the weight tensor's amax slot; the epilogue multiplies by 2^-(se_x + se_w).
//
// Lookahead and tiles.  LDS_BYTES = 2 XS_BYTES + NSTAGE WS_STAGE = 2 x 16 KB + (A + 1) x (BN / 32) x 2 KB: with A = 3 that is 64 / 48 / 40 KB for the
// 128 / 64 / 32-column tiles, of 160 KB -- LDS would allow A = 15.  What bounds A is the producers' register sets: the activations are float32 in memory
// whatever the scheme, an item is 256 px x 32 ch x 4 B = 32 KB of loads = 32 VGPRs per producer thread and item of lookahead, and a workgroup of 12 waves
// leaves a wave 168 VGPRs: A = 3 is 96 of them (fp16x2's budget: its kernels sit at 168 without scratch), A = 4 would be 128 and spill.
// What A has to cover: an item is a third of fp16x2's matrix time -- 16 MFMAs x 16 cycles per consumer wave on the 128-column tile, two waves per SIMD:
// ~512 cycles = 0.21 us -- while its 32 KB of activations take ~1 us at a CU's share of HBM (8 TB/s / 256 CUs = 31 B/ns).  So every shape here is bound
// by the float32 activations, not by the matrix pipe, and the lookahead is there to keep BYTES in flight, not to hide one latency behind matrix time:
// 3 items = 96 KB per CU in flight (as fp16x2), above latency x bandwidth share (~2 us loaded x 31 B/ns = 62 KB).  More would not move anything sooner.
// For the same reason the WIDEST tile a layer's N allows is taken (256 px x 128, x 64, and x 32 for N = 32 mod 64, as pnnp_gemm_h2s_launch picks them):
// a staged item then feeds the most columns, and the activations are read N / BN times.  The 512-pixel tiles of bf16x3 would double the register sets.
// The 32-column tile's stage is two 1 KB LDS-DMA pieces for four producer waves: waves 2 and 3 repeat piece 1 (same bytes, same place).
#include "h2.h"
#include "gemm_s.h"

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

int pnnp_gemm_h1s_launch(const H2Args& a, hipStream_t s);
int pnnp_gemm_h1a_launch(const H2Args& a, hipStream_t s);

namespace {

struct H1g {
    using Args = H2Args;
    static __host__ __device__ const IgemmArgs& g(const H2Args& h) { return h.g; }
    static constexpr int CH = 32, PIECES = 1, NAF = 1, NPROD = 1;
    // (BITS false: an eval forward reads and writes no sign bits)
    static constexpr bool SCALED = true, BITS = false;
    static constexpr bool gen_lean(int, int) { return true; }        // (as fp16x2: the residual epilogue of the 1x1 shortcut on the register diet)
    static constexpr int nwm(int, int) { return 4; }                 // always 256 pixels
    static constexpr int lookahead(int) { return 3; }
    static __device__ __forceinline__ void scale_exps(const H2Args& ha, int& se_x, int& se_w) {
        unsigned ax = ha.amax_in[0] ? ha.amax_in[0][0] : 0u;
        if (ha.amax_in[1]) { const unsigned a2 = ha.amax_in[1][0]; ax = a2 > ax ? a2 : ax; }
        se_x = __builtin_amdgcn_readfirstlane(pnnp_h2_scale_exp(ax));
        se_w = __builtin_amdgcn_readfirstlane(ha.amax_w ? pnnp_h2_scale_exp(ha.amax_w[0]) : 0);
    }
    static __device__ __forceinline__ void split(float a0, float a1, float sx, unsigned (&p)[1]) { p[0] = h2_hi(a0, a1, sx); }
    // the one operand form on either side: K group q16 = (half q16 >> 1, octet q16 & 1) reads image plane / weight row 2 half + octet = octet q16
    static constexpr int AH[1] = {2}, AC[1] = {0};
    static constexpr int WH[1] = {2}, WC[1] = {0}, WO = 1;
    static constexpr int fa(int) { return 0; }
    static constexpr int fb(int) { return 0; }
    static __device__ __forceinline__ f32x4 mfma(u32x4 b, u32x4 a, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, b), __builtin_bit_cast(f16x8, a), c, 0, 0, 0);
    }
};

// plain (bias, activation) or general (the 1x1 shortcut's residual) epilogue: the only two an eval forward needs
template <int BN, int WN>
int launch_h1g(const H2Args& ha, hipStream_t s) {
    static_assert(H1g::SCALED && !H1g::BITS, "launch_gs_ek's sign-bit dispatch is not taken here");
    return ha.g.addsrc ? launch_gs<H1g, BN, WN, EK_GEN>(ha, s) : launch_gs<H1g, BN, WN, EK_FWD>(ha, s);
}

// ---- the same scheme with fp16 ACTIVATIONS on both sides ("h1a": csrc/gemm_s.h GElem): the source's halves are the operands as they are (se_x = 0, no amax slot
// read), the destination is float16(y) of the float32 value H1g stores, its amax slot still max |y| before the rounding.  Same pack (kind 8), same MFMA order.
struct H1ga : H1g {
    static constexpr bool SRC16 = true, DST16 = true;
    static __device__ __forceinline__ void scale_exps(const H2Args& ha, int& se_x, int& se_w) {
        se_x = 0; se_w = __builtin_amdgcn_readfirstlane(ha.amax_w ? pnnp_h2_scale_exp(ha.amax_w[0]) : 0);
    }
};

}  // namespace

// pnnp_gemm_h1s_launch with fp16 activations on both sides (the up-sampling layers of an fp16-storage eval forward): every K segment an fp16 NHWC tensor
// (cstride and coff in multiples of 8), dst[0] fp16 (channel stride in multiples of 8).  The plain epilogue only: a residual is refused with everything
// pnnp_gemm_h1s_launch refuses.  (The caller's validation, pnnp_gemm_x3_check, counts the 2 GB limit of one image in 2-byte elements for such a launch.)
int pnnp_gemm_h1a_launch(const H2Args& ha, hipStream_t s) {
    const IgemmArgs& b = ha.g;
    if (!ha.amax_w || b.amax_out[1] || !b.dst[0]) return PNNP_E_INVALID;
    if ((((uintptr_t)ha.amax_w) | ((uintptr_t)b.amax_out[0])) & 3) return PNNP_E_INVALID;
    if (b.mask[0] || b.mask[1] || b.mask_mode[0] || b.mask_mode[1] || b.accum[0] || b.accum[1] || b.dst[1] || ha.bits_out || ha.bits_in[0] || ha.bits_in[1] ||
        ha.unpool_g || ha.unpool_codes || ha.dgrad_plain || ha.head_out || ha.ksplit > 1 || b.pool_dst || b.pool_codes || b.addsrc) return PNNP_E_UNSUPPORTED;
    if (b.Ntot % 32 || b.chunks_per_seg <= 0 || (b.dst_cs[0] & 7)) return PNNP_E_UNSUPPORTED;
    for (int i = 0; i < b.nseg; ++i)
        if ((b.seg[i].cstride & 7) || (b.seg[i].coff & 7)) return PNNP_E_UNSUPPORTED;
    H2Args h = ha;
    h.amax_in[0] = nullptr; h.amax_in[1] = nullptr;
    if (b.Ntot % 128 == 0) return launch_gs<H1ga, 128, 64, EK_FWD>(h, s);
    if (b.Ntot % 64 == 0) return launch_gs<H1ga, 64, 32, EK_FWD>(h, s);
    return launch_gs<H1ga, 32, 32, EK_FWD>(h, s);
}

// pnnp_gemm_h2s_launch restricted to what an eval forward launches.  `ha.g`: validated like pnnp_gemm_x3_launch's argument (csrc/gemm_x3.hip), with
// chunks_per_seg = 32-channel items per K segment and Ntot a multiple of 32; weights = the kind-8 pack (csrc/pack_jobs.hip).  Anything with a mask, a bit
// image, an accumulating destination or a second destination -- what only a backward launch sets: PNNP_E_UNSUPPORTED.
int pnnp_gemm_h1s_launch(const H2Args& ha, hipStream_t s) {
    const IgemmArgs& b = ha.g;
    if (!ha.amax_in[0] || !ha.amax_w || b.amax_out[1] || !b.dst[0]) return PNNP_E_INVALID;
    if ((((uintptr_t)ha.amax_in[0]) | ((uintptr_t)ha.amax_in[1]) | ((uintptr_t)ha.amax_w) | ((uintptr_t)b.amax_out[0]) | ((uintptr_t)b.amax_out[1])) & 3) return PNNP_E_INVALID;
    if (b.mask[0] || b.mask[1] || b.mask_mode[0] || b.mask_mode[1] || b.accum[0] || b.accum[1] || b.dst[1] || ha.bits_out || ha.bits_in[0] || ha.bits_in[1] ||
        ha.unpool_g || ha.unpool_codes || ha.dgrad_plain || ha.head_out || ha.ksplit > 1 || b.pool_dst || b.pool_codes) return PNNP_E_UNSUPPORTED;
    if (b.Ntot % 32 || b.chunks_per_seg <= 0) return PNNP_E_UNSUPPORTED;
    if (b.Ntot % 128 == 0) return launch_h1g<128, 64>(ha, s);
    if (b.Ntot % 64 == 0) return launch_h1g<64, 32>(ha, s);
    return launch_h1g<32, 32>(ha, s);
}

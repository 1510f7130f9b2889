// Pointwise convolutions on the fp16 matrix cores (round 5): the kernel of csrc/gemm_s.h on the fp16x2 scheme of csrc/h2.h -- the same GEMMs as
// csrc/gemm_x3s.hip, the kernel of the default train step.  What the scheme is:
//   * an ITEM is 32 channels (two 16-channel halves h0, h1), so that the `hi lo'` products of the two halves share one K = 32 instruction:
//       pixels [hi h0 | lo h0] x weights [hi' h0 | hi' h0]     = hi hi' + lo hi' of h0
//       pixels [hi h1 | lo h1] x weights [hi' h1 | hi' h1]     =   ...           of h1
//       pixels [hi h0 | hi h1] x weights [lo' h0 | lo' h1]     = hi lo' of both
//     3 v_mfma_f32_16x16x32_f16 per 32 channels and 16 x 16 block where bf16x3 needs 6: 3 executed FLOP per algorithmic FLOP instead of 6;
//   * images [piece 2][octet 4][pixel] 16-byte words (activations x 2^se_x, hi / lo by v_fma_mix*_f16), weights [piece 2][octet 4][32][8] fp16 = 4096 bytes
//     per item and 32-column block (csrc/pack_jobs.hip kind 6), scaled with the weight tensor's amax slot; the activations' scale comes from the amax slots
//     of the K segments' tensors; the epilogue multiplies by 2^-(se_x + se_w) first;
//   * an item carries twice the bytes of a bf16x3 item at the same matrix-pipe time, so the lookahead is 3 items (96 KB per CU in flight).
// Tiles: 256 px x 128 columns (4 x 2 consumer waves of 64 px x 64), 256 px x 64 (4 x 2 waves of 64 px x 32) and, for GEMMs with 32 (mod 64) columns, 256 px x 32
// (4 x 1 waves of 64 px x 32; the other four consumer waves only keep the barriers -- these layers move 32 KB per item for 384 matrix-pipe cycles: HBM-bound).
#include "h2.h"
#include "gemm_s.h"

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

int pnnp_gemm_h2s_launch(const H2Args& a, hipStream_t s);

namespace {

struct H2s {
    using Args = H2Args;
    static __host__ __device__ const IgemmArgs& g(const H2Args& h) { return h.g; }
    static constexpr int CH = 32, PIECES = 2, NAF = 3, NPROD = 3;
    static constexpr bool SCALED = true, BITS = true;
    static constexpr bool gen_lean(int, int) { return true; }
    static constexpr int nwm(int, int) { return 4; }                 // always 256 pixels
    static constexpr int lookahead(int) { return 3; }
    // (csrc/h2.h) se_x from the largest amax of the K segments' tensors, se_w from the weight tensor's
    static __device__ __forceinline__ void scale_exps(const H2Args& ha, int& se_x, int& se_w) {
        unsigned ax = ha.amax_in[0] ? ha.amax_in[0][0] : 0u;
        if (ha.amax_in[1]) { const unsigned a2 = ha.amax_in[1][0]; ax = a2 > ax ? a2 : ax; }
        se_x = __builtin_amdgcn_readfirstlane(pnnp_h2_scale_exp(ax));
        se_w = __builtin_amdgcn_readfirstlane(ha.amax_w ? pnnp_h2_scale_exp(ha.amax_w[0]) : 0);
    }
    static __device__ __forceinline__ void split(float a0, float a1, float sx, unsigned (&p)[2]) { split_h2(a0, a1, sx, p[0], p[1]); }
    // operand forms (k-group q16 of an instruction): pixels 0 = [hi h0 | lo h0], 1 = [hi h1 | lo h1], 2 = [hi h0 | hi h1];
    // weights 0 = [hi' h0 | hi' h0], 1 = [hi' h1 | hi' h1], 2 = [lo' h0 | lo' h1]   (h0 / h1 = octets 0,1 / 2,3 of the 32-channel item).  As coefficients (csrc/gemm_s.h):
    // image plane = AH half + AC + octet, weight row = WH half + WC + WO octet, for K group q16 = (half q16 >> 1, octet q16 & 1)
    static constexpr int AH[3] = {4, 4, 2}, AC[3] = {0, 2, 0};      // images [piece 2][octet 4]: (hi, lo) of octets 0,1 / of octets 2,3 / hi of octets (0,1), (2,3)
    static constexpr int WH[3] = {0, 0, 2}, WC[3] = {0, 2, 4}, WO = 1;      // weights [piece 2][octet 4]: hi' of octets 0,1 twice / of 2,3 twice / lo' of octets (0,1), (2,3)
    // hi lo' of both halves first, then the two halves' hi hi' + lo hi'
    static constexpr int fa(int sp) { return 2 - sp; }
    static constexpr int fb(int sp) { return 2 - sp; }
    static __device__ __forceinline__ f32x4 mfma(u32x4 b, u32x4 a, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, b), __builtin_bit_cast(f16x8, a), c, 0, 0, 0);
    }
};

}  // namespace

// `ha.g`: validated like pnnp_gemm_x3_launch's argument (csrc/gemm_x3.hip), with chunks_per_seg = 32-channel items per K segment (every
// segment a multiple of 32 channels) and Ntot a multiple of 32; weights = the kind-6 pack (csrc/pack_jobs.hip), amax slots as in csrc/h2.h.
int pnnp_gemm_h2s_launch(const H2Args& ha, hipStream_t s) {
    const IgemmArgs& b = ha.g;
    if (!ha.amax_in[0] || !ha.amax_w || b.amax_out[1] || ha.bits_out || ha.bits_in[1]) return PNNP_E_INVALID;
    if (b.Ntot % 32 || b.chunks_per_seg <= 0) return PNNP_E_UNSUPPORTED;
    if (b.Ntot % 128 == 0) return launch_gs_ek<H2s, 128, 64>(ha, s);
    if (b.Ntot % 64 == 0) return launch_gs_ek<H2s, 64, 32>(ha, s);
    return launch_gs_ek<H2s, 32, 32>(ha, s);                        // (round 6) 256 px x 32 columns: ResUnet's 32-column layers at 512 x 512 (pool1 backward-data, sc9, upv9 beside them)
}

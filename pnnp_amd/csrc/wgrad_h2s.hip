// Weight gradient of a 3x3 / stride 1 / pad 1 convolution on the fp16 matrix cores: the kernel of csrc/wgrad_s.h on the fp16x2 scheme of csrc/h2.h (round 5;
// the default).  Both operands are activations / gradients split on the fly into TWO scaled fp16 pieces: G with 2^se_g (odd pixel splits: -2^se_g, the
// alternating sign costs nothing), X with 2^se_x from the amax slots of the tensors; THREE v_mfma_f32_32x32x16_f16 per (16-pixel k-step, tap) where
// bf16x3 (csrc/wgrad_x3s.hip) issues six; the slab values are multiplied by 2^-(se_g + se_x) where they leave the accumulators.
#include "h2.h"
#include "wgrad_s.h"

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

namespace {

#ifndef WHS_G_AUX
#define WHS_G_AUX 2                    // cache-policy bits of the producers' G loads: 2 = nt -- G is read exactly once by this kernel (X's halo rows are shared between
#endif                                 // tiles and keep the default): step +0.3 % on two boxes, config 5 equal (profiles/r6/ab_stream_load_policy.txt)
#ifndef WHS_ROLL
#define WHS_ROLL 1                     // producers: rolling refill of the staging registers (csrc/wgrad_s.h roll_tile; 0 = round 5's order)
#endif
struct Wh2s {
    static constexpr int PIECES = 2, MFMAS = 3, G_AUX = WHS_G_AUX;
    static constexpr bool SCALED = true, ROLL = WHS_ROLL;
    // 64 x 64 tiles: one consumer owns both 32-row blocks (WsCfg): -3 ... -6 % per layer; 64 x 32 tiles +6 %: they keep one block per wave
    // (profiles/r5/ab_wgrad_two_blocks_per_wave.txt)
    static constexpr bool MW2 = true;
    // The LDS images are two planes instead of three, so pixel tiles could be taller than bf16x3's.  Measured (profiles/r5/ab_wgrad_tile_heights.txt): 3 / 4 / 6 rows
    // for the 64x64 / 64x32 / 32x32 tiles spill 11-18 registers in the producers and are 8-25 % SLOWER; 32x64 at 3 rows fits: -8 %
    static constexpr int TH22 = 2, TH21 = 3, TH12 = 3, TH11 = 4;
    static constexpr int pa(int G) { return G == 1 ? 1 : 0; }         // smallest terms first: (hi, lo') (lo, hi') (hi, hi')
    static constexpr int pb(int G) { return G == 0 ? 1 : 0; }
    static __device__ __forceinline__ f32x16 mfma(u32x4 a, u32x4 b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    }
    static __device__ __forceinline__ void scale_exps(const WsArgs& a, int& se_g, int& se_x) {
        unsigned axb = a.amax_x[0] ? a.amax_x[0][0] : 0u;
        if (a.amax_x[1]) { const unsigned a2 = a.amax_x[1][0]; axb = a2 > axb ? a2 : axb; }
        se_x = __builtin_amdgcn_readfirstlane(pnnp_h2_scale_exp(axb));
        se_g = __builtin_amdgcn_readfirstlane(a.amax_g ? pnnp_h2_scale_exp(a.amax_g[0]) : 0);
    }
    static __device__ __forceinline__ float unscale(float v, int dexp) { return __builtin_ldexpf(v, dexp); }
    static __device__ __forceinline__ void split(f32x4 v, float sc, unsigned (&p)[2][2]) {
        split_h2(v.x, v.y, sc, p[0][0], p[1][0]);
        split_h2(v.z, v.w, sc, p[0][1], p[1][1]);
    }
};

}  // namespace

int pnnp_wh2s_th(int M, int N) { return ws_th<Wh2s>(M, N); }
int pnnp_wh2s_launch(const WsArgs& a, hipStream_t s) { return ws_launch<Wh2s>(a, s); }

// Weight gradients of the POINTWISE / STRIDED layers on the fp16 matrix cores: the kernel of csrc/wgrad_g.h (geometries, tiles, staging layout, slabs)
// on the fp16x2 scheme of csrc/h2.h (round 5).  Both operands are scaled by a power of two from their tensors' amax slots (U: amax_u; S: the larger of
// amax_s[0..1]) and split into TWO fp16 pieces on the way into LDS; a (tap, 32 x 32 block) is THREE v_mfma_f32_32x32x16_f16 -- (hi, lo') (lo, hi')
// (hi, hi') -- where bf16x3 (csrc/wgrad_x3g.hip) needs six; a staging slice is 5 steps instead of 11; the slab store multiplies by 2^-(se_u + se_s).
// Odd pixel splits still stage -U (alternating-sign slabs), the bias sums use the unscaled values.
#include "h2.h"
#include "wgrad_g.h"

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

namespace {

#ifndef WHG_ROLL
#define WHG_ROLL 1                     // rolling refill of the staging registers (csrc/wgrad_g.h stage_piece; 0 = round 5's order)
#endif
struct H2g {
    static constexpr int PIECES = 2, MFMAS = 3, NSTEP = 5;            // steps: 0 hi, 1 bias sums, 2 lo, 3-4 stores
    static constexpr int REFILL_STEP = 2;
    static constexpr bool SCALED = true, ROLL = WHG_ROLL;
    static constexpr int pa(int G) { return G == 1 ? 1 : 0; }         // smallest terms first: (hi, lo') (lo, hi') (hi, hi')
    static constexpr int pb(int G) { return G == 0 ? 1 : 0; }
    static __device__ __forceinline__ f32x16 mfma(u32x4 a, u32x4 b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    }
    static __device__ __forceinline__ void scale_exps(const WxgArgs& a, int& se_u, int& se_s) {
        unsigned as_ = a.amax_s[0] ? a.amax_s[0][0] : 0u;
        if (a.amax_s[1]) { const unsigned a2 = a.amax_s[1][0]; as_ = a2 > as_ ? a2 : as_; }
        se_u = __builtin_amdgcn_readfirstlane(pnnp_h2_scale_exp(a.amax_u ? a.amax_u[0] : 0u));
        se_s = __builtin_amdgcn_readfirstlane(pnnp_h2_scale_exp(as_));
    }
    static __device__ __forceinline__ float unscale(float v, int dexp) { return __builtin_ldexpf(v, dexp); }
    static __device__ __forceinline__ void split(f32x4 v, float sc, unsigned (&p)[2][2]) {
        p[0][0] = h2_hi(v.x, v.y, sc); p[0][1] = h2_hi(v.z, v.w, sc);
        p[1][0] = h2_lo(v.x, v.y, sc, p[0][0]); p[1][1] = h2_lo(v.z, v.w, sc, p[0][1]);
    }
    static __device__ __forceinline__ void split_step(int step, f32x4& v, float sc, unsigned (&p)[2][2]) {
        if (step == 0) { p[0][0] = h2_hi(v.x, v.y, sc); p[0][1] = h2_hi(v.z, v.w, sc); }
        if (step == 2) { p[1][0] = h2_lo(v.x, v.y, sc, p[0][0]); p[1][1] = h2_lo(v.z, v.w, sc, p[0][1]); }
    }
};

// Configurations (output tile M x N of the workgroup, U pixels per tile): those of csrc/wgrad_x3g.hip and, two pieces per operand leaving the LDS room,
template <int... C> using Tile = WxgLaunch<H2g, C...>;
using CtA = Tile<GEO_CT, 2, 1, 4, 2, 1, 16, 1>;
using CtB = Tile<GEO_CT, 1, 1, 4, 2, 1, 16, 1>;
using CtC = Tile<GEO_CT, 1, 1, 2, 1, 4, 32, 2>;
using S2A = Tile<GEO_S2, 1, 1, 4, 1, 2, 32, 1>;
using S2B = Tile<GEO_S2, 1, 1, 2, 1, 4, 32, 2>;          // 64 x 32 (64 px; M = Cout = 64: pool1 of the ResUnet -- no bf16x3 twin, it ran on fp32 MFMA)
using PwA = Tile<GEO_PW, 2, 2, 2, 2, 2, 32, 1>;
using PwB = Tile<GEO_PW, 1, 2, 2, 2, 2, 32, 1>;
using PwC = Tile<GEO_PW, 1, 1, 1, 2, 4, 32, 2>;          // 32 x 64 (64 px; M = Cout = 32: sc9 of the ResUnet -- round 6: it ran on fp32 MFMA)

int wxg_config(H2g, int geo, int M, int N) {
    if (M <= 0 || N <= 0 || (M & 31) || (N & 31)) return 0;
    if (geo == GEO_CT) return (M % 256 == 0 && N % 64 == 0) ? 1 : ((M % 128 == 0 && N % 64 == 0) ? 2 : ((M % 64 == 0) ? 3 : 0));
    if (geo == GEO_S2) return (M % 128 == 0) ? 4 : ((M % 64 == 0) ? 7 : 0);
    if (geo == GEO_PW) return (N % 128 == 0 && M % 64 == 0) ? ((M % 128 == 0) ? 5 : 6) : ((N % 64 == 0) ? 8 : 0);
    return 0;
}
template <class F> auto wxg_dispatch(H2g, int cfg, F&& f) {
    switch (cfg) {
        case 1: return f(CtA{});
        case 2: return f(CtB{});
        case 3: return f(CtC{});
        case 4: return f(S2A{});
        case 5: return f(PwA{});
        case 7: return f(S2B{});
        case 8: return f(PwC{});
        default: return f(PwB{});
    }
}

}  // namespace

extern "C" {

// Contracts of the _x3_ entries of csrc/wgrad_x3g.hip, plus the amax slots of the two tensors that are split on the fly (csrc/h2.h).  Shapes and
// workspace: pnnp_h2g_wgrad_supported / pnnp_h2g_wgrad_workspace_floats -- everything pnnp_x3g_wgrad_* takes and, in addition, the stride-2
// layer with Cout % 64 == 0 (a 64 x 32 tile) and the 1x1 layer with Cin % 64 == 0 (a 32 x 64 tile).
/* kind: 0 = Conv2d 1x1 (M = Cout, N = Cin), 1 = ConvTranspose2d 2x2 s2 (M = Cin, N = Cout), 2 = Conv2d 3x3 s2 (M = Cout, N = Cin) */
int pnnp_h2g_wgrad_supported(int kind, int M, int N) { return wxg_config(H2g{}, kind, M, N) ? 1 : 0; }
int64_t pnnp_h2g_wgrad_workspace_floats(int kind, int B, int UH, int UW, int M, int N) { return wxg_workspace_floats<H2g>(kind, B, UH, UW, M, N); }
int pnnp_convt2x2_h2_bwd_weight_f32(const float* x, int Cin, const unsigned* amax_x, const float* g, int Cout, const unsigned* amax_g, float* dW, float* dbias,
                                    int B, int H, int W, int accumulate, float* workspace, int64_t workspace_floats, void* stream) {
    if (!x || !g || !dW || !workspace || B <= 0 || H <= 0 || W <= 0) return PNNP_E_INVALID;
    return wxg_run<H2g>(GEO_CT, x, Cin, Cin, amax_x, g, Cout, Cout, amax_g, nullptr, 0, 0, nullptr, B, H, W, 2 * H, 2 * W, dW, dbias, true, accumulate,
                        workspace, workspace_floats, as_stream(stream));
}
int pnnp_conv3x3s2_h2_bwd_weight_f32(const float* g, int Cout, const unsigned* amax_g, const float* x, int Cin, const unsigned* amax_x, float* dW, float* dbias,
                                     int B, int H, int W, int accumulate, float* workspace, int64_t workspace_floats, void* stream) {
    if (!g || !x || !dW || !workspace || B <= 0 || H <= 0 || W <= 0 || (H & 1) || (W & 1)) return PNNP_E_INVALID;
    return wxg_run<H2g>(GEO_S2, g, Cout, Cout, amax_g, x, Cin, Cin, amax_x, nullptr, 0, 0, nullptr, B, H / 2, W / 2, H, W, dW, dbias, false, accumulate,
                        workspace, workspace_floats, as_stream(stream));
}
int pnnp_conv1x1_h2_bwd_weight_f32(const float* g, int g_cs, int Cout, const unsigned* amax_g, const float* x1, int x1_cs, int C1, const unsigned* amax_x1,
                                   const float* x2, int x2_cs, int C2, const unsigned* amax_x2, float* dW, float* dbias,
                                   int B, int H, int W, int accumulate, float* workspace, int64_t workspace_floats, void* stream) {
    if (!g || !x1 || !dW || !workspace || B <= 0 || H <= 0 || W <= 0) return PNNP_E_INVALID;
    return wxg_run<H2g>(GEO_PW, g, g_cs, Cout, amax_g, x1, x1_cs, C1, amax_x1, x2, x2_cs, C2, amax_x2, B, H, W, H, W, dW, dbias, false, accumulate,
                        workspace, workspace_floats, as_stream(stream));
}

}  // extern "C"

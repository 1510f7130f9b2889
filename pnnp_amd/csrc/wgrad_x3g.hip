// Weight gradients of the POINTWISE / STRIDED layers on the bf16 matrix cores: the kernel of csrc/wgrad_g.h (geometries, tiles, staging layout, slabs)
// on the bf16x3 scheme of csrc/conv_x3s.hip and csrc/wgrad_x3.hip (round 4).  Both operands are split into THREE bf16 pieces on the way into LDS, unscaled;
// a (tap, 32 x 32 block) is SIX v_mfma_f32_32x32x16_bf16; a staging slice is 11 steps of 2-4 VALU instructions.
#include "x3.h"
#include "wgrad_g.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

namespace {

struct X3g {
    static constexpr int PIECES = 3, MFMAS = 6, NSTEP = 11;           // steps: 0 hi, 1 bias sums, 2-3 residual, 4 mid, 5-6 residual, 7 lo, 8-10 stores
    // ROLL stays off (the tile after next is requested behind the last MFMA, round 4's order): two instantiations sit at 254 VGPRs as it is
    static constexpr bool SCALED = false, ROLL = false;
    // smallest terms first: (hi,lo) (lo,hi) (mid,mid) (hi,mid) (mid,hi) (hi,hi)
    static constexpr int pa(int G) { return G == 0 ? 0 : (G == 1 ? 2 : (G == 2 ? 1 : (G == 3 ? 0 : (G == 4 ? 1 : 0)))); }
    static constexpr int pb(int G) { return G == 0 ? 2 : (G == 1 ? 0 : (G == 2 ? 1 : (G == 3 ? 1 : (G == 4 ? 0 : 0)))); }
    static __device__ __forceinline__ f32x16 mfma(u32x4 a, u32x4 b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    }
    static __device__ __forceinline__ void scale_exps(const WxgArgs&, int& se_u, int& se_s) { se_u = se_s = 0; }
    static __device__ __forceinline__ float unscale(float v, int) { return v; }
    static __device__ __forceinline__ void split(f32x4 v, float, unsigned (&p)[3][2]) {
        split2(v.x, v.y, p[0][0], p[1][0], p[2][0]);
        split2(v.z, v.w, p[0][1], p[1][1], p[2][1]);
    }
    static __device__ __forceinline__ void split_step(int step, f32x4& v, float, unsigned (&p)[3][2]) {
        if (step == 0 || step == 4 || step == 7) { const int i = step == 0 ? 0 : (step == 4 ? 1 : 2); p[i][0] = cvt_pk_bf16(v.x, v.y); p[i][1] = cvt_pk_bf16(v.z, v.w); }
        if (step == 2 || step == 5) { const unsigned h = p[step == 2 ? 0 : 1][0]; v.x -= __uint_as_float(h << 16); v.y -= __uint_as_float(h & 0xffff0000u); }
        if (step == 3 || step == 6) { const unsigned h = p[step == 3 ? 0 : 1][1]; v.z -= __uint_as_float(h << 16); v.w -= __uint_as_float(h & 0xffff0000u); }
    }
};

// Configurations (output tile M x N of the workgroup, U pixels per tile):
//   ConvTranspose2d  A 256 x 64 (16 px): two M blocks per wave against one staged S block   B 128 x 64 (16 px)   C 64 x 32 (64 px)
//   3x3 stride 2     128 x 32 (32 px; M = Cout in multiples of 128: pool2 .. pool4 of the ResUnet)
//   1x1              128 x 128 (32 px; two M and two N blocks per wave)   64 x 128 (32 px)
template <int... C> using Tile = WxgLaunch<X3g, C...>;
using CtA = Tile<GEO_CT, 2, 1, 4, 2, 1, 16, 1>;
using CtB = Tile<GEO_CT, 1, 1, 4, 2, 1, 16, 1>;
using CtC = Tile<GEO_CT, 1, 1, 2, 1, 4, 32, 2>;
using S2A = Tile<GEO_S2, 1, 1, 4, 1, 2, 32, 1>;
using PwA = Tile<GEO_PW, 2, 2, 2, 2, 2, 32, 1>;
using PwB = Tile<GEO_PW, 1, 2, 2, 2, 2, 32, 1>;

int wxg_config(X3g, int geo, int M, int N) {
    if (M <= 0 || N <= 0 || (M & 31) || (N & 31)) return 0;
    if (geo == GEO_CT) return (M % 256 == 0 && N % 64 == 0) ? 1 : ((M % 128 == 0 && N % 64 == 0) ? 2 : ((M % 64 == 0) ? 3 : 0));
    if (geo == GEO_S2) return (M % 128 == 0) ? 4 : 0;
    if (geo == GEO_PW) return (N % 128 == 0) ? ((M % 128 == 0) ? 5 : ((M % 64 == 0) ? 6 : 0)) : 0;
    return 0;
}
template <class F> auto wxg_dispatch(X3g, int cfg, F&& f) {
    switch (cfg) {
        case 1: return f(CtA{});
        case 2: return f(CtB{});
        case 3: return f(CtC{});
        case 4: return f(S2A{});
        case 5: return f(PwA{});
        default: return f(PwB{});
    }
}

}  // namespace

extern "C" {

/* kind: 0 = Conv2d 1x1 (M = Cout, N = Cin), 1 = ConvTranspose2d 2x2 s2 (M = Cin, N = Cout), 2 = Conv2d 3x3 s2 (M = Cout, N = Cin) */
int pnnp_x3g_wgrad_supported(int kind, int M, int N) { return wxg_config(X3g{}, kind, M, N) ? 1 : 0; }

/* workspace (floats) for the U-resolution map B x UH x UW (the LOW-resolution side of the strided layers) */
int64_t pnnp_x3g_wgrad_workspace_floats(int kind, int B, int UH, int UW, int M, int N) { return wxg_workspace_floats<X3g>(kind, B, UH, UW, M, N); }

// dW [Cin][Cout][2][2] (+ dbias [Cout] = channel sums of g) of ConvTranspose2d(Cin, Cout, 2, stride 2): same contract as pnnp_convt2x2_bwd_weight_f32
int pnnp_convt2x2_x3_bwd_weight_f32(const float* x, int Cin, const float* g, int Cout, float* dW, float* dbias,
                                    int B, int H, int W, int accumulate, float* workspace, int64_t workspace_floats, void* stream) {
    if (!x || !g || !dW || !workspace || B <= 0 || H <= 0 || W <= 0) return PNNP_E_INVALID;
    return wxg_run<X3g>(GEO_CT, x, Cin, Cin, nullptr, g, Cout, Cout, nullptr, nullptr, 0, 0, nullptr, B, H, W, 2 * H, 2 * W, dW, dbias, true, accumulate,
                        workspace, workspace_floats, as_stream(stream));
}

// dW [Cout][Cin][3][3] (+ dbias [Cout]) of Conv2d 3x3 stride 2 pad 1: g [B][H/2][W/2][Cout], x [B][H][W][Cin]; same contract as
// pnnp_conv3x3s2_bwd_weight_f32
int pnnp_conv3x3s2_x3_bwd_weight_f32(const float* g, int Cout, const float* x, int Cin, float* dW, float* dbias,
                                     int B, int H, int W, int accumulate, float* workspace, int64_t workspace_floats, void* stream) {
    if (!g || !x || !dW || !workspace || B <= 0 || H <= 0 || W <= 0 || (H & 1) || (W & 1)) return PNNP_E_INVALID;
    return wxg_run<X3g>(GEO_S2, g, Cout, Cout, nullptr, x, Cin, Cin, nullptr, nullptr, 0, 0, nullptr, B, H / 2, W / 2, H, W, dW, dbias, false, accumulate,
                        workspace, workspace_floats, as_stream(stream));
}

// dW [Cout][C1 + C2] (+ dbias [Cout]) of Conv2d 1x1: same contract as pnnp_conv_bwd_weight_f32 with taps = 1
int pnnp_conv1x1_x3_bwd_weight_f32(const float* g, int g_cs, int Cout, const float* x1, int x1_cs, int C1,
                                   const float* x2, int x2_cs, int C2, float* dW, float* dbias,
                                   int B, int H, int W, int accumulate, float* workspace, int64_t workspace_floats, void* stream) {
    if (!g || !x1 || !dW || !workspace || B <= 0 || H <= 0 || W <= 0) return PNNP_E_INVALID;
    return wxg_run<X3g>(GEO_PW, g, g_cs, Cout, nullptr, x1, x1_cs, C1, nullptr, x2, x2_cs, C2, nullptr, B, H, W, H, W, dW, dbias, false, accumulate,
                        workspace, workspace_floats, as_stream(stream));
}

}  // extern "C"

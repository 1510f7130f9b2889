// Weight gradient of a 3x3 / stride 1 / pad 1 convolution on the matrix cores: the host side -- shape rules, pixel splits, workspace, the
// slab reduce -- shared by the two kernels that compute it: csrc/wgrad_x3s.hip (bf16x3: float32 operands split exactly into three bf16 pieces)
// and csrc/wgrad_h2s.hip (fp16x2: scaled per tensor and split in two; the default).
//
//   dW[m][n][t] = sum over pixels p of  G[p][m] * X[p + tap(t)][n]        (archs/Unet.py:16-50 via autograd;
//   G = dL/d(pre-activation output) [B][H][W][M = Cout], X = the layer's input [B][H][W][N = Cin], possibly the
//   un-materialised cat of two tensors), plus the bias gradient dbias[m] = sum_p G[p][m].
//
// GEMM view: M = Cout, N = Cin, K = pixels, split over Z workgroups per output tile; partial results go to per-workgroup slabs that
// wx3_reduce_kernel sums in a fixed order with alternating signs (deterministic, no float atomics; odd splits accumulate -G X so that the matrix
// core's round-toward-minus-infinity accumulation cancels: DESIGN Appendix A.1b).  Round 2-3's kernel (8 waves, each a 32 x 32 x 9-tap
// accumulator block and its own share of the staging) lived in this file until round 5 (git history: wgrad_x3_kernel).
#include "wgrad_s.h"

namespace {

// out[o(i)] (+)= sum_z (-1)^z slab[z][i] (odd splits accumulated -G * X: WX3_ALT_SIGN); i = (t * M + m) * N + n  ->  o = (m * N + n) * taps + t
// (the parameter's own layout).  ONE launch reduces the weight slabs and, behind them (i >= n), the bias slabs [Z][nb] into bias_out.
__global__ void __launch_bounds__(256)
wx3_reduce_kernel(const float* __restrict__ slab, float* __restrict__ out, int64_t n, int Z, int accumulate, int64_t mn, int taps,
                  const float* __restrict__ bias_slab, float* __restrict__ bias_out, int nb) {
    __shared__ float red[8][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const float sg = (WX3_ALT_SIGN && (ty & 1)) ? -1.f : 1.f;      // a thread row sums splits ty, ty + 8, ...: one parity, one sign (odd splits hold -partial)
    const int64_t ntot = n + (bias_slab ? nb : 0);
    for (int64_t i0 = (int64_t)blockIdx.x * 32; i0 < ntot; i0 += (int64_t)gridDim.x * 32) {
        const int64_t i = i0 + tx;
        const bool isb = i >= n;                                    // (n is a multiple of 32: a 32-wide group never straddles the two parts)
        const float* src = isb ? bias_slab + (i - n) : slab + i;
        const int64_t zs = isb ? nb : n;
        // (eight independent loads in flight per thread: with two, a layer with few weights and many slabs -- conv1_2: 9216 x 256 --
        //  was one memory latency per pair, 11 us for 9 MB)
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        if (i < ntot) {
            int zz = ty;
            for (; zz + 56 < Z; zz += 64) {
                const float v0 = src[(int64_t)zz * zs], v1 = src[(int64_t)(zz + 8) * zs], v2 = src[(int64_t)(zz + 16) * zs], v3 = src[(int64_t)(zz + 24) * zs];
                const float v4 = src[(int64_t)(zz + 32) * zs], v5 = src[(int64_t)(zz + 40) * zs], v6 = src[(int64_t)(zz + 48) * zs], v7 = src[(int64_t)(zz + 56) * zs];
                s0 += v0; s1 += v1; s2 += v2; s3 += v3; s0 += v4; s1 += v5; s2 += v6; s3 += v7;
            }
            for (; zz + 8 < Z; zz += 16) { s0 += src[(int64_t)zz * zs]; s1 += src[(int64_t)(zz + 8) * zs]; }
            for (; zz < Z; zz += 8) s0 += src[(int64_t)zz * zs];
        }
        red[ty][tx] = sg * ((s0 + s1) + (s2 + s3));
        __syncthreads();
        if (ty == 0 && i < ntot) {
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < 8; ++k) s += red[k][tx];
            float* o = isb ? bias_out + (i - n) : out + (taps == 1 ? i : (i % mn) * taps + i / mn);
            *o = accumulate ? *o + s : s;
        }
        __syncthreads();
    }
}

// pixel splits of a layer: output tiles 64 x 64 / 64 x 32 / 32 x 64 / 32 x 32 (what the channel counts allow), `share` workgroups per CU.
// share = pnnp_get_persistent_split() (1 by default): with n > 1 every workgroup carries 1 / n of a CU's pixels and the hardware dispatcher hands
// the surplus workgroups to whichever CU frees up first -- what keeps a weight gradient from doubling its time beside a resident collective
// (round 5: VERDICT round 4, item 6a; the forward / backward-data grids do the same, csrc/capi.hip).  The slabs are still summed by INDEX in a
// fixed order, so the result is deterministic for a given share; another share is another partition of the pixel sum (it differs by rounding).
int wx3_splits(int B, int H, int W, int M, int N, int th, int share) {
    const int bm = M % 64 == 0 ? 64 : 32, bn = N % 64 == 0 ? 64 : 32;
    const int tiles = ((W + 31) / 32) * ((H + th - 1) / th) * B;      // at most one split per pixel tile (th rows x 32 px) of the kernel that runs
    const int out_tiles = (M / bm) * (N / bn);
    int cus = pnnp_device_cus();
    if (cus <= 0) cus = 256;
    if (share < 1) share = 1;
    int z = (cus * share + out_tiles - 1) / out_tiles;
    if (z > tiles) z = tiles;
    return z < 1 ? 1 : z;
}

}  // namespace

// slabs [Z][taps][M][N] (+ bias slabs [Z][nb] behind them) -> dW in the parameter's layout [M][N][taps] (+ dbias), alternating signs over z
// (also used by csrc/wgrad_g.h)
int pnnp_wx3_reduce_launch(const float* slab, float* dW, int64_t mn, int taps, int Z, int accumulate,
                           const float* bias_slab, float* dbias, int nb, hipStream_t st) {
    const int64_t n = mn * taps, ntot = n + (bias_slab ? nb : 0);       // n % 32 == 0 (channels in multiples of 32)
    hipLaunchKernelGGL(wx3_reduce_kernel, dim3((unsigned)((ntot + 31) / 32 > 4096 ? 4096 : (ntot + 31) / 32)), dim3(256), 0, st,
                       slab, dW, n, Z, accumulate, mn, taps, bias_slab, dbias, nb);
    return pnnp_launch_status();
}

extern "C" {

int pnnp_x3_wgrad_supported(int H, int W, int Cout, int C1, int C2) {
    return (H > 0 && W > 0 && Cout > 0 && C1 > 0 && Cout % 32 == 0 && C1 % 32 == 0 && C2 % 32 == 0) ? 1 : 0;
}

// the backward-weight kernel addresses the WHOLE batch of a map through one 32-bit byte offset: does [B][H][W][cstride] fit?
int pnnp_x3_wgrad_fits(int B, int H, int W, int cstride) {
    return (B > 0 && H > 0 && W > 0 && cstride > 0 && ((int64_t)B * H + 2) * W * cstride * 4 < (1ll << 31)) ? 1 : 0;
}

int64_t pnnp_x3_wgrad_workspace_floats(int B, int H, int W, int Cout, int Cin) {
    if (Cout % 32 || Cin % 32) return 0;
    // sized for up to 4 workgroups per CU, whatever pnnp_set_persistent_split says when the caller asks (the engines size it once per shape)
    const int cur = pnnp_get_persistent_split();
    // ... and with the bf16x3 tile heights, the shortest: never fewer splits than either scheme takes
    return (int64_t)wx3_splits(B, H, W, Cout, Cin, pnnp_wx3s_th(Cout, Cin), cur > 4 ? cur : 4) * ((int64_t)9 * Cout * Cin + Cout);
}

}  // extern "C"

namespace {

// One host path for both schemes: validation, arguments, pixel splits, the scheme's kernel (launch / th: its launcher and its pixel-tile height), the reduce.
// amax_*: the scaled scheme's slots (need_amax), null otherwise.
int wx3_run(int (*launch)(const WsArgs&, hipStream_t), int (*th)(int, int), bool need_amax,
            const float* g, int g_cs, int Cout, const unsigned* amax_g, const float* x1, int x1_cs, int C1, const unsigned* amax_x1,
            const float* x2, int x2_cs, int C2, const unsigned* amax_x2, float* dW, float* dbias,
            int B, int H, int W, int accumulate, float* workspace, int64_t workspace_floats, void* stream) {
    if (!g || !x1 || !dW || !workspace || B <= 0 || H <= 0 || W <= 0) return PNNP_E_INVALID;
    if (need_amax && (!amax_g || !amax_x1 || (x2 && !amax_x2))) return PNNP_E_INVALID;
    const int N = C1 + (x2 ? C2 : 0);
    if (!pnnp_x3_wgrad_supported(H, W, Cout, C1, x2 ? C2 : 0)) return PNNP_E_UNSUPPORTED;
    if (g_cs < Cout || x1_cs < C1 || (x2 && x2_cs < C2) || (g_cs & 3) || (x1_cs & 3) || (x2 && (x2_cs & 3))) return PNNP_E_INVALID;
    if ((((uintptr_t)g) | ((uintptr_t)x1) | ((uintptr_t)x2)) & 15) return PNNP_E_INVALID;
    // 32-bit byte offsets into the whole tensors (bit 31 marks "outside")
    const int cmax = g_cs > x1_cs ? g_cs : x1_cs;
    if (!pnnp_x3_wgrad_fits(B, H, W, cmax) || (x2 && !pnnp_x3_wgrad_fits(B, H, W, x2_cs))) return PNNP_E_UNSUPPORTED;
    if (workspace_floats < pnnp_x3_wgrad_workspace_floats(B, H, W, Cout, N)) return PNNP_E_WORKSPACE;
    hipStream_t st = as_stream(stream);
    WsArgs a{};
    a.G = g; a.Gcs = g_cs;
    a.X[0] = x1; a.Xcs[0] = x1_cs; a.X[1] = x2 ? x2 : x1; a.Xcs[1] = x2 ? x2_cs : x1_cs; a.n_split = x2 ? C1 : (1 << 30);
    a.B = B; a.H = H; a.W = W; a.M = Cout; a.N = N;
    a.Z = wx3_splits(B, H, W, Cout, N, th(Cout, N), pnnp_get_persistent_split());
    a.slab = workspace;
    a.bias_slab = dbias ? workspace + (int64_t)a.Z * 9 * Cout * N : nullptr;
    if (need_amax) { a.amax_g = amax_g; a.amax_x[0] = amax_x1; a.amax_x[1] = x2 ? amax_x2 : nullptr; }
    const int rc = launch(a, st);
    if (rc != PNNP_OK) return rc;
    return pnnp_wx3_reduce_launch(a.slab, dW, (int64_t)Cout * N, 9, a.Z, accumulate, a.bias_slab, dbias, Cout, st);
}

}  // namespace

extern "C" {

// dW [Cout][C1+C2][3][3] (+ dbias [Cout]) of a 3x3 / stride 1 / pad 1 convolution on the bf16x3 kernel (csrc/wgrad_x3s.hip); same contract as
// pnnp_conv_bwd_weight_f32 with taps = 9 (g: dL/d(pre-activation output), x1 / x2: the layer's input(s)).
int pnnp_conv3x3_x3_bwd_weight_f32(const float* g, int g_cs, int Cout, const float* x1, int x1_cs, int C1,
                                   const float* x2, int x2_cs, int C2, float* dW, float* dbias,
                                   int B, int H, int W, int accumulate, float* workspace, int64_t workspace_floats, void* stream) {
    return wx3_run(pnnp_wx3s_launch, pnnp_wx3s_th, false, g, g_cs, Cout, nullptr, x1, x1_cs, C1, nullptr, x2, x2_cs, C2, nullptr, dW, dbias,
                   B, H, W, accumulate, workspace, workspace_floats, stream);
}

// The same weight gradient on the fp16 matrix cores (csrc/wgrad_h2s.hip, csrc/h2.h): both operands are split into two scaled fp16 pieces
// on the fly, so each comes with its amax slot.  Same output tiles, slabs, workspace and reduce.
int pnnp_conv3x3_h2_bwd_weight_f32(const float* g, int g_cs, int Cout, const unsigned* amax_g, const float* x1, int x1_cs, int C1, const unsigned* amax_x1,
                                   const float* x2, int x2_cs, int C2, const unsigned* amax_x2, float* dW, float* dbias,
                                   int B, int H, int W, int accumulate, float* workspace, int64_t workspace_floats, void* stream) {
    return wx3_run(pnnp_wh2s_launch, pnnp_wh2s_th, true, g, g_cs, Cout, amax_g, x1, x1_cs, C1, amax_x1, x2, x2_cs, C2, amax_x2, dW, dbias,
                   B, H, W, accumulate, workspace, workspace_floats, stream);
}

}  // extern "C"

// Unet_Loss (losses/base_loss.py:33-107) and its gradient on the device: the plain L1, the Charbonnier form mean sqrt(d^2 + 1e-6), the 4-level
// average-pool pyramid (weights 1, 1/2, 1/4, 1/8 over their sum 1.875) and the Sobel edge term `grad_loss`, between engine.forward and
// engine.backward as streaming passes over pred and hr (NCHW float32, C <= 8).  Semantics of l1_clamp_kernel (csrc/misc.hip) throughout:
// scale[b] multiplies pred before the clamp, clamp_target clamps the target, grad_weight scales the gradient only, the clamp passes gradient on
// the closed interval [0, 1], a NaN prediction gives a NaN loss, loss_out[1 + b] is the SSE of the clamped pair at full resolution.
//
//   unet_loss_kernel<PYR, CHARB, HALVES>
//     PYR = 0: the thread-strided pixel walk of l1_clamp_kernel.  With CHARB = 0 too it IS that kernel's arithmetic, operation for operation
//              (partials in float, the same trees), so loss, SSE and gradient are its bits.
//     PYR = 1: AvgPool2d(2, 2) applied three times partitions a plane into nested 2x2, 4x4 and 8x8 blocks, so all four levels of a pixel live in
//              its own aligned 8x8 block and
//                  dL/dpred[b,c,y,x] = inv_n ratio_b grad_weight [0 <= p <= 1] sum_l (lam_l / 1.875) f'(d_l[block_l(y, x)]),   inv_n = 1 / (B C H W)
//              (the 1 / 4^l of the pooling and the level's element count cancel).  Eight neighbouring lanes own one 8x8 block: lane bit 0 is the
//              4-pixel half of a row, bits 1-2 the row pair, so a lane loads two float4 per tensor and channel.  Level 1 is in-register; level 2 takes
//              the row-pair neighbour's two values (lane ^ 2), level 3 the three other quadrants (lane ^ 1, ^ 4, ^ 5).  Levels are pooled successively,
//              each window summed in the order ((a00 + a01) + a10) + a11 and multiplied by 0.25, as Pyramid_Sample's AvgPool2d does -- never as one
//              64-element sum.  No pooled tensor, no halo, no second pass: pred and hr are read once, the gradient is written once.
//     L1 under PYR: the gradient of an element is k / 15 of the coefficient with the integer k = 8 s0 + 4 s1 + 2 s2 + s3 (s_l the sign at level l), so
//              equal sign patterns give equal bits whatever the order of anything else.
//   sobel_loss_kernel: every output channel of the reference's [C,C,3,3] expansion is the Sobel of the channel sum S, so the kernel works on S_low
//              and S_high with zero padding 1: an LDS tile of S with a halo of 2, the sign field r = sign(|u| - |v|) sign(u) one ring beyond the
//              outputs, then dL/dlow[c][q] = (1 / (B H W)) sum_k Sobel[k] r[q - k + 1] for both directions, through the same clamp mask, ratio and
//              grad_weight, ADDED to the gradient the main kernel wrote.
//
// Reductions are deterministic: per-block partials in the workspace (fixed trees), a one-wave finish in a fixed order.  Outside the L1 / no-pyramid
// mode the sums are carried in double from the thread on, so a term is the float32 nearest to the sum of its float32 elements (to ~1e-16).
#include "common.h"

namespace {

constexpr int BPC = 64;                 // blocks per crop, as l1_clamp_kernel
constexpr float CHARB_EPS = 1e-6f;      // L1_Charbonnier_loss.eps

__device__ __forceinline__ float sgnf(float d) { return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); }
__device__ __forceinline__ int sgni(float d) { return d > 0.f ? 1 : (d < 0.f ? -1 : 0); }
// AvgPool2d(2, 2) of one window in the reference's order
__device__ __forceinline__ float pool4(float a00, float a01, float a10, float a11) { return (((a00 + a01) + a10) + a11) * 0.25f; }

// sum of v over the 256 threads of the block, valid in thread 0 (shuffle tree per wave, then the four waves in order)
__device__ __forceinline__ double block_sum(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();                                   // red may still be read from the previous call
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

template <bool CHARB>
struct Term {
    // f(d) and f'(d)
    static __device__ __forceinline__ float f(float d) {
        if constexpr (CHARB) return sqrtf(d * d + CHARB_EPS); else return fabsf(d);
    }
    static __device__ __forceinline__ float df(float d) {
        if constexpr (CHARB) return d / sqrtf(d * d + CHARB_EPS); else return sgnf(d);
    }
};

// workspace: floats [0, 2 B BPC) = {loss partial (L1 / no-pyramid mode only), SSE partial} per block; then doubles, 8-byte aligned:
// level l of block k at dbl[l * B * BPC + k] (l < 4), the Sobel partial of block k at dbl[4 * B * BPC + k]
// HALVES (PYR only): 1 for C <= 4, 2 for C <= 8 -- the four-channel groups a lane keeps gradients for
template <bool PYR, bool CHARB, int HALVES>
__global__ void __launch_bounds__(256)
unet_loss_kernel(const float* __restrict__ pred, const float* __restrict__ hr, const float* __restrict__ scale, float* __restrict__ grad_nhwc,
                 float* __restrict__ grad_nchw, float* __restrict__ partial, double* __restrict__ dpartial, int B, int C, int H, int W, int Cp,
                 float inv_n, int clamp_target, int clamp_pred, float grad_weight) {
    constexpr bool LEGACY = !PYR && !CHARB;
    const int b = blockIdx.x / BPC, blk = blockIdx.x % BPC;
    const int64_t hw = (int64_t)H * W;
    const float sc = scale ? scale[b] : 1.f;            // `ori`: pred * ratio before the loss (trainer_SID.py:97-98)
    const float gsc = inv_n * sc * grad_weight;
    float l1 = 0.f, sse = 0.f;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    __shared__ double dred[4];
    if constexpr (!PYR) {
        for (int64_t s = (int64_t)blk * 256 + threadIdx.x; s < hw; s += (int64_t)BPC * 256) {
            float g[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) g[k] = 0.f;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                if (c < C) {
                    const int64_t i = ((int64_t)b * C + c) * hw + s;
                    const float p = pred[i] * sc, t0 = hr[i];
                    const float t = clamp_target ? pnnp_clampf(t0, 0.f, 1.f) : t0;
                    const float pc = clamp_pred ? pnnp_clampf(p, 0.f, 1.f) : p;
                    const float d = pc - t;
                    if constexpr (LEGACY) l1 += fabsf(d); else acc[0] += (double)Term<CHARB>::f(d);
                    const float tc = pnnp_clampf(t, 0.f, 1.f);            // PSNR uses the clamped pair (trainer_SID.py:112-114)
                    const float e = pnnp_clampf(pc, 0.f, 1.f) - tc;
                    sse += e * e;                                         // a multiply, then an add: what l1_clamp_kernel compiles to
                    const bool pass = !clamp_pred || (p >= 0.f && p <= 1.f);    // the clamp passes gradient on [0, 1]
                    g[c] = pass ? Term<CHARB>::df(d) * gsc : 0.f;
                    if (grad_nchw) grad_nchw[i] = g[c];
                }
            }
            if (grad_nhwc) {
                float* d = grad_nhwc + ((int64_t)b * hw + s) * Cp;
                *reinterpret_cast<float4*>(d) = make_float4(g[0], g[1], g[2], g[3]);
                if (Cp >= 8) *reinterpret_cast<float4*>(d + 4) = make_float4(g[4], g[5], g[6], g[7]);
            }
        }
    } else {
        const float g15 = gsc * (1.f / 15.f);
        constexpr float w0 = 1.f / 1.875f, w1 = 0.5f / 1.875f, w2 = 0.25f / 1.875f, w3 = 0.125f / 1.875f;
        const int wb = W >> 3;                                     // 8x8 blocks per row of blocks
        const int64_t nblk = (int64_t)(H >> 3) * wb;
        const int sub = threadIdx.x & 7, hx = sub & 1, ry = (sub >> 1) & 3, vb = sub >> 2;
        // uniform trip count: every lane of a wave takes part in the exchanges; a lane without a block works on the crop's last block (so its loads
        // are plain 16-byte loads of valid memory, not predicated ones) and neither accumulates nor stores
        for (int64_t q0 = (int64_t)blk * 32; q0 < nblk; q0 += (int64_t)BPC * 32) {
            const int64_t q = q0 + (threadIdx.x >> 3);
            const bool live = q < nblk;
            const int64_t qv = live ? q : nblk - 1;
            const int by = (int)(qv / wb), bx = (int)(qv % wb);
            const int y0 = by * 8 + ry * 2, x0 = bx * 8 + hx * 4;
            const int64_t pix = (int64_t)y0 * W + x0;              // first of the lane's 2 x 4 pixels (second row: + W)
            float g[4 * HALVES][8];
#pragma unroll
            for (int c = 0; c < 4 * HALVES; ++c)
#pragma unroll
                for (int k = 0; k < 8; ++k) g[c][k] = 0.f;
#pragma unroll
            for (int c0 = 0; c0 < 4 * HALVES; c0 += 4) {
              // four channels' loads are issued before the first of them is used: 16 x 16 bytes in flight per lane
              float4 a0[4], a1[4], h0[4], h1[4];
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                  // (a channel past C re-reads the last one instead of branching around its loads)
                  const int64_t i = ((int64_t)b * C + (c0 + j < C ? c0 + j : C - 1)) * hw + pix;
                  a0[j] = *reinterpret_cast<const float4*>(pred + i); a1[j] = *reinterpret_cast<const float4*>(pred + i + W);
                  h0[j] = *reinterpret_cast<const float4*>(hr + i); h1[j] = *reinterpret_cast<const float4*>(hr + i + W);
              }
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                const int c = c0 + j;
                if (c < C) {
                    const int64_t i = ((int64_t)b * C + c) * hw + pix;
                    float p[8], t[8], pc[8];
                    p[0] = a0[j].x; p[1] = a0[j].y; p[2] = a0[j].z; p[3] = a0[j].w; p[4] = a1[j].x; p[5] = a1[j].y; p[6] = a1[j].z; p[7] = a1[j].w;
                    t[0] = h0[j].x; t[1] = h0[j].y; t[2] = h0[j].z; t[3] = h0[j].w; t[4] = h1[j].x; t[5] = h1[j].y; t[6] = h1[j].z; t[7] = h1[j].w;
                    float d0[8], f0 = 0.f, es = 0.f;
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        p[k] = p[k] * sc;
                        t[k] = clamp_target ? pnnp_clampf(t[k], 0.f, 1.f) : t[k];
                        pc[k] = clamp_pred ? pnnp_clampf(p[k], 0.f, 1.f) : p[k];
                        d0[k] = pc[k] - t[k];
                        f0 += Term<CHARB>::f(d0[k]);
                        const float e = pnnp_clampf(pc[k], 0.f, 1.f) - pnnp_clampf(t[k], 0.f, 1.f);
                        es += e * e;
                    }
                    // level 1: the lane's two 2x2 windows
                    const float pl1[2] = {pool4(pc[0], pc[1], pc[4], pc[5]), pool4(pc[2], pc[3], pc[6], pc[7])};
                    const float tl1[2] = {pool4(t[0], t[1], t[4], t[5]), pool4(t[2], t[3], t[6], t[7])};
                    const float d1[2] = {pl1[0] - tl1[0], pl1[1] - tl1[1]};
                    // level 2: with the other row pair of the 4x4 quadrant (lane ^ 2); both lanes compute the same value
                    const bool low = ry & 1;
                    const float po0 = __shfl_xor(pl1[0], 2, 64), po1 = __shfl_xor(pl1[1], 2, 64);
                    const float to0 = __shfl_xor(tl1[0], 2, 64), to1 = __shfl_xor(tl1[1], 2, 64);
                    const float pl2 = low ? pool4(po0, po1, pl1[0], pl1[1]) : pool4(pl1[0], pl1[1], po0, po1);
                    const float tl2 = low ? pool4(to0, to1, tl1[0], tl1[1]) : pool4(tl1[0], tl1[1], to0, to1);
                    const float d2 = pl2 - tl2;
                    // level 3: the four quadrants; this lane's is (row vb, column hx)
                    const float ph = __shfl_xor(pl2, 1, 64), pv = __shfl_xor(pl2, 4, 64), pd = __shfl_xor(pl2, 5, 64);
                    const float th = __shfl_xor(tl2, 1, 64), tv = __shfl_xor(tl2, 4, 64), td = __shfl_xor(tl2, 5, 64);
                    const float pts = vb ? pv : pl2, pto = vb ? pd : ph, pbs = vb ? pl2 : pv, pbo = vb ? ph : pd;     // top / bottom row, same / other column
                    const float tts = vb ? tv : tl2, tto = vb ? td : th, tbs = vb ? tl2 : tv, tbo = vb ? th : td;
                    const float pl3 = hx ? pool4(pto, pts, pbo, pbs) : pool4(pts, pto, pbs, pbo);
                    const float tl3 = hx ? pool4(tto, tts, tbo, tbs) : pool4(tts, tto, tbs, tbo);
                    const float d3 = pl3 - tl3;
                    if (live) {
                        sse += es;
                        acc[0] += (double)f0;
                        acc[1] += (double)(Term<CHARB>::f(d1[0]) + Term<CHARB>::f(d1[1]));
                        if (!low) acc[2] += (double)Term<CHARB>::f(d2);            // one of the two lanes that hold it
                        if (sub == 0) acc[3] += (double)Term<CHARB>::f(d3);        // one of the eight
                    }
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        const int j = (k & 3) >> 1;
                        const bool pass = !clamp_pred || (p[k] >= 0.f && p[k] <= 1.f);
                        float gk;
                        if constexpr (CHARB) {
                            gk = (((w0 * Term<true>::df(d0[k]) + w1 * Term<true>::df(d1[j])) + w2 * Term<true>::df(d2)) + w3 * Term<true>::df(d3)) * gsc;
                        } else {
                            gk = (float)(8 * sgni(d0[k]) + 4 * sgni(d1[j]) + 2 * sgni(d2) + sgni(d3)) * g15;
                        }
                        g[c][k] = pass ? gk : 0.f;
                    }
                    if (grad_nchw && live) {
                        *reinterpret_cast<float4*>(grad_nchw + i) = make_float4(g[c][0], g[c][1], g[c][2], g[c][3]);
                        *reinterpret_cast<float4*>(grad_nchw + i + W) = make_float4(g[c][4], g[c][5], g[c][6], g[c][7]);
                    }
                }
              }
            }
            if (grad_nhwc && live) {
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    float* d = grad_nhwc + ((int64_t)b * hw + pix + (k >> 2) * (int64_t)W + (k & 3)) * Cp;
                    *reinterpret_cast<float4*>(d) = make_float4(g[0][k], g[1][k], g[2][k], g[3][k]);
                    if constexpr (HALVES == 2) {
                        if (Cp >= 8) *reinterpret_cast<float4*>(d + 4) = make_float4(g[4][k], g[5][k], g[6][k], g[7][k]);
                    } else {
                        if (Cp >= 8) *reinterpret_cast<float4*>(d + 4) = make_float4(0.f, 0.f, 0.f, 0.f);
                    }
                }
            }
        }
    }
    __shared__ float r1[256], r2[256];
    r1[threadIdx.x] = l1; r2[threadIdx.x] = sse;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (threadIdx.x < k) { r1[threadIdx.x] += r1[threadIdx.x + k]; r2[threadIdx.x] += r2[threadIdx.x + k]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { partial[2 * blockIdx.x] = r1[0]; partial[2 * blockIdx.x + 1] = r2[0]; }
    if constexpr (!LEGACY) {
        const int64_t nb = (int64_t)B * BPC;
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            const double s = block_sum(acc[l], dred);
            if (threadIdx.x == 0) dpartial[l * nb + blockIdx.x] = s;
        }
    }
}

// out[0] = the loss, out[1 + b] = SSE of crop b, terms[0..3] (optional) = the level means before weighting, terms[4] = 0.
// mode 0 (L1, no pyramid) is l1_finish_kernel; the other modes sum their double partials lane-strided, then a shuffle tree.
__global__ void __launch_bounds__(64)
unet_loss_finish_kernel(const float* __restrict__ partial, const double* __restrict__ dpartial, float* __restrict__ out, float* __restrict__ terms,
                        int B, float inv_n, double n0, double n1, double n2, double n3, int legacy, int pyramid) {
    const int lane = threadIdx.x;
    float tot = 0.f;
    for (int b = 0; b < B; ++b) {
        float l = 0.f, s = 0.f;
        for (int k = lane; k < BPC; k += 64) { l += partial[2 * (b * BPC + k)]; s += partial[2 * (b * BPC + k) + 1]; }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { l += __shfl_xor(l, o); s += __shfl_xor(s, o); }
        tot += l;
        if (lane == 0) out[1 + b] = s;
    }
    float t[4] = {tot * inv_n, 0.f, 0.f, 0.f};
    if (!legacy) {
        const double n[4] = {n0, n1, n2, n3};
        const int nb = B * BPC;
        for (int l = 0; l < (pyramid ? 4 : 1); ++l) {
            double s = 0.0;
            for (int k = lane; k < nb; k += 64) s += dpartial[(int64_t)l * nb + k];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
            t[l] = (float)(s / n[l]);
        }
    }
    if (lane == 0) {
        // Pyramid_Loss(rate=0.5, norm=True): the terms are added in level order, then divided by the sum of the weights
        out[0] = pyramid ? (((t[0] + t[1] * 0.5f) + t[2] * 0.25f) + t[3] * 0.125f) / 1.875f : t[0];
        if (terms) { terms[0] = t[0]; terms[1] = t[1]; terms[2] = t[2]; terms[3] = t[3]; terms[4] = 0.f; }
    }
}

// ------------------------------------------------------------------------------------------------ Sobel edge term (grad_loss)
constexpr int STW = 32, STH = 8;                   // outputs per tile: one per thread
constexpr int SW = STW + 4, SH = STH + 4;          // S with a halo of 2
constexpr int RW = STW + 2, RH = STH + 2;          // r with a halo of 1

__global__ void __launch_bounds__(256)
sobel_loss_kernel(const float* __restrict__ pred, const float* __restrict__ hr, const float* __restrict__ scale, float* __restrict__ grad_nhwc,
                  float* __restrict__ grad_nchw, double* __restrict__ dpartial, int B, int C, int H, int W, int Cp, float inv_bhw, int clamp_target,
                  int clamp_pred, float grad_weight, float grad_lambda) {
    __shared__ float s_lo[SH][SW], s_hi[SH][SW];
    __shared__ int r_x[RH][RW], r_y[RH][RW];
    __shared__ double dred[4];
    const int b = blockIdx.x / BPC, blk = blockIdx.x % BPC;
    const int64_t hw = (int64_t)H * W;
    const float sc = scale ? scale[b] : 1.f;
    const float coef = inv_bhw * sc * grad_weight * grad_lambda;
    const int tw = (W + STW - 1) / STW, th = (H + STH - 1) / STH;
    const int64_t ntiles = (int64_t)tw * th;
    const int tx = threadIdx.x % STW, ty = threadIdx.x / STW;
    double acc = 0.0;
    for (int64_t tile = blk; tile < ntiles; tile += BPC) {          // block-uniform trip count: the barriers below are reached by every thread
        const int y0 = (int)(tile / tw) * STH, x0 = (int)(tile % tw) * STW;
        for (int e = threadIdx.x; e < SH * SW; e += 256) {
            const int iy = e / SW, ix = e % SW, y = y0 - 2 + iy, x = x0 - 2 + ix;
            float lo = 0.f, hi = 0.f;                               // zero padding, and nothing is read outside the image
            if (y >= 0 && y < H && x >= 0 && x < W) {
                for (int c = 0; c < C; ++c) {
                    const int64_t i = ((int64_t)b * C + c) * hw + (int64_t)y * W + x;
                    const float p = pred[i] * sc, t0 = hr[i];
                    lo += clamp_pred ? pnnp_clampf(p, 0.f, 1.f) : p;
                    hi += clamp_target ? pnnp_clampf(t0, 0.f, 1.f) : t0;
                }
            }
            s_lo[iy][ix] = lo; s_hi[iy][ix] = hi;
        }
        __syncthreads();
        for (int e = threadIdx.x; e < RH * RW; e += 256) {
            const int iy = e / RW, ix = e % RW, y = y0 - 1 + iy, x = x0 - 1 + ix;
            int rx = 0, ry = 0;
            if (y >= 0 && y < H && x >= 0 && x < W) {
                // S rows iy .. iy + 2, columns ix .. ix + 2 of the tile are the 3x3 neighbourhood of (y, x)
                const float a00 = s_lo[iy][ix], a01 = s_lo[iy][ix + 1], a02 = s_lo[iy][ix + 2], a10 = s_lo[iy + 1][ix], a12 = s_lo[iy + 1][ix + 2];
                const float a20 = s_lo[iy + 2][ix], a21 = s_lo[iy + 2][ix + 1], a22 = s_lo[iy + 2][ix + 2];
                const float h00 = s_hi[iy][ix], h01 = s_hi[iy][ix + 1], h02 = s_hi[iy][ix + 2], h10 = s_hi[iy + 1][ix], h12 = s_hi[iy + 1][ix + 2];
                const float h20 = s_hi[iy + 2][ix], h21 = s_hi[iy + 2][ix + 1], h22 = s_hi[iy + 2][ix + 2];
                const float ux = ((a20 + 2.f * a21) + a22) - ((a00 + 2.f * a01) + a02), vx = ((h20 + 2.f * h21) + h22) - ((h00 + 2.f * h01) + h02);
                const float uy = ((a02 + 2.f * a12) + a22) - ((a00 + 2.f * a10) + a20), vy = ((h02 + 2.f * h12) + h22) - ((h00 + 2.f * h10) + h20);
                const float ex = fabsf(ux) - fabsf(vx), ey = fabsf(uy) - fabsf(vy);
                rx = sgni(ex) * sgni(ux); ry = sgni(ey) * sgni(uy);
                if (iy >= 1 && iy <= STH && ix >= 1 && ix <= STW) acc += (double)(fabsf(ex) + fabsf(ey));     // the tile's own outputs (a NaN stays one)
            }
            r_x[iy][ix] = rx; r_y[iy][ix] = ry;
        }
        __syncthreads();
        const int y = y0 + ty, x = x0 + tx;
        if (y < H && x < W && (grad_nhwc || grad_nchw)) {
            // dS[q] = sum_k Sobel[k] r[q - k + 1]: r rows ty .. ty + 2 are image rows y - 1 .. y + 1 (k = 2 reads y - 1)
            const int kx = (r_x[ty][tx] + 2 * r_x[ty][tx + 1] + r_x[ty][tx + 2]) - (r_x[ty + 2][tx] + 2 * r_x[ty + 2][tx + 1] + r_x[ty + 2][tx + 2]);
            const int ky = (r_y[ty][tx] + 2 * r_y[ty + 1][tx] + r_y[ty + 2][tx]) - (r_y[ty][tx + 2] + 2 * r_y[ty + 1][tx + 2] + r_y[ty + 2][tx + 2]);
            const float gq = (float)(kx + ky) * coef;
            const int64_t s = (int64_t)y * W + x;
            float g[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                g[c] = 0.f;
                if (c < C) {
                    const int64_t i = ((int64_t)b * C + c) * hw + s;
                    const float p = pred[i] * sc;
                    g[c] = (!clamp_pred || (p >= 0.f && p <= 1.f)) ? gq : 0.f;
                    if (grad_nchw) grad_nchw[i] += g[c];
                }
            }
            if (grad_nhwc) {
                float4* d = reinterpret_cast<float4*>(grad_nhwc + ((int64_t)b * hw + s) * Cp);
                float4 v = d[0];
                v.x += g[0]; v.y += g[1]; v.z += g[2]; v.w += g[3];
                d[0] = v;
                if (Cp >= 8) { v = d[1]; v.x += g[4]; v.y += g[5]; v.z += g[6]; v.w += g[7]; d[1] = v; }
            }
        }
        // the next trip's first barrier separates these reads of r from its writes; S is rewritten only after every thread has passed the
        // second barrier above, that is after all reads of S
    }
    const double s = block_sum(acc, dred);
    if (threadIdx.x == 0) dpartial[blockIdx.x] = s;
}

// terms[4] = the Sobel term, out[0] += grad_lambda * term (recon = 0: out[0] = grad_lambda * term, the SSE slots and terms[0..3] zeroed)
__global__ void __launch_bounds__(64)
sobel_finish_kernel(const double* __restrict__ dpartial, float* __restrict__ out, float* __restrict__ terms, int B, double n, float grad_lambda, int recon) {
    const int lane = threadIdx.x;
    double s = 0.0;
    for (int k = lane; k < B * BPC; k += 64) s += dpartial[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    const float term = (float)(s / n);
    if (!recon) for (int b = lane; b < B; b += 64) out[1 + b] = 0.f;
    if (lane == 0) {
        out[0] = recon ? out[0] + grad_lambda * term : grad_lambda * term;
        if (terms) {
            if (!recon) { terms[0] = 0.f; terms[1] = 0.f; terms[2] = 0.f; terms[3] = 0.f; }
            terms[4] = term;
        }
    }
}

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

extern "C" {

int64_t pnnp_unet_loss_workspace_floats(int B) { return B > 0 ? (int64_t)B * BPC * 12 : 0; }      // 2 floats + 5 doubles per block

int pnnp_unet_loss_f32(const float* pred, const float* hr, const float* scale, float* grad_nhwc, float* grad_nchw, float* loss_out, float* terms,
                       int B, int C, int H, int W, int Cp, float* workspace, int64_t workspace_floats, int clamp_target, int clamp_pred,
                       float grad_weight, int charbonnier, int pyramid, float grad_lambda, int recon, void* stream) {
    if (!pred || !hr || !loss_out || !workspace || B <= 0 || B > (1 << 20) || C <= 0 || C > 8 || H <= 0 || W <= 0) return PNNP_E_INVALID;
    if (grad_nhwc && (Cp < C || (Cp != 4 && Cp != 8) || !aligned(grad_nhwc, 16))) return PNNP_E_INVALID;
    if ((clamp_target | clamp_pred | charbonnier | pyramid | recon) & ~1) return PNNP_E_INVALID;
    if (!(grad_lambda >= 0.f) || !(grad_lambda <= 3.0e38f) || !(grad_weight == grad_weight)) return PNNP_E_INVALID;
    if (!recon && !(grad_lambda > 0.f)) return PNNP_E_INVALID;                       // nothing to compute
    if (pyramid && grad_lambda > 0.f) return PNNP_E_INVALID;                         // the reference never defines the pyramid of the edge term
    if (pyramid && ((H & 7) || (W & 7) || !aligned(pred, 16) || !aligned(hr, 16) || (grad_nchw && !aligned(grad_nchw, 16)))) return PNNP_E_INVALID;
    if (!aligned(workspace, 8)) return PNNP_E_INVALID;
    if (workspace_floats < pnnp_unet_loss_workspace_floats(B)) return PNNP_E_WORKSPACE;
    const int64_t nb = (int64_t)B * BPC;
    double* dws = reinterpret_cast<double*>(workspace + 2 * nb);
    const double n0 = (double)B * C * H * W;
    const float inv_n = 1.0f / ((float)B * C * H * W);
    hipStream_t st = as_stream(stream);
    if (recon) {
        auto kern = !pyramid ? (charbonnier ? unet_loss_kernel<false, true, 2> : unet_loss_kernel<false, false, 2>)
                    : C <= 4 ? (charbonnier ? unet_loss_kernel<true, true, 1> : unet_loss_kernel<true, false, 1>)
                             : (charbonnier ? unet_loss_kernel<true, true, 2> : unet_loss_kernel<true, false, 2>);
        hipLaunchKernelGGL(kern, dim3((unsigned)nb), dim3(256), 0, st, pred, hr, scale, grad_nhwc, grad_nchw, workspace, dws, B, C, H, W, Cp, inv_n,
                           clamp_target, clamp_pred, grad_weight);
        hipLaunchKernelGGL(unet_loss_finish_kernel, dim3(1), dim3(64), 0, st, workspace, dws, loss_out, terms, B, inv_n, n0, n0 / 4, n0 / 16, n0 / 64,
                           (!pyramid && !charbonnier) ? 1 : 0, pyramid);
    } else {
        if (grad_nhwc && hipMemsetAsync(grad_nhwc, 0, sizeof(float) * (size_t)B * H * W * Cp, st) != hipSuccess) return PNNP_E_LAUNCH;
        if (grad_nchw && hipMemsetAsync(grad_nchw, 0, sizeof(float) * (size_t)B * C * H * W, st) != hipSuccess) return PNNP_E_LAUNCH;
    }
    if (grad_lambda > 0.f) {
        hipLaunchKernelGGL(sobel_loss_kernel, dim3((unsigned)nb), dim3(256), 0, st, pred, hr, scale, grad_nhwc, grad_nchw, dws + 4 * nb, B, C, H, W, Cp,
                           1.0f / ((float)B * H * W), clamp_target, clamp_pred, grad_weight, grad_lambda);
        hipLaunchKernelGGL(sobel_finish_kernel, dim3(1), dim3(64), 0, st, dws + 4 * nb, loss_out, terms, B, (double)B * H * W, grad_lambda, recon);
    }
    return pnnp_launch_status();
}

}  // extern "C"

// Backward of NoiseFlow.sample: the vector-Jacobian product of one [AffineCoupling^-1, Conv2d1x1^-1] pair of the reversed chain
// (csrc/nf.hip runs its forward; reference: archs/noise_flow.py:173-188, flow_layers/affine_coupling.py:27-34,245-295,
// conv2d1x1.py:47-92, gain.py:79-93, signal_dependant.py:37-57; the backward is what autograd derives for those lines, except that the
// reference's Conv2d1x1 inverse goes through .cpu() and cuts its own graph there -- the true derivative is computed here).
//
// A pair maps u [B][4][H][W] to out:
//   h1 = conv3x3(u[0:2]);  a1 = relu(BN1(h1));  h2 = W2 a1;  a2 = relu(BN2(h2))             (h1, h2 WITHOUT their conv biases, see below)
//   raw3 = conv3x3_valid(pad1([a2, ring])) + b3;  out3 = raw3 * exp(3 logs);  shift = out3[0:2];  ls = scale * tanh(out3[2:4])
//   y   = [u0, u1, (u2 - shift_a) * exp(-ls_a), (u3 - shift_b) * exp(-ls_b)]
//   out = (Winv y) * s            Winv: the Conv2d1x1 inverse (x the GainISO scalar where it applies);  s = sqrt(a*clean + b), last pair only
// This is the coupling network of csrc/nf_train.hip run in the other direction, and the passes are modelled on that file: HBM-streaming
// passes over 4-plane fp32 maps, 32x32 tiles + halo in LDS, parameter sums as per-workgroup partial rows followed by a column reduction
// in double (no float atomics: results are bitwise repeatable).  The caller keeps only each pair's INPUT u; the hidden maps are
// recomputed here (two passes) instead of being stored by the forward, whose values must stay those of nf_step_kernel bit for bit:
//   hidden   u[0:2]                 -> h1, h2                       (tile pass; BatchNorm from the `bn` block, no reductions)
//   out3     h2                     -> out3                         (tile pass)
//   couple   u, out3, h2, dout      -> dy2, du (du[0:2] = d y[0:2] so far), sums [215]
//   conv2    h1, h2, dy2            -> dy1, sums [28]               (pointwise pass)
//   conv1    u[0:2], h1, dy1, du    -> du[0:2] += conv1^T(d h1), sums [76]
// BatchNorm is y = G * (h - mean) * rstd + BE with the `bn` block of nf_train.hip (mean1[4] rstd1[4] var1[4] mean2[4] rstd2[4] var2[4]):
//   batch statistics (training mode): the block pnnp_nf_train_stats_f32 left for the forward; mean and rstd depend on u, and the
//     backward carries the two statistics terms  d h = G rstd (dy - mean(dy) - xhat mean(dy xhat)),  reduced between the passes;
//   running statistics (eval mode):   a fixed affine: mean = running_mean - conv bias, rstd = 1 / sqrt(running_var + eps), formed by the
//     caller; the same passes with the statistics terms switched off.
// h1 / h2 are bias-free in both modes for the reason given at the top of nf_train.hip ((h - mean) must not suffer the cancellation of
// (h + b) - (mean + b)); the conv-bias gradients are sum(d h), which is mathematically zero under batch statistics.
// Parameter block `prm` [301] and its gradient `gprm`: the layout documented at the top of nf_train.hip.
#include "common.h"

namespace {

constexpr int TS = 32, HS = TS + 2;            // output tile, tile + halo 1
constexpr int P_W1 = 0, P_G1 = 76, P_BE1 = 80, P_W2 = 84, P_G2 = 104, P_BE2 = 108, P_W3 = 112, P_B3 = 292, P_LOGS = 296, P_SCALE = 300;

// the wave / workgroup sums of nf_train.hip (DPP row steps, then row_bcast15 / row_bcast31: the total lands in lane 63)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_add(float v) {
    return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, 0xf, false));
}
__device__ __forceinline__ float wave_sum_lane63(float v) {
    v = dpp_add<0xB1, 0xf>(v);       // quad_perm [1,0,3,2]
    v = dpp_add<0x4E, 0xf>(v);       // quad_perm [2,3,0,1]
    v = dpp_add<0x141, 0xf>(v);      // row_half_mirror
    v = dpp_add<0x140, 0xf>(v);      // row_mirror
    v = dpp_add<0x142, 0xa>(v);      // row_bcast15 into rows 1 and 3
    v = dpp_add<0x143, 0xc>(v);      // row_bcast31 into rows 2 and 3
    return v;
}
template <int N>
__device__ __forceinline__ void block_sum_store(const float (&v)[N], float* __restrict__ out, float (*red)[4]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const float s = wave_sum_lane63(v[i]);
        if (lane == 63) red[i][wave] = s;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < N; i += 256) out[i] = (red[i][0] + red[i][1]) + (red[i][2] + red[i][3]);
}

struct SPair {
    const float* u;          // [B][4][H][W] the pair's input
    const float* clean;      // [B][4][H][W] or null
    const float* ab;         // device {a, b} of the signal-dependent scale (used iff clean)
    const float* winv;       // device [4][4]
    const float* prm;        // device [301]
    const float* bn;         // device [24]
    int H, W;
};

// ---------------------------------------------------------------------------------------------------- recomputed forward
// h1 = conv2d_1(u[0:2]) and h2 = conv2d_2(relu(BN1(h1))), both bias-free
__global__ void __launch_bounds__(256)
nfs_hidden_kernel(SPair p, float* __restrict__ h1, float* __restrict__ h2) {
    __shared__ float us[2][HS][HS + 1];
    const int b = blockIdx.z, ty0 = blockIdx.y * TS, tx0 = blockIdx.x * TS, H = p.H, W = p.W;
    const int64_t plane = (int64_t)H * W;
    const float* ub = p.u + (int64_t)b * 4 * plane;
    for (int i = threadIdx.x; i < HS * HS; i += 256) {
        const int r = i / HS, q = i % HS, gy = ty0 + r - 1, gx = tx0 + q - 1;
        const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
        const int64_t pix = (int64_t)gy * W + gx;
        us[0][r][q] = in ? ub[pix] : 0.f; us[1][r][q] = in ? ub[plane + pix] : 0.f;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < TS * TS; i += 256) {
        const int r = i / TS, q = i % TS, gy = ty0 + r, gx = tx0 + q;
        if (gy >= H || gx >= W) continue;
        const int64_t base = (int64_t)b * 4 * plane + (int64_t)gy * W + gx;
        float a1[4];
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            float s = 0.f;
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int t = 0; t < 9; ++t) s += p.prm[P_W1 + (o * 2 + c) * 9 + t] * us[c][r + t / 3][q + t % 3];
            h1[base + o * plane] = s;
            a1[o] = fmaxf(p.prm[P_G1 + o] * ((s - p.bn[o]) * p.bn[4 + o]) + p.prm[P_BE1 + o], 0.f);
        }
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            float s = 0.f;
#pragma unroll
            for (int c = 0; c < 4; ++c) s += p.prm[P_W2 + o * 4 + c] * a1[c];
            h2[base + o * plane] = s;
        }
    }
}

// a2 = relu(BN2(h2)) on tile + halo 1 (zero outside the image: the ConstantPad3d ring)
__device__ __forceinline__ void stage_a2(const SPair& p, const float* __restrict__ h2b, float (*a2s)[HS][HS + 1], int ty0, int tx0) {
    const int64_t plane = (int64_t)p.H * p.W;
    for (int i = threadIdx.x; i < HS * HS; i += 256) {
        const int r = i / HS, q = i % HS, gy = ty0 + r - 1, gx = tx0 + q - 1;
        const bool in = gy >= 0 && gy < p.H && gx >= 0 && gx < p.W;
#pragma unroll
        for (int c = 0; c < 4; ++c)
            a2s[c][r][q] = in ? fmaxf(p.prm[P_G2 + c] * ((h2b[c * plane + (int64_t)gy * p.W + gx] - p.bn[12 + c]) * p.bn[16 + c]) +
                                          p.prm[P_BE2 + c], 0.f)
                              : 0.f;
    }
}

// out3 = (conv2d_3([a2, ring]) + b3) * exp(3 logs)
__global__ void __launch_bounds__(256)
nfs_out3_kernel(SPair p, const float* __restrict__ h2, float* __restrict__ out3) {
    __shared__ float a2s[4][HS][HS + 1];
    const int b = blockIdx.z, ty0 = blockIdx.y * TS, tx0 = blockIdx.x * TS, H = p.H, W = p.W;
    const int64_t plane = (int64_t)H * W;
    stage_a2(p, h2 + (int64_t)b * 4 * plane, a2s, ty0, tx0);
    __syncthreads();
    for (int i = threadIdx.x; i < TS * TS; i += 256) {
        const int r = i / TS, q = i % TS, gy = ty0 + r, gx = tx0 + q;
        if (gy >= H || gx >= W) continue;
        const int64_t pix = (int64_t)gy * W + gx;
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            float s = p.prm[P_B3 + o];
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int yy = gy + t / 3 - 1, xx = gx + t % 3 - 1;
#pragma unroll
                for (int c = 0; c < 4; ++c) s += p.prm[P_W3 + (o * 5 + c) * 9 + t] * a2s[c][r + t / 3][q + t % 3];
                if (yy < 0 || yy >= H || xx < 0 || xx >= W) s += p.prm[P_W3 + (o * 5 + 4) * 9 + t];
            }
            out3[((int64_t)b * 4 + o) * plane + pix] = s * expf(3.f * p.prm[P_LOGS + o]);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------- backward
// deterministic column sums: part [rows][cols] -> out[cols] (double accumulation), one workgroup per column
__global__ void __launch_bounds__(256)
nfs_colsum_kernel(const float* __restrict__ part, int rows, int cols, float* __restrict__ out) {
    __shared__ double red[256];
    const int col = blockIdx.x;
    double s = 0.0;
    for (int r = threadIdx.x; r < rows; r += 256) s += (double)part[(int64_t)r * cols + col];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[col] = (float)red[0];
}

constexpr int NB1 = 215;     // dW3[180] db3[4] dlogs[4] dscale[1] sum dy2[4] sum dy2*xhat2[4] dWinv[16] da db
constexpr int NB2 = 28;      // dW2[16] db2[4] sum dy1[4] sum dy1*xhat1[4]
constexpr int NB3 = 76;      // dW1[72] db1[4]

// backward pass 1: through the output scale, the Conv2d1x1 inverse, the coupling and conv2d_3 down to dy2 = dL/d(BN2 output)
// (ReLU mask applied).  Writes du: planes 2,3 final, planes 0,1 = d y[0:2] (pass 3 adds the coupling network's share).
__global__ void __launch_bounds__(256)
nfs_bwd_couple_kernel(SPair p, const float* __restrict__ h2, const float* __restrict__ out3, const float* __restrict__ dout,
                      float* __restrict__ dy2, float* __restrict__ du, float* __restrict__ part) {
    __shared__ float a2s[4][HS][HS + 1];
    __shared__ float gs[4][HS][HS + 1];        // d raw3 on tile + halo 1 (zero outside the image)
    __shared__ float red[48][4];
    const int b = blockIdx.z, ty0 = blockIdx.y * TS, tx0 = blockIdx.x * TS, H = p.H, W = p.W;
    const int64_t plane = (int64_t)H * W;
    const float* ub = p.u + (int64_t)b * 4 * plane;
    const float* cb = p.clean ? p.clean + (int64_t)b * 4 * plane : nullptr;
    const float* h2b = h2 + (int64_t)b * 4 * plane;
    const float* ob = out3 + (int64_t)b * 4 * plane;
    const float* gb = dout + (int64_t)b * 4 * plane;
    float* dub = du + (int64_t)b * 4 * plane;
    float* row = part + (((int64_t)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * NB1;
    stage_a2(p, h2b, a2s, ty0, tx0);
    const float scale = p.prm[P_SCALE];
    const float sa = cb ? p.ab[0] : 0.f, sb = cb ? p.ab[1] : 1.f;
    float sm[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};       // db3[4], dlogs[4], dscale
    float wa[18];                                                       // dWinv[16], da, db
#pragma unroll
    for (int j = 0; j < 18; ++j) wa[j] = 0.f;
    for (int i = threadIdx.x; i < HS * HS; i += 256) {
        const int r = i / HS, q = i % HS, gy = ty0 + r - 1, gx = tx0 + q - 1;
        float g[4] = {0.f, 0.f, 0.f, 0.f};
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const int64_t pix = (int64_t)gy * W + gx;
            float go[4], sc[4], dr[4], dyv[4] = {0.f, 0.f, 0.f, 0.f};       // d out, s, d (Winv y), d y
#pragma unroll
            for (int o = 0; o < 4; ++o) {
                go[o] = gb[o * plane + pix];
                sc[o] = cb ? sqrtf(sa * cb[o * plane + pix] + sb) : 1.f;
                dr[o] = go[o] * sc[o];
#pragma unroll
                for (int c = 0; c < 4; ++c) dyv[c] += p.winv[o * 4 + c] * dr[o];
            }
            const float o0 = ob[pix], o1 = ob[plane + pix], o2 = ob[2 * plane + pix], o3 = ob[3 * plane + pix];
            const float ta = tanhf(o2), tb = tanhf(o3), ea = expf(-(scale * ta)), eb = expf(-(scale * tb));
            const float y2 = (ub[2 * plane + pix] - o0) * ea, y3 = (ub[3 * plane + pix] - o1) * eb;
            const float dlsa = -(dyv[2] * y2), dlsb = -(dyv[3] * y3);
            const float d3[4] = {-(dyv[2] * ea), -(dyv[3] * eb), dlsa * scale * (1.f - ta * ta), dlsb * scale * (1.f - tb * tb)};
            const float outv[4] = {o0, o1, o2, o3};
#pragma unroll
            for (int o = 0; o < 4; ++o) g[o] = d3[o] * expf(3.f * p.prm[P_LOGS + o]);
            const bool interior = r >= 1 && r <= TS && q >= 1 && q <= TS;        // this workgroup owns the pixel
            if (interior) {
#pragma unroll
                for (int o = 0; o < 4; ++o) { sm[o] += g[o]; sm[4 + o] += 3.f * d3[o] * outv[o]; }
                sm[8] += dlsa * ta + dlsb * tb;
                dub[pix] = dyv[0]; dub[plane + pix] = dyv[1]; dub[2 * plane + pix] = dyv[2] * ea; dub[3 * plane + pix] = dyv[3] * eb;
                const float y[4] = {ub[pix], ub[plane + pix], y2, y3};
#pragma unroll
                for (int o = 0; o < 4; ++o) {
                    float rv = 0.f;
#pragma unroll
                    for (int c = 0; c < 4; ++c) { wa[o * 4 + c] += dr[o] * y[c]; rv += p.winv[o * 4 + c] * y[c]; }
                    if (cb) {          // out = rv * s, s = sqrt(a*clean + b)
                        const float ds2 = go[o] * rv / (2.f * sc[o]);
                        wa[16] += ds2 * cb[o * plane + pix]; wa[17] += ds2;
                    }
                }
            }
        }
#pragma unroll
        for (int o = 0; o < 4; ++o) gs[o][r][q] = g[o];
    }
    __syncthreads();
    // d a2 = conv3^T(g), ReLU mask, BatchNorm-backward sums
    float bs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int i = threadIdx.x; i < TS * TS; i += 256) {
        const int r = i / TS, q = i % TS, gy = ty0 + r, gx = tx0 + q;
        if (gy >= H || gx >= W) continue;
        const int64_t pix = (int64_t)gy * W + gx;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float s = 0.f;
#pragma unroll
            for (int o = 0; o < 4; ++o)
#pragma unroll
                for (int t = 0; t < 9; ++t)      // output pixel (p - (t - centre)) used a2(p) through tap t
                    s += p.prm[P_W3 + (o * 5 + c) * 9 + t] * gs[o][r + 2 - t / 3][q + 2 - t % 3];
            const float hv = h2b[c * plane + pix];
            const float xh = (hv - p.bn[12 + c]) * p.bn[16 + c];
            const float pre = p.prm[P_G2 + c] * xh + p.prm[P_BE2 + c];
            const float d = pre > 0.f ? s : 0.f;
            dy2[((int64_t)b * 4 + c) * plane + pix] = d;
            bs[c] += d; bs[4 + c] += d * xh;
        }
    }
    // dW3[o][c][t] = sum_p g[o](p) * pad(a2)[c](p + t): one output channel at a time, as in nf_train.hip
#pragma unroll 1
    for (int o = 0; o < 4; ++o) {
        float acc[45];
#pragma unroll
        for (int j = 0; j < 45; ++j) acc[j] = 0.f;
        for (int i = threadIdx.x; i < TS * TS; i += 256) {
            const int r = i / TS, q = i % TS, gy = ty0 + r, gx = tx0 + q;
            if (gy >= H || gx >= W) continue;
            const float gv = gs[o][r + 1][q + 1];
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int yy = gy + t / 3 - 1, xx = gx + t % 3 - 1;
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[c * 9 + t] += gv * a2s[c][r + t / 3][q + t % 3];
                if (yy < 0 || yy >= H || xx < 0 || xx >= W) acc[36 + t] += gv;
            }
        }
        block_sum_store<45>(acc, row + o * 45, red);
    }
    block_sum_store<9>(sm, row + 180, red);
    block_sum_store<8>(bs, row + 189, red);
    block_sum_store<18>(wa, row + 197, red);
}

// backward pass 2 (pointwise): BatchNorm2 backward, conv2d_2 backward, ReLU mask of layer 1.
//   s2 [8] = reduced (sum dy2[4], sum dy2*xhat2[4]);  stat_w = 1/(B H W) with batch statistics, 0 with running statistics (the
//   statistics terms switched off).  Writes dy1 = dL/d(BN1 output).
__global__ void __launch_bounds__(256)
nfs_bwd_conv2_kernel(const float* __restrict__ h1, const float* __restrict__ h2, const float* __restrict__ dy2, const float* __restrict__ prm,
                     const float* __restrict__ bn, const float* __restrict__ s2, float stat_w, float* __restrict__ dy1,
                     float* __restrict__ part, int64_t plane, int64_t npix) {
    __shared__ float red[NB2][4];
    float acc[NB2];
#pragma unroll
    for (int j = 0; j < NB2; ++j) acc[j] = 0.f;
    for (int k = 0; k < 4; ++k) {
        const int64_t g = (int64_t)blockIdx.x * 1024 + k * 256 + threadIdx.x;
        if (g >= npix) break;
        const int64_t b = g / plane, pix = g - b * plane, base = b * 4 * plane + pix;
        float a1[4], pre1[4], xh1[4], dh2[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            xh1[c] = (h1[base + c * plane] - bn[c]) * bn[4 + c];
            pre1[c] = prm[P_G1 + c] * xh1[c] + prm[P_BE1 + c];
            a1[c] = fmaxf(pre1[c], 0.f);
            const float xh2 = (h2[base + c * plane] - bn[12 + c]) * bn[16 + c];
            dh2[c] = prm[P_G2 + c] * bn[16 + c] * (dy2[base + c * plane] - s2[c] * stat_w - xh2 * (s2[4 + c] * stat_w));
        }
#pragma unroll
        for (int o = 0; o < 4; ++o) {
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[o * 4 + c] += dh2[o] * a1[c];
            acc[16 + o] += dh2[o];
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float s = 0.f;
#pragma unroll
            for (int o = 0; o < 4; ++o) s += prm[P_W2 + o * 4 + c] * dh2[o];
            const float d = pre1[c] > 0.f ? s : 0.f;
            dy1[base + c * plane] = d;
            acc[20 + c] += d; acc[24 + c] += d * xh1[c];
        }
    }
    block_sum_store<NB2>(acc, part + (int64_t)blockIdx.x * NB2, red);
}

// backward pass 3: BatchNorm1 backward, conv2d_1 backward; adds conv1^T(d h1) to du planes 0,1 (each pixel is read and written by
// the one thread that owns it).   s1 [8] = reduced (sum dy1[4], sum dy1*xhat1[4]).
__global__ void __launch_bounds__(256)
nfs_bwd_conv1_kernel(SPair p, const float* __restrict__ h1, const float* __restrict__ dy1, const float* __restrict__ s1, float stat_w,
                     float* __restrict__ du, float* __restrict__ part) {
    __shared__ float us[2][HS][HS + 1];
    __shared__ float ds[4][HS][HS + 1];        // d h1 on tile + halo 1 (zero outside the image)
    __shared__ float red[NB3][4];
    const int b = blockIdx.z, ty0 = blockIdx.y * TS, tx0 = blockIdx.x * TS, H = p.H, W = p.W;
    const int64_t plane = (int64_t)H * W;
    const float* ub = p.u + (int64_t)b * 4 * plane;
    const float* h1b = h1 + (int64_t)b * 4 * plane;
    const float* dyb = dy1 + (int64_t)b * 4 * plane;
    for (int i = threadIdx.x; i < HS * HS; i += 256) {
        const int r = i / HS, q = i % HS, gy = ty0 + r - 1, gx = tx0 + q - 1;
        float u0 = 0.f, u1 = 0.f, d[4] = {0.f, 0.f, 0.f, 0.f};
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const int64_t pix = (int64_t)gy * W + gx;
            u0 = ub[pix]; u1 = ub[plane + pix];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float xh = (h1b[c * plane + pix] - p.bn[c]) * p.bn[4 + c];
                d[c] = p.prm[P_G1 + c] * p.bn[4 + c] * (dyb[c * plane + pix] - s1[c] * stat_w - xh * (s1[4 + c] * stat_w));
            }
        }
        us[0][r][q] = u0; us[1][r][q] = u1;
#pragma unroll
        for (int c = 0; c < 4; ++c) ds[c][r][q] = d[c];
    }
    __syncthreads();
    float acc[NB3];
#pragma unroll
    for (int j = 0; j < NB3; ++j) acc[j] = 0.f;
    for (int i = threadIdx.x; i < TS * TS; i += 256) {
        const int r = i / TS, q = i % TS, gy = ty0 + r, gx = tx0 + q;
        if (gy >= H || gx >= W) continue;
        const int64_t pix = (int64_t)gy * W + gx;
        float* dub = du + (int64_t)b * 4 * plane + pix;
        float dv[2] = {dub[0], dub[plane]};
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            const float dc = ds[o][r + 1][q + 1];
            acc[72 + o] += dc;
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int t = 0; t < 9; ++t) {
                    acc[(o * 2 + c) * 9 + t] += dc * us[c][r + t / 3][q + t % 3];
                    dv[c] += p.prm[P_W1 + (o * 2 + c) * 9 + t] * ds[o][r + 2 - t / 3][q + 2 - t % 3];
                }
        }
        dub[0] = dv[0]; dub[plane] = dv[1];
    }
    block_sum_store<NB3>(acc, part + (((int64_t)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * NB3, red);
}

// sums [319] -> the gradient block in the prm layout, d Winv, (d a, d b)
__global__ void __launch_bounds__(320)
nfs_scatter_kernel(const float* __restrict__ sums, float* __restrict__ gprm, float* __restrict__ dwinv, float* __restrict__ dab) {
    constexpr int O2 = NB1, O3 = NB1 + NB2;
    const int i = threadIdx.x;
    if (i < 72) gprm[i] = sums[O3 + i];                             // W1
    else if (i < 76) gprm[i] = sums[O3 + i];                        // B1 (dW1[72] db1[4] are contiguous)
    else if (i < 80) gprm[i] = sums[O2 + 24 + (i - 76)];            // G1
    else if (i < 84) gprm[i] = sums[O2 + 20 + (i - 80)];            // BE1
    else if (i < 104) gprm[i] = sums[O2 + (i - 84)];                // W2, B2
    else if (i < 108) gprm[i] = sums[193 + (i - 104)];              // G2
    else if (i < 112) gprm[i] = sums[189 + (i - 108)];              // BE2
    else if (i < 301) gprm[i] = sums[i - 112];                      // W3, B3, LOGS, SCALE
    else if (i < 317) dwinv[i - 301] = sums[197 + (i - 301)];
    else if (i < 319 && dab) dab[i - 317] = sums[213 + (i - 317)];
}

inline bool bad_shape(int B, int H, int W) { return B <= 0 || H <= 0 || W <= 0; }
inline int n_tiles(int B, int H, int W) { return B * ((H + TS - 1) / TS) * ((W + TS - 1) / TS); }
inline int n_pblocks(int B, int H, int W) { return (int)(((int64_t)B * H * W + 1023) / 1024); }

}  // namespace

extern "C" {

// floats of the `part` scratch of pnnp_nf_sample_bwd_pair_f32 (0 for a bad shape)
int64_t pnnp_nf_sample_bwd_part_floats(int B, int H, int W) {
    if (bad_shape(B, H, W)) return 0;
    const int64_t a = (int64_t)n_tiles(B, H, W) * NB1, b = (int64_t)n_pblocks(B, H, W) * NB2;
    return a > b ? a : b;
}

// VJP of one sample-direction pair (see the top of the file).  All pointers are device pointers.
//   u          the pair's input;  dout: gradient of its output;  du: gradient of its input (must not alias u or dout)
//   clean, ab  SignalDependantISO (last pair) or null;  winv [4][4];  prm [301];  bn [24]
//   bn_batch   1: bn holds the batch statistics of u (training mode), 0: a fixed affine (eval mode)
//   gprm [301] dwinv [16] dab [2] (dab may be null without clean; with clean it is required)
//   scratch: h1, h2, out3, dy2, dy1 [B][4][H][W] each, sums [319], part [pnnp_nf_sample_bwd_part_floats]
int pnnp_nf_sample_bwd_pair_f32(const float* u, const float* clean, const float* ab, const float* winv, const float* prm, const float* bn,
                                int bn_batch, const float* dout, float* du, float* gprm, float* dwinv, float* dab, float* h1, float* h2,
                                float* out3, float* dy2, float* dy1, float* sums, float* part, int B, int H, int W, void* stream) {
    if (bad_shape(B, H, W) || !u || !winv || !prm || !bn || !dout || !du || !gprm || !dwinv || !h1 || !h2 || !out3 || !dy2 || !dy1 || !sums ||
        !part || (clean && (!ab || !dab)) || du == dout || du == u)
        return PNNP_E_INVALID;
    hipStream_t st = as_stream(stream);
    const SPair p{u, clean, ab, winv, prm, bn, H, W};
    const dim3 grid((W + TS - 1) / TS, (H + TS - 1) / TS, B);
    const int tiles = n_tiles(B, H, W), pb = n_pblocks(B, H, W);
    const int64_t plane = (int64_t)H * W, npix = (int64_t)B * plane;
    const float stat_w = bn_batch ? (float)(1.0 / (double)npix) : 0.f;
    hipLaunchKernelGGL(nfs_hidden_kernel, grid, dim3(256), 0, st, p, h1, h2);
    hipLaunchKernelGGL(nfs_out3_kernel, grid, dim3(256), 0, st, p, h2, out3);
    hipLaunchKernelGGL(nfs_bwd_couple_kernel, grid, dim3(256), 0, st, p, h2, out3, dout, dy2, du, part);
    hipLaunchKernelGGL(nfs_colsum_kernel, dim3(NB1), dim3(256), 0, st, part, tiles, NB1, sums);
    hipLaunchKernelGGL(nfs_bwd_conv2_kernel, dim3(pb), dim3(256), 0, st, h1, h2, dy2, prm, bn, sums + 189, stat_w, dy1, part, plane, npix);
    hipLaunchKernelGGL(nfs_colsum_kernel, dim3(NB2), dim3(256), 0, st, part, pb, NB2, sums + NB1);
    hipLaunchKernelGGL(nfs_bwd_conv1_kernel, grid, dim3(256), 0, st, p, h1, dy1, sums + NB1 + 20, stat_w, du, part);
    hipLaunchKernelGGL(nfs_colsum_kernel, dim3(NB3), dim3(256), 0, st, part, tiles, NB3, sums + NB1 + NB2);
    hipLaunchKernelGGL(nfs_scatter_kernel, dim3(1), dim3(320), 0, st, sums, gprm, dwinv, clean ? dab : nullptr);
    return pnnp_launch_status();
}

}  // extern "C"

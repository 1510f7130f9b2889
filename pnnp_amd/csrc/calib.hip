// Dark-frame calibration on the device: the two streaming passes over a bias stack and the row means of a map.
// The estimators built on them are defined in include/pnnp_hip.h and in pnnp_amd/calibrate.py.
//
// Both streaming kernels give one workgroup one sensor row y and one thread 8 consecutive pixels of it (a "group"); a thread walks the
// row's groups g = tid, tid + T, ... and, for each, the chunk's frames, four loads in flight.  The host picks the workgroup size T (a
// multiple of 64, at most 256) that leaves the fewest idle lanes in the row's last round.
//
// accum: one 16-byte load per group and frame.  The 8 sums (uint32) and 8 sums of squares (uint64, one 32 x 32 + 64 multiply-add each)
// stay in registers across the frames and are added to sum / sumsq once: every pixel has one owner, so that needs no atomics.  Per frame
// the even-column and odd-column partial sums are reduced across the wave with shuffles and lane 0 adds them to the row's LDS slots
// [frame][parity]; a row has one workgroup, so rowsum is written with plain stores at the end and is not read.  Everything is integer
// arithmetic: the results do not depend on any order.  A launch takes at most ACC_FRAMES frames (its LDS slots); the host entry loops.
//
// residual: out = (float(v) - ds) - rowoff, two float32 subtractions (this file is built with -ffp-contract=off); ds is read once per
// group, rowoff[f][y][0..1] once per frame, 2 B read and 4 B written per pixel and frame.
//
// The wide path (16-byte accesses) needs W % 8 == 0 and 16-byte aligned arrays; otherwise the same arithmetic runs with element accesses
// and a guard on the row's tail.  Every access is guarded by g < ceil(W / 8) and, on the narrow path, x < W; y is the block index < H.
#include "common.h"

namespace {

constexpr int CAL_MAX_T = 256;
constexpr int ACC_FRAMES = 1024;          // frames per launch: 8 KiB of LDS row slots, per-thread sums below 2^26
constexpr int ACC_FLIGHT = 4;             // frames whose loads are in flight together
constexpr int CAL_MAX_FRAMES = 32768;    // 32768 * 65535 < 2^31: the int32 sum
constexpr int CAL_MAX_W = 65536;          // 32768 * 65535 < 2^31: the int32 row sum of one parity

typedef unsigned long long u64;
typedef u64 u64x2 __attribute__((ext_vector_type(2)));

template <bool VEC>
__device__ __forceinline__ void load8(const uint16_t* p, int x0, int W, unsigned (&v)[8]) {
    if constexpr (VEC) {
        const u32x4 q = *reinterpret_cast<const u32x4*>(p);
#pragma unroll
        for (int j = 0; j < 4; ++j) { v[2 * j] = q[j] & 0xffffu; v[2 * j + 1] = q[j] >> 16; }
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (x0 + j < W) ? (unsigned)p[j] : 0u;
    }
}

template <bool VEC>
__global__ void __launch_bounds__(CAL_MAX_T) calib_accum_kernel(const uint16_t* __restrict__ frames, int n, int H, int W, unsigned* __restrict__ sum,
                                                                u64* __restrict__ sumsq, unsigned* __restrict__ rowsum) {
    __shared__ unsigned rowacc[ACC_FRAMES * 2];
    const int y = blockIdx.x, T = blockDim.x, G = (W + 7) >> 3;
    for (int i = threadIdx.x; i < 2 * n; i += T) rowacc[i] = 0u;
    __syncthreads();
    const int64_t plane = (int64_t)H * W, row = (int64_t)y * W;
    // every lane of a wave runs the same number of rounds, so that the shuffles below always see 64 lanes; a lane beyond the row adds zeros
    const int rounds = (G + T - 1) / T;
    for (int k = 0; k < rounds; ++k) {
        const int g = k * T + threadIdx.x, x0 = g * 8;
        const bool live = g < G;
        unsigned s[8];
        u64 ss[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) { s[j] = 0u; ss[j] = 0ull; }
        const uint16_t* p = frames + row + (live ? x0 : 0);
        for (int f0 = 0; f0 < n; f0 += ACC_FLIGHT) {                // the batch's loads are issued before any of them is used
            unsigned v[ACC_FLIGHT][8];
#pragma unroll
            for (int u = 0; u < ACC_FLIGHT; ++u) {
                if (live && f0 + u < n) load8<VEC>(p + (int64_t)(f0 + u) * plane, x0, W, v[u]);
                else {
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[u][j] = 0u;
                }
            }
#pragma unroll
            for (int u = 0; u < ACC_FLIGHT; ++u) {
#pragma unroll
                for (int j = 0; j < 8; ++j) { s[j] += v[u][j]; ss[j] += (u64)v[u][j] * v[u][j]; }
                unsigned e = (v[u][0] + v[u][2]) + (v[u][4] + v[u][6]), o = (v[u][1] + v[u][3]) + (v[u][5] + v[u][7]);
#pragma unroll
                for (int sft = 32; sft >= 1; sft >>= 1) { e += __shfl_xor(e, sft, 64); o += __shfl_xor(o, sft, 64); }
                if ((threadIdx.x & 63) == 0 && f0 + u < n) { atomicAdd(&rowacc[2 * (f0 + u)], e); atomicAdd(&rowacc[2 * (f0 + u) + 1], o); }
            }
        }
        if (!live) continue;
        if constexpr (VEC) {
            u32x4* ps = reinterpret_cast<u32x4*>(sum + row + x0);
            u32x4 a = ps[0], b = ps[1];
            a[0] += s[0]; a[1] += s[1]; a[2] += s[2]; a[3] += s[3];
            b[0] += s[4]; b[1] += s[5]; b[2] += s[6]; b[3] += s[7];
            ps[0] = a; ps[1] = b;
            u64x2* pq = reinterpret_cast<u64x2*>(sumsq + row + x0);
#pragma unroll
            for (int j = 0; j < 4; ++j) { u64x2 q = pq[j]; q[0] += ss[2 * j]; q[1] += ss[2 * j + 1]; pq[j] = q; }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (x0 + j < W) { sum[row + x0 + j] += s[j]; sumsq[row + x0 + j] += ss[j]; }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * n; i += T) rowsum[((int64_t)(i >> 1) * H + y) * 2 + (i & 1)] = rowacc[i];
}

template <bool VEC>
__global__ void __launch_bounds__(CAL_MAX_T) calib_residual_kernel(const uint16_t* __restrict__ frames, int n, int H, int W, const float* __restrict__ ds,
                                                                   const float* __restrict__ rowoff, float* __restrict__ out) {
    const int y = blockIdx.x, T = blockDim.x, G = (W + 7) >> 3;
    const int64_t plane = (int64_t)H * W, row = (int64_t)y * W;
    for (int g = threadIdx.x; g < G; g += T) {
        const int x0 = g * 8;
        float d[8];
        if constexpr (VEC) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(ds + row + x0), b = *reinterpret_cast<const f32x4*>(ds + row + x0 + 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) { d[j] = a[j]; d[4 + j] = b[j]; }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) d[j] = (x0 + j < W) ? ds[row + x0 + j] : 0.f;
        }
#pragma unroll 4
        for (int f = 0; f < n; ++f) {
            unsigned v[8];
            load8<VEC>(frames + (int64_t)f * plane + row + x0, x0, W, v);
            const float r0 = rowoff[((int64_t)f * H + y) * 2], r1 = rowoff[((int64_t)f * H + y) * 2 + 1];      // x0 is even: pixel j has parity j & 1
            float* po = out + (int64_t)f * plane + row + x0;
            float r[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) r[j] = ((float)v[j] - d[j]) - ((j & 1) ? r1 : r0);
            if constexpr (VEC) {
                f32x4 a, b;
#pragma unroll
                for (int j = 0; j < 4; ++j) { a[j] = r[j]; b[j] = r[4 + j]; }
                reinterpret_cast<f32x4*>(po)[0] = a;
                reinterpret_cast<f32x4*>(po)[1] = b;
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (x0 + j < W) po[j] = r[j];
            }
        }
    }
}

// the mean of a row in float64: thread t adds x = t, t + 256, ... in that order, then the 256 partial sums fold in halves through LDS
__global__ void __launch_bounds__(CAL_MAX_T) calib_rowmean_kernel(const float* __restrict__ map, int H, int W, double* __restrict__ out) {
    __shared__ double part[CAL_MAX_T];
    const int y = blockIdx.x;
    const float* p = map + (int64_t)y * W;
    double acc = 0.0;
    for (int x = threadIdx.x; x < W; x += CAL_MAX_T) acc += (double)p[x];
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int h = CAL_MAX_T / 2; h >= 1; h >>= 1) {
        if ((int)threadIdx.x < h) part[threadIdx.x] += part[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[y] = part[0] / (double)W;
}

// the workgroup size (a multiple of 64) with the fewest idle lanes over the row's rounds; the larger one on a tie
inline int cal_threads(int W) {
    const int G = (W + 7) / 8;
    int best = 64, waste = 1 << 30;
    for (int T = 64; T <= CAL_MAX_T; T += 64) {
        const int w = (G + T - 1) / T * T - G;
        if (w <= waste) { waste = w; best = T; }
    }
    return best;
}

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
inline bool cal_shape(int n, int H, int W) {
    return n >= 1 && n <= CAL_MAX_FRAMES && H >= 2 && W >= 2 && !(H & 1) && !(W & 1) && W <= CAL_MAX_W && H <= (1 << 24);
}

}  // namespace

extern "C" {

int pnnp_calib_accum_u16(const uint16_t* frames, int n, int H, int W, int32_t* sum_i32, int64_t* sumsq_i64, int32_t* rowsum_i32, void* stream) {
    if (!frames || !sum_i32 || !sumsq_i64 || !rowsum_i32 || !cal_shape(n, H, W)) return PNNP_E_INVALID;
    if (!aligned(frames, 2) || !aligned(sum_i32, 4) || !aligned(sumsq_i64, 8) || !aligned(rowsum_i32, 4)) return PNNP_E_INVALID;
    const bool vec = W % 8 == 0 && aligned(frames, 16) && aligned(sum_i32, 16) && aligned(sumsq_i64, 16);
    const dim3 grid((unsigned)H), block((unsigned)cal_threads(W));
    for (int f0 = 0; f0 < n; f0 += ACC_FRAMES) {
        const int m = n - f0 < ACC_FRAMES ? n - f0 : ACC_FRAMES;
        const uint16_t* fr = frames + (int64_t)f0 * H * W;
        unsigned* rs = reinterpret_cast<unsigned*>(rowsum_i32) + (int64_t)f0 * H * 2;
        if (vec) hipLaunchKernelGGL(calib_accum_kernel<true>, grid, block, 0, as_stream(stream), fr, m, H, W, reinterpret_cast<unsigned*>(sum_i32),
                                    reinterpret_cast<u64*>(sumsq_i64), rs);
        else hipLaunchKernelGGL(calib_accum_kernel<false>, grid, block, 0, as_stream(stream), fr, m, H, W, reinterpret_cast<unsigned*>(sum_i32),
                                reinterpret_cast<u64*>(sumsq_i64), rs);
        if (pnnp_launch_status() != PNNP_OK) return PNNP_E_LAUNCH;
    }
    return PNNP_OK;
}

int pnnp_calib_residual_u16(const uint16_t* frames, int n, int H, int W, const float* ds_f32, const float* rowoff_f32, float* out_f32, void* stream) {
    if (!frames || !ds_f32 || !rowoff_f32 || !out_f32 || !cal_shape(n, H, W)) return PNNP_E_INVALID;
    if (!aligned(frames, 2) || !aligned(ds_f32, 4) || !aligned(rowoff_f32, 4) || !aligned(out_f32, 4)) return PNNP_E_INVALID;
    const bool vec = W % 8 == 0 && aligned(frames, 16) && aligned(ds_f32, 16) && aligned(out_f32, 16);
    const dim3 grid((unsigned)H), block((unsigned)cal_threads(W));
    if (vec) hipLaunchKernelGGL(calib_residual_kernel<true>, grid, block, 0, as_stream(stream), frames, n, H, W, ds_f32, rowoff_f32, out_f32);
    else hipLaunchKernelGGL(calib_residual_kernel<false>, grid, block, 0, as_stream(stream), frames, n, H, W, ds_f32, rowoff_f32, out_f32);
    return pnnp_launch_status();
}

int pnnp_calib_rowmean_f32(const float* map, int H, int W, double* out_f64, void* stream) {
    if (!map || !out_f64 || H < 1 || W < 1 || H > (1 << 24) || !aligned(map, 4) || !aligned(out_f64, 8)) return PNNP_E_INVALID;
    hipLaunchKernelGGL(calib_rowmean_kernel, dim3((unsigned)H), dim3(CAL_MAX_T), 0, as_stream(stream), map, H, W, out_f64);
    return pnnp_launch_status();
}

}  // extern "C"

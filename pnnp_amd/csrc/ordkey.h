// Shared by the distribution-loss kernels (ddl.hip, quantile.hip): the float -> ordered unsigned key mapping, the (key, element index) words
// built on it, and the streaming read of an operand that starts at any element and has any length.
#pragma once
#include "common.h"

namespace {

constexpr int DD_THREADS = 1024;
constexpr int DD_WAVES = DD_THREADS / 64;
constexpr int DD_DEPTH = 2;                                    // 16-byte loads in flight per thread

typedef float dd_f4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) const dd_f4 dd_gf4;  // global, not flat: the loads do not count against the LDS operations' lgkmcnt
typedef __attribute__((address_space(1))) const float dd_gf;
typedef unsigned long long dd_u64;

// float -> unsigned that orders like the float (-0.0 first mapped to +0.0), and back
__device__ __forceinline__ unsigned dd_ord(float v) {
    if (v == 0.f) v = 0.f;
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float dd_unord(unsigned o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }
__device__ __forceinline__ dd_u64 dd_minkey(float v, unsigned idx) { return ((dd_u64)dd_ord(v) << 32) | idx; }
__device__ __forceinline__ dd_u64 dd_maxkey(float v, unsigned idx) { return ((dd_u64)dd_ord(v) << 32) | (unsigned)~idx; }
__device__ __forceinline__ float dd_keyval(dd_u64 k) { return dd_unord((unsigned)(k >> 32)); }
__device__ __forceinline__ int dd_minidx(dd_u64 k) { return (int)(unsigned)k; }
__device__ __forceinline__ int dd_maxidx(dd_u64 k) { return (int)~(unsigned)k; }

// elements [0, head) and [head + 4 nq, n) are read one by one, the nq 16-byte words between them as vectors: any start element, any length
struct DdSpan { long long head, nq; };
__device__ __forceinline__ DdSpan dd_span(const float* a, long long n) {
    long long h = (long long)(((16u - (unsigned)((uintptr_t)a & 15u)) & 15u) >> 2);
    if (h > n) h = n;
    return {h, (n - h) >> 2};
}
__device__ __forceinline__ dd_f4 dd_ld4(const float* a, long long e) { return *(dd_gf4*)(a + e); }
__device__ __forceinline__ float dd_ld1(const float* a, long long e) { return *(dd_gf*)(a + e); }

// the operand's blocks (gridDim.x of them, DD_THREADS threads each) share its elements: one(value, element index) for every element, vectors
// DD_DEPTH loads ahead of their use
template <class F>
__device__ __forceinline__ void dd_sweep(const float* a, long long n, F&& one) {
    const DdSpan sp = dd_span(a, n);
    const long long stride = (long long)gridDim.x * DD_THREADS, t0 = (long long)blockIdx.x * DD_THREADS + threadIdx.x;
    auto four = [&](const dd_f4& v, long long e) {
        one(v.x, (unsigned)e); one(v.y, (unsigned)(e + 1)); one(v.z, (unsigned)(e + 2)); one(v.w, (unsigned)(e + 3));
    };
    long long q = t0;
    for (; q + (DD_DEPTH - 1) * stride < sp.nq; q += DD_DEPTH * stride) {
        dd_f4 v[DD_DEPTH];
#pragma unroll
        for (int u = 0; u < DD_DEPTH; ++u) v[u] = dd_ld4(a, sp.head + 4 * (q + u * stride));
#pragma unroll
        for (int u = 0; u < DD_DEPTH; ++u) four(v[u], sp.head + 4 * (q + u * stride));
    }
    for (; q < sp.nq; q += stride) four(dd_ld4(a, sp.head + 4 * q), sp.head + 4 * q);
    const long long nscalar = n - 4 * sp.nq;
    for (long long j = t0; j < nscalar; j += stride) {
        const long long e = j < sp.head ? j : j + 4 * sp.nq;
        one(dd_ld1(a, e), (unsigned)e);
    }
}

__device__ __forceinline__ double dd_wave_sum(double v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}

// block sum in a fixed order; every thread gets the result
__device__ __forceinline__ double dd_block_sum(double v, double* red) {
    v = dd_wave_sum(v);
    __syncthreads();                                           // (red may still be read from the previous sum)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = red[0];
    for (int w = 1; w < DD_WAVES; ++w) s += red[w];
    return s;
}

__device__ __forceinline__ float dd_sign(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

}  // namespace

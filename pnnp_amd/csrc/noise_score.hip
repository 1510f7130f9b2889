// Score of a noise model on the device: what trainer_NF_SID.py:163-174 logs after every epoch -- the integer-DN
// histogram KL divergence of the real and the sampled noise (utils/kld_div.py:163-200, kl_div_norm with bl given) and the population std of
// the two noisy images -- without a copy to the host.
//
// The definition is the reference's, quirks included (tests/test_host_kld.py restates it in numpy against the reference's own outputs):
//   pair mode   inputs = clip(clean, 0, 1);  output = sampled_noise + inputs;  p = rint((real - inputs) s);  q = rint((output - inputs) s)
//               in float32, unfused (this file is built with -ffp-contract=off), s = float32(wp_data - bl_data)       (trainer_NF_SID.py:165-170)
//   DN mode     p, q are given.
//   shift       iff min(p) < 0 with numpy's NaN-propagating min: any NaN in p means no shift, -0.0 is not negative.  Then p += bl, q += bl.
//   key         k = clip(rint(v), 0, wp); +-inf go to the ends; a NaN has no key (it counts in n only).
//   bin         that of float32(k) / float32(wp) against the float64 edges np.arange(0, 1 + 1/wp, 1/wp) under np.histogram's rule.  This is NOT
//               bin k (at wp = 16383 more than half of the keys land elsewhere, and above k = 1024 bins alternately take two keys and none), and it
//               depends on wp alone: the host builds the table key -> bin with numpy itself (metrics._kld_bin_lut) and the finishing kernel folds
//               the raw key counts through it.
//   KL          y = counts / n in float64; over the bins where both are > 0: fwd = sum yp (log yp - log yq), inv = sum yq (log yq - log yp).
//
// Launches per call (behind one memset of the counters), no host round trip:
//   pair mode  ONE pass over the three images.  p and q are integers there, so rint(p + bl) = p + bl exactly and the key with and without
//              the shift both follow from one window index w = clip(p, -bl, wp) + bl in [0, wp + bl]:  shifted key = min(w, wp), unshifted key =
//              max(w - bl, 0).  The pass counts w (2 x 16896 words = 132 KB of the CU's 160 KB LDS), sets the has-negative / has-NaN flags of p
//              (atomicOr) and writes per-block float64 partial sums of (x - x0), (x - x0)^2 for real and output (x0 = the crop's first element:
//              shifted sums keep the variance of an image whose mean is far from zero).  bl must be an integer in [0, 512] for this.
//   DN mode    two passes, because for non-integer inputs rint(x + bl) is not rint(x) + bl: a flags pass over p, then a count pass over p and q
//              that reads the flags from device memory and counts final keys.
//   count      one 1024-thread workgroup per CU holds the two histograms in LDS; every sample is one LDS integer add, except that the lanes
//              which share the key of the wave's first lane add once, with their number (aimed at a constant image or the clipped ends, where a wave's 64
//              adds hit one word; measured only with it: profiles/r7/noise_score.txt).  A workgroup merges into the crop's global histogram with one 32-bit atomic per non-zero word.
//   finish     one workgroup per crop: window -> key by the flags, key -> bin through the table (LDS integer adds), y = count / n, the three KLs
//              and the moments in float64 with a fixed summation order.
// Counts are 32-bit integer atomics only and every float64 sum has a fixed order: results are bitwise reproducible from run to run.
// Loads are global (not flat) 16-byte loads with a scalar head and tail: the arrays may start at any element and have any length.
#include "common.h"

namespace {

constexpr int NS_THREADS = 1024;
constexpr int NS_WAVES = NS_THREADS / 64;
constexpr int NS_RAW = PNNP_NOISE_SCORE_MAX_WP + 1;            // 16384 keys
constexpr int NS_WIN_BL = 512;                                 // pair mode: the window reaches this far below key 0
constexpr int NS_WIN = NS_RAW + NS_WIN_BL;                     // 16896 words per histogram
constexpr int NS_LDS_BYTES = 2 * NS_WIN * (int)sizeof(unsigned);
constexpr unsigned NS_NOKEY = 0xffffffffu;
constexpr int NS_CHUNK = 16384;                                // a block is worth launching for this many elements
constexpr int NS_DEPTH = 2;                                    // 16-byte loads in flight per array and thread (4, and non-temporal loads, measured
                                                               // no faster: profiles/r7/noise_score.txt, part 3)
typedef float ns_f4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) const ns_f4 ns_gf4;  // global, not flat: the loads then do not count against the LDS adds' lgkmcnt
typedef __attribute__((address_space(1))) const float ns_gf;

// elements [0, head) and [head + 4 nq, n) are read one by one, the nq 16-byte words between them as vectors
struct NsSpan { long long head, nq; };
__device__ __forceinline__ NsSpan ns_span(const float* a, long long n, bool vec) {
    if (!vec) return {n, 0};
    long long h = (long long)(((16u - (unsigned)((uintptr_t)a & 15u)) & 15u) >> 2);
    if (h > n) h = n;
    return {h, (n - h) >> 2};
}

// the crop's blocks share its elements: pv(lv(e)) for every aligned vector starting at element e (NS_DEPTH loads ahead of their use),
// fs(e) for every scalar element
template <class LV, class PV, class FS>
__device__ __forceinline__ void ns_sweep(const NsSpan sp, long long n, LV&& lv, PV&& pv, FS&& fs) {
    const long long stride = (long long)gridDim.x * NS_THREADS, t0 = (long long)blockIdx.x * NS_THREADS + threadIdx.x;
    long long q = t0;
    for (; q + (NS_DEPTH - 1) * stride < sp.nq; q += NS_DEPTH * stride) {
        decltype(lv(0LL)) v[NS_DEPTH];
#pragma unroll
        for (int u = 0; u < NS_DEPTH; ++u) v[u] = lv(sp.head + 4 * (q + u * stride));
#pragma unroll
        for (int u = 0; u < NS_DEPTH; ++u) pv(v[u]);
    }
    for (; q < sp.nq; q += stride) pv(lv(sp.head + 4 * q));
    const long long nscalar = n - 4 * sp.nq;
    for (long long j = t0; j < nscalar; j += stride) fs(j < sp.head ? j : j + 4 * sp.nq);
}

__device__ __forceinline__ ns_f4 ns_ld4(const float* a, long long e) { return *(ns_gf4*)(a + e); }
__device__ __forceinline__ float ns_ld1(const float* a, long long e) { return *(ns_gf*)(a + e); }

__device__ __forceinline__ double ns_wave_sum(double v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}

// block sum of K doubles per thread, fixed order; the result is valid in thread 0
template <int K>
__device__ __forceinline__ void ns_block_sum(double (&v)[K], double (*red)[K]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = ns_wave_sum(v[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) red[wave][k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) { double s = red[0][k]; for (int w = 1; w < NS_WAVES; ++w) s += red[w][k]; v[k] = s; }
    }
}

__device__ __forceinline__ unsigned ns_flag_of(float p) { return (p < 0.f ? 1u : 0u) | (p != p ? 2u : 0u); }      // -0.0 < 0 is false

// pair mode, trainer_NF_SID.py:166-170 in float32
struct NsPair { float p, q, out; };
__device__ __forceinline__ NsPair ns_pair(float clean, float real, float noise, float s) {
    const float in = pnnp_clampf(clean, 0.f, 1.f);             // np.clip: a NaN stays a NaN
    const float out = noise + in;
    NsPair r;
    r.out = out;
    r.p = rintf((real - in) * s);                              // np.round: half to even
    r.q = rintf((out - in) * s);                               // (NOT noise * s: the reference adds, then subtracts)
    return r;
}

// kl_div_norm's key of a DN value: (+ bl), round, clip to [0, wp]; NS_NOKEY for a NaN
__device__ __forceinline__ unsigned ns_key(float v, bool shift, float bl, float wp) {
    if (shift) v = v + bl;
    v = pnnp_clampf(rintf(v), 0.f, wp);
    return v == v ? (unsigned)(int)v : NS_NOKEY;
}

// one LDS add per key; the lanes that hold the first active lane's key add once, together
__device__ __forceinline__ void ns_add(unsigned* h, unsigned key) {
    const unsigned lead = (unsigned)__builtin_amdgcn_readfirstlane((int)key);
    const bool mine = key == lead;
    const unsigned long long m = __ballot(mine);
    if (mine) {
        if (key != NS_NOKEY && (int)__lane_id() == __ffsll((long long)m) - 1) atomicAdd(h + key, (unsigned)__popcll(m));
    } else if (key != NS_NOKEY) {
        atomicAdd(h + key, 1u);
    }
}

struct NsV3 { ns_f4 c, r, z; };
__device__ __forceinline__ bool ns_same_word(const float* a, const float* b, const float* c) {
    return (((uintptr_t)a ^ (uintptr_t)b) & 15u) == 0 && (((uintptr_t)a ^ (uintptr_t)c) & 15u) == 0;
}

// pair mode's window index of an integer-valued p or q: clip(v, -bl, wp) + bl; NS_NOKEY for a NaN
__device__ __forceinline__ unsigned ns_wkey(float v, float bl, float wp, int bli) {
    v = pnnp_clampf(v, -bl, wp);
    return v == v ? (unsigned)((int)v + bli) : NS_NOKEY;
}

// pair mode: flags, moments and window counts in one pass
__global__ void __launch_bounds__(NS_THREADS)
ns_pair_kernel(const float* __restrict__ clean, const float* __restrict__ real, const float* __restrict__ noise, long long n, float s, float bl, float wp,
               unsigned* __restrict__ flags, double* __restrict__ part, unsigned* __restrict__ raw) {
    extern __shared__ __attribute__((aligned(16))) unsigned ns_h[];                  // [2][NS_WIN]
    __shared__ double red[NS_WAVES][4];
    for (int i = threadIdx.x; i < 2 * NS_WIN; i += NS_THREADS) ns_h[i] = 0u;
    __syncthreads();
    const int crop = blockIdx.y, bli = (int)bl;
    const float* x0 = clean + (long long)crop * n;
    const float* x1 = real + (long long)crop * n;
    const float* x2 = noise + (long long)crop * n;
    const double kr = (double)ns_ld1(x1, 0), ko = (double)(ns_ld1(x2, 0) + pnnp_clampf(ns_ld1(x0, 0), 0.f, 1.f));
    unsigned f = 0;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    auto one = [&](float c, float r, float z) {
        const NsPair v = ns_pair(c, r, z, s);
        f |= ns_flag_of(v.p);
        const double dr = (double)r - kr, dq = (double)v.out - ko;
        acc[0] += dr; acc[1] += dr * dr; acc[2] += dq; acc[3] += dq * dq;
        ns_add(ns_h, ns_wkey(v.p, bl, wp, bli));
        ns_add(ns_h + NS_WIN, ns_wkey(v.q, bl, wp, bli));
    };
    ns_sweep(ns_span(x0, n, ns_same_word(x0, x1, x2)), n,
             [&](long long e) { return NsV3{ns_ld4(x0, e), ns_ld4(x1, e), ns_ld4(x2, e)}; },
             [&](const NsV3& v) { one(v.c.x, v.r.x, v.z.x); one(v.c.y, v.r.y, v.z.y); one(v.c.z, v.r.z, v.z.z); one(v.c.w, v.r.w, v.z.w); },
             [&](long long e) { one(ns_ld1(x0, e), ns_ld1(x1, e), ns_ld1(x2, e)); });
    const unsigned any = (__syncthreads_or((int)(f & 1u)) ? 1u : 0u) | (__syncthreads_or((int)(f & 2u)) ? 2u : 0u);      // (also: every add is done)
    if (threadIdx.x == 0 && any) atomicOr(flags + crop, any);
    unsigned* g = raw + (long long)crop * 2 * NS_WIN;
    for (int i = threadIdx.x; i < 2 * NS_WIN; i += NS_THREADS) {
        const unsigned v = ns_h[i];
        if (v) atomicAdd(g + i, v);
    }
    ns_block_sum<4>(acc, red);
    if (threadIdx.x == 0) {
        double* o = part + ((long long)crop * gridDim.x + blockIdx.x) * 4;
        o[0] = acc[0]; o[1] = acc[1]; o[2] = acc[2]; o[3] = acc[3];
    }
}

// DN mode, pass 1: the flags of p
__global__ void __launch_bounds__(NS_THREADS)
ns_flags_kernel(const float* __restrict__ p, long long n, unsigned* __restrict__ flags) {
    const int crop = blockIdx.y;
    const float* x = p + (long long)crop * n;
    unsigned f = 0;
    ns_sweep(ns_span(x, n, true), n,
             [&](long long e) { return ns_ld4(x, e); },
             [&](const ns_f4& v) { f |= ns_flag_of(v.x) | ns_flag_of(v.y) | ns_flag_of(v.z) | ns_flag_of(v.w); },
             [&](long long e) { f |= ns_flag_of(ns_ld1(x, e)); });
    const unsigned any = (__syncthreads_or((int)(f & 1u)) ? 1u : 0u) | (__syncthreads_or((int)(f & 2u)) ? 2u : 0u);
    if (threadIdx.x == 0 && any) atomicOr(flags + crop, any);
}

// DN mode, pass 2: final keys
__global__ void __launch_bounds__(NS_THREADS)
ns_count_kernel(const float* __restrict__ p, const float* __restrict__ q, long long n, float bl, float wp, const unsigned* __restrict__ flags,
                unsigned* __restrict__ raw) {
    extern __shared__ __attribute__((aligned(16))) unsigned ns_h[];                  // [2][NS_WIN], the first NS_RAW words of each used
    for (int i = threadIdx.x; i < 2 * NS_WIN; i += NS_THREADS) ns_h[i] = 0u;
    const int crop = blockIdx.y;
    const bool shift = (flags[crop] & 3u) == 1u;               // some p < 0 and no NaN in p (flags kernel, same stream)
    __syncthreads();
    for (int which = 0; which < 2; ++which) {                  // p and q may start at different offsets inside a 16-byte word: one sweep each
        const float* x = (which ? q : p) + (long long)crop * n;
        unsigned* h = ns_h + which * NS_WIN;
        auto one = [&](float v) { ns_add(h, ns_key(v, shift, bl, wp)); };
        ns_sweep(ns_span(x, n, true), n,
                 [&](long long e) { return ns_ld4(x, e); },
                 [&](const ns_f4& v) { one(v.x); one(v.y); one(v.z); one(v.w); },
                 [&](long long e) { one(ns_ld1(x, e)); });
    }
    __syncthreads();
    unsigned* g = raw + (long long)crop * 2 * NS_WIN;
    for (int i = threadIdx.x; i < 2 * NS_WIN; i += NS_THREADS) {
        const unsigned v = ns_h[i];
        if (v) atomicAdd(g + i, v);
    }
}

// the yardstick of tools/noise_score_bench.py: the same grid, the same loads of the same three images, and nothing else (one word per block out)
__global__ void __launch_bounds__(NS_THREADS)
ns_read_kernel(const float* __restrict__ a0, const float* __restrict__ a1, const float* __restrict__ a2, long long n, unsigned* __restrict__ out) {
    const int crop = blockIdx.y;
    const float* x0 = a0 + (long long)crop * n;
    const float* x1 = a1 + (long long)crop * n;
    const float* x2 = a2 + (long long)crop * n;
    unsigned acc = 0;
    auto one = [&](ns_f4 v) { acc ^= __float_as_uint(v.x) ^ __float_as_uint(v.y) ^ __float_as_uint(v.z) ^ __float_as_uint(v.w); };
    ns_sweep(ns_span(x0, n, ns_same_word(x0, x1, x2)), n,
             [&](long long e) { return NsV3{ns_ld4(x0, e), ns_ld4(x1, e), ns_ld4(x2, e)}; },
             [&](const NsV3& v) { one(v.c); one(v.r); one(v.z); },
             [&](long long e) { acc ^= __float_as_uint(ns_ld1(x0, e)) ^ __float_as_uint(ns_ld1(x1, e)) ^ __float_as_uint(ns_ld1(x2, e)); });
#pragma unroll
    for (int sft = 32; sft >= 1; sft >>= 1) acc ^= (unsigned)__shfl_xor((int)acc, sft, 64);
    __shared__ unsigned red[NS_WAVES];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < NS_WAVES; ++w) acc ^= red[w];
        out[(long long)crop * gridDim.x + blockIdx.x] = acc;
    }
}

// one workgroup per crop
__global__ void __launch_bounds__(NS_THREADS)
ns_finish_kernel(const unsigned* __restrict__ raw, const unsigned* __restrict__ flags, const int* __restrict__ lut, int nbins, int wp, int win_bl,
                 long long n, const double* __restrict__ part, int nblk, double* __restrict__ hist, double* __restrict__ result) {
    extern __shared__ __attribute__((aligned(16))) unsigned ns_h[];                  // [2][NS_RAW] binned counts
    __shared__ double red[NS_WAVES][2];
    const int crop = blockIdx.x;
    for (int i = threadIdx.x; i < 2 * NS_RAW; i += NS_THREADS) ns_h[i] = 0u;
    __syncthreads();
    const unsigned* g = raw + (long long)crop * 2 * NS_WIN;
    const bool pair = win_bl >= 0, shift = (flags[crop] & 3u) == 1u;
    for (int w = threadIdx.x; w <= wp + (pair ? win_bl : 0); w += NS_THREADS) {
        const int k = !pair ? w : (shift ? (w < wp ? w : wp) : (w > win_bl ? w - win_bl : 0));      // pair mode counted window indices
        const int b = lut[k];
        if (b < 0 || b >= nbins) continue;                     // -1: beyond the last edge, in no bin
        const unsigned cp = g[w], cq = g[NS_WIN + w];
        if (cp) atomicAdd(ns_h + b, cp);
        if (cq) atomicAdd(ns_h + NS_RAW + b, cq);
    }
    __syncthreads();
    const double dn = (double)n;
    double* yp_out = hist + (long long)crop * 2 * nbins;
    double* yq_out = yp_out + nbins;
    double kl[2] = {0.0, 0.0};
    for (int i = threadIdx.x; i < nbins; i += NS_THREADS) {
        const unsigned cp = ns_h[i], cq = ns_h[NS_RAW + i];
        const double yp = (double)cp / dn, yq = (double)cq / dn;
        yp_out[i] = yp; yq_out[i] = yq;
        if (cp && cq) {
            const double lp = log(yp), lq = log(yq);
            kl[0] += yp * (lp - lq);
            kl[1] += yq * (lq - lp);
        }
    }
    ns_block_sum<2>(kl, red);
    if (threadIdx.x == 0) {
        double* r = result + (long long)crop * PNNP_NOISE_SCORE_ROW;
        r[0] = kl[0]; r[1] = kl[1]; r[2] = (kl[0] + kl[1]) / 2.0;
        double gt = 0.0, out = 0.0, diff = 0.0;
        if (pair) {
            double s[4] = {0.0, 0.0, 0.0, 0.0};
            const double* p = part + (long long)crop * nblk * 4;
            for (int b = 0; b < nblk; ++b) { s[0] += p[4 * b]; s[1] += p[4 * b + 1]; s[2] += p[4 * b + 2]; s[3] += p[4 * b + 3]; }
            double vr = (s[1] - s[0] * s[0] / dn) / dn, vo = (s[3] - s[2] * s[2] / dn) / dn;
            vr = vr < 0.0 ? 0.0 : vr; vo = vo < 0.0 ? 0.0 : vo;                      // (a NaN falls through)
            gt = sqrt(vr); out = sqrt(vo);
            diff = 100.0 * (gt - out) / gt;
        }
        r[3] = gt; r[4] = out; r[5] = diff; r[6] = (double)(flags[crop] & 3u); r[7] = 0.0;
    }
}

int ns_blocks(int ncrops, int64_t n) {
    int cus = pnnp_device_cus();
    if (cus < 1) cus = 256;
    int64_t cap = cus / ncrops;                                // one 132 KB workgroup per CU
    if (cap < 1) cap = 1;
    int64_t want = (n + NS_CHUNK - 1) / NS_CHUNK;
    if (want < 1) want = 1;
    return (int)(want < cap ? want : cap);
}

int64_t ns_flag_bytes(int ncrops) { return (((int64_t)ncrops * 4 + 255) / 256) * 256; }
int64_t ns_head_bytes(int ncrops) { return ns_flag_bytes(ncrops) + (int64_t)ncrops * 2 * NS_WIN * 4; }      // flags, counts: zeroed per call

int ns_check(int ncrops, int64_t n, float bl, int wp, const int* lut, int nbins, void* ws, double* hist, double* result) {
    if (ncrops <= 0 || ncrops > 65535 || n <= 0 || wp < 1 || !lut || nbins < 1 || !ws || !hist || !result || !(bl == bl) || (((uintptr_t)ws) & 15))
        return PNNP_E_INVALID;
    if (n >= ((int64_t)1 << 32) || wp > PNNP_NOISE_SCORE_MAX_WP || nbins > NS_RAW) return PNNP_E_UNSUPPORTED;
    return PNNP_OK;
}

PnnpPerDevice ns_lds_pair, ns_lds_count, ns_lds_finish;

int ns_run(const float* a0, const float* a1, const float* a2, int ncrops, int64_t n, float s, float bl, int wp, const int* lut, int nbins,
           void* ws, double* hist, double* result, void* stream) {
    const bool pair = a2 != nullptr;
    const int rc = ns_check(ncrops, n, bl, wp, lut, nbins, ws, hist, result);
    if (rc != PNNP_OK) return rc;
    if (!a0 || !a1 || (((uintptr_t)a0 | (uintptr_t)a1 | (uintptr_t)a2) & 3)) return PNNP_E_INVALID;
    if (pair && !(bl >= 0.f && bl <= (float)NS_WIN_BL && bl == (float)(int)bl)) return PNNP_E_UNSUPPORTED;      // the one-pass window
    if (pnnp_allow_lds(ns_lds_pair, ns_pair_kernel, NS_LDS_BYTES) != PNNP_OK || pnnp_allow_lds(ns_lds_count, ns_count_kernel, NS_LDS_BYTES) != PNNP_OK ||
        pnnp_allow_lds(ns_lds_finish, ns_finish_kernel, NS_LDS_BYTES) != PNNP_OK) return PNNP_E_LAUNCH;
    const int nblk = ns_blocks(ncrops, n);
    unsigned* flags = (unsigned*)ws;
    unsigned* raw = (unsigned*)((char*)ws + ns_flag_bytes(ncrops));
    double* part = (double*)((char*)ws + ns_head_bytes(ncrops));
    if (hipMemsetAsync(ws, 0, (size_t)ns_head_bytes(ncrops), as_stream(stream)) != hipSuccess) return PNNP_E_LAUNCH;
    const dim3 grid(nblk, ncrops);
    if (pair) {
        hipLaunchKernelGGL(ns_pair_kernel, grid, dim3(NS_THREADS), NS_LDS_BYTES, as_stream(stream), a0, a1, a2, (long long)n, s, bl, (float)wp, flags, part, raw);
    } else {
        hipLaunchKernelGGL(ns_flags_kernel, grid, dim3(NS_THREADS), 0, as_stream(stream), a0, (long long)n, flags);
        hipLaunchKernelGGL(ns_count_kernel, grid, dim3(NS_THREADS), NS_LDS_BYTES, as_stream(stream), a0, a1, (long long)n, bl, (float)wp,
                           (const unsigned*)flags, raw);
    }
    hipLaunchKernelGGL(ns_finish_kernel, dim3(ncrops), dim3(NS_THREADS), NS_LDS_BYTES, as_stream(stream), (const unsigned*)raw, (const unsigned*)flags, lut, nbins, wp,
                       pair ? (int)bl : -1, (long long)n, (const double*)part, nblk, hist, result);
    return pnnp_launch_status();
}

}  // namespace

extern "C" {

int64_t pnnp_noise_score_ws_bytes(int ncrops, int64_t n) {
    if (ncrops <= 0 || ncrops > 65535 || n <= 0) return PNNP_E_INVALID;
    return ns_head_bytes(ncrops) + (int64_t)ncrops * ns_blocks(ncrops, n) * 4 * (int64_t)sizeof(double);
}

int pnnp_kl_div_norm_f32(const float* p, const float* q, int ncrops, int64_t n, float bl, int wp, const int* lut, int nbins,
                         void* ws, double* hist, double* result, void* stream) {
    return ns_run(p, q, nullptr, ncrops, n, 0.f, bl, wp, lut, nbins, ws, hist, result, stream);
}

int pnnp_noise_score_f32(const float* clean, const float* real, const float* sampled_noise, int ncrops, int64_t n, float s, float bl, int wp,
                         const int* lut, int nbins, void* ws, double* hist, double* result, void* stream) {
    if (!(s == s) || !sampled_noise) return PNNP_E_INVALID;
    return ns_run(clean, real, sampled_noise, ncrops, n, s, bl, wp, lut, nbins, ws, hist, result, stream);
}

// Measurement aid of tools/noise_score_bench.py, NOT part of the C ABI (include/pnnp_hip.h does not declare it): read the three images with the
// score's grid and loads, and nothing else.  out: one word per block, at least ncrops * 256 words.
int pnnp_noise_score_read_f32(const float* clean, const float* real, const float* sampled_noise, int ncrops, int64_t n, unsigned* out, void* stream) {
    if (!clean || !real || !sampled_noise || !out || ncrops <= 0 || ncrops > 65535 || n <= 0 || n >= ((int64_t)1 << 32) ||
        (((uintptr_t)clean | (uintptr_t)real | (uintptr_t)sampled_noise) & 3)) return PNNP_E_INVALID;
    hipLaunchKernelGGL(ns_read_kernel, dim3(ns_blocks(ncrops, n), ncrops), dim3(NS_THREADS), 0, as_stream(stream), clean, real, sampled_noise,
                       (long long)n, out);
    return pnnp_launch_status();
}

}  // extern "C"

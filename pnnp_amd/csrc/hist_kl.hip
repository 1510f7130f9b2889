// Histogram KL over caller-given float edges on the device: what utils/kld_div.py:100-161 and :202-210
// compute with np.histogram -- get_histogram, kl_div_3_data -- and the bl=None branch of kl_div_norm (:166-169), without a copy to the host.
//
// The definition is the reference's, i.e. np.histogram's for an array of edges e[0..nb] (tests/_kl_data_np.py restates it in numpy against the
// reference's own outputs):
//   bin      the largest i in [0, nb - 1] with e[i] <= x, for e[0] <= x <= e[nb]: half-open bins, the last one closed, equal neighbours give an
//            empty bin.  x < e[0], x > e[nb] and NaN are in no bin and count in n only.  The comparison is exact: a float32 sample is widened
//            to float64 and compared with the float64 edge (float32 arithmetic puts 489 of the 1001 values float32(k / 1000) in the wrong bin).
//   search   with a hint (e0, scale = nb / (e[nb] - e0), given by the host when the edges came from arange): the guess int((x - e0) scale),
//            clamped, then moved down while e[g] > x and up while e[g + 1] <= x -- until the rule holds, however far that is.  Without one
//            (scale = 0): a branch-free binary search over e[0..nb - 1].
//   y        counts / n in float64, each array by its own n.
//   KL       over the bins where both are > 0: fwd = sum yp (log yp - log yq), inv = sum yq (log yq - log yp), sym = (fwd + inv) / 2.
//
// Launches per call (behind one memset of the counters), no host round trip:
//   count    one 1024-thread workgroup per CU holds the crop's two histograms in LDS, and the edge table too up to HK_LDS_EDGES_NB bins (beyond
//            it the table is read from global memory: 131 KB at 16384 bins, L2-resident).  Every sample is one LDS integer add, except that
//            the lanes which share the key of the wave's first lane add once, with their number (the catch-all bins).  A workgroup merges into
//            the crop's global histogram with one 32-bit atomic per non-zero word.
//   finish   one workgroup per crop: y and the three KLs in float64 with a fixed summation order.
// Counts are 32-bit integer atomics only and every float64 sum has a fixed order: results are bitwise reproducible from run to run.
// Loads are global (not flat) 16-byte loads with a scalar head and tail: the arrays may start at any element and have any length.
//
// The range pass (pnnp_minmax_f) serves the bl=None port: min and max of the finite samples of p and q through 64-bit integer atomics on
// order-preserving keys (min and max do not depend on the order: deterministic), and a flag for a NaN or an inf.
#include "common.h"

namespace {

constexpr int HK_THREADS = 1024;
constexpr int HK_WAVES = HK_THREADS / 64;
constexpr int HK_MAX_NB = PNNP_HIST_EDGES_MAX_BINS;            // 16384
constexpr int HK_LDS_EDGES_NB = 10000;                         // up to here the edges live in LDS beside the histograms: 16 nb + 16 <= 160 016 bytes
constexpr int HK_CHUNK = 16384;                                // a block is worth launching for this many elements
constexpr int HK_DEPTH = 2;                                    // 16-byte loads in flight per thread
constexpr unsigned HK_NOKEY = 0xffffffffu;
typedef unsigned long long hk_u64;
typedef __attribute__((address_space(1))) const double hk_gd;

__host__ __device__ constexpr int hk_edge_slots(int nb) { return (nb + 2) & ~1; }      // nb + 1 doubles, the histograms behind them stay 16-byte aligned

// the crop's blocks share its elements: one(x) for every element; elements before the first and after the last whole 16-byte word are read
// one by one, the words between them as vectors, HK_DEPTH loads ahead of their use.  `a` is aligned to its element size.
template <class T, class F>
__device__ __forceinline__ void hk_sweep(const T* a, long long n, F&& one) {
    constexpr int N = 16 / (int)sizeof(T);
    typedef T V __attribute__((ext_vector_type(N)));
    typedef __attribute__((address_space(1))) const V GV;
    typedef __attribute__((address_space(1))) const T GT;
    long long head = (long long)(((16u - (unsigned)((uintptr_t)a & 15u)) & 15u) / (unsigned)sizeof(T));
    if (head > n) head = n;
    const long long nv = (n - head) / N;
    const long long stride = (long long)gridDim.x * HK_THREADS, t0 = (long long)blockIdx.x * HK_THREADS + threadIdx.x;
    long long q = t0;
    for (; q + (HK_DEPTH - 1) * stride < nv; q += HK_DEPTH * stride) {
        V v[HK_DEPTH];
#pragma unroll
        for (int u = 0; u < HK_DEPTH; ++u) v[u] = *(GV*)(a + head + N * (q + u * stride));
#pragma unroll
        for (int u = 0; u < HK_DEPTH; ++u) {
#pragma unroll
            for (int j = 0; j < N; ++j) one(v[u][j]);
        }
    }
    for (; q < nv; q += stride) {
        const V v = *(GV*)(a + head + N * q);
#pragma unroll
        for (int j = 0; j < N; ++j) one(v[j]);
    }
    const long long nscalar = n - N * nv;
    for (long long j = t0; j < nscalar; j += stride) one(*(GT*)(a + (j < head ? j : j + N * nv)));
}

// one LDS add per key; the lanes that hold the first active lane's key add once, together
__device__ __forceinline__ void hk_add(unsigned* h, unsigned key) {
    const unsigned lead = (unsigned)__builtin_amdgcn_readfirstlane((int)key);
    const bool mine = key == lead;
    const unsigned long long m = __ballot(mine);
    if (mine) {
        if (key != HK_NOKEY && (int)__lane_id() == __ffsll((long long)m) - 1) atomicAdd(h + key, (unsigned)__popcll(m));
    } else if (key != HK_NOKEY) {
        atomicAdd(h + key, 1u);
    }
}

__device__ __forceinline__ double hk_wave_sum(double v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}

// LDS_E: the edge table is in LDS (nb <= HK_LDS_EDGES_NB), else in global memory
template <class T, bool LDS_E>
__global__ void __launch_bounds__(HK_THREADS)
hk_count_kernel(const T* __restrict__ p, const T* __restrict__ q, long long n_p, long long n_q, const double* __restrict__ edges, int nb,
                double h0, double hs, unsigned* __restrict__ raw) {
    extern __shared__ __attribute__((aligned(16))) unsigned char hk_lds[];           // LDS_E: [hk_edge_slots(nb)] doubles; then [2][nb] counts
    double* se = (double*)hk_lds;
    unsigned* sh = (unsigned*)(hk_lds + (LDS_E ? (size_t)hk_edge_slots(nb) * sizeof(double) : 0));
    const int nh = q ? 2 * nb : nb;
    for (int i = threadIdx.x; i < nh; i += HK_THREADS) sh[i] = 0u;
    if (LDS_E) {
        for (int i = threadIdx.x; i <= nb; i += HK_THREADS) se[i] = edges[i];
    }
    __syncthreads();
    auto edge = [&](int i) -> double {                         // i in [0, nb]
        if constexpr (LDS_E) return se[i];
        else return *(hk_gd*)(edges + i);
    };
    const double e0 = edge(0), elast = edge(nb);
    int top = 1;
    while (2 * top <= nb - 1) top *= 2;                        // the largest power of two <= max(nb - 1, 1)
    const int crop = blockIdx.y;
    for (int which = 0; which < (q ? 2 : 1); ++which) {        // p and q may have different lengths and alignments: one sweep each
        const long long n = which ? n_q : n_p;
        const T* x = (which ? q : p) + (long long)crop * n;
        unsigned* h = sh + which * nb;
        auto one = [&](T xv) {
            const double v = (double)xv;                       // exact
            unsigned key = HK_NOKEY;
            if (v >= e0 && v <= elast) {                       // (a NaN fails both)
                int g;
                if (hs > 0.0) {
                    const double t = (v - e0) * hs;            // >= 0
                    g = !(t < (double)(nb - 1)) ? nb - 1 : (int)t;
                    while (g > 0 && edge(g) > v) --g;          // now e[g] <= v (e[0] <= v)
                    while (g < nb - 1 && edge(g + 1) <= v) ++g;
                } else {
                    g = 0;                                     // e[0] <= v; the largest g in [0, nb - 1] with e[g] <= v
                    for (int s = top; s > 0; s >>= 1) {
                        const int c = g + s;
                        if (c < nb && edge(c) <= v) g = c;
                    }
                }
                key = (unsigned)g;
            }
            hk_add(h, key);
        };
        hk_sweep<T>(x, n, one);
    }
    __syncthreads();
    unsigned* g = raw + (long long)crop * 2 * nb;
    for (int i = threadIdx.x; i < nh; i += HK_THREADS) {
        const unsigned v = sh[i];
        if (v) atomicAdd(g + i, v);
    }
}

// one workgroup per crop.  two = 1: hist [crop][2][nb], kl [crop][3]; two = 0: hist [crop][nb], kl untouched
__global__ void __launch_bounds__(HK_THREADS)
hk_finish_kernel(const unsigned* __restrict__ raw, int nb, long long n_p, long long n_q, int two, double* __restrict__ hist, double* __restrict__ kl) {
    __shared__ double red[HK_WAVES][2];
    const int crop = blockIdx.x;
    const unsigned* g = raw + (long long)crop * 2 * nb;
    const double dp = (double)n_p, dq = (double)n_q;
    double* yp_out = hist + (long long)crop * (two ? 2 : 1) * nb;
    double* yq_out = yp_out + nb;
    double s0 = 0.0, s1 = 0.0;
    for (int i = threadIdx.x; i < nb; i += HK_THREADS) {
        const unsigned cp = g[i];
        const double yp = (double)cp / dp;
        yp_out[i] = yp;
        if (two) {
            const unsigned cq = g[nb + i];
            const double yq = (double)cq / dq;
            yq_out[i] = yq;
            if (cp && cq) {
                const double lp = log(yp), lq = log(yq);
                s0 += yp * (lp - lq);
                s1 += yq * (lq - lp);
            }
        }
    }
    if (!two) return;
    s0 = hk_wave_sum(s0); s1 = hk_wave_sum(s1);
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = s0; red[threadIdx.x >> 6][1] = s1; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double f = red[0][0], v = red[0][1];
        for (int w = 1; w < HK_WAVES; ++w) { f += red[w][0]; v += red[w][1]; }
        double* r = kl + (long long)crop * 3;
        r[0] = f; r[1] = v; r[2] = (f + v) / 2.0;
    }
}

// ---- range pass: double -> unsigned that orders like the double (-0.0 first mapped to +0.0), and back
__device__ __forceinline__ hk_u64 hk_ord(double v) {
    if (v == 0.0) v = 0.0;
    const hk_u64 u = (hk_u64)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double hk_unord(hk_u64 o) {
    return __longlong_as_double((long long)((o >> 63) ? (o & 0x7fffffffffffffffull) : ~o));
}

// out as keys: [0] min p, [1] max p, [2] min q, [3] max q, [4] flag
__global__ void hk_range_init_kernel(hk_u64* out) {
    if (threadIdx.x < 5) out[threadIdx.x] = (threadIdx.x == 0 || threadIdx.x == 2) ? ~0ull : 0ull;
}

template <class T>
__global__ void __launch_bounds__(HK_THREADS)
hk_range_kernel(const T* __restrict__ p, const T* __restrict__ q, long long n_p, long long n_q, hk_u64* __restrict__ out) {
    __shared__ hk_u64 red[HK_WAVES][2];
    const int which = blockIdx.y;
    const T* x = which ? q : p;
    const long long n = which ? n_q : n_p;
    hk_u64 lo = ~0ull, hi = 0ull;
    int bad = 0;
    hk_sweep<T>(x, n, [&](T xv) {
        const double v = (double)xv;
        if (fabs(v) < __builtin_huge_val()) {                  // finite
            const hk_u64 k = hk_ord(v);
            lo = k < lo ? k : lo; hi = k > hi ? k : hi;
        } else {
            bad = 1;                                           // NaN or +-inf
        }
    });
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const hk_u64 a = (hk_u64)__shfl_xor((long long)lo, s, 64), b = (hk_u64)__shfl_xor((long long)hi, s, 64);
        lo = a < lo ? a : lo; hi = b > hi ? b : hi;
    }
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = lo; red[threadIdx.x >> 6][1] = hi; }
    const int any_bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) {
        for (int w = 1; w < HK_WAVES; ++w) { lo = red[w][0] < lo ? red[w][0] : lo; hi = red[w][1] > hi ? red[w][1] : hi; }
        if (lo != ~0ull) { atomicMin(out + 2 * which, lo); atomicMax(out + 2 * which + 1, hi); }
        if (any_bad) atomicOr(out + 4, 1ull);
    }
}

// keys -> doubles in place: min p, max p, min q, max q (p's without a q), flag (1.0: a NaN or an inf), 0
__global__ void hk_range_fin_kernel(hk_u64* out, int has_q) {
    if (threadIdx.x != 0) return;
    double* d = (double*)out;
    hk_u64 k[4] = {out[0], out[1], out[2], out[3]};
    if (!has_q) { k[2] = k[0]; k[3] = k[1]; }
    const double flag = out[4] ? 1.0 : 0.0;
    for (int i = 0; i < 4; ++i) d[i] = hk_unord(k[i]);         // (a set with no finite sample leaves NaNs here: the flag is set then)
    d[4] = flag; d[5] = 0.0;
}

int hk_blocks(int ncrops, int64_t n) {
    int cus = pnnp_device_cus();
    if (cus < 1) cus = 256;
    int64_t cap = cus / ncrops;                                // one workgroup per CU
    if (cap < 1) cap = 1;
    int64_t want = (n + HK_CHUNK - 1) / HK_CHUNK;
    if (want < 1) want = 1;
    return (int)(want < cap ? want : cap);
}

int64_t hk_ws_bytes(int ncrops, int nbins) { return (((int64_t)ncrops * 2 * nbins * 4 + 255) / 256) * 256; }

constexpr int HK_LDS_MAX_E = hk_edge_slots(HK_LDS_EDGES_NB) * 8 + 2 * HK_LDS_EDGES_NB * 4;      // 160 016
constexpr int HK_LDS_MAX_G = 2 * HK_MAX_NB * 4;                                                 // 131 072
PnnpPerDevice hk_lds_once[4];

template <class T, bool LDS_E>
int hk_launch_count(PnnpPerDevice& once, const void* p, const void* q, int ncrops, int64_t n_p, int64_t n_q, const double* edges, int nb,
                    double h0, double hs, unsigned* raw, void* stream) {
    // the limit is raised once per device, so to the variant's largest request
    if (pnnp_allow_lds(once, hk_count_kernel<T, LDS_E>, LDS_E ? HK_LDS_MAX_E : HK_LDS_MAX_G) != PNNP_OK) return PNNP_E_LAUNCH;
    const int lds = (LDS_E ? hk_edge_slots(nb) * 8 : 0) + 2 * nb * 4;
    const dim3 grid(hk_blocks(ncrops, n_p > n_q ? n_p : n_q), ncrops);
    hipLaunchKernelGGL((hk_count_kernel<T, LDS_E>), grid, dim3(HK_THREADS), lds, as_stream(stream), (const T*)p, (const T*)q, (long long)n_p,
                       (long long)n_q, edges, nb, h0, hs, raw);
    return PNNP_OK;
}

}  // namespace

extern "C" {

int64_t pnnp_hist_edges_ws_bytes(int ncrops, int nbins) {
    if (ncrops <= 0 || ncrops > 65535 || nbins < 1) return PNNP_E_INVALID;
    if (nbins > HK_MAX_NB) return PNNP_E_UNSUPPORTED;
    return hk_ws_bytes(ncrops, nbins);
}

int pnnp_hist_edges_f64(const void* p, const void* q, int elem_f64, int ncrops, int64_t n_p, int64_t n_q, const double* edges, int nbins,
                        double hint_e0, double hint_scale, void* ws, double* hist, double* kl, void* stream) {
    const uintptr_t amask = elem_f64 ? 7u : 3u;
    if (!p || (elem_f64 != 0 && elem_f64 != 1) || ncrops <= 0 || ncrops > 65535 || n_p <= 0 || (q && n_q <= 0) || !edges || nbins < 1 || !ws ||
        !hist || (q && !kl) || (((uintptr_t)p | (uintptr_t)q) & amask) || (((uintptr_t)ws) & 15) || (((uintptr_t)edges | (uintptr_t)hist | (uintptr_t)kl) & 7))
        return PNNP_E_INVALID;
    if (hint_scale != 0.0 && !(hint_scale > 0.0 && hint_scale < __builtin_huge_val() && hint_e0 == hint_e0)) return PNNP_E_INVALID;
    if (!q) n_q = 0;
    if (nbins > HK_MAX_NB || n_p >= ((int64_t)1 << 32) || n_q >= ((int64_t)1 << 32)) return PNNP_E_UNSUPPORTED;
    if (hipMemsetAsync(ws, 0, (size_t)hk_ws_bytes(ncrops, nbins), as_stream(stream)) != hipSuccess) return PNNP_E_LAUNCH;
    unsigned* raw = (unsigned*)ws;
    const bool lds_e = nbins <= HK_LDS_EDGES_NB;
    int rc;
    if (elem_f64) rc = lds_e ? hk_launch_count<double, true>(hk_lds_once[0], p, q, ncrops, n_p, n_q, edges, nbins, hint_e0, hint_scale, raw, stream)
                             : hk_launch_count<double, false>(hk_lds_once[1], p, q, ncrops, n_p, n_q, edges, nbins, hint_e0, hint_scale, raw, stream);
    else rc = lds_e ? hk_launch_count<float, true>(hk_lds_once[2], p, q, ncrops, n_p, n_q, edges, nbins, hint_e0, hint_scale, raw, stream)
                    : hk_launch_count<float, false>(hk_lds_once[3], p, q, ncrops, n_p, n_q, edges, nbins, hint_e0, hint_scale, raw, stream);
    if (rc != PNNP_OK) return rc;
    hipLaunchKernelGGL(hk_finish_kernel, dim3(ncrops), dim3(HK_THREADS), 0, as_stream(stream), (const unsigned*)raw, nbins, (long long)n_p,
                       (long long)n_q, q ? 1 : 0, hist, kl);
    return pnnp_launch_status();
}

int pnnp_minmax_f(const void* p, const void* q, int elem_f64, int64_t n_p, int64_t n_q, void* out, void* stream) {
    const uintptr_t amask = elem_f64 ? 7u : 3u;
    if (!p || (elem_f64 != 0 && elem_f64 != 1) || n_p <= 0 || (q && n_q <= 0) || !out || (((uintptr_t)p | (uintptr_t)q) & amask) ||
        (((uintptr_t)out) & 7)) return PNNP_E_INVALID;
    if (!q) n_q = 0;
    if (n_p >= ((int64_t)1 << 32) || n_q >= ((int64_t)1 << 32)) return PNNP_E_UNSUPPORTED;
    hk_u64* keys = (hk_u64*)out;
    hipLaunchKernelGGL(hk_range_init_kernel, dim3(1), dim3(64), 0, as_stream(stream), keys);
    const dim3 grid(hk_blocks(q ? 2 : 1, n_p > n_q ? n_p : n_q), q ? 2 : 1);
    if (elem_f64) hipLaunchKernelGGL(hk_range_kernel<double>, grid, dim3(HK_THREADS), 0, as_stream(stream), (const double*)p, (const double*)q,
                                     (long long)n_p, (long long)n_q, keys);
    else hipLaunchKernelGGL(hk_range_kernel<float>, grid, dim3(HK_THREADS), 0, as_stream(stream), (const float*)p, (const float*)q, (long long)n_p,
                            (long long)n_q, keys);
    hipLaunchKernelGGL(hk_range_fin_kernel, dim3(1), dim3(64), 0, as_stream(stream), keys, q ? 1 : 0);
    return pnnp_launch_status();
}

}  // extern "C"

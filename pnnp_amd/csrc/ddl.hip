// Differentiable distribution losses on the device: the linearly interpolated empirical CDF of a sample set at
// K ascending points (utils/kld_div.py:21-46, CDFPPF.get_cdf), the losses built on it (CDFLoss :56-60, KLD :62-74 with cdf2pdf :76-78) and the
// gradient with respect to the samples -- without the reference's sort, inf padding, searchsorted and gather.
//
// For samples d[0..N) and ascending points x[0..K), the reference's value at a point depends on three facts only:
//   xc[k] = clamp(x[k], min d, max d)
//   c[k]  = #{ d < xc[k] }                          (the reference's idx - 1)
//   hi[k] = min{ d : d >= xc[k] }                   (sorted_data_pad[idx])
//   lo[k] = max{ d : d < xc[k] }, -inf if c[k] = 0  (sorted_data_pad[idx - 1])
//   w = hi - xc;  diff = hi - lo;  delta = w / diff;  cdf[k] = ((float(c[k] + 1) - delta) - 1) / float(N - 1)      in float32, in this order
// (this file is built with -ffp-contract=off).  With the bin of a sample j(d) = #{ k : xc[k] <= d } in [0, K]: c[k] is the prefix sum of the bin
// counts over bins <= k, lo[k] the running maximum of the bins' maxima over bins <= k, hi[k] the running minimum from the right of the bins'
// minima over bins > k.  So ONE streaming pass that keeps a count, a minimum and a maximum per bin is enough.
//
// Launches per call (behind two memsets of the tables), no host round trip, nothing allocated:
//   range    min and max of every operand with the element index of each: 64-bit keys, one atomic pair per workgroup.
//   census   the hot path.  A 1024-thread workgroup clamps the points into LDS and keeps per bin a 32-bit count, a 64-bit minimum key and a 64-bit
//            maximum key there (24 bytes per point: 96 KB at K = 4096).  A sample finds its bin by a fixed-length binary search in the LDS copy of xc,
//            adds 1 to the count (the lanes that share the first lane's bin add once, together) and issues the LDS min / max only when its key
//            improves on the value just read.  key = (ordered float bits << 32) | index for the minimum, the index complemented for the maximum:
//            among equal values the LOWEST index wins both; -0.0 counts as +0.0.  Non-empty bins are merged into the operand's global tables with
//            integer atomics.
//   finish   one workgroup per operand: the three scans, then cdf, arg hi, arg lo per point.
//   loss     (fused losses) one workgroup: the scalar and dL/dcdf of both operands, float64 sums in a fixed order.
//   backward memset of grad[N], then one workgroup: per point (ATen's evaluation order; the closed form is NaN where lo = -inf, autograd gives 0)
//                gd = -g[k] / float(N-1);  gw = gd / diff;  gdiff = -gd * ((w / diff) / diff)
//                grad[arg hi] += gw + gdiff;  grad[arg lo] += -gdiff (if lo exists);  x[k] < min d: grad[arg min] += -gw;  x[k] > max d: grad[arg max] += -gw
//            The points that share an element are contiguous runs of k: one thread sums a run in order (float64, rounded once).  No float atomics.
// Integer atomics and fixed-order float sums only: two runs give identical bits.  NaN samples are not supported (a NaN has no place in the order).
#include "ordkey.h"                                            // the ordered keys, dd_sweep, the fixed-order block sum

// DD_AB: measurement builds of tools/ddl_bench.py (tools/build_variant.sh; their results are wrong on purpose): 1 = no binary search, 2 = no LDS
// atomics, 3 = no minimum / maximum.  The product is built with 0.
#ifndef DD_AB
#define DD_AB 0
#endif

namespace {

constexpr int DD_MAX_K = PNNP_DDL_MAX_K;
constexpr int DD_CHUNK = 16384;                                // a block is worth launching for this many elements
constexpr int DD_PER_THREAD = (DD_MAX_K + 1 + DD_THREADS - 1) / DD_THREADS;      // bins a thread of the finishing workgroup scans
constexpr unsigned long long DD_NOMIN = ~0ull;                 // an empty bin's minimum key (a real key's top word is never 0xffffffff: NaN only)
constexpr unsigned long long DD_NOMAX = 0ull;                  // an empty bin's maximum key (a real key's top word is never 0)

struct DdOps { const float* d[2]; long long n[2]; };           // the operands of one call (output, gt)

// workspace, in 64-bit words.  Per operand a zeroed part [range max key][bin max key (K+1)][bin count (K+1) x 32 bit] and a part filled with ones
// [range min key][bin min key (K+1)]; all zeroed parts first, so that two memsets initialise a call.
__host__ __device__ inline long long dd_zwords(int K) { return 1 + (long long)(K + 1) + (K + 2) / 2; }
__host__ __device__ inline long long dd_fwords(int K) { return 1 + (long long)(K + 1); }
struct DdWs { dd_u64 *rmax, *bmax, *rmin, *bmin; unsigned* cnt; };
__host__ __device__ inline DdWs dd_ws(void* ws, int nops, int K, int op) {
    dd_u64* z = (dd_u64*)ws + op * dd_zwords(K);
    dd_u64* f = (dd_u64*)ws + nops * dd_zwords(K) + op * dd_fwords(K);
    return {z, z + 1, f, f + 1, (unsigned*)(z + 1 + (K + 1))};
}

__device__ __forceinline__ dd_u64 dd_shfl64(dd_u64 v, int s) {
    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, s, 64), hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), s, 64);
    return ((dd_u64)hi << 32) | lo;
}

// ---- range: min / max keys of every operand
__global__ void __launch_bounds__(DD_THREADS)
dd_range_kernel(DdOps ops, int nops, int K, void* ws) {
    __shared__ dd_u64 red[2][DD_WAVES];
    const int op = blockIdx.y;
    dd_u64 mn = DD_NOMIN, mx = DD_NOMAX;
    dd_sweep(ops.d[op], ops.n[op], [&](float v, unsigned e) {
        const dd_u64 a = dd_minkey(v, e), b = dd_maxkey(v, e);
        mn = a < mn ? a : mn; mx = b > mx ? b : mx;
    });
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const dd_u64 a = dd_shfl64(mn, s), b = dd_shfl64(mx, s);
        mn = a < mn ? a : mn; mx = b > mx ? b : mx;
    }
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = mn; red[1][threadIdx.x >> 6] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < DD_WAVES; ++w) { mn = red[0][w] < mn ? red[0][w] : mn; mx = red[1][w] > mx ? red[1][w] : mx; }
        const DdWs t = dd_ws(ws, nops, K, op);
        if (mn != DD_NOMIN) atomicMin(t.rmin, mn);
        if (mx != DD_NOMAX) atomicMax(t.rmax, mx);
    }
}

// ---- census: per bin a count, a minimum key and a maximum key
__global__ void __launch_bounds__(DD_THREADS)
dd_census_kernel(DdOps ops, int nops, const float* __restrict__ x, int K, int top, void* ws) {
    extern __shared__ __attribute__((aligned(16))) dd_u64 dd_lds[];                  // [K+1] min keys, [K+1] max keys, [K+1] counts, [K] xc
    dd_u64* bmin = dd_lds;
    dd_u64* bmax = dd_lds + (K + 1);
    unsigned* cnt = (unsigned*)(dd_lds + 2 * (K + 1));
    float* xc = (float*)(cnt + (K + 1));
    const int op = blockIdx.y;
    const DdWs t = dd_ws(ws, nops, K, op);
    const float dmin = dd_keyval(*t.rmin), dmax = dd_keyval(*t.rmax);                // the range kernel, same stream
    for (int i = threadIdx.x; i <= K; i += DD_THREADS) {
        bmin[i] = DD_NOMIN; bmax[i] = DD_NOMAX; cnt[i] = 0u;
        if (i < K) xc[i] = pnnp_clampf(x[i], dmin, dmax);
    }
    __syncthreads();
#if DD_AB == 2
    unsigned ab_sink = 0;
#endif
    dd_sweep(ops.d[op], ops.n[op], [&](float v, unsigned e) {
#if DD_AB == 1
        int bin = (int)(__float_as_uint(v) & 1023u);           // A/B: no search (a bin from the mantissa's low bits)
        bin = bin > K ? K : bin;
#else
        int bin = 0;                                           // #{ k : xc[k] <= v }: the same number of steps in every lane
        for (int step = top; step > 0; step >>= 1) {
            const int nb = bin + step;
            if (nb <= K && xc[nb - 1] <= v) bin = nb;
        }
#endif
#if DD_AB == 2
        ab_sink ^= (unsigned)bin + e;                          // A/B: the search alone
#else
        const int lead = __builtin_amdgcn_readfirstlane(bin);
        const bool mine = bin == lead;
        const unsigned long long m = __ballot(mine);
        if (mine) {
            if ((int)__lane_id() == __ffsll((long long)m) - 1) atomicAdd(cnt + bin, (unsigned)__popcll(m));
        } else {
            atomicAdd(cnt + bin, 1u);
        }
#if DD_AB != 3                                                  // A/B 3: the search and the count, no minimum / maximum
        const dd_u64 a = dd_minkey(v, e), b = dd_maxkey(v, e);
        if (a < bmin[bin]) atomicMin(bmin + bin, a);
        if (b > bmax[bin]) atomicMax(bmax + bin, b);
#endif
#endif
    });
#if DD_AB == 2
    if (ab_sink == 0x9e3779b9u) atomicAdd(cnt, 1u);
#endif
    __syncthreads();
    for (int i = threadIdx.x; i <= K; i += DD_THREADS) {
        const unsigned c = cnt[i];
        if (c) { atomicAdd(t.cnt + i, c); atomicMin(t.bmin + i, bmin[i]); atomicMax(t.bmax + i, bmax[i]); }
    }
}

// the yardstick of tools/ddl_bench.py lives in noise_score.hip (pnnp_noise_score_read_f32): the plain read of the same bytes

// inclusive scan over the block's threads in thread order (Hillis-Steele through LDS)
template <class T, class Op>
__device__ __forceinline__ T dd_block_scan(T v, T* buf, Op&& op) {
    const int t = threadIdx.x;
    buf[t] = v;
    __syncthreads();
    for (int s = 1; s < DD_THREADS; s <<= 1) {
        T o = v;
        const bool has = t >= s;
        if (has) o = buf[t - s];
        __syncthreads();
        if (has) v = op(o, v);
        buf[t] = v;
        __syncthreads();
    }
    return v;
}

// ---- finish: scans, then cdf and the bracket indices.  brackets [2K + 2] int32: arg hi [K], arg lo [K] (-1: none), arg min, arg max
__global__ void __launch_bounds__(DD_THREADS)
dd_finish_kernel(DdOps ops, int nops, const float* __restrict__ x, int K, void* ws, float* __restrict__ cdf, int* __restrict__ brackets) {
    extern __shared__ __attribute__((aligned(16))) dd_u64 dd_lds[];                  // [K+1] suffix min, [K+1] prefix max, [K+1] prefix count
    __shared__ dd_u64 sbuf[DD_THREADS];
    dd_u64* smin = dd_lds;
    dd_u64* pmax = dd_lds + (K + 1);
    unsigned* pcnt = (unsigned*)(dd_lds + 2 * (K + 1));
    const int op = blockIdx.x, t = threadIdx.x, nb = K + 1;
    const DdWs g = dd_ws(ws, nops, K, op);
    const int per = (nb + DD_THREADS - 1) / DD_THREADS;        // <= DD_PER_THREAD
    const int b0 = t * per;
    // prefix over bins b0 .. b0 + per - 1, suffix over the mirrored bins nb - 1 - (b0 .. b0 + per - 1)
    unsigned c[DD_PER_THREAD]; dd_u64 mx[DD_PER_THREAD], mn[DD_PER_THREAD];
#pragma unroll
    for (int u = 0; u < DD_PER_THREAD; ++u) {
        const int b = b0 + u;
        const bool in = u < per && b < nb;
        c[u] = in ? g.cnt[b] : 0u;
        mx[u] = in ? g.bmax[b] : DD_NOMAX;
        mn[u] = in ? g.bmin[nb - 1 - b] : DD_NOMIN;
        if (u > 0) { c[u] += c[u - 1]; mx[u] = mx[u - 1] > mx[u] ? mx[u - 1] : mx[u]; mn[u] = mn[u - 1] < mn[u] ? mn[u - 1] : mn[u]; }
    }
    const unsigned ci = (unsigned)dd_block_scan((dd_u64)c[DD_PER_THREAD - 1], sbuf, [](dd_u64 a, dd_u64 b) { return a + b; }) - c[DD_PER_THREAD - 1];
    const dd_u64 mxi = dd_block_scan(mx[DD_PER_THREAD - 1], sbuf, [](dd_u64 a, dd_u64 b) { return a > b ? a : b; });
    const dd_u64 mni = dd_block_scan(mn[DD_PER_THREAD - 1], sbuf, [](dd_u64 a, dd_u64 b) { return a < b ? a : b; });
    // the exclusive part of a maximum / minimum scan: the previous thread's inclusive value
    sbuf[t] = mxi;
    __syncthreads();
    const dd_u64 mxe = t ? sbuf[t - 1] : DD_NOMAX;
    __syncthreads();
    sbuf[t] = mni;
    __syncthreads();
    const dd_u64 mne = t ? sbuf[t - 1] : DD_NOMIN;
#pragma unroll
    for (int u = 0; u < DD_PER_THREAD; ++u) {
        const int b = b0 + u;
        if (u < per && b < nb) {
            pcnt[b] = ci + c[u];
            pmax[b] = mxe > mx[u] ? mxe : mx[u];
            smin[nb - 1 - b] = mne < mn[u] ? mne : mn[u];
        }
    }
    __syncthreads();
    const dd_u64 rmin = *g.rmin, rmax = *g.rmax;
    const float dmin = dd_keyval(rmin), dmax = dd_keyval(rmax);
    const float nm1 = (float)(ops.n[op] - 1);
    float* co = cdf + (long long)op * K;
    int* br = brackets + (long long)op * (2 * K + 2);
    for (int k = t; k < K; k += DD_THREADS) {
        const float xk = pnnp_clampf(x[k], dmin, dmax);
        const unsigned ck = pcnt[k];
        const dd_u64 hk = smin[k + 1], lk = pmax[k];
        const float hi = dd_keyval(hk), lo = ck ? dd_keyval(lk) : -__builtin_inff();
        const float w = hi - xk, diff = hi - lo, delta = w / diff;
        co[k] = (((float)((long long)ck + 1) - delta) - 1.f) / nm1;
        br[k] = dd_minidx(hk);
        br[K + k] = ck ? dd_maxidx(lk) : -1;
    }
    if (t == 0) { br[2 * K] = dd_minidx(rmin); br[2 * K + 1] = dd_maxidx(rmax); }
}

// ---- loss: kind 0 = CDFLoss (mean |cdf_o - cdf_g|), kind 1 = KLD (utils/kld_div.py:62-74).  cdf [2][K] (output, gt); dcdf [2][K] = dL/dcdf
__global__ void __launch_bounds__(DD_THREADS)
dd_loss_kernel(const float* __restrict__ cdf, int K, int kind, float* __restrict__ loss, float* __restrict__ dcdf) {
    __shared__ double red[DD_WAVES];
    const float* co = cdf;
    const float* cg = cdf + K;
    float* go = dcdf;
    float* gg = dcdf + K;
    const int t = threadIdx.x;
    if (kind == 0) {
        double acc = 0.0;
        const float invk = 1.f / (float)K;
        for (int k = t; k < K; k += DD_THREADS) {
            const float df = co[k] - cg[k];
            acc += (double)fabsf(df);
            const float s = dd_sign(df) * invk;
            go[k] = s; gg[k] = -s;
        }
        const double sum = dd_block_sum(acc, red);
        if (t == 0) loss[0] = (float)(sum / (double)K);
        return;
    }
    // q from output, p from gt: |cdf[k] - cdf[k+1]| in float32, clamped at float32(1e-9) (no gradient below the clamp), divided by the larger sum
    const float floor32 = 1e-9f;
    const int M = K - 1;
    double sq = 0.0, sp = 0.0;
    for (int k = t; k < M; k += DD_THREADS) {
        const float q = fabsf(co[k] - co[k + 1]), p = fabsf(cg[k] - cg[k + 1]);
        sq += (double)(q < floor32 ? floor32 : q);
        sp += (double)(p < floor32 ? floor32 : p);
    }
    sq = dd_block_sum(sq, red);
    sp = dd_block_sum(sp, red);
    const double S = sq > sp ? sq : sp;                        // detached
    double acc = 0.0;
    // dL/dcdf[k] = G[k] s[k] - G[k-1] s[k-1], G the gradient with respect to the clamped difference, s the sign of the raw difference
    auto term = [&](int k, double& gq, double& gp) -> double {
        const float rq = co[k] - co[k + 1], rp = cg[k] - cg[k + 1];
        const float aq = fabsf(rq), ap = fabsf(rp);
        const double q = (double)(aq < floor32 ? floor32 : aq) / S, p = (double)(ap < floor32 ? floor32 : ap) / S;
        const double lp = log(p), lq = log(q);
        gq = aq >= floor32 ? (-p / q) / S * (double)dd_sign(rq) : 0.0;
        gp = ap >= floor32 ? ((lp - lq) + 1.0) / S * (double)dd_sign(rp) : 0.0;
        return p * (lp - lq);
    };
    for (int k = t; k < K; k += DD_THREADS) {
        double gq = 0.0, gp = 0.0, gq1 = 0.0, gp1 = 0.0;
        if (k < M) acc += term(k, gq, gp);
        if (k > 0) term(k - 1, gq1, gp1);
        go[k] = (float)(gq - gq1);
        gg[k] = (float)(gp - gp1);
    }
    const double sum = dd_block_sum(acc, red);
    if (t == 0) loss[0] = (float)sum;
}

// ---- backward of the cdf with respect to the samples; grad[N] is zero on entry.  g [K]: upstream gradient, times scale[0] if scale is given
__global__ void __launch_bounds__(DD_THREADS)
dd_bwd_kernel(const float* __restrict__ d, long long n, const float* __restrict__ x, int K, const int* __restrict__ br, const float* __restrict__ g,
              const float* __restrict__ scale, float* __restrict__ grad) {
    __shared__ float a_hi[DD_MAX_K], a_lo[DD_MAX_K], a_x[DD_MAX_K];                  // a_x: the clamp's share, 0 inside the range
    __shared__ signed char side[DD_MAX_K];
    const int t = threadIdx.x;
    const int amin = br[2 * K], amax = br[2 * K + 1];
    const float dmin = dd_ld1(d, amin), dmax = dd_ld1(d, amax), nm1 = (float)(n - 1), sc = scale ? scale[0] : 1.f;
    for (int k = t; k < K; k += DD_THREADS) {
        int ih = br[k], il = br[K + k];
        const bool valid = (unsigned)ih < (unsigned long long)n && il < n;      // (a NaN point has no bracket: it contributes nothing)
        if (!valid) { ih = 0; il = -1; }
        const float xk = x[k], xc = pnnp_clampf(xk, dmin, dmax);
        const float hi = dd_ld1(d, ih), lo = il >= 0 ? dd_ld1(d, il) : -__builtin_inff();
        const float w = hi - xc, diff = hi - lo;
        const float gk = scale ? g[k] * sc : g[k];
        const float gd = -gk / nm1;
        const float gw = gd / diff;
        const float gdiff = -gd * ((w / diff) / diff);
        a_hi[k] = valid ? gw + gdiff : 0.f;
        a_lo[k] = valid && il >= 0 ? -gdiff : 0.f;
        a_x[k] = -gw;
        side[k] = !valid ? 0 : (xk < dmin ? -1 : (xk > dmax ? 1 : 0));
    }
    __syncthreads();
    for (int k = t; k < K; k += DD_THREADS) {                  // runs of arg hi: distinct runs are distinct elements
        const int ih = br[k];
        if ((unsigned)ih >= (unsigned long long)n || (k && br[k - 1] == ih)) continue;
        double s = 0.0;
        for (int j = k; j < K && br[j] == ih; ++j) s += (double)a_hi[j];
        grad[ih] = (float)s;
    }
    __syncthreads();
    for (int k = t; k < K; k += DD_THREADS) {                  // runs of arg lo
        const int il = br[K + k];
        if (il < 0 || il >= n || (k && br[K + k - 1] == il)) continue;
        double s = 0.0;
        for (int j = k; j < K && br[K + j] == il; ++j) s += (double)a_lo[j];
        grad[il] += (float)s;
    }
    __syncthreads();
    if (t == 0) {                                              // the clamp: points below the minimum, then points above the maximum
        double s = 0.0; bool any = false;
        for (int k = 0; k < K; ++k) if (side[k] < 0) { s += (double)a_x[k]; any = true; }
        if (any) grad[amin] += (float)s;
        s = 0.0; any = false;
        for (int k = 0; k < K; ++k) if (side[k] > 0) { s += (double)a_x[k]; any = true; }
        if (any) grad[amax] += (float)s;
    }
}

int dd_census_lds(int K) { return (K + 1) * 20 + K * 4 + 16; }
int dd_finish_lds(int K) { return (K + 1) * 20 + 16; }

int dd_blocks(int nops, int64_t nmax, int K) {
    int cus = pnnp_device_cus();
    if (cus < 1) cus = 256;
    int64_t cap = (int64_t)cus * (dd_census_lds(K) <= 80 * 1024 ? 2 : 1) / nops;      // 1024-thread workgroups: two per CU where the LDS allows
    if (cap < 1) cap = 1;
    int64_t want = (nmax + DD_CHUNK - 1) / DD_CHUNK;
    if (want < 1) want = 1;
    return (int)(want < cap ? want : cap);
}

int dd_check(const float* const* d, const int64_t* n, int nops, const float* x, int K, void* ws) {
    if (!x || !ws || (((uintptr_t)ws) & 15) || (((uintptr_t)x) & 3)) return PNNP_E_INVALID;
    for (int i = 0; i < nops; ++i)
        if (!d[i] || (((uintptr_t)d[i]) & 3)) return PNNP_E_INVALID;
    if (K < 1 || K > DD_MAX_K) return PNNP_E_UNSUPPORTED;
    for (int i = 0; i < nops; ++i)
        if (n[i] < 2 || n[i] >= ((int64_t)1 << 31)) return PNNP_E_UNSUPPORTED;
    return PNNP_OK;
}

PnnpPerDevice dd_lds_census, dd_lds_finish;

// range, census and finish of nops operands: cdf [nops][K], brackets [nops][2K + 2]
int dd_forward(const float* const* d, const int64_t* n, int nops, const float* x, int K, void* ws, float* cdf, int* brackets, void* stream) {
    if (pnnp_allow_lds(dd_lds_census, dd_census_kernel, dd_census_lds(DD_MAX_K)) != PNNP_OK ||
        pnnp_allow_lds(dd_lds_finish, dd_finish_kernel, dd_finish_lds(DD_MAX_K)) != PNNP_OK) return PNNP_E_LAUNCH;
    DdOps ops;
    int64_t nmax = 0;
    for (int i = 0; i < 2; ++i) {
        ops.d[i] = d[i < nops ? i : 0]; ops.n[i] = n[i < nops ? i : 0];
        nmax = ops.n[i] > nmax ? ops.n[i] : nmax;
    }
    const size_t zb = (size_t)(nops * dd_zwords(K)) * 8, fb = (size_t)(nops * dd_fwords(K)) * 8;
    if (hipMemsetAsync(ws, 0, zb, as_stream(stream)) != hipSuccess ||
        hipMemsetAsync((char*)ws + zb, 0xff, fb, as_stream(stream)) != hipSuccess) return PNNP_E_LAUNCH;
    int top = 1;
    while (top * 2 <= K) top *= 2;
    const dim3 grid(dd_blocks(nops, nmax, K), nops);
    hipLaunchKernelGGL(dd_range_kernel, grid, dim3(DD_THREADS), 0, as_stream(stream), ops, nops, K, ws);
    hipLaunchKernelGGL(dd_census_kernel, grid, dim3(DD_THREADS), dd_census_lds(K), as_stream(stream), ops, nops, x, K, top, ws);
    hipLaunchKernelGGL(dd_finish_kernel, dim3(nops), dim3(DD_THREADS), dd_finish_lds(K), as_stream(stream), ops, nops, x, K, ws, cdf, brackets);
    return pnnp_launch_status();
}

int dd_loss(int kind, const float* output, int64_t n_output, const float* gt, int64_t n_gt, const float* x, int K, void* ws,
            float* cdf, int* brackets, float* loss, float* dcdf, void* stream) {
    const float* d[2] = {output, gt};
    const int64_t n[2] = {n_output, n_gt};
    const int rc = dd_check(d, n, 2, x, K, ws);
    if (rc != PNNP_OK) return rc;
    if (!cdf || !brackets || !loss || !dcdf) return PNNP_E_INVALID;
    if (kind == 1 && K < 2) return PNNP_E_UNSUPPORTED;
    const int rf = dd_forward(d, n, 2, x, K, ws, cdf, brackets, stream);
    if (rf != PNNP_OK) return rf;
    hipLaunchKernelGGL(dd_loss_kernel, dim3(1), dim3(DD_THREADS), 0, as_stream(stream), (const float*)cdf, K, kind, loss, dcdf);
    return pnnp_launch_status();
}

}  // namespace

extern "C" {

int64_t pnnp_ddl_ws_bytes(int nops, int k) {
    if (nops < 1 || nops > 2 || k < 1) return PNNP_E_INVALID;
    if (k > DD_MAX_K) return PNNP_E_UNSUPPORTED;
    return (int64_t)nops * (dd_zwords(k) + dd_fwords(k)) * 8;
}

int pnnp_ecdf_f32(const float* data, int64_t n, const float* x, int k, void* ws, float* cdf, int* brackets, void* stream) {
    const int rc = dd_check(&data, &n, 1, x, k, ws);
    if (rc != PNNP_OK) return rc;
    if (!cdf || !brackets) return PNNP_E_INVALID;
    return dd_forward(&data, &n, 1, x, k, ws, cdf, brackets, stream);
}

int pnnp_ecdf_bwd_f32(const float* data, int64_t n, const float* x, int k, const int* brackets, const float* g, const float* scale, float* grad,
                      void* stream) {
    if (!data || !x || !brackets || !g || !grad || ((((uintptr_t)data) | ((uintptr_t)x) | ((uintptr_t)g) | ((uintptr_t)grad)) & 3)) return PNNP_E_INVALID;
    if (k < 1 || k > DD_MAX_K || n < 2 || n >= ((int64_t)1 << 31)) return PNNP_E_UNSUPPORTED;
    if (hipMemsetAsync(grad, 0, (size_t)n * sizeof(float), as_stream(stream)) != hipSuccess) return PNNP_E_LAUNCH;
    hipLaunchKernelGGL(dd_bwd_kernel, dim3(1), dim3(DD_THREADS), 0, as_stream(stream), data, (long long)n, x, k, brackets, g, scale, grad);
    return pnnp_launch_status();
}

int pnnp_cdf_loss_f32(const float* output, int64_t n_output, const float* gt, int64_t n_gt, const float* x, int k, void* ws,
                      float* cdf, int* brackets, float* loss, float* dcdf, void* stream) {
    return dd_loss(0, output, n_output, gt, n_gt, x, k, ws, cdf, brackets, loss, dcdf, stream);
}

int pnnp_kld_loss_f32(const float* output, int64_t n_output, const float* gt, int64_t n_gt, const float* x, int k, void* ws,
                      float* cdf, int* brackets, float* loss, float* dcdf, void* stream) {
    return dd_loss(1, output, n_output, gt, n_gt, x, k, ws, cdf, brackets, loss, dcdf, stream);
}

}  // extern "C"

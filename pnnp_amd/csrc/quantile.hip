// QuantileLoss on the device (utils/kld_div.py:49-53): torch.quantile(..., dim=-1, interpolation='linear') of
// every row of one or two operands, the L1 mean between them and the gradient with respect to the samples -- by an exact multi-rank select,
// without the reference's sort of every sample set.
//
// Per row of n samples and probability q[k], in float32 (this file is built with -ffp-contract=off):
//   pos = q * float(n - 1);  lo = floor(pos);  hi = ceil(pos);  w = pos - floor(pos);  lo, hi clamped into [0, n - 1]
//   value = w < 0.5 ? a + w * (b - a) : b - (b - a) * (1 - w)            a = s[lo], b = s[hi], s the row sorted ascending
// so a row needs up to 2K order statistics ("entries": 2k is s[lo[k]], 2k + 1 is s[hi[k]]) and, for the gradient, the element that holds each:
// among equal values the LOWEST index (ddl.hip's convention), so an entry is answered by its 32-bit ordered key and the lowest index of that key.
//
// A (row, operand) pair is a "ro".  Launches per call (behind one memset of the tables), no host round trip, nothing allocated, three passes
// over the samples whatever they hold:
//   range    the smallest and largest FINITE value of every ro: one 32-bit atomic pair per workgroup.
//   census   QT_B = 2^15 bins, linear in the value over that range (-inf falls into the first bin, +inf into the last; any monotone map keeps the
//            select exact): 32-bit counts in 128 KB of LDS, merged per workgroup with integer atomics.
//   scan     one workgroup per ro: prefix sums of the bins; per entry the rank (the float32 rule above), the bin that holds it and the rank
//            inside that bin; the bins that hold an entry ("slots", at most 2K) get consecutive segments of the ro's gather buffer.
//   gather   a sample whose bin is a slot appends (key << 32 | index) to the slot's segment: one returning integer atomic per appended sample
//            (a few percent of the samples where the data spreads over the bins).  The order inside a segment depends on the run; nothing
//            read from it does.
//   finish   one workgroup per slot at a time (two launches: 256 threads for the short segments, 1024 for the rest): a segment of up to QT_CAP words is
//            sorted in LDS (bitonic); the entry's word stands at its rank, and the first word with that key holds the lowest index.  A longer segment (heavy ties, all-equal data, an outlier that stretches the
//            range) is answered from global memory by a four-digit radix select on the key and one pass for the lowest index; entries that
//            fall into the run of equal keys just found reuse it.
//   eval     one workgroup: values, arg lo / arg hi and w of every operand; for the loss the float64 sum in a fixed order and dL/dvalue.
//   backward memset of grad, then one workgroup per row: the 2K contributions g (1 - w) -> arg lo, g w -> arg hi are sorted by (element, entry)
//            in LDS and each run summed by one thread in float64, rounded once.  No float atomics.
// Integer atomics and fixed-order float sums only: two runs give identical bits.  NaN samples are not supported; every index derived from the
// data is clamped or guarded before it addresses memory.
#include "ordkey.h"

namespace {

constexpr int QT_MAX_K = PNNP_QUANTILE_MAX_K;
constexpr int QT_B = 32768;                                    // census bins
constexpr int QT_WORDS = QT_B / 32;                            // words of the slot bitmap (= DD_THREADS: one per thread of the scan)
constexpr int QT_CAP = 8192;                                   // the longest segment sorted in LDS (64 KB of 64-bit words)
constexpr int QT_SHORT = 4096;                                 // the longest segment the 256-thread finish sorts (32 KB)
constexpr int QT_SHORT_GRID = 512, QT_LONG_GRID = 64;          // workgroups per ro of the two finish launches (fewer where there are fewer entries)
constexpr int QT_CHUNK = 65536;                                // a block is worth launching for this many elements
constexpr int QT_HDR = 8;                                      // [0] ~(smallest finite key) [1] largest finite key (0: none) [2] slots
static_assert(QT_WORDS == DD_THREADS, "the scan gives every thread one bitmap word");

struct QtOps { const float* d[2]; long long n[2]; int rows, K; };

// workspace: per ro a table of 32-bit words, then (16-byte aligned) the gather buffers, 64-bit words, n per row
__host__ __device__ inline long long qt_table_words(int K) { return (long long)QT_B + QT_WORDS + QT_HDR + 14ll * K; }
__host__ __device__ inline long long qt_tables_bytes(int nro, int K) { return ((long long)nro * qt_table_words(K) * 4 + 15) & ~15ll; }
struct QtWs { unsigned *cnt, *bitmap, *hdr, *slot_bin, *slot_start, *slot_cnt, *e_bin, *e_res, *e_key, *e_idx; dd_u64* seg; };
__host__ __device__ inline QtWs qt_ws(void* ws, const QtOps& o, int nops, int op, int r) {
    const int S = 2 * o.K;
    unsigned* t = (unsigned*)ws + ((long long)op * o.rows + r) * qt_table_words(o.K);
    dd_u64* seg = (dd_u64*)((char*)ws + qt_tables_bytes(nops * o.rows, o.K)) + (op ? (long long)o.rows * o.n[0] : 0ll) + (long long)r * o.n[op];
    unsigned* s = t + QT_B + QT_WORDS + QT_HDR;
    return {t, t + QT_B, t + QT_B + QT_WORDS, s, s + S, s + 2 * S, s + 3 * S, s + 4 * S, s + 5 * S, s + 6 * S, seg};
}

// the float32 rank rule; a q outside [0, 1] or NaN still gives ranks inside the row
struct QtRank { unsigned lo, hi; float w; };
__device__ __forceinline__ unsigned qt_clamp_rank(float f, long long n) {
    if (!(f >= 0.f)) return 0u;
    if (f >= 2147483648.f) return (unsigned)(n - 1);
    const long long i = (long long)f;
    return (unsigned)(i < n - 1 ? i : n - 1);
}
__device__ __forceinline__ QtRank qt_rank(float q, long long n) {
    const float pos = q * (float)(n - 1);
    const float fl = floorf(pos);
    return {qt_clamp_rank(fl, n), qt_clamp_rank(ceilf(pos), n), pos - fl};
}

// the census bin of a value: monotone in the value, whatever fmin and scale are
struct QtMap { float fmin, scale; };
__device__ __forceinline__ QtMap qt_map(const unsigned* hdr) {
    const unsigned kmin = ~hdr[0], kmax = hdr[1];
    if (kmax == 0u) return {0.f, 0.f};                        // no finite value: one bin
    const float fmin = dd_unord(kmin), range = dd_unord(kmax) - fmin;
    return {fmin, (range > 0.f && range < __builtin_inff()) ? (float)QT_B / range : 0.f};
}
__device__ __forceinline__ int qt_bin(float v, const QtMap& m) {
    const float t = (v - m.fmin) * m.scale;
    return t >= 0.f ? (t < (float)(QT_B - 1) ? (int)t : QT_B - 1) : 0;      // (a NaN product: bin 0)
}

// counts[bin] += 1 in LDS; the lanes that share the first lane's bin add once, together
__device__ __forceinline__ void qt_count(unsigned* counts, int bin) {
    const int lead = __builtin_amdgcn_readfirstlane(bin);
    const bool mine = bin == lead;
    const unsigned long long m = __ballot(mine);
    if (mine) {
        if ((int)__lane_id() == __ffsll((long long)m) - 1) atomicAdd(counts + bin, (unsigned)__popcll(m));
    } else {
        atomicAdd(counts + bin, 1u);
    }
}

__device__ __forceinline__ int qt_ro(const QtOps& o, int& op) { const int ro = blockIdx.y; op = ro / o.rows; return ro - op * o.rows; }

// ---- range: the finite minimum and maximum of every ro
__global__ void __launch_bounds__(DD_THREADS)
qt_range_kernel(QtOps o, int nops, void* ws) {
    __shared__ unsigned red[2][DD_WAVES];
    int op; const int r = qt_ro(o, op);
    unsigned mn = 0xffffffffu, mx = 0u;
    dd_sweep(o.d[op] + (long long)r * o.n[op], o.n[op], [&](float v, unsigned) {
        if (fabsf(v) < __builtin_inff()) { const unsigned k = dd_ord(v); mn = k < mn ? k : mn; mx = k > mx ? k : mx; }
    });
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const unsigned a = (unsigned)__shfl_xor((int)mn, s, 64), b = (unsigned)__shfl_xor((int)mx, s, 64);
        mn = a < mn ? a : mn; mx = b > mx ? b : mx;
    }
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = mn; red[1][threadIdx.x >> 6] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < DD_WAVES; ++w) { mn = red[0][w] < mn ? red[0][w] : mn; mx = red[1][w] > mx ? red[1][w] : mx; }
        const QtWs t = qt_ws(ws, o, nops, op, r);
        if (mx != 0u) { atomicMax(t.hdr, ~mn); atomicMax(t.hdr + 1, mx); }
    }
}

// ---- census: the count of every bin
__global__ void __launch_bounds__(DD_THREADS)
qt_census_kernel(QtOps o, int nops, void* ws) {
    extern __shared__ __attribute__((aligned(16))) unsigned qt_lds[];                // [QT_B] counts
    int op; const int r = qt_ro(o, op);
    const QtWs t = qt_ws(ws, o, nops, op, r);
    const QtMap m = qt_map(t.hdr);                             // the range kernel, same stream
    for (int i = threadIdx.x; i < QT_B; i += DD_THREADS) qt_lds[i] = 0u;
    __syncthreads();
    dd_sweep(o.d[op] + (long long)r * o.n[op], o.n[op], [&](float v, unsigned) { qt_count(qt_lds, qt_bin(v, m)); });
    __syncthreads();
    for (int i = threadIdx.x; i < QT_B; i += DD_THREADS) {
        const unsigned c = qt_lds[i];
        if (c) atomicAdd(t.cnt + i, c);
    }
}

// inclusive scan over the block's threads in thread order (Hillis-Steele through LDS)
__device__ __forceinline__ unsigned qt_block_scan(unsigned v, unsigned* buf) {
    const int t = threadIdx.x;
    __syncthreads();                                           // (buf may still be read from the previous scan)
    buf[t] = v;
    __syncthreads();
    for (int s = 1; s < DD_THREADS; s <<= 1) {
        const unsigned o = t >= s ? buf[t - s] : 0u;
        __syncthreads();
        v += o;
        buf[t] = v;
        __syncthreads();
    }
    return v;
}

// ---- scan: entries -> (bin, rank inside the bin); the bins that hold an entry become slots with consecutive segments
__global__ void __launch_bounds__(DD_THREADS)
qt_scan_kernel(QtOps o, int nops, const float* __restrict__ q, void* ws) {
    extern __shared__ __attribute__((aligned(16))) unsigned qt_lds[];                // [QT_B] inclusive prefix counts
    __shared__ unsigned sbuf[DD_THREADS], bm[QT_WORDS];
    const int ro = blockIdx.x, op = ro / o.rows, r = ro - op * o.rows, t = threadIdx.x, S = 2 * o.K;
    const QtWs g = qt_ws(ws, o, nops, op, r);
    const long long n = o.n[op];
    unsigned run = 0u;
    for (int u = 0; u < 32; ++u) { run += g.cnt[32 * t + u]; qt_lds[32 * t + u] = run; }
    const unsigned before = qt_block_scan(run, sbuf) - run;
    for (int u = 0; u < 32; ++u) qt_lds[32 * t + u] += before;
    bm[t] = 0u;
    __syncthreads();
    for (int j = t; j < S; j += DD_THREADS) {
        const QtRank rk = qt_rank(q[j >> 1], n);
        const unsigned rank = (j & 1) ? rk.hi : rk.lo;
        int b = 0;                                             // #{ bins whose inclusive prefix <= rank }: the bin that holds the rank
        for (int step = QT_B / 2; step > 0; step >>= 1)
            if (qt_lds[b + step - 1] <= rank) b += step;
        const unsigned below = b ? qt_lds[b - 1] : 0u;
        atomicOr(bm + (b >> 5), 1u << (b & 31));
        g.e_bin[j] = (unsigned)b;
        g.e_res[j] = rank >= below ? rank - below : 0u;
    }
    __syncthreads();
    const unsigned word = bm[t];
    unsigned held = 0u;
    for (unsigned wd = word; wd; wd &= wd - 1) {
        const int b = 32 * t + __ffs((int)wd) - 1;
        held += qt_lds[b] - (b ? qt_lds[b - 1] : 0u);
    }
    const unsigned nact = (unsigned)__popc(word);
    const unsigned slots = qt_block_scan(nact, sbuf), words = qt_block_scan(held, sbuf);
    unsigned s = slots - nact, off = words - held;
    for (unsigned wd = word; wd; wd &= wd - 1) {
        const int b = 32 * t + __ffs((int)wd) - 1;
        const unsigned c = qt_lds[b] - (b ? qt_lds[b - 1] : 0u);
        if (s < (unsigned)S) { g.slot_bin[s] = (unsigned)b; g.slot_start[s] = off; g.slot_cnt[s] = c; }
        g.cnt[b] = off;                                        // the gather's cursor
        ++s; off += c;
    }
    g.bitmap[t] = word;
    if (t == DD_THREADS - 1) g.hdr[2] = slots < (unsigned)S ? slots : (unsigned)S;
}

// ---- gather: the samples of the slots' bins, as (key << 32 | index), into the slots' segments
__global__ void __launch_bounds__(DD_THREADS)
qt_gather_kernel(QtOps o, int nops, void* ws) {
    __shared__ unsigned bm[QT_WORDS];
    int op; const int r = qt_ro(o, op);
    const QtWs t = qt_ws(ws, o, nops, op, r);
    const QtMap m = qt_map(t.hdr);
    const unsigned long long n = (unsigned long long)o.n[op];
    bm[threadIdx.x] = t.bitmap[threadIdx.x];
    __syncthreads();
    dd_sweep(o.d[op] + (long long)r * o.n[op], o.n[op], [&](float v, unsigned e) {
        const int bin = qt_bin(v, m);
        if (!((bm[bin >> 5] >> (bin & 31)) & 1u)) return;
        const unsigned pos = atomicAdd(t.cnt + bin, 1u);
        if (pos < n) t.seg[pos] = dd_minkey(v, e);
    });
}

// ---- finish: a workgroup answers the entries of one slot's bin at a time: e_key, e_idx.  Two launches share the slots: 256 threads and 32 KB of
// LDS for the segments of up to QT_SHORT words (nearly all of them: several workgroups per CU), 1024 threads and 64 KB for the longer ones
template <int THREADS, int CAP, bool LONG>
__device__ __forceinline__ void qt_finish_slot(const QtOps& o, const QtWs& g, int op, unsigned slot, unsigned above, dd_u64* qt_sort) {
    unsigned& lowest = *(unsigned*)(qt_sort + CAP);
    const int t = threadIdx.x, S = 2 * o.K;
    const unsigned bin = g.slot_bin[slot], start = g.slot_start[slot], n = g.slot_cnt[slot];
    if (n <= above || (unsigned long long)start + n > (unsigned long long)o.n[op]) return;    // (the other launch's, or none)
    const dd_u64* seg = g.seg + start;
    if (n <= (unsigned)CAP) {
        unsigned P = 64;
        while (P < n) P <<= 1;
        for (unsigned i = t; i < P; i += THREADS) qt_sort[i] = i < n ? seg[i] : ~0ull;
        __syncthreads();
        for (unsigned k = 2; k <= P; k <<= 1)
            for (unsigned j = k >> 1; j > 0; j >>= 1) {
                for (unsigned i = t; i < P; i += THREADS) {
                    const unsigned x = i ^ j;
                    if (x > i) {
                        const dd_u64 a = qt_sort[i], b = qt_sort[x];
                        if ((a > b) == ((i & k) == 0u)) { qt_sort[i] = b; qt_sort[x] = a; }
                    }
                }
                __syncthreads();
            }
        for (int j = t; j < S; j += THREADS) {
            if (g.e_bin[j] != bin) continue;
            unsigned res = g.e_res[j];
            res = res < n ? res : n - 1;
            const unsigned key = (unsigned)(qt_sort[res] >> 32);
            unsigned lo = 0, hi = res;                         // the first word with this key
            while (lo < hi) {
                const unsigned mid = (lo + hi) >> 1;
                if ((unsigned)(qt_sort[mid] >> 32) < key) lo = mid + 1; else hi = mid;
            }
            g.e_key[j] = key;
            g.e_idx[j] = (unsigned)qt_sort[lo];
        }
        return;
    }
    if constexpr (!LONG) return;
    // a segment that does not fit: per entry a radix select on the key, most significant digit first, then the lowest index of that key.
    // Every thread follows the same path (the loop conditions are uniform).
    unsigned* hist = (unsigned*)qt_sort;
    bool have = false;
    unsigned c_lt = 0u, c_le = 0u, ckey = 0u, cidx = 0u;      // the last answer: its key fills the ranks [c_lt, c_le) of the segment
    for (int j = 0; j < S; ++j) {
        if (g.e_bin[j] != bin) continue;
        unsigned res = g.e_res[j];
        res = res < n ? res : n - 1;
        if (!(have && res >= c_lt && res < c_le)) {
            unsigned prefix = 0u, rem = res, base = 0u, last = 0u;
            for (int d = 3; d >= 0; --d) {
                if (t < 256) hist[t] = 0u;
                __syncthreads();
                for (unsigned i = t; i < n; i += THREADS) {
                    const unsigned key = (unsigned)(seg[i] >> 32);
                    if (d == 3 || (key >> (8 * d + 8)) == prefix) qt_count(hist, (int)((key >> (8 * d)) & 255u));
                }
                __syncthreads();
                unsigned cum = 0u;
                int dg = 0;
                for (; dg < 255; ++dg) {
                    const unsigned h = hist[dg];
                    if (cum + h > rem) break;
                    cum += h;
                }
                rem -= cum < rem ? cum : rem;
                base += cum;
                prefix = (prefix << 8) | (unsigned)dg;
                last = hist[dg];
                __syncthreads();
            }
            ckey = prefix; c_lt = base; c_le = base + last;
            if (t == 0) lowest = 0xffffffffu;
            __syncthreads();
            unsigned mn = 0xffffffffu;
            for (unsigned i = t; i < n; i += THREADS) {
                const dd_u64 w = seg[i];
                if ((unsigned)(w >> 32) == ckey) { const unsigned e = (unsigned)w; mn = e < mn ? e : mn; }
            }
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) { const unsigned a = (unsigned)__shfl_xor((int)mn, s, 64); mn = a < mn ? a : mn; }
            if ((t & 63) == 0) atomicMin(&lowest, mn);
            __syncthreads();
            cidx = lowest;
            __syncthreads();
            have = true;
        }
        if (t == 0) { g.e_key[j] = ckey; g.e_idx[j] = cidx; }
    }
}

// a workgroup takes the slots blockIdx.x, blockIdx.x + gridDim.x, ... of its ro
template <int THREADS, int CAP, bool LONG>
__global__ void __launch_bounds__(THREADS)
qt_finish_kernel(QtOps o, int nops, void* ws, unsigned above) {
    extern __shared__ __attribute__((aligned(16))) dd_u64 qt_sort[];                 // [CAP] words (the radix select keeps its 256 counts here), [1] lowest
    const int ro = blockIdx.y, op = ro / o.rows, r = ro - op * o.rows;
    const QtWs g = qt_ws(ws, o, nops, op, r);
    const unsigned slots = g.hdr[2];
    for (unsigned slot = blockIdx.x; slot < slots; slot += gridDim.x) {
        qt_finish_slot<THREADS, CAP, LONG>(o, g, op, slot, above, qt_sort);
        __syncthreads();                                       // (the next slot reuses the LDS)
    }
}

// ---- eval: values [nops][K][rows], arg [nops][2][rows][K], w [nops][K]; with loss: the L1 mean and dq [2][K][rows] = dL/dvalue
__global__ void __launch_bounds__(DD_THREADS)
qt_eval_kernel(QtOps o, int nops, const float* __restrict__ q, void* ws, float* __restrict__ values, int* __restrict__ arg, float* __restrict__ w,
               float* __restrict__ loss, float* __restrict__ dq) {
    __shared__ double red[DD_WAVES];
    const int R = o.rows, K = o.K, total = R * K;
    const float inv = 1.f / (float)total;
    double acc = 0.0;
    for (int i = threadIdx.x; i < total; i += DD_THREADS) {
        const int r = i / K, k = i - r * K;
        float v[2] = {0.f, 0.f};
#pragma unroll
        for (int op = 0; op < 2; ++op) {
            if (op >= nops) break;
            const QtWs g = qt_ws(ws, o, nops, op, r);
            const long long n = o.n[op];
            const QtRank rk = qt_rank(q[k], n);
            const float a = dd_unord(g.e_key[2 * k]), b = dd_unord(g.e_key[2 * k + 1]);
            const float d = b - a;
            v[op] = rk.w < 0.5f ? a + rk.w * d : b - d * (1.f - rk.w);
            values[(long long)op * total + (long long)k * R + r] = v[op];
            const unsigned il = g.e_idx[2 * k], ih = g.e_idx[2 * k + 1];
            arg[((long long)(op * 2 + 0) * R + r) * K + k] = (int)(il < (unsigned long long)n ? il : (unsigned)(n - 1));
            arg[((long long)(op * 2 + 1) * R + r) * K + k] = (int)(ih < (unsigned long long)n ? ih : (unsigned)(n - 1));
            if (r == 0) w[op * K + k] = rk.w;
        }
        if (loss) {
            const float df = v[0] - v[1];
            acc += (double)fabsf(df);
            const float s = dd_sign(df) * inv;
            dq[(long long)k * R + r] = s;
            dq[(long long)total + (long long)k * R + r] = -s;
        }
    }
    if (loss) {
        const double sum = dd_block_sum(acc, red);
        if (threadIdx.x == 0) loss[0] = (float)(sum / (double)total);
    }
}

// ---- backward: grad [rows][n] is zero on entry.  arg [2][rows][K], w [K], g [K][rows] (times scale[0] if scale is given)
__global__ void __launch_bounds__(DD_THREADS)
qt_bwd_kernel(int R, long long n, int K, const int* __restrict__ arg, const float* __restrict__ w, const float* __restrict__ g,
              const float* __restrict__ scale, float* __restrict__ grad) {
    __shared__ dd_u64 word[2 * QT_MAX_K];                      // (element << 32) | entry, sorted
    __shared__ float part[2 * QT_MAX_K];
    const int r = blockIdx.x, t = threadIdx.x, S = 2 * K;
    const float sc = scale ? scale[0] : 1.f;
    unsigned P = 64;
    while (P < (unsigned)S) P <<= 1;
    for (unsigned j = t; j < P; j += DD_THREADS) {
        if (j >= (unsigned)S) { word[j] = ~0ull; continue; }
        const int k = j >> 1, side = j & 1;
        const float gk = scale ? g[(long long)k * R + r] * sc : g[(long long)k * R + r], wk = w[k];
        part[j] = side ? gk * wk : gk * (1.f - wk);
        word[j] = ((dd_u64)(unsigned)arg[((long long)side * R + r) * K + k] << 32) | j;
    }
    __syncthreads();
    for (unsigned k = 2; k <= P; k <<= 1)
        for (unsigned j = k >> 1; j > 0; j >>= 1) {
            for (unsigned i = t; i < P; i += DD_THREADS) {
                const unsigned x = i ^ j;
                if (x > i) {
                    const dd_u64 a = word[i], b = word[x];
                    if ((a > b) == ((i & k) == 0u)) { word[i] = b; word[x] = a; }
                }
            }
            __syncthreads();
        }
    for (int j = t; j < S; j += DD_THREADS) {                  // runs of one element: the thread at a run's start sums it in order
        const unsigned e = (unsigned)(word[j] >> 32);
        if ((j && (unsigned)(word[j - 1] >> 32) == e) || e >= (unsigned long long)n) continue;
        double s = 0.0;
        for (int i = j; i < S && (unsigned)(word[i] >> 32) == e; ++i) s += (double)part[(unsigned)word[i]];
        grad[(long long)r * n + e] = (float)s;
    }
}

int qt_blocks(int nro, int64_t nmax) {
    int cus = pnnp_device_cus();
    if (cus < 1) cus = 256;
    int64_t cap = cus / nro;                                   // the census takes 128 KB of LDS: one workgroup per CU
    if (cap < 1) cap = 1;
    int64_t want = (nmax + QT_CHUNK - 1) / QT_CHUNK;
    if (want < 1) want = 1;
    return (int)(want < cap ? want : cap);
}

int qt_check(const float* const* d, const int64_t* n, int nops, int rows, const float* q, int K, void* ws) {
    if (!q || !ws || (((uintptr_t)ws) & 15) || (((uintptr_t)q) & 3)) return PNNP_E_INVALID;
    for (int i = 0; i < nops; ++i)
        if (!d[i] || (((uintptr_t)d[i]) & 3)) return PNNP_E_INVALID;
    if (K < 1 || K > QT_MAX_K || rows < 1 || (int64_t)rows * K >= ((int64_t)1 << 31) || (int64_t)rows * nops > 65535) return PNNP_E_UNSUPPORTED;
    for (int i = 0; i < nops; ++i)
        if (n[i] < 1 || n[i] >= ((int64_t)1 << 31)) return PNNP_E_UNSUPPORTED;
    return PNNP_OK;
}

PnnpPerDevice qt_lds_census, qt_lds_scan, qt_lds_finish;
constexpr int QT_FINISH_LDS = QT_CAP * 8 + 16;

// the select of nops operands, then eval
int qt_forward(const float* const* d, const int64_t* n, int nops, int rows, const float* q, int K, void* ws, float* values, int* arg, float* w,
               float* loss, float* dq, void* stream) {
    if (pnnp_allow_lds(qt_lds_census, qt_census_kernel, QT_B * 4) != PNNP_OK || pnnp_allow_lds(qt_lds_scan, qt_scan_kernel, QT_B * 4) != PNNP_OK ||
        pnnp_allow_lds(qt_lds_finish, qt_finish_kernel<DD_THREADS, QT_CAP, true>, QT_FINISH_LDS) != PNNP_OK) return PNNP_E_LAUNCH;
    QtOps o;
    int64_t nmax = 0;
    for (int i = 0; i < 2; ++i) {
        o.d[i] = d[i < nops ? i : 0]; o.n[i] = n[i < nops ? i : 0];
        nmax = o.n[i] > nmax ? o.n[i] : nmax;
    }
    o.rows = rows; o.K = K;
    const int nro = nops * rows;
    if (hipMemsetAsync(ws, 0, (size_t)qt_tables_bytes(nro, K), as_stream(stream)) != hipSuccess) return PNNP_E_LAUNCH;
    const dim3 grid(qt_blocks(nro, nmax), nro);
    hipLaunchKernelGGL(qt_range_kernel, grid, dim3(DD_THREADS), 0, as_stream(stream), o, nops, ws);
    hipLaunchKernelGGL(qt_census_kernel, grid, dim3(DD_THREADS), QT_B * 4, as_stream(stream), o, nops, ws);
    hipLaunchKernelGGL(qt_scan_kernel, dim3(nro), dim3(DD_THREADS), QT_B * 4, as_stream(stream), o, nops, q, ws);
    hipLaunchKernelGGL(qt_gather_kernel, grid, dim3(DD_THREADS), 0, as_stream(stream), o, nops, ws);
    const int gs = 2 * K < QT_SHORT_GRID ? 2 * K : QT_SHORT_GRID, gl = 2 * K < QT_LONG_GRID ? 2 * K : QT_LONG_GRID;
    hipLaunchKernelGGL((qt_finish_kernel<256, QT_SHORT, false>), dim3(gs, nro), dim3(256), QT_SHORT * 8 + 16, as_stream(stream), o, nops, ws, 0u);
    hipLaunchKernelGGL((qt_finish_kernel<DD_THREADS, QT_CAP, true>), dim3(gl, nro), dim3(DD_THREADS), QT_FINISH_LDS, as_stream(stream), o, nops, ws,
                       (unsigned)QT_SHORT);
    hipLaunchKernelGGL(qt_eval_kernel, dim3(1), dim3(DD_THREADS), 0, as_stream(stream), o, nops, q, ws, values, arg, w, loss, dq);
    return pnnp_launch_status();
}

}  // namespace

extern "C" {

int64_t pnnp_quantile_ws_bytes(int rows, int64_t n_a, int64_t n_b, int k) {
    if (rows < 1 || n_a < 1 || n_b < 0 || k < 1) return PNNP_E_INVALID;
    if (k > QT_MAX_K || n_a >= ((int64_t)1 << 31) || n_b >= ((int64_t)1 << 31) || (int64_t)rows * 2 > 65535) return PNNP_E_UNSUPPORTED;
    return qt_tables_bytes((n_b ? 2 : 1) * rows, k) + (int64_t)rows * (n_a + n_b) * 8;
}

int pnnp_quantile_f32(const float* data, int rows, int64_t n, const float* q, int k, void* ws, float* values, int* arg, float* w, void* stream) {
    const int rc = qt_check(&data, &n, 1, rows, q, k, ws);
    if (rc != PNNP_OK) return rc;
    if (!values || !arg || !w) return PNNP_E_INVALID;
    return qt_forward(&data, &n, 1, rows, q, k, ws, values, arg, w, nullptr, nullptr, stream);
}

int pnnp_quantile_bwd_f32(int rows, int64_t n, int k, const int* arg, const float* w, const float* g, const float* scale, float* grad, void* stream) {
    if (!arg || !w || !g || !grad || ((((uintptr_t)arg) | ((uintptr_t)w) | ((uintptr_t)g) | ((uintptr_t)grad)) & 3)) return PNNP_E_INVALID;
    if (k < 1 || k > QT_MAX_K || rows < 1 || rows > 65535 || n < 1 || n >= ((int64_t)1 << 31)) return PNNP_E_UNSUPPORTED;
    if (hipMemsetAsync(grad, 0, (size_t)rows * (size_t)n * sizeof(float), as_stream(stream)) != hipSuccess) return PNNP_E_LAUNCH;
    hipLaunchKernelGGL(qt_bwd_kernel, dim3(rows), dim3(DD_THREADS), 0, as_stream(stream), rows, (long long)n, k, arg, w, g, scale, grad);
    return pnnp_launch_status();
}

int pnnp_quantile_loss_f32(const float* output, int64_t n_output, const float* gt, int64_t n_gt, int rows, const float* q, int k, void* ws,
                           float* values, int* arg, float* w, float* loss, float* dq, void* stream) {
    const float* d[2] = {output, gt};
    const int64_t n[2] = {n_output, n_gt};
    const int rc = qt_check(d, n, 2, rows, q, k, ws);
    if (rc != PNNP_OK) return rc;
    if (!values || !arg || !w || !loss || !dq) return PNNP_E_INVALID;
    return qt_forward(d, n, 2, rows, q, k, ws, values, arg, w, loss, dq, stream);
}

}  // extern "C"

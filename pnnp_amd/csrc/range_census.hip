// Range census of the tensors the fp16x2 ("h2") kernels split (csrc/h2.h): per (tensor, amax slot) job, an integer histogram of how far
// below the slot's value each element lies, in binades.  It reads the tensors AFTER the kernels that used them are done, so nothing the
// network computes changes; HipTrainStep runs it every `range_every` steps and check_range() turns the table into a report (INTEGRATION.md
// section 3).
//
//   A = the float32 value whose bits the slot holds: the exact maximum the h2 kernels took the tensor's scale s = 2^pnnp_h2_scale_exp(A) from.
//   For a finite non-zero element x:  k = floor(log2 A) - floor(log2 |x|)  (both from the exponent bits; fp32 subnormals get their true
//   floor(log2)), counted in bin min(max(k, 0), 47); bins 0 .. 46 are single binades, bin 47 holds k >= 47.  Per job also:
//     zero       x == 0
//     nonfinite  inf / NaN
//     over       |x| > A  (the slot contract, include/pnnp_hip.h: a slot may over-estimate, never under-estimate -- non-zero is a bug report)
//   A slot of exponent 255 (inf / NaN: the kernels use s = 1) counts `nonfinite` only and skips the bins.
//
// Significand bits the split keeps per bin.  s A lies in [2^14, 2^15), so s|x| has exponent e = 14 - k.  hi = f16(s x) and lo = f16(s x - hi)
// round to nearest even; fp16's smallest normal is 2^-14 and its subnormal spacing 2^-24.
//   k <= 17:   |s x - hi| <= 2^(e - 11) >= 2^-14: lo is a normal fp16, hi + lo keeps 11 + 11 = 22 bits (|error| <= 2^-22 |x|: h2.h).
//   18 .. 28:  lo is an fp16 subnormal (spacing 2^-24): hi + lo keeps the bits of s x from 2^e down to 2^-24, i.e. 39 - k of them.
//   k >= 29:   hi itself is subnormal (e <= -15); lo rounds to 0 and hi alone keeps 39 - k bits.
//   k >= 39:   nothing (s x < 2^-24 rounds to 0 or to the smallest subnormal).
// So bits(k) = max(0, min(22, 39 - k)); a job's low-bit share (HipTrainStep range_min_bits = m) is the fraction of its finite non-zero
// elements in bins k >= 40 - m (k >= 24 for m = 16).  tests/test_host_range_census.py checks the mapping against the split itself.
//
// One launch per census: the job table is a DEVICE array (ops.RangeCensus builds it once per job set); every workgroup takes an equal
// share of the concatenated jobs' 8192-element chunks, so blocks are dealt over the jobs by element count.  Counting: each thread owns a
// column of a [48 bins][256 threads] LDS histogram (a bin's 64 lanes hit 64 different words: one conflict-free ds_add per element, where
// a shared histogram would serialise on the 3-6 bins most elements share), zero / nonfinite / over in registers; a workgroup merges its
// columns once per job it touched, with one 32-bit global atomic per non-empty counter.  Integer atomics only: the counts are bitwise
// reproducible.  A second, one-workgroup launch adds the census's counts into the running table, computes each job's low-bit share
// and keeps its maximum with the step it was reached at.
#include "common.h"
#include "h2.h"

namespace {

constexpr int RC_THREADS = 256;
constexpr int RC_LBINS = PNNP_CENSUS_BINS;           // 48
constexpr int RC_CHUNK = 8192;                       // elements per work item
constexpr int RC_BLOCKS_PER_CU = 3;                  // 52 KB of LDS each: three fill a CU
typedef float rc_f4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) const rc_f4 rc_gf4;   // global, not flat: the loads then do not count against the LDS adds' lgkmcnt

// floor(log2 |x|) of a finite, non-zero float from its magnitude bits
__device__ __forceinline__ int rc_flog2(unsigned ax) {
    const int E = (int)(ax >> 23);
    return E ? E - 127 : (31 - __builtin_clz(ax)) - 149;
}

__device__ __forceinline__ unsigned* rc_scratch(uint64_t* table, int row) {
    return reinterpret_cast<unsigned*>(table + PNNP_CENSUS_HDR_WORDS + (int64_t)row * PNNP_CENSUS_ROW_WORDS + PNNP_CENSUS_SCRATCH);
}

__device__ __forceinline__ unsigned rc_wave_sum(unsigned v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += (unsigned)__shfl_xor((int)v, s, 64);
    return v;
}

__global__ void __launch_bounds__(RC_THREADS) range_census_kernel(const PnnpCensusJob* __restrict__ jobs, int njobs, uint64_t* __restrict__ table) {
    __shared__ unsigned hist[RC_LBINS * RC_THREADS];                 // [bin][thread]
    __shared__ long long pre[PNNP_CENSUS_MAX_JOBS + 1];              // chunk prefix over the jobs
    __shared__ unsigned red[RC_THREADS / 64][3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < RC_LBINS * RC_THREADS; i += RC_THREADS) hist[i] = 0u;
    if (wave == 0) {                                                 // inclusive scan of the jobs' chunk counts, 64 at a time
        long long carry = 0;
        if (lane == 0) pre[0] = 0;
        for (int b = 0; b < njobs; b += 64) {
            const int j = b + lane;
            long long v = j < njobs ? (jobs[j].n + RC_CHUNK - 1) / RC_CHUNK : 0;
#pragma unroll
            for (int s = 1; s < 64; s <<= 1) {
                const long long o = __shfl_up(v, s, 64);
                if (lane >= s) v += o;
            }
            if (j < njobs) pre[j + 1] = carry + v;
            carry += __shfl(v, 63, 64);
        }
    }
    __syncthreads();
    const long long total = pre[njobs];
    const long long c0 = total * blockIdx.x / gridDim.x, c1 = total * (blockIdx.x + 1) / gridDim.x;
    if (c0 >= c1) return;
    int j = 0;
    {
        int lo = 0, hi = njobs - 1;                                  // the job holding chunk c0: the last j with pre[j] <= c0
        while (lo < hi) { const int m = (lo + hi + 1) >> 1; if (pre[m] <= c0) lo = m; else hi = m - 1; }
        j = lo;
    }
    long long c = c0;
    for (; c < c1 && j < njobs; ++j) {
        const long long cend = pre[j + 1] < c1 ? pre[j + 1] : c1;
        if (c >= cend) continue;                                     // (an empty job)
        const PnnpCensusJob job = jobs[j];
        const unsigned abits = *job.slot & 0x7fffffffu;
        const bool afin = abits < 0x7f800000u;
        const int ea = abits ? rc_flog2(abits) : 0;
        const long long e0 = (c - pre[j]) * RC_CHUNK, e1n = (cend - pre[j]) * RC_CHUNK;
        const long long e1 = e1n < job.n ? e1n : job.n;
        unsigned nzero = 0, nnonfin = 0, nover = 0;
        auto put = [&](float v) {
            const unsigned ax = __float_as_uint(v) & 0x7fffffffu;
            nnonfin += ax >= 0x7f800000u;
            if (!afin) return;
            nzero += ax == 0u;
            if (ax != 0u && ax < 0x7f800000u) {
                nover += ax > abits;
                int k = ea - rc_flog2(ax);
                k = k < 0 ? 0 : (k > RC_LBINS - 1 ? RC_LBINS - 1 : k);
                atomicAdd(&hist[k * RC_THREADS + tid], 1u);
            }
        };
        rc_gf4* __restrict__ x4 = (rc_gf4*)job.x;
        const long long q0 = e0 >> 2, q1 = e1 >> 2;                  // e0 % 4 == 0 (chunk start); whole float4 words below q1
        long long q = q0 + tid;
        for (; q + 3 * RC_THREADS < q1; q += 4 * RC_THREADS) {       // four 16-byte non-temporal loads in flight per thread
            rc_f4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = __builtin_nontemporal_load(x4 + q + u * RC_THREADS);
#pragma unroll
            for (int u = 0; u < 4; ++u) { put(v[u].x); put(v[u].y); put(v[u].z); put(v[u].w); }
        }
        for (; q < q1; q += RC_THREADS) {
            const rc_f4 v = __builtin_nontemporal_load(x4 + q);
            put(v.x); put(v.y); put(v.z); put(v.w);
        }
        for (long long e = q1 * 4 + tid; e < e1; e += RC_THREADS) put(job.x[e]);      // the job's last 1-3 elements
        // merge: the block's columns -> one atomic per non-empty counter into the job's scratch row; the columns are zeroed for the next job
        nzero = rc_wave_sum(nzero); nnonfin = rc_wave_sum(nnonfin); nover = rc_wave_sum(nover);
        if (lane == 0) { red[wave][0] = nzero; red[wave][1] = nnonfin; red[wave][2] = nover; }
        __syncthreads();
        unsigned* sc = rc_scratch(table, job.row);
        for (int b = wave; b < RC_LBINS; b += RC_THREADS / 64) {
            unsigned s = 0;
#pragma unroll
            for (int r = 0; r < RC_THREADS; r += 64) { s += hist[b * RC_THREADS + r + lane]; hist[b * RC_THREADS + r + lane] = 0u; }
            s = rc_wave_sum(s);
            if (lane == 0 && s) atomicAdd(sc + b, s);
        }
        if (tid < 3) {
            const unsigned s = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
            if (s) atomicAdd(sc + PNNP_CENSUS_ZERO + tid, s);        // ZERO, NONFINITE, OVER are consecutive
        }
        __syncthreads();
        c = cend;
    }
}

// One workgroup: this census's counts -> the running table; low-bit share, its maximum and the step of the maximum; scratch back to zero.
__global__ void __launch_bounds__(RC_THREADS) range_census_finalize(const PnnpCensusJob* __restrict__ jobs, int njobs, uint64_t* __restrict__ table,
                                                                    long long step) {
    const int kmin = (int)table[0];
    for (int j = threadIdx.x; j < njobs; j += RC_THREADS) {
        const PnnpCensusJob job = jobs[j];
        uint64_t* row = table + PNNP_CENSUS_HDR_WORDS + (int64_t)job.row * PNNP_CENSUS_ROW_WORDS;
        unsigned* sc = rc_scratch(table, job.row);
        uint64_t all = 0, low = 0;
        for (int b = 0; b < PNNP_CENSUS_COUNTERS; ++b) {
            const unsigned v = sc[b];
            row[b] += v;
            sc[b] = 0u;
            if (b < RC_LBINS) { all += v; low += b >= kmin ? v : 0u; }
        }
        const float share = all ? (float)((double)low / (double)all) : 0.f;
        const unsigned sbits = __float_as_uint(share);
        if (row[PNNP_CENSUS_CENSUSES] == 0 || sbits > (unsigned)row[PNNP_CENSUS_WORST]) {     // (non-negative floats order like their bits)
            row[PNNP_CENSUS_WORST] = sbits;
            row[PNNP_CENSUS_WORST_STEP] = (uint64_t)step;
        }
        row[PNNP_CENSUS_LAST] = sbits;
        row[PNNP_CENSUS_AMAX] = *job.slot;
        row[PNNP_CENSUS_CENSUSES] += 1;
    }
    if (threadIdx.x == 0) { table[1] += 1; table[2] = (uint64_t)step; }
}

}  // namespace

extern "C" {

int pnnp_census_job_bytes(void) { return (int)sizeof(PnnpCensusJob); }
int64_t pnnp_census_table_words(int rows) { return rows < 0 ? -1 : PNNP_CENSUS_HDR_WORDS + (int64_t)rows * PNNP_CENSUS_ROW_WORDS; }

int pnnp_range_census_f32(const PnnpCensusJob* jobs, int njobs, uint64_t* table, long long step, void* stream) {
    if (!jobs || !table || njobs <= 0 || njobs > PNNP_CENSUS_MAX_JOBS || (((uintptr_t)jobs) & 15) || (((uintptr_t)table) & 15)) return PNNP_E_INVALID;
    const int grid = RC_BLOCKS_PER_CU * pnnp_device_cus();
    hipLaunchKernelGGL(range_census_kernel, dim3(grid), dim3(RC_THREADS), 0, as_stream(stream), jobs, njobs, table);
    hipLaunchKernelGGL(range_census_finalize, dim3(1), dim3(RC_THREADS), 0, as_stream(stream), jobs, njobs, table, step);
    return pnnp_launch_status();
}

}  // extern "C"

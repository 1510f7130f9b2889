// Pointwise convolutions as a float32 GEMM on the low-precision matrix cores, float32 operands split into pieces on the fly: ConvTranspose2d(k2, s2)
// forward / backward-data, 1x1 shortcuts, the stride-2 3x3 convolution as 9 strided taps and its backward-data per input-pixel parity class -- one tap
// per K segment, described by IgemmArgs (csrc/gemm_x3.hip's contract).  ONE kernel for all split schemes; what a scheme is comes from the `Scheme` of
// csrc/gemm_x3s.hip (bf16x3, exact three-way split), csrc/gemm_h2s.hip (fp16x2, two scaled pieces) or csrc/gemm_h1s.hip (fp16x1, one scaled piece: eval forward
// only), which also pick the tile of a launch.
//
// A workgroup has SPECIALISED waves:
//   8 CONSUMER waves (two per SIMD), 64 pixels x WN = 64 (32) columns each: ds_read_b128 + v_mfma_f32_16x16x32 only (pieces concatenated along K, weights
//     as the first operand), epilogue straight from the accumulators, stores left in flight;
//   4 PRODUCER waves (one per SIMD): per K item (Scheme::CH channels) the weights by LDS-DMA into a ring of A + 1 stages and the activations fp32 global ->
//     one of A register sets -> split -> the other of two LDS images [piece][octet][pixel] of 16-byte words, both requested A items ahead.  vmcnt completes
//     in issue order, so the weights must be requested as early as the activations.
// One s_barrier per item.  A workgroup walks tiles t, t + G, ... (persistent grid) with a cursor over (tile, K segment, item).  The packed weights hold, per
// 32-column block and item, WBLK1 contiguous bytes (csrc/pack_jobs.hip), fetched as 1 KB LDS-DMA pieces.  Three epilogues -- plain (bias, activation), act'
// masks, general (residual, accumulation) -- and, where the scheme has it, act' masks as the 3x3 forward kernel's sign bits (EK_BWDB).
//
// A Scheme provides: Args (the kernel argument) and g() (its IgemmArgs part); CH channels per K item and PIECES per value (images [PIECES][CH / 8][pixel], WBLK1 =
// PIECES x CH / 8 x 512 bytes); nwm(BN, WN) consumer waves along the pixels (tile = 64 nwm pixels; the others of the 8 only keep the barriers) and lookahead(PT) = A;
// split() of two values into their pieces (the producers); gen_lean(BN, WN): the general epilogue on a register diet (see there); the consumers' NAF pixel-operand forms and NPROD (three, or fp16x1's one) weight-operand forms as the coefficients AH, AC / WH, WC, WO
// of the image plane [piece][octet] / the row [32][16 B] of a weight block that a K group of a form reads (see the consumers' offsets),
// fa(sp) / fb(sp) = the forms of product sp of the NPROD per (pixel block, column block), and mfma(); SCALED / scale_exps(): power-of-two operand scales
// from the tensors' amax slots, undone in the epilogue; BITS: whether Args carries sign-bit masks (EK_BWDB).
#pragma once
#include "igemm.h"

namespace {

constexpr int NCW = 8, NPW = 4, NTHR = 64 * (NCW + NPW), PTHR = 64 * NPW;
constexpr int MT = 2;                                              // pixel rows (of 32 px) per consumer wave
constexpr unsigned OOB = 0x80000000u;
#ifndef GEMMS_STORE_AUX
#define GEMMS_STORE_AUX 2            // cache-policy bits of the epilogue's stores: 2 = nt (non-temporal, as in csrc/conv_s.h: config 3 +0.3 %, config 5 +0.6 %,
                                   // three alternating same-box pairs: profiles/r4/ab_store_policy.txt)
#endif
#define GS_VMCNT(N) (0x0f70 | ((N) & 15) | (((N) >> 4) << 14))
#define GS_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")      // (see csrc/conv_s.h: not __syncthreads())

// Element types of the activations (csrc/gemm_h1s.hip H1ga; the 3x3 twin: csrc/conv_s.h SElem): a scheme with SRC16 reads its K segments as fp16 NHWC tensors
// (one 16-byte load per staging slot, the word goes into the image as loaded: no split, no scale), one with DST16 stores dst[0] as fp16 (one round to
// nearest even of the float32 value the plain epilogue would store).  A scheme that names neither has float32 on both sides.
template <class S, class = void> struct GElem { static constexpr bool SRC16 = false, DST16 = false; };
template <class S> struct GElem<S, std::void_t<decltype(S::SRC16), decltype(S::DST16)>> { static constexpr bool SRC16 = S::SRC16, DST16 = S::DST16; };

template <class Scheme, int BN, int WN_> struct GCfg {
    static constexpr int WN = WN_;                                 // columns per consumer wave: 64 or 32
    static constexpr int OCT = Scheme::CH / 8, OSH = Scheme::CH / 16;      // 8-channel octets of an item: 2 / 4, and their log2
    static constexpr int WBLK1 = Scheme::PIECES * OCT * 32 * 16;   // one item of one 32-column block: 3072 / 4096 bytes
    static constexpr int NWN = BN / WN, NWM = Scheme::nwm(BN, WN); // consumer waves along N and along the pixels
    static constexpr int NACT = NWN * NWM;                         // consumer waves that compute
    static constexpr int TH = NWM * MT, PT = TH * 32;              // tile: 8 / 16 rows of 32 px = 256 / 512 pixels
    static constexpr int NB = WN / 16, NTW = WN / 32;              // 16-column accumulator blocks / 32-column blocks per wave
    static constexpr int XS_F4 = Scheme::PIECES * OCT * PT, XS_BYTES = XS_F4 * 16;      // one image: [piece][octet][pixel] 16-byte words
    static constexpr int WS_STAGE = (BN / 32) * WBLK1;
    static constexpr int NDMA = WS_STAGE / 1024, DPW = (NDMA + NPW - 1) / NPW;
    static constexpr int NSL = OCT * PT / PTHR;                    // (pixel, octet) staging slots per producer thread and item
    static constexpr int A = Scheme::lookahead(PT);                // items of lookahead (= register sets of the producers); ring of A + 1 weight stages
    static constexpr int NSTAGE = A + 1;
    static constexpr int LDS_BYTES = 2 * XS_BYTES + NSTAGE * WS_STAGE;
    static_assert(NWN * WN == BN && (NWN == 1 || NWN == 2) && NACT <= NCW && OCT == 1 << OSH, "tile shapes");
    static_assert(LDS_BYTES <= 160 * 1024, "a workgroup's LDS");
    static_assert(A * 2 * NSL + (A - 1) * DPW <= 63, "the producers' vmcnt");
};

__device__ __forceinline__ int xcd_remap(int id, int n) {
    const int q = n >> 3, r = n & 7, x = id & 7, k = id >> 3;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + k;
}

// -DGEMMS_STAMPS (debug build): cycle sums per wave, dumped into dst[0] as 8 floats per wave at ((workgroup x 12 + wave) x 8): a producer's
// [requests, split, vmcnt wait, barrier, whole kernel, items], a consumer's [MFMAs, epilogue, barrier, loop top, whole kernel, items]; [6], [7] unused
#ifdef GEMMS_STAMPS
#define GS_T(v) { const long long now_ = clock64(); v += now_ - tlast_; tlast_ = now_; }
#else
#define GS_T(v)
#endif
enum { EK_FWD = 0, EK_BWD = 1, EK_GEN = 2, EK_BWDB = 3 };          // the epilogue a kernel carries: plain / act' masks (float32) / residual + accumulation / act' masks as the
                                                                   // 3x3 forward kernel's SIGN BITS (round 6: ConvTranspose2d backward-data read 503 MB of float32 activations per step as masks)

template <class Scheme, int BN, int WN, int EK>
__global__ void __launch_bounds__(NTHR, 1)
gemm_s_kernel(const typename Scheme::Args ha) {
    const IgemmArgs& a = Scheme::g(ha);
    using Cfg = GCfg<Scheme, BN, WN>;
    constexpr int TH = Cfg::TH, PT = Cfg::PT, NB = Cfg::NB, NTW = Cfg::NTW, NSL = Cfg::NSL, D = Cfg::DPW, XS_F4 = Cfg::XS_F4, A = Cfg::A, NSTAGE = Cfg::NSTAGE;
    constexpr int OCT = Cfg::OCT, WBLK1 = Cfg::WBLK1, NP1 = WBLK1 / 1024;      // (NP1: 1 KB LDS-DMA pieces per 32-column block and item)
    constexpr bool SRC16 = GElem<Scheme>::SRC16, DST16 = GElem<Scheme>::DST16;
    constexpr int SRC_ES = SRC16 ? 2 : 4, LPS = SRC16 ? 1 : 2;       // bytes per source element; 16-byte loads per staging slot (8 channels)
    static_assert(!DST16 || EK == EK_FWD, "the epilogue with an fp16 destination");
    static_assert(!SRC16 || Scheme::PIECES == 1, "an fp16 source is its own single piece");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    u32x4* xs = reinterpret_cast<u32x4*>(smem);                     // two activation images
    char* wsb = smem + 2 * Cfg::XS_BYTES;                           // the weight ring

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);       // 0 .. 7 consumers, 8 .. 11 producers
    int se_x = 0, se_w = 0;                                          // scale exponents of the activations / the weights (scaled schemes)
    if constexpr (Scheme::SCALED) Scheme::scale_exps(ha, se_x, se_w);

    const int tiles_x = (a.DW + 31) >> 5, tiles_y = (a.DH + TH - 1) / TH;
    const int n_tiles = (a.Ntot + BN - 1) / BN;
    const int total = tiles_x * tiles_y * a.B * n_tiles;
    const int G = gridDim.x;
    const int nitems = a.nseg * a.chunks_per_seg;                   // items of K
    struct Tile { int b, y0, x0, n0; };
    auto decode = [&](int t) {
        Tile o;
        const int nt_i = t % n_tiles;
        int m_i = t / n_tiles;
        const int tx = m_i % tiles_x; m_i /= tiles_x;
        o.x0 = tx * 32; o.y0 = (m_i % tiles_y) * TH; o.b = m_i / tiles_y; o.n0 = nt_i * BN;
        return o;
    };
    // A cursor walks this workgroup's items (tile t, t + G, ...; inside a tile the K segments, inside a segment its items) ONE
    // item at a time with additions and carries only: decoding a tile number costs six integer divisions by run-time values, and with
    // one decode per lookahead per item (first version) the producers spent 1750 of an item's 3100 cycles on bookkeeping.
    const Tile gstep = decode(G);
    auto advance = [&](Tile o) {
        o.n0 += gstep.n0; if (o.n0 >= n_tiles * BN) { o.n0 -= n_tiles * BN; o.x0 += 32; }
        o.x0 += gstep.x0; if (o.x0 >= tiles_x * 32) { o.x0 -= tiles_x * 32; o.y0 += TH; }
        o.y0 += gstep.y0; if (o.y0 >= tiles_y * TH) { o.y0 -= tiles_y * TH; o.b += 1; }
        o.b += gstep.b;
        return o;
    };
    struct It { Tile tile; int t, g, si, cc; bool ok; };
    auto step = [&](It& c) {
        ++c.g;
        if (++c.cc == a.chunks_per_seg) { c.cc = 0; ++c.si; }
        if (c.g == nitems) { c.g = 0; c.si = 0; c.cc = 0; c.t += G; c.tile = advance(c.tile); c.ok = c.t < total; }
    };
    It cu;                                                           // the current item
    cu.t = xcd_remap(blockIdx.x, G);
    if (cu.t >= total) return;
    cu.tile = decode(cu.t); cu.g = 0; cu.si = 0; cu.cc = 0; cu.ok = true;

    if (wave >= NCW) {
        // =============================================== PRODUCER ===============================================
        const int pw = wave - NCW, ptid = tid - 64 * NCW;
        // staging slots: s = ptid + 256 k -> (pixel s / OCT, channel octet s % OCT): OCT consecutive lanes read the contiguous bytes of a pixel
        const int oct = ptid & (OCT - 1);
        const float sx = __uint_as_float((unsigned)(se_x + 127) << 23);      // 2^se_x
        int prow[NSL], pcol[NSL], xdst[NSL];
#pragma unroll
        for (int k = 0; k < NSL; ++k) {
            const int pix = (ptid + PTHR * k) >> Cfg::OSH;
            prow[k] = pix >> 5; pcol[k] = pix & 31;
            xdst[k] = oct * PT + pix;                               // + piece * OCT PT (+ image * XS_F4)
        }
        const __amdgpu_buffer_rsrc_t rsw = __builtin_amdgcn_make_buffer_rsrc((void*)a.w, 0, 0x7fffffff, 0x00020000);
        f32x4 ra[A][NSL][LPS];                                      // A register sets: the activations of the next A items (SRC16: one word per slot, fp16 as loaded)
        // What a request needs is computed once per (tile, K segment) -- resource, scalar offset, the slots' lane offsets and validity -- and
        // once per tile for the weights; inside a segment the next item is CH channels (4 CH bytes) on, the next k-step of the pack WBLK1 bytes
        // on.  (A producer shares its SIMD with two MFMA waves and gets an issue slot every ~8 cycles: the ~150 instructions of a request
        // computed from scratch took 1200 cycles of a 1536-cycle item.)
        const float* la_base = a.w; int la_soff = 0; unsigned la_vo[NSL];      // (the resource is re-made from the pointer: 4 scalar moves)
        static_assert(D <= 4, "LDS-DMA pieces per producer wave");
        int la_wsoff[4]; unsigned la_wvo[4];                        // (a literal size: with [D] the host pass of hipcc 7.2 silently drops the kernel stubs)
#pragma unroll
        for (int k = 0; k < NSL; ++k) la_vo[k] = OOB;
#pragma unroll
        for (int i = 0; i < 4; ++i) { la_wsoff[i] = 0; la_wvo[i] = OOB; }
        auto load_item = [&](const It& q, auto set_tag) {
            constexpr int set = decltype(set_tag)::value;
            if (q.cc == 0) {                                        // first item of a segment (of a tile)
                const Tile& tl = q.tile;
                const IgemmSeg sg = a.seg[q.si];
                const int mul = a.in_mul;
                const int shift = (a.IW + 1) * sg.cstride;         // the resource starts before the image: offsets >= -1 pixel stay >= 0
                const int64_t first = (int64_t)tl.b * a.IH * a.IW * sg.cstride - shift;      // (elements)
                la_base = SRC16 ? reinterpret_cast<const float*>(reinterpret_cast<const _Float16*>(sg.ptr) + first) : sg.ptr + first;
                la_soff = (((tl.y0 * mul + sg.yoff) * a.IW + tl.x0 * mul + sg.xoff) * sg.cstride + sg.coff + shift) * SRC_ES;
                const unsigned cs4 = (unsigned)sg.cstride * (unsigned)SRC_ES;
#pragma unroll
                for (int k = 0; k < NSL; ++k) {
                    const int iy = (tl.y0 + prow[k]) * mul + sg.yoff, ix = (tl.x0 + pcol[k]) * mul + sg.xoff;
                    const int bad = iy | (a.IH - 1 - iy) | ix | (a.IW - 1 - ix) | (a.DH - 1 - tl.y0 - prow[k]) | (a.DW - 1 - tl.x0 - pcol[k]) | (q.ok ? 0 : -1);
                    la_vo[k] = bad < 0 ? OOB : __umul24((unsigned)((prow[k] * a.IW + pcol[k]) * mul), cs4) + oct * (8 * SRC_ES);
                }
            }
            const __amdgpu_buffer_rsrc_t la_rs = __builtin_amdgcn_make_buffer_rsrc((void*)la_base, 0, 0x7fffffff, 0x00020000);
#pragma unroll
            for (int k = 0; k < NSL; ++k) {
                ra[set][k][0] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(la_rs, la_vo[k], la_soff, 0));
                if constexpr (!SRC16) ra[set][k][1] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(la_rs, la_vo[k], la_soff + 16, 0));
            }
            la_soff += Scheme::CH * SRC_ES;
        };
        auto stage_set = [&](auto set_tag, int img) {
            constexpr int set = decltype(set_tag)::value;
#pragma unroll
            for (int k = 0; k < NSL; ++k) {
                if constexpr (SRC16) {                               // the eight halves are the image's word: nothing to split, no scale (se_x = 0)
                    xs[img * XS_F4 + xdst[k]] = __builtin_bit_cast(u32x4, ra[set][k][0]);
                    continue;
                }
                u32x4 sp[Scheme::PIECES];
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const f32x4 v = ra[set][k][SRC16 ? 0 : p >> 1];
                    unsigned pc[Scheme::PIECES];
                    Scheme::split(v[(p & 1) * 2], v[(p & 1) * 2 + 1], sx, pc);
#pragma unroll
                    for (int i = 0; i < Scheme::PIECES; ++i) sp[i][p] = pc[i];
                }
                u32x4* d = xs + img * XS_F4 + xdst[k];
#pragma unroll
                for (int i = 0; i < Scheme::PIECES; ++i) d[i * OCT * PT] = sp[i];
            }
        };
        // LDS-DMA of the weights of item q into stage st: per 32-column block the WBLK1 contiguous bytes of its k-step, as 1 KB pieces
        auto dma_weights = [&](const It& q, int st) {
            if (q.g == 0) {                                         // first item of a tile
#pragma unroll
                for (int i = 0; i < D; ++i) {
                    const int ins = min(pw + NPW * i, Cfg::NDMA - 1);
                    const int j = NP1 == 4 ? ins >> 2 : ins / NP1, r = ins - NP1 * j;      // (ins >= 0: the shift spares the sign fix-up of a signed division)
                    const int nb = (q.tile.n0 >> 5) + j;
                    const bool ok = q.ok && nb * 32 < a.Ntot;
                    la_wsoff[i] = ok ? (nb * nitems * WBLK1 + r * 1024) : 0;
                    la_wvo[i] = ok ? (unsigned)lane * 16u : OOB;
                }
            }
#pragma unroll
            for (int i = 0; i < D; ++i) {
                const int ins = min(pw + NPW * i, Cfg::NDMA - 1);
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsw, (__attribute__((address_space(3))) void*)(wsb + st * Cfg::WS_STAGE + ins * 1024),
                                                         16, la_wvo[i], la_wsoff[i], 0, 0);
                la_wsoff[i] += WBLK1;
            }
        };
        // ---- prologue: weights and activations of items 0 .. A - 1 (stage j, set j); item 0 straight into image 0
        It la = cu;                                                  // the lookahead cursor: A items ahead of cu
        static_for<0, A>([&](auto J) { constexpr int j = decltype(J)::value; dma_weights(la, j); load_item(la, J); step(la); });
        stage_set(std::integral_constant<int, 0>{}, 0);
        GS_BARRIER();                                               // barrier 0 (the wait for set 0 covered the weights of item 0)
        int it = 0, st = 0;                                          // items since the start (image it & 1); stage of item it
        // Item it, S = it mod A: [weights of item it + A -> the stage item it - 1 left] [activations of item it + A -> set S, split during
        // item it - 1] [split the set of item it + 1 into image (it + 1) & 1]; in front of the barrier the weights of item it + 1
        // (requested A - 1 blocks ago) must have landed: vmcnt(what was issued behind them = A x the loads of an item + (A - 1) x its LDS-DMAs).
#ifdef GEMMS_STAMPS
        long long t_req = 0, t_split = 0, t_wait = 0, t_bar = 0, tlast_ = clock64(), tall = tlast_;
#endif
        auto block = [&](auto s_tag) __attribute__((always_inline)) {
            constexpr int S = decltype(s_tag)::value;
            dma_weights(la, st == 0 ? NSTAGE - 1 : st - 1);
            load_item(la, s_tag);
            step(la);
            GS_T(t_req)
            stage_set(std::integral_constant<int, (S + 1) % A>{}, (it + 1) & 1);
            GS_T(t_split)
            __builtin_amdgcn_s_waitcnt(GS_VMCNT(A * LPS * NSL + (A - 1) * D));
            GS_T(t_wait)
            step(cu);
            if (!cu.ok) return false;
            GS_BARRIER();
            GS_T(t_bar)
            ++it; st = st == NSTAGE - 1 ? 0 : st + 1;
            return true;
        };
        for (;;) {
            bool go = true;
            static_for<0, A>([&](auto S) { if (go) go = block(S); });
            if (!go) break;
        }
#ifdef GEMMS_STAMPS
        if (lane == 0) {
            float* d = a.dst[0] + ((int64_t)blockIdx.x * (NCW + NPW) + wave) * 8;
            d[0] = (float)t_req; d[1] = (float)t_split; d[2] = (float)t_wait; d[3] = (float)t_bar; d[4] = (float)(clock64() - tall); d[5] = (float)(it + 1);
        }
#endif
        return;
    }

    // =============================================== CONSUMER ===============================================
    if constexpr (Cfg::NACT < NCW) {
        if (wave >= Cfg::NACT) {                                     // a consumer wave without a share: the barriers of the item loop, nothing else
            GS_BARRIER();
            for (;;) {
                step(cu);
                if (!cu.ok) break;
                GS_BARRIER();
            }
            return;
        }
    }
    const int wn = wave % Cfg::NWN, wm = wave / Cfg::NWN;             // this wave's column group / pixel-row pair
    constexpr int MB = 2 * MT, NAF = Scheme::NAF, NPR = Scheme::NPROD;      // pixel-operand forms; products (= weight-operand forms) per (pixel block, column block)
    f32x4 acc[MB][NB];
#pragma unroll
    for (int i = 0; i < MB; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int r16 = lane & 15, q16 = lane >> 4;                      // pixel / column of the block; the lane's K group of 8
    // The lane's offsets of the operand forms.  K group q16 = (half q16 >> 1, octet q16 & 1) of pixel form f reads image plane AH[f] half + AC[f] + octet, of weight
    // form f the rows WH[f] half + WC[f] + WO octet of a block's [.][32][16 B].  (Written out here, not as functions of the scheme, and with `q16 & 2` for 2 half:
    // behind a function the compiler keeps one register per operand address instead of one base and the reads' immediate offsets.)
    const int pb = wm * (MT * 32) + r16;
#define GS_AOFF(f) (((Scheme::AH[f] == 2 ? (q16 & 2) : (q16 >> 1) * Scheme::AH[f]) + Scheme::AC[f] + (q16 & 1)) * PT + pb)
#define GS_BOFF(f) ((((Scheme::WH[f] == 2 ? (q16 & 2) : (q16 >> 1) * Scheme::WH[f]) + Scheme::WC[f] + (q16 & 1) * Scheme::WO) * 32 + r16) * 16)
    // (a scheme with fewer forms repeats its last one: the unused offsets fold away)
    const int aoff0 = GS_AOFF(0), aoff1 = GS_AOFF(NAF > 1 ? 1 : 0), aoff2 = GS_AOFF(NAF - 1);
    const int boff0 = GS_BOFF(0), boff1 = GS_BOFF(NPR > 1 ? 1 : 0), boff2 = GS_BOFF(NPR - 1);
#undef GS_AOFF
#undef GS_BOFF
    auto mfma_item = [&](int st, int img) {
        const char* wst = wsb + st * Cfg::WS_STAGE + wn * NTW * WBLK1;
        const u32x4* xim = xs + img * XS_F4;
        u32x4 Av[MB][NAF], Bv[2][NPR];
        auto a_read = [&](int mb, int f) { Av[mb][f] = xim[(f == 0 ? aoff0 : (f == 1 ? aoff1 : aoff2)) + (mb >> 1) * 32 + 16 * (mb & 1)]; };
        auto b_read = [&](int j, int f, int buf) {
            Bv[buf][f] = *reinterpret_cast<const u32x4*>(wst + (j >> 1) * WBLK1 + (f == 0 ? boff0 : (f == 1 ? boff1 : boff2)) + (j & 1) * 256);
        };
#pragma unroll
        for (int f = 0; f < NPR; ++f) b_read(0, NPR - 1 - f, 0);
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
#pragma unroll
            for (int f = NAF - 1; f >= 0; --f) a_read(mb, f);
        __builtin_amdgcn_sched_barrier(0);
        static_for<0, NB * MB * NPR>([&](auto Gc) {
            constexpr int gi = decltype(Gc)::value;
            constexpr int j = gi / (MB * NPR), w = gi % (MB * NPR), mb = w / NPR, sp = w % NPR, buf = j & 1;
            acc[mb][j] = Scheme::mfma(Bv[buf][Scheme::fb(sp)], Av[mb][Scheme::fa(sp)], acc[mb][j]);      // smallest terms first
            if constexpr (w < NPR && j + 1 < NB) b_read(j + 1, NPR - 1 - w, buf ^ 1);
            __builtin_amdgcn_sched_barrier(0);
        });
    };

    // ---- epilogue, straight from the accumulators (a lane holds 4 consecutive channels of one pixel): sub-pixel scatter of ConvTranspose2d
    // forward (n_sub), strided / offset outputs (out_mul, out_yoff / out_xoff), two destinations (n_split), bias, activation, act' mask,
    // residual, accumulation -- csrc/gemm_x3.hip's contract
    float amx0 = 0.f;                                                // max |stored value| of this lane, destination 0 (a.amax_out[0]; the launcher refuses [1])
    auto epilogue = [&](const Tile& tl) __attribute__((always_inline)) {
        const int b = tl.b;
        // LEAN (Scheme::gen_lean(BN, WN)): the general epilogue on a register diet -- the lane number as an OPAQUE value (csrc/conv_s_body.h: what is derived from it is computed
        // here, per tile, instead of being hoisted in front of the item loop and carried through it), one 32-column block's offsets and bias words at a time, one pixel
        // row of mask / residual / previous words in flight.  fp16x2's 128-column kernel needs it (it spilled without); bf16x3's kernels have the registers for
        // everything up front and both rows in flight (168, no spills), and were 2.5-5.7 % slower on the diet at ResUnet's 256^2 and 512^2 maps (stride-2 backward-data
        // accumulating, 1x1 forward + residual; 256 px x 128, 512 px x 64 and 512 px x 32 tiles) -- bf16x3's 256 px x 64 tile, the small layers', stays lean: 127 registers
        // and 4 waves per SIMD where everything up front takes 129 and 3.  The other epilogues sit at exactly 168 registers without spilling as they are.
        constexpr bool LEAN = EK == EK_GEN && Scheme::gen_lean(BN, WN);
        int lane_e = lane;
        if constexpr (LEAN) asm volatile("" : "+v"(lane_e));
        const int p16 = lane_e & 15, c4 = (lane_e >> 4) * 4;
        const int py0 = tl.y0 + wm * MT, px0 = tl.x0 + p16;
        int du_[NTW], cs_[NTW], bch_[NTW]; bool blk_[NTW];
        unsigned vo[NTW][MT][2];
        // the destination, the channel and the lanes' byte offsets of 32-column block k
        [[maybe_unused]] auto block_setup = [&](int k) __attribute__((always_inline)) {
            const int nwv = __builtin_amdgcn_readfirstlane(tl.n0 + wn * WN + k * 32);
            const int du = nwv >= a.n_split ? 1 : 0;
            const int subu = a.n_sub ? nwv / a.n_sub : 0;
            const int chw = nwv - subu * a.n_sub - (du ? a.n_split : 0);
            const int yo2 = a.out_yoff + (subu >> 1), xo2 = a.out_xoff + (subu & 1);
            du_[k] = du; cs_[k] = a.dst_cs[du]; blk_[k] = nwv < a.Ntot; bch_[k] = nwv - subu * a.n_sub;
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int py = py0 + i, px = px0 + 16 * h;
                    const int oy = py * a.out_mul + yo2, ox = px * a.out_mul + xo2;
                    const bool ok = blk_[k] && py < a.DH && px < a.DW && oy >= 0 && oy < a.OH && ox >= 0 && ox < a.OW;
                    vo[k][i][h] = ok ? (unsigned)(((oy * a.OW + ox) * cs_[k] + chw + c4) * 4) : OOB;
                }
        };
        // (block_setup and, below, bias_load WRITTEN OUT for the epilogues that keep everything up front: through the lambdas they come out in another schedule,
        //  and the 128-column fp16x2 kernel with float masks, which sits at 168 registers, spills 5 of them into a 24-byte scratch frame)
        if constexpr (!LEAN) {
#pragma unroll
            for (int k = 0; k < NTW; ++k) {
                const int nwv = __builtin_amdgcn_readfirstlane(tl.n0 + wn * WN + k * 32);
                const int du = nwv >= a.n_split ? 1 : 0;
                const int subu = a.n_sub ? nwv / a.n_sub : 0;
                const int chw = nwv - subu * a.n_sub - (du ? a.n_split : 0);
                const int yo2 = a.out_yoff + (subu >> 1), xo2 = a.out_xoff + (subu & 1);
                du_[k] = du; cs_[k] = a.dst_cs[du]; blk_[k] = nwv < a.Ntot; bch_[k] = nwv - subu * a.n_sub;
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const int py = py0 + i, px = px0 + 16 * h;
                        const int oy = py * a.out_mul + yo2, ox = px * a.out_mul + xo2;
                        const bool ok = blk_[k] && py < a.DH && px < a.DW && oy >= 0 && oy < a.OH && ox >= 0 && ox < a.OW;
                        vo[k][i][h] = ok ? (unsigned)(((oy * a.OW + ox) * cs_[k] + chw + c4) * (DST16 ? 2 : 4)) : OOB;      // (bytes of the destination's element type)
                    }
            }
        }
        auto rsrc = [&](const float* base, int k) {
            return __builtin_amdgcn_make_buffer_rsrc((void*)(base + (int64_t)b * a.OH * a.OW * cs_[k]), 0, a.OH * a.OW * cs_[k] * 4, 0x00020000);
        };
        const float aslope = a.act == 1 ? 0.2f : (a.act == 2 ? 0.f : 1.f);
        f32x4 bias4[NB];
        [[maybe_unused]] auto bias_load = [&](int j) __attribute__((always_inline)) {
            bias4[j] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (a.bias && blk_[j >> 1]) bias4[j] = *reinterpret_cast<const f32x4*>(a.bias + bch_[j >> 1] + 16 * (j & 1) + c4);
        };
        if constexpr (!LEAN) {
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                bias4[j] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (a.bias && blk_[j >> 1]) bias4[j] = *reinterpret_cast<const f32x4*>(a.bias + bch_[j >> 1] + 16 * (j & 1) + c4);
            }
        }
        auto act4 = [&](f32x4 o) {
            const f32x4 t = o * aslope;
#pragma unroll
            for (int c = 0; c < 4; ++c) o[c] = fmaxf(o[c], t[c]);
            return o;
        };
        // (scaled schemes) undoing the operand scales: x 2^dexp (exact) as one multiplier while 2^dexp is a normal float32; tensors so small / large that it is
        // not first take the remainder in a pass over the accumulators (csrc/conv_s_body.h)
        float dsc = 1.f;
        if constexpr (Scheme::SCALED) {
            const int dexp = -(se_x + se_w);
            const int dexp_c = dexp < -120 ? -120 : (dexp > 120 ? 120 : dexp);      // (|.| <= 120: 0.2 x 2^dexp_c stays a normal float32: mask_scale)
            dsc = __uint_as_float((unsigned)(dexp_c + 127) << 23);
            if (dexp != dexp_c) {
#pragma unroll
                for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                    for (int j = 0; j < NB; ++j)
#pragma unroll
                        for (int c = 0; c < 4; ++c) acc[mb][j][c] = __builtin_ldexpf(acc[mb][j][c], dexp - dexp_c);
            }
        }
        auto raw = [&](int mb, int j) { const f32x4 v = acc[mb][j]; acc[mb][j] = f32x4{0.f, 0.f, 0.f, 0.f}; return v; };
        auto take = [&](int mb, int j) { if constexpr (Scheme::SCALED) return raw(mb, j) * dsc; else return raw(mb, j); };
        // max |.| of a stored block into the lane's running maximum of destination du (uniform); lanes whose store is dropped do not count
        auto track = [&](f32x4 o, bool valid, int du) {
            const float m = fmaxf(fmaxf(fabsf(o.x), fabsf(o.y)), fmaxf(fabsf(o.z), fabsf(o.w)));
            amx0 = fmaxf(amx0, (valid && !du) ? m : 0.f);
        };
        if constexpr (EK != EK_GEN) {
            constexpr bool MASKED = EK == EK_BWD, BITS = EK == EK_BWDB;
            // FULL-LINE memory pattern (csrc/conv_s_body.h): the two 16-column blocks of a 32-column block trade halves between lanes p and p + 8
            // of a 16-lane row, so that each 16-byte store instruction writes 8 pixels x 128 bytes (whole lines) instead of 16 x 64; the
            // act' masks come in by the same pattern and are traded back.
            if constexpr (DST16) {
                // 2-byte channels (csrc/conv_s_body.h pack16): the four lanes of a pixel swap quads (v_permlane16_swap) so that 16-lane row q holds the 8 CONSECUTIVE
                // channels 16 (q & 1) + 8 (q >> 1) .. + 7 of its 32-column block, and one 16-byte store instruction writes 16 pixels x 64 bytes -- through the
                // ConvTranspose2d scatter (n_sub, out_mul) like the float32 pattern's.  One round to nearest even; amax from the float32 values.
                typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
                const int ch16 = ((lane_e >> 4) & 1) * 16 + (lane_e >> 5) * 8;
#pragma unroll
                for (int k = 0; k < NTW; ++k) {
                    const __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc((void*)(reinterpret_cast<_Float16*>(a.dst[0]) + (int64_t)b * a.OH * a.OW * cs_[k]), 0,
                                                                                        a.OH * a.OW * cs_[k] * 2, 0x00020000);
#pragma unroll
                    for (int i = 0; i < MT; ++i)
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            const f32x4 v0 = raw(2 * i + h, 2 * k), v1 = raw(2 * i + h, 2 * k + 1);
                            f32x4 o0, o1;
#pragma unroll
                            for (int c = 0; c < 4; ++c) { o0[c] = __builtin_fmaf(v0[c], dsc, bias4[2 * k][c]); o1[c] = __builtin_fmaf(v1[c], dsc, bias4[2 * k + 1][c]); }
                            o0 = act4(o0); o1 = act4(o1);           // (no branch: without an activation the slope is 1 and max(o, 1 o) = o bit for bit)
                            track(o0, vo[k][i][h] != OOB, du_[k]); track(o1, vo[k][i][h] != OOB, du_[k]);
                            const unsigned a0 = __builtin_bit_cast(unsigned, f16x2{(_Float16)o0.x, (_Float16)o0.y}), a1 = __builtin_bit_cast(unsigned, f16x2{(_Float16)o0.z, (_Float16)o0.w});
                            const unsigned b0 = __builtin_bit_cast(unsigned, f16x2{(_Float16)o1.x, (_Float16)o1.y}), b1 = __builtin_bit_cast(unsigned, f16x2{(_Float16)o1.z, (_Float16)o1.w});
                            const auto s0 = __builtin_amdgcn_permlane16_swap(a0, b0, false, false), s1 = __builtin_amdgcn_permlane16_swap(a1, b1, false, false);
                            // vo: the byte offset of (pixel, channel chw + c4) in 2-byte elements; the word of this lane starts at channel chw + ch16
                            const unsigned off = vo[k][i][h] != OOB ? vo[k][i][h] + (unsigned)((ch16 - c4) * 2) : OOB;
                            __builtin_amdgcn_raw_buffer_store_b128(u32x4{s0[0], s1[0], s0[1], s1[1]}, rd, off, 0, GEMMS_STORE_AUX);
                            __builtin_amdgcn_sched_barrier(0);
                        }
                }
                return;
            }
            const bool lo8 = p16 < 8;
            auto ror8 = [&](f32x4 v) {
                float r0, r1, r2, r3;
                asm volatile("s_nop 1\n\tv_mov_b32_dpp %0, %4 row_ror:8 row_mask:0xf bank_mask:0xf\n\tv_mov_b32_dpp %1, %5 row_ror:8 row_mask:0xf bank_mask:0xf\n\t"
                             "v_mov_b32_dpp %2, %6 row_ror:8 row_mask:0xf bank_mask:0xf\n\tv_mov_b32_dpp %3, %7 row_ror:8 row_mask:0xf bank_mask:0xf"
                             : "=&v"(r0), "=&v"(r1), "=&v"(r2), "=&v"(r3) : "v"(v.x), "v"(v.y), "v"(v.z), "v"(v.w));
                return f32x4{r0, r1, r2, r3};
            };
            auto sel = [&](bool c, f32x4 x, f32x4 y) { return f32x4{c ? x.x : y.x, c ? x.y : y.y, c ? x.z : y.z, c ? x.w : y.w}; };
            // this lane's byte offsets in instruction 1 (pixel p16 & 7 of the half) and 2 (eight pixels on) of block k
            unsigned wo[NTW][MT][2][2];
            unsigned mbits[BITS ? NTW : 1];                          // (EK_BWDB) this lane's word of the tile-private sign-bit image (csrc/h2.h) per 32-column block
            const int pxl = tl.x0 + (p16 & 7);
#pragma unroll
            for (int k = 0; k < NTW; ++k) {
                const int nwv = __builtin_amdgcn_readfirstlane(tl.n0 + wn * WN + k * 32);
                const int subu = a.n_sub ? nwv / a.n_sub : 0;
                const int chw = nwv - subu * a.n_sub - (du_[k] ? a.n_split : 0);
                if constexpr (BITS) {
                    // The 3x3 kernel's word (16-row tile ty, tile column, 32-channel block, its consumer wave w16, lane) holds rows 2 w16 + i, pixels 16 h + (lane & 15),
                    // channels 16 jj + 4 (lane >> 4) + c of the block -- exactly the 32 values THIS lane holds of the block (this wave's rows py0, py0 + 1: py0 even),
                    // in the order the loop below walks them.  Plain output geometry only (the launcher checks): out pixel = tile pixel.
                    const int tiles_x16 = (a.OW + 31) >> 5, tiles_y16 = (a.OH + 15) >> 4, nblk = ha.bits_nblk[0];
                    const int tile_id = (b * tiles_y16 + (py0 >> 4)) * tiles_x16 + (tl.x0 >> 5);
                    const unsigned word = (unsigned)((((tile_id * nblk + (chw >> 5)) * 8 + ((py0 & 15) >> 1)) * 64 + lane) * 4);
                    const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc((void*)ha.bits_in[0], 0, a.B * tiles_y16 * tiles_x16 * nblk * 8 * 64 * 4, 0x00020000);
                    mbits[k] = __builtin_amdgcn_raw_buffer_load_b32(rb, (blk_[k] && a.mask_mode[du_[k]] && !du_[k] && py0 < a.DH) ? word : OOB, 0, 0);
                }
                const int yo2 = a.out_yoff + (subu >> 1), xo2 = a.out_xoff + (subu & 1);
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int h = 0; h < 2; ++h)
#pragma unroll
                        for (int e = 0; e < 2; ++e) {
                            const int py = py0 + i, px = pxl + 16 * h + 8 * e;
                            const int oy = py * a.out_mul + yo2, ox = px * a.out_mul + xo2;
                            const bool ok = blk_[k] && py < a.DH && px < a.DW && oy >= 0 && oy < a.OH && ox >= 0 && ox < a.OW;
                            wo[k][i][h][e] = ok ? (unsigned)(((oy * a.OW + ox) * cs_[k] + chw + (lo8 ? 0 : 16) + c4) * 4) : OOB;
                        }
            }
            f32x4 mk[MASKED ? MB : 1][MASKED ? NB : 1];              // [.][2 k] = what instruction 1 fetched, [.][2 k + 1] = instruction 2
            if constexpr (MASKED) {
#pragma unroll
                for (int k = 0; k < NTW; ++k) {
                    const int mm = a.mask_mode[du_[k]];
                    const __amdgpu_buffer_rsrc_t rm = rsrc(mm ? a.mask[du_[k]] : a.dst[du_[k]], k);
#pragma unroll
                    for (int i = 0; i < MT; ++i)
#pragma unroll
                        for (int h = 0; h < 2; ++h)
#pragma unroll
                            for (int e = 0; e < 2; ++e)
                                mk[2 * i + h][2 * k + e] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rm, mm ? wo[k][i][h][e] : OOB, 0, 0));
                }
            }
#pragma unroll
            for (int k = 0; k < NTW; ++k) {
                const __amdgpu_buffer_rsrc_t rd = rsrc(a.dst[du_[k]], k);
                const int mm = a.mask_mode[du_[k]];
                const float msl = mm == 1 ? 0.2f : (mm == 0 ? 1.f : 0.f);      // act'(x <= 0); 1 for a destination without a mask
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        f32x4 o0, o1;
                        if constexpr (BITS) {
                            // scale and mask in three instructions per element (csrc/conv_s_body.h mask_scale): next bit -> vcc, 2^dexp or msl 2^dexp, multiply
                            const f32x4 v0 = raw(2 * i + h, 2 * k), v1 = raw(2 * i + h, 2 * k + 1);
                            const float fneg = dsc * msl;
                            auto ms = [&](float v) __attribute__((always_inline)) {
                                float f, o;
                                asm("v_add_co_u32 %2, vcc, %2, %2\n\tv_cndmask_b32 %1, %4, %3, vcc\n\tv_mul_f32 %0, %1, %5" : "=v"(o), "=&v"(f), "+v"(mbits[k]) : "v"(dsc), "v"(fneg), "v"(v) : "vcc");
                                return o;
                            };
#pragma unroll
                            for (int c = 0; c < 4; ++c) o0[c] = ms(v0[c]);
#pragma unroll
                            for (int c = 0; c < 4; ++c) o1[c] = ms(v1[c]);
                        } else if constexpr (!MASKED) {
                            // forward: scale and bias (scaled schemes: in ONE fma per element), then the activation only where the layer has one (ConvTranspose2d has
                            // none: it used to pay a multiply and a maximum per element for max(o, 1.0 o))
                            const f32x4 v0 = raw(2 * i + h, 2 * k), v1 = raw(2 * i + h, 2 * k + 1);
                            if constexpr (Scheme::SCALED) {
#pragma unroll
                                for (int c = 0; c < 4; ++c) { o0[c] = __builtin_fmaf(v0[c], dsc, bias4[2 * k][c]); o1[c] = __builtin_fmaf(v1[c], dsc, bias4[2 * k + 1][c]); }
                            } else { o0 = v0 + bias4[2 * k]; o1 = v1 + bias4[2 * k + 1]; }
                            if (a.act) { o0 = act4(o0); o1 = act4(o1); }
                        } else {                                    // (backward-data: no bias, no activation -- the launcher checks)
                            o0 = take(2 * i + h, 2 * k); o1 = take(2 * i + h, 2 * k + 1);
                            const f32x4 m1 = mk[2 * i + h][2 * k], m2 = mk[2 * i + h][2 * k + 1], mx = ror8(sel(lo8, m2, m1));
                            const f32x4 q0 = sel(lo8, m1, mx), q1 = sel(lo8, mx, m2);
                            const f32x4 t0 = o0 * msl, t1 = o1 * msl;
#pragma unroll
                            for (int c = 0; c < 4; ++c) { o0[c] = q0[c] > 0.f ? o0[c] : t0[c]; o1[c] = q1[c] > 0.f ? o1[c] : t1[c]; }
                        }
                        track(o0, vo[k][i][h] != OOB, du_[k]); track(o1, vo[k][i][h] != OOB, du_[k]);
                        const f32x4 ox = ror8(sel(lo8, o1, o0));
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, sel(lo8, o0, ox)), rd, wo[k][i][h][0], 0, GEMMS_STORE_AUX);
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, sel(lo8, ox, o1)), rd, wo[k][i][h][1], 0, GEMMS_STORE_AUX);
                    }
            }
            return;
        }
        // the general case (residual, accumulation), branch-free: what a block does not use is requested out of range (zeros, no traffic)
#pragma unroll
        for (int k = 0; k < NTW; ++k) {
            if constexpr (LEAN) { block_setup(k); bias_load(2 * k); bias_load(2 * k + 1); }
            const int du = du_[k], mm2 = a.mask_mode[du], acc2 = a.accum[du];
            const bool use_add2 = a.addsrc && du == 0;
            const __amdgpu_buffer_rsrc_t rd = rsrc(a.dst[du], k);
            const __amdgpu_buffer_rsrc_t rm = rsrc(mm2 ? a.mask[du] : a.dst[du], k);
            const __amdgpu_buffer_rsrc_t rad = rsrc(use_add2 ? a.addsrc : a.dst[du], k);
            const float msl = mm2 == 1 ? 0.2f : 0.f;
            constexpr int RIF = LEAN ? 1 : MT;                      // pixel rows in flight (LEAN: with both -- 48 registers -- the 128-column fp16x2 kernel spilled 7 into a 32-byte scratch frame)
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) {
#pragma unroll
                for (int i0 = 0; i0 < MT; i0 += RIF) {
                    f32x4 m2[RIF][2], ad2[RIF][2], pr2[RIF][2];
#pragma unroll
                    for (int r = 0; r < RIF; ++r)
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            m2[r][h] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rm, mm2 ? vo[k][i0 + r][h] : OOB, jj * 64, 0));
                            ad2[r][h] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rad, use_add2 ? vo[k][i0 + r][h] : OOB, jj * 64, 0));
                            pr2[r][h] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rd, acc2 ? vo[k][i0 + r][h] : OOB, jj * 64, 0));
                        }
#pragma unroll
                    for (int r = 0; r < RIF; ++r)
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            const int i = i0 + r;
                            f32x4 o = act4(take(2 * i + h, 2 * k + jj) + bias4[2 * k + jj] + ad2[r][h]);
#pragma unroll
                            for (int c = 0; c < 4; ++c) o[c] *= (m2[r][h][c] > 0.f || !mm2) ? 1.f : msl;
                            o += pr2[r][h];
                            track(o, vo[k][i][h] != OOB, du);
                            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), rd, vo[k][i][h], jj * 64, 0);
                        }
                }
            }
        }
    };

    int it = 0, st = 0;
#ifdef GEMMS_STAMPS
    long long t_mfma = 0, t_epi = 0, t_bar = 0, t_top = 0, tlast_ = clock64(), tall = tlast_;
#endif
    GS_BARRIER();                                                   // barrier 0
    GS_T(t_bar)
    for (;;) {
        GS_T(t_top)
        mfma_item(st, it & 1);
        GS_T(t_mfma)
        if (cu.g == nitems - 1) epilogue(cu.tile);
        GS_T(t_epi)
        step(cu);
        if (!cu.ok) break;
        GS_BARRIER();
        GS_T(t_bar)
        ++it; st = st == NSTAGE - 1 ? 0 : st + 1;
    }
    if (a.amax_out[0]) pnnp_amax_commit(amx0, a.amax_out[0]);
#ifdef GEMMS_STAMPS
    __builtin_amdgcn_s_waitcnt(0x0f70);
    if (lane == 0) {
        float* d = a.dst[0] + ((int64_t)blockIdx.x * (NCW + NPW) + wave) * 8;
        d[0] = (float)t_mfma; d[1] = (float)t_epi; d[2] = (float)t_bar; d[3] = (float)t_top; d[4] = (float)(clock64() - tall); d[5] = (float)(it + 1);
    }
#endif
}

template <class Scheme, int BN, int WN, int EK>
int launch_gs(const typename Scheme::Args& ha, hipStream_t s) {
    using Cfg = GCfg<Scheme, BN, WN>;
    const IgemmArgs& a = Scheme::g(ha);
    auto kern = gemm_s_kernel<Scheme, BN, WN, EK>;
    static PnnpPerDevice lds_once;
    if (pnnp_allow_lds(lds_once, kern, Cfg::LDS_BYTES) != PNNP_OK) return PNNP_E_LAUNCH;
    const int tiles = ((a.DW + 31) / 32) * ((a.DH + Cfg::TH - 1) / Cfg::TH) * a.B * ((a.Ntot + BN - 1) / BN);
    if (tiles <= 0) return PNNP_OK;
    const int wgs = pnnp_persistent_grid(tiles);
    hipLaunchKernelGGL(kern, dim3(wgs), dim3(NTHR), Cfg::LDS_BYTES, s, ha);
    return pnnp_launch_status();
}

// the epilogue a launch needs
template <class Scheme, int BN, int WN>
int launch_gs_ek(const typename Scheme::Args& ha, hipStream_t s) {
    const IgemmArgs& b = Scheme::g(ha);
    const bool two = b.dst[1] != nullptr;
    const bool plain = !b.addsrc && !b.accum[0] && !(two && b.accum[1]);
    const bool any_mask = b.mask_mode[0] || (two && b.mask_mode[1]);
    if (plain && !any_mask) return launch_gs<Scheme, BN, WN, EK_FWD>(ha, s);
    if constexpr (Scheme::BITS) {
        if (ha.bits_in[0]) {
            // sign-bit masks: one plain destination in the tile domain's own geometry (ConvTranspose2d backward-data), the bit image must fit a buffer resource
            if (!plain || two || b.act || b.bias || !b.mask_mode[0] || b.n_sub || b.out_mul != 1 || b.out_yoff || b.out_xoff || b.OH != b.DH || b.OW != b.DW ||
                ha.bits_nblk[0] * 32 != b.dst_cs[0] || (int64_t)b.B * ((b.OH + 15) / 16) * ((b.OW + 31) / 32) * ha.bits_nblk[0] * 2048 >= (1ll << 31)) return PNNP_E_UNSUPPORTED;
            return launch_gs<Scheme, BN, WN, EK_BWDB>(ha, s);
        }
    }
    if (plain && !b.act && !b.bias) return launch_gs<Scheme, BN, WN, EK_BWD>(ha, s);
    return launch_gs<Scheme, BN, WN, EK_GEN>(ha, s);
}

}  // namespace

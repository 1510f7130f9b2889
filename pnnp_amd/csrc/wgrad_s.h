// Weight gradient of a 3x3 / stride 1 / pad 1 convolution on the low-precision matrix cores with SPECIALISED waves, float32 operands split into pieces on
// the fly.  ONE kernel for both split schemes; what a scheme is -- its pieces, its MFMA and product list, its scales, its tile heights -- comes from the
// `Scheme` of csrc/wgrad_x3s.hip (bf16x3: exact three-way split, six products) or csrc/wgrad_h2s.hip (fp16x2: two scaled pieces, three products; the
// default).  The host side (shape rules, pixel splits, workspace, the slab reduce) is csrc/wgrad_x3.hip.
//
// Round 2-3's kernel had eight waves that each carried a 32 x 32 x 9-tap accumulator block (144 registers) and split their share of the next pixel tile
// between their own MFMAs; a wave's own vector instructions are ADDED to its MFMA time (tools/ubench/mfma_valu_coissue.hip), and 144 + operands leave no
// room for a third wave per SIMD.  Here a workgroup is
//   12 CONSUMER waves (three per SIMD): wave (mo, no, tr, wk) owns the 32 x 32 block (mo, no) of a (32 MO) x (32 NO) output tile for the three taps of
//     filter ROW tr -- 48 accumulator registers -- and 1 / WK of a pixel tile's k-steps (64 x 64 tiles have one consumer per (block, row), 32 x 32 tiles
//     four that are summed through LDS at the end; MW = 2: one consumer owns both blocks of a 64-row tile, see WsCfg); transposed LDS reads + MFMAs only;
//   4 PRODUCER waves (one per SIMD): the next pixel tile (G: TH rows x 32 px, X: its (TH + 2) x 34 halo) fp32 global -> registers (one tile ahead) ->
//     split -> the other LDS image [32-channel block][piece][pixel][32 ch]; the bias gradient (column sums of G) on the way.
// 1024 threads, <= 128 registers each, one barrier per pixel tile.  Partial sums go to per-workgroup slabs with alternating signs and one deterministic
// reduce (csrc/wgrad_x3.hip).  (The 16 x 16 x 32 MFMA shape was tried in this kernel too -- commit 936596b, WXS_M16: parity-green, 44 transposed reads per
// k-step instead of 24, 4-5 % slower; profiles/r4/ab_wgrad_specialised.txt.)
//
// A Scheme provides: PIECES per operand; MFMAS products per (16-pixel k-step, tap) with the piece pair pa(G), pb(G) of product G, smallest terms first,
// and the instruction mfma(); split() of a float4 into its pieces; SCALED / scale_exps() / unscale(): power-of-two operand scales from the tensors' amax
// slots, undone where the values leave the accumulators (and with them where an odd pixel split's minus sign goes: see sgs); ROLL: the producers' rolling
// refill (see roll_tile); G_AUX: cache-policy bits of the G loads; MW2: whether 64 x 64 tiles run with MW = 2; TH22 / TH21 / TH12 / TH11: pixel-tile
// heights of the 64 x 64 / 64 x 32 / 32 x 64 / 32 x 32 output tiles.
#pragma once
#include "common.h"

struct WsArgs {
    const float* G; int Gcs;            // [B][H][W][Gcs], channels [0, M) used
    const float* X[2]; int Xcs[2];      // n < n_split -> X[0][n], else X[1][n - n_split]
    int n_split;
    int B, H, W, M, N;
    float* slab;                        // [Z][9][M][N]
    float* bias_slab;                   // [Z][M] or null
    int Z;
    const unsigned* amax_g; const unsigned* amax_x[2];      // (scaled schemes; null otherwise) amax slots of G and of the X tensor(s) (csrc/h2.h); amax_x[1] null without a second one
};
int pnnp_wx3s_launch(const WsArgs& a, hipStream_t s);             // csrc/wgrad_x3s.hip (bf16x3)
int pnnp_wx3s_th(int M, int N);                                     // its pixel-tile height for (M, N)
int pnnp_wh2s_launch(const WsArgs& a, hipStream_t s);             // csrc/wgrad_h2s.hip (fp16x2: same output tiles, same slabs, same reduce)
int pnnp_wh2s_th(int M, int N);

#ifndef WX3_ALT_SIGN
#define WX3_ALT_SIGN 1                 // odd pixel splits accumulate -G * X (csrc/wgrad_x3.hip: the matrix core's accumulation rounds toward minus infinity)
#endif

namespace {

constexpr int NCW = 12, NPW = 4, NTHR = 64 * (NCW + NPW);
constexpr int XC = 34;
constexpr unsigned OOB = 0x80000000u;
#define WS_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")
#ifdef WHS_STAMPS                     // debug build of either scheme's file: cycle sums per wave, dumped into the slab (tools/whs_stamps.py; the results are then garbage)
#define WS_T(v) { const long long now_ = clock64(); v += now_ - tlast_; tlast_ = now_; }
#else
#define WS_T(v)
#endif

template <class Scheme, int MO, int NO, int TH, int MW = 1> struct WsCfg {
    // MW: 32 x 32 blocks along M that ONE consumer owns (1, or 2 = both of a 64-row tile: the X words of a tap then feed two blocks, 20 transposed
    // reads per 18 MFMAs instead of 16 per 9 -- the fp16x2 kernel is LDS-bandwidth-bound with one block per wave: 12 waves x 16 reads x 512 B per k-step
    // are 89 % of the LDS's 128 B / clk at full matrix rate)
    static constexpr int P = Scheme::PIECES;
    static constexpr int WK = 4 * MW / (MO * NO);                  // consumers that share a (block, filter row): pixel split inside the workgroup
    static constexpr int KS = TH * 2, KSW = KS / WK;               // 16-pixel k-steps per pixel tile; per consumer
    static constexpr int GPIX = TH * 32, XPIX = (TH + 2) * XC;
    static constexpr int G_BYTES = MO * P * GPIX * 64, X_BYTES = NO * P * XPIX * 64, IMG_BYTES = G_BYTES + X_BYTES, LDS_BYTES = 2 * IMG_BYTES;
    static constexpr int GT = 256 / MO, XT = 256 / NO;             // producer threads per 32-channel block of G / X
    static constexpr int NG = GPIX * 8 / GT, NX = (XPIX * 8 + XT - 1) / XT;      // float4 staging slots per producer thread
    static_assert(MO * NO * WK == 4 * MW && KSW * WK == KS && (MW == 1 || MW == MO), "wave layout");
    static_assert((GPIX * 8) % GT == 0, "G slots divide evenly (the bias sums count every pixel once)");
    static_assert(LDS_BYTES <= 160 * 1024 && LDS_BYTES >= NCW * 16 * 64 * 4, "LDS budget (images; the final reduction aliases them, one accumulator block at a time)");
};

template <class Scheme, int MO, int NO, int TH, int MW>
__global__ void __launch_bounds__(NTHR, 1)
wgrad_s_kernel(const WsArgs a) {
    using Cfg = WsCfg<Scheme, MO, NO, TH, MW>;
    constexpr int P = Cfg::P, WK = Cfg::WK, KSW = Cfg::KSW, GPIX = Cfg::GPIX, XPIX = Cfg::XPIX, G_BYTES = Cfg::G_BYTES, IMG_BYTES = Cfg::IMG_BYTES, NG = Cfg::NG, NX = Cfg::NX;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);       // 0 .. 11 consumers, 12 .. 15 producers

    int se_g = 0, se_x = 0;                                          // scale exponents of G / X (scaled schemes)
    if constexpr (Scheme::SCALED) Scheme::scale_exps(a, se_g, se_x);
    const int n_tiles = a.N / (32 * NO);
    int id = blockIdx.x;
    const int z = id % a.Z; id /= a.Z;
    const int ni = id % n_tiles, mi = id / n_tiles;
    const int m0 = mi * 32 * MO, n0 = ni * 32 * NO;
    const int tiles_x = (a.W + 31) >> 5, tiles_y = (a.H + TH - 1) / TH;
    const int ntile = tiles_x * tiles_y * a.B;
    if (z >= ntile) return;                                          // (Z <= ntile: never)

    if (wave >= NCW) {
        // =============================================== PRODUCER ===============================================
        const int pw = wave - NCW;
        const int q8 = lane & 7;                                     // channel quad of the block (8 lanes read a pixel's 128 contiguous bytes)
        // the waves that stage 32-channel block gblk of G (GT threads) / xblk of X (XT threads): wave-uniform, like the tensors behind them
        const int gblk = MO == 2 ? pw >> 1 : 0, lg = MO == 2 ? (pw & 1) * 64 + lane : pw * 64 + lane;
        const int xblk = NO == 2 ? pw >> 1 : 0, lx = NO == 2 ? (pw & 1) * 64 + lane : pw * 64 + lane;
        // Staging slots WITHOUT per-slot address registers (with them -- 4 per slot -- the taller pixel tiles that two planes per operand leave room
        // for did not fit 128 registers).  G: slot k of a thread is pixel gp0 + GSTEP k of the 32-wide tile, i.e. row (GSTEP k) >> 5 (a compile-time
        // number) and column gp0 + (GSTEP k & 31): one base offset, the rest is a scalar.  X: the (TH + 2) x 34 halo does not divide that way: one
        // packed (row << 8 | column) per slot, everything else derived per tile.
        constexpr int GSTEP = Cfg::GT / 8;
        const int gp0 = lg >> 3;                                     // < GSTEP <= 32
        const unsigned g_base = (unsigned)(gp0 * a.Gcs + q8 * 4) * 4u;
        const int g_dst0 = (gblk * P * GPIX + gp0) * 64 + q8 * 8;   // byte offset in an image; + GSTEP k * 64; + piece * GPIX * 64
        const int xd = (n0 + 32 * xblk >= a.n_split) ? 1 : 0;        // wave-uniform source of this wave's X block
        const int xch0 = n0 + 32 * xblk - (xd ? a.n_split : 0);
        const int xcs = a.Xcs[xd];
        int x_rc[NX];
#pragma unroll
        for (int k = 0; k < NX; ++k) {
            int j = lx + Cfg::XT * k;
            if (j >= XPIX * 8) j -= Cfg::XT;                         // a slot past the end repeats the thread's previous one
            const int pix = j >> 3;
            const int r = pix / XC;
            x_rc[k] = (r << 8) | (pix - r * XC);                     // halo coordinates: image pixel (y0 - 1 + r, x0 - 1 + c)
        }
        const __amdgpu_buffer_rsrc_t rsg = __builtin_amdgcn_make_buffer_rsrc((void*)(a.G + m0 + 32 * gblk), 0, 0x7fffffff, 0x00020000);
        const int xshift = (a.W + 1) * xcs;                          // the X resource starts one row + one pixel BEFORE the tensor
        const __amdgpu_buffer_rsrc_t rsx = __builtin_amdgcn_make_buffer_rsrc((void*)(a.X[xd] + xch0 - xshift), 0, 0x7fffffff, 0x00020000);
        f32x4 rg[NG], rx[NX];
        float bsum[4] = {0.f, 0.f, 0.f, 0.f};
        // The scales as floats.  Odd pixel splits stage -G (the matrix core's accumulation rounds toward minus infinity: csrc/wgrad_x3.hip): a scaled scheme
        // carries the sign on G's scale, where it costs nothing; an unscaled one flips G's sign bit behind the bias sums -- the same values either way.
        // (Written out here, not behind scheme functions: with the sign computed ahead of the expression or inside a function the fp16x2 kernels came out with the
        // same registers but a few scalar instructions in another order, <2,1,3,1> with other staging registers too; this form compiles to round 6's stream.)
        const float sgs = __uint_as_float(((unsigned)(se_g + 127) << 23) | ((Scheme::SCALED && WX3_ALT_SIGN && (z & 1)) ? 0x80000000u : 0u));
        const float sxs = __uint_as_float((unsigned)(se_x + 127) << 23);
        const unsigned sflip = (!Scheme::SCALED && WX3_ALT_SIGN && (z & 1)) ? 0x80000000u : 0u;
        // one tile's scalars, then per staging slot: request (global -> registers) and stage (registers -> every plane of an image)
        struct TileSc { int gso, xso, rlim, clim, y0, x0; };
        auto tile_sc = [&](int tile) {
            int q = tile;
            const int tx = q % tiles_x; q /= tiles_x;
            const int ty = q % tiles_y;
            const int b = q / tiles_y;
            TileSc t;
            t.x0 = tx * 32; t.y0 = ty * TH;
            t.gso = (((b * a.H + t.y0) * a.W) + t.x0) * a.Gcs * 4;
            t.xso = ((((b * a.H + t.y0 - 1) * a.W) + t.x0 - 1) * xcs + xshift) * 4;
            t.rlim = a.H - t.y0; t.clim = a.W - t.x0;
            return t;
        };
        auto load_g = [&](auto ktag, const TileSc& t) {
            constexpr int k = decltype(ktag)::value;
            const int gr = (GSTEP * k) >> 5, gc = gp0 + ((GSTEP * k) & 31);
            const int bad = (t.rlim - 1 - gr) | (t.clim - 1 - gc);                             // sign bit set <=> pixel outside the image
            rg[k] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsg, bad < 0 ? OOB : g_base, t.gso + (gr * a.W + ((GSTEP * k) & 31)) * a.Gcs * 4, Scheme::G_AUX));
        };
        auto load_x = [&](auto ktag, const TileSc& t) {
            constexpr int k = decltype(ktag)::value;
            const int xr = x_rc[k] >> 8, xc = x_rc[k] & 255;
            const int yy = t.y0 - 1 + xr, xx = t.x0 - 1 + xc;
            const int bad = yy | (a.H - 1 - yy) | xx | (a.W - 1 - xx);
            rx[k] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsx, bad < 0 ? OOB : (unsigned)((xr * a.W + xc) * xcs + q8 * 4) * 4u, t.xso, 0));
        };
        auto load_tile = [&](int tile) {
            const TileSc t = tile_sc(tile);
            static_for<0, NG>([&](auto kt) { load_g(kt, t); });
            static_for<0, NX>([&](auto kt) { load_x(kt, t); });
        };
        auto stage = [&](f32x4 v, float sc, char* ib, int dst, int pstride) {
            unsigned pc[P][2];
            Scheme::split(v, sc, pc);
#pragma unroll
            for (int p = 0; p < P; ++p) *reinterpret_cast<u32x2*>(ib + dst + p * pstride) = u32x2{pc[p][0], pc[p][1]};
        };
        auto stage_g = [&](auto ktag, char* ib) {
            constexpr int k = decltype(ktag)::value;
            f32x4 v = rg[k];
            bsum[0] += v.x; bsum[1] += v.y; bsum[2] += v.z; bsum[3] += v.w;         // bias gradient: column sums of G (unscaled, unsigned)
            if constexpr (!Scheme::SCALED)
                v = f32x4{__uint_as_float(__float_as_uint(v.x) ^ sflip), __uint_as_float(__float_as_uint(v.y) ^ sflip),
                          __uint_as_float(__float_as_uint(v.z) ^ sflip), __uint_as_float(__float_as_uint(v.w) ^ sflip)};
            stage(v, sgs, ib, g_dst0 + GSTEP * k * 64, GPIX * 64);
        };
        auto stage_x = [&](auto ktag, char* ib) {
            constexpr int k = decltype(ktag)::value;
            stage(rx[k], sxs, ib, G_BYTES + (xblk * P * XPIX + (x_rc[k] >> 8) * XC + (x_rc[k] & 255)) * 64 + q8 * 8, XPIX * 64);
        };
        auto stage_tile = [&](int img) {
            char* ib = smem + img * IMG_BYTES;
            static_for<0, NG>([&](auto kt) { stage_g(kt, ib); });
            static_for<0, NX>([&](auto kt) { stage_x(kt, ib); });
        };
        // ROLLING refill (Scheme::ROLL, round 6): slot k of the next tile is staged and the SAME registers immediately re-requested for the tile after it, slot by
        // slot -- every load is then in flight for a whole period (stage-everything-then-request-everything left them the barrier wait only: the
        // producers' period was load latency + staging + issue, 4 100 cycles where the consumers need 1 800-2 900: profiles/r6/wgrad_stamps.txt).
        // Buffer loads return in order, so slot k has landed when at most NG + NX - 1 later requests are outstanding (the compiler counts them:
        // s_waitcnt vmcnt(NG + NX - 1) in front of every slot; the scheduling barriers keep it from regrouping the requests).
        auto roll_tile = [&](int img, int tile_after) {
            char* ib = smem + img * IMG_BYTES;
            const TileSc t = tile_sc(tile_after);
            static_for<0, NG>([&](auto kt) { stage_g(kt, ib); load_g(kt, t); __builtin_amdgcn_sched_barrier(0); });
            static_for<0, NX>([&](auto kt) { stage_x(kt, ib); load_x(kt, t); __builtin_amdgcn_sched_barrier(0); });
        };
        // the first tile straight into image 0, the second into the registers
        load_tile(z);
        stage_tile(0);
        if (z + a.Z < ntile) load_tile(z + a.Z);
        int img = 0;
#ifdef WHS_STAMPS
        long long t_stage = 0, t_issue = 0, t_bar = 0, tlast_ = clock64(), tall = tlast_; int ntl = 0;
#endif
        for (int tile = z; tile < ntile; tile += a.Z) {
            WS_BARRIER();                                           // image img is complete; every consumer is done with the other one
            WS_T(t_bar)
#ifdef WHS_STAMPS
            ++ntl;
#endif
            if (Scheme::ROLL && tile + 2 * a.Z < ntile) {
                roll_tile(img ^ 1, tile + 2 * a.Z);
                WS_T(t_stage)
            } else if (tile + a.Z < ntile) {
                stage_tile(img ^ 1);                                // the next tile (requested a whole tile ago)
                WS_T(t_stage)
                if (tile + 2 * a.Z < ntile) load_tile(tile + 2 * a.Z);
                WS_T(t_issue)
            }
            img ^= 1;
        }
#ifdef WHS_STAMPS
        if (lane == 0) {
            float* d = a.slab + ((int64_t)blockIdx.x * (NCW + NPW) + wave) * 8;
            d[0] = (float)t_stage; d[1] = (float)t_issue; d[2] = (float)t_bar; d[4] = (float)(clock64() - tall); d[5] = (float)ntl;
        }
#endif
        // ---- (the consumers' pixel-split reduction: 2 barriers per tap of a row when WK > 1) then the bias gradient of this pixel split: add up
        // the threads that share (block, q8) through LDS (the images are dead)
        if (WK > 1) {
#pragma unroll
            for (int i = 0; i < 6 * MW; ++i) WS_BARRIER();
        }
        WS_BARRIER();
        constexpr int NSLOTS = Cfg::GT / 8;                           // threads per (block, quad)
        if (a.bias_slab && ni == 0) {                               // block-uniform
            float* bs = reinterpret_cast<float*>(smem);             // [MO blocks][8 quads][4][NSLOTS]
            const int slot = lg >> 3;
#pragma unroll
            for (int c = 0; c < 4; ++c) bs[((gblk * 8 + q8) * 4 + c) * NSLOTS + slot] = bsum[c];
        }
        WS_BARRIER();
        if (a.bias_slab && ni == 0 && pw < 1 && lane < 32 * MO) {    // one producer wave: 32 MO channels
            float* bs = reinterpret_cast<float*>(smem);
            const int b2 = lane >> 5, ch = lane & 31;
            float s = 0.f;
            for (int k = 0; k < NSLOTS; ++k) s += bs[((b2 * 8 + (ch >> 2)) * 4 + (ch & 3)) * NSLOTS + k];
            a.bias_slab[(int64_t)z * a.M + m0 + b2 * 32 + ch] = (WX3_ALT_SIGN && (z & 1)) ? -s : s;      // (the reduce kernel adds odd splits with a minus sign)
        }
        return;
    }

    // =============================================== CONSUMER ===============================================
    const int tr = wave % 3, rest = wave / 3;                        // filter row; (block, pixel split)
    const int wk = rest % WK, no = (rest / WK) % NO, mo = MW == 1 ? rest / (WK * NO) : 0;      // (MW = 2: the wave owns blocks mo = 0 and 1)
    const int l31 = lane & 31, half = lane >> 5;
    f32x16 acc[MW][3];
#pragma unroll
    for (int mb = 0; mb < MW; ++mb)
#pragma unroll
        for (int t = 0; t < 3; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mb][t][r] = 0.f;
    // transposed-read lane geometry: 16-lane group g reads channels 16 (g & 1) .., pixels 8 (g >> 1) ..; inside a group lane 4 q + p supplies the
    // address of pixel row q, channel chunk 4 p
    const int tr_lane = ((8 * (lane >> 5) + ((lane & 15) >> 2)) * 64) + (16 * ((lane >> 4) & 1) + 4 * (lane & 3)) * 2;
    auto tr_read = [&](const char* base) {                           // 8 pixels x 1 channel per lane: two transposed reads
        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(base));
        const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(base + 4 * 64));
        const u32x2 a0 = __builtin_bit_cast(u32x2, lo), a1 = __builtin_bit_cast(u32x2, hi);
        return u32x4{a0.x, a0.y, a1.x, a1.y};
    };
    int img = 0;
#ifdef WHS_STAMPS
    long long t_mfma = 0, t_bar = 0, tlast_ = clock64(), tall = tlast_; int ntl = 0;
    const long long t_entry = tlast_;
    long long t_first = 0;
#endif
    for (int tile = z; tile < ntile; tile += a.Z) {
        WS_BARRIER();
        WS_T(t_bar)
#ifdef WHS_STAMPS
        if (!ntl) t_first = tlast_ - t_entry;                       // kernel entry -> the first tile is staged
        ++ntl;
#endif
        const char* gimg = smem + img * IMG_BYTES;
        const char* ximg = gimg + G_BYTES;
        // MW = 1: operand words double-buffered (the next step's are read while this step's MFMAs issue).  MW = 2: 96 accumulator registers
        // leave room for ONE set (128 registers per wave at 16 waves): the next step's words are requested right BEHIND this step's MFMAs --
        // the matrix core has captured its operands by then -- and the LDS latency is covered by the SIMD's other two consumer waves.
        constexpr int NBUF = MW == 1 ? 2 : 1;
        u32x4 av[NBUF][MW][P], bv[NBUF][P];
        auto gload = [&](int kl, u32x4 (&ax)[MW][P]) {               // kl: this consumer's kl-th k-step of the tile
            const int ks = wk * KSW + kl;
#pragma unroll
            for (int mb = 0; mb < MW; ++mb) {
                const char* gbase = gimg + (((mo + mb) * P) * GPIX + (ks >> 1) * 32 + (ks & 1) * 16) * 64 + tr_lane;
#pragma unroll
                for (int p = 0; p < P; ++p) ax[mb][p] = tr_read(gbase + p * GPIX * 64);
            }
        };
        auto xload = [&](int kl, int dx, u32x4 (&bx)[P]) {
            const int ks = wk * KSW + kl;
            const char* xbase = ximg + ((no * P) * XPIX + ((ks >> 1) + tr) * XC + (ks & 1) * 16 + dx) * 64 + tr_lane;
#pragma unroll
            for (int p = 0; p < P; ++p) bx[p] = tr_read(xbase + p * XPIX * 64);
        };
        gload(0, av[0]);
        xload(0, 0, bv[0]);
#pragma unroll
        for (int kl = 0; kl < KSW; ++kl) {
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const int s = kl * 3 + dx;
                if constexpr (NBUF == 2) {
                    // the next step's X words (and, at a k-step's last tap, the next k-step's G words) one step ahead
                    if (s + 1 < KSW * 3) xload((s + 1) / 3, (s + 1) % 3, bv[(s + 1) & 1]);
                    if (dx == 2 && kl + 1 < KSW) gload(kl + 1, av[(kl + 1) & 1]);
                    __builtin_amdgcn_sched_barrier(0);
                }
                const u32x4 (&ax)[MW][P] = av[NBUF == 2 ? (kl & 1) : 0];
                const u32x4 (&bx)[P] = bv[NBUF == 2 ? (s & 1) : 0];
#pragma unroll
                for (int mb = 0; mb < MW; ++mb)
#pragma unroll
                    for (int G = 0; G < Scheme::MFMAS; ++G) acc[mb][dx] = Scheme::mfma(ax[mb][Scheme::pa(G)], bx[Scheme::pb(G)], acc[mb][dx]);
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (NBUF == 1) {
                    if (s + 1 < KSW * 3) xload((s + 1) / 3, (s + 1) % 3, bv[0]);
                    if (dx == 2 && kl + 1 < KSW) gload(kl + 1, av[0]);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        img ^= 1;
#ifdef WHS_STAMPS
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_nop 0" ::: "memory");
#endif
        WS_T(t_mfma)
    }
#ifdef WHS_STAMPS
    const long long t_loop_end = clock64();
#endif
    // ---- the pixel splits of a (block, row) are added up through LDS (the images are dead; one accumulator block at a time), then the slab
    // [z][tap][m][n]: 32 x 32 x 16 accumulator layout: column l31, row (r & 3) + 8 (r >> 2) + 4 half
    float* red = reinterpret_cast<float*>(smem);
    const int dexp = -(se_g + se_x);                                 // undo the operand scales (exact: a power of two)
    float* const slab_z = a.slab + (int64_t)z * a.M * a.N * 9;      // this split's slab: 9 M N < 2^31 floats (the launcher checks), so the index inside it is 32-bit
#pragma unroll
    for (int mb = 0; mb < MW; ++mb)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
        f32x16 v = acc[mb][dx];
        const int t = tr * 3 + dx;
        if constexpr (WK > 1) {
            // Through LDS in the accumulator layout, back out ROW-major: a lane of the storing wave takes 4 consecutive columns of rows (lane >> 3) + 8 i, adds the WK
            // partial sums in the order k = 0, 1, ... and stores 16 bytes -- 4 store instructions of 8 rows x 128 bytes per (block, tap) where the
            // accumulator layout needed 16 of 2 x 128 bytes (the epilogue was ~13 000 cycles per workgroup, most of it these stores: profiles/r6/wgrad_stamps.txt)
            WS_BARRIER();
#pragma unroll
            for (int r = 0; r < 16; ++r) red[(wave * 16 + r) * 64 + lane] = v[r];
            WS_BARRIER();
            if (wk == 0) {
                const int c4 = (lane & 7) * 4;
                const unsigned n_u = (unsigned)a.N;
                const unsigned base = (unsigned)((t * a.M + m0 + (mo + mb) * 32) * a.N + n0 + no * 32 + c4);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int row = (lane >> 3) + 8 * i;             // row (r & 3) + 8 (r >> 2) + 4 half of the 32 x 32 block
                    const int r = ((row >> 3) << 2) | (row & 3), hf = (row >> 2) & 1;
                    f32x4 sum = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int k = 0; k < WK; ++k) sum += *reinterpret_cast<const f32x4*>(red + ((wave + 3 * k) * 16 + r) * 64 + hf * 32 + c4);      // (the split index steps the wave number by 3)
#pragma unroll
                    for (int c = 0; c < 4; ++c) sum[c] = Scheme::unscale(sum[c], dexp);
                    *reinterpret_cast<f32x4*>(slab_z + base + (unsigned)row * n_u) = sum;
                }
            }
        } else if (wk == 0) {
            // one base index per (block, tap); the 16 rows of the accumulator layout are compile-time multiples of N behind it (with a 64-bit index per
            // element the compiler hoisted 16 address pairs and spilled: 12 bytes of scratch in the fp16x2 64 x 64 kernel)
            const unsigned base = (unsigned)((t * a.M + m0 + (mo + mb) * 32 + 4 * half) * a.N + n0 + no * 32 + l31);
            const unsigned n_u = (unsigned)a.N;
#pragma unroll
            for (int r = 0; r < 16; ++r) slab_z[base + (unsigned)((r & 3) + 8 * (r >> 2)) * n_u] = Scheme::unscale(v[r], dexp);
        }
    }
    WS_BARRIER();                                                   // (the producers' bias reduction: two more barriers for every wave)
    WS_BARRIER();
#ifdef WHS_STAMPS
    __builtin_amdgcn_s_waitcnt(0x0f70);                             // (the slab stores have left: what follows overwrites a corner of the slab)
    if (lane == 0) {
        float* d = a.slab + ((int64_t)blockIdx.x * (NCW + NPW) + wave) * 8;
        d[0] = (float)t_mfma; d[1] = (float)t_first; d[2] = (float)t_bar; d[3] = (float)(clock64() - t_loop_end); d[4] = (float)(t_loop_end - tall); d[5] = (float)ntl;
    }
#endif
}

template <class Scheme, int MO, int NO, int TH, int MW = 1>
int ws_launch_tile(const WsArgs& a, hipStream_t s) {
    using Cfg = WsCfg<Scheme, MO, NO, TH, MW>;
    auto kern = wgrad_s_kernel<Scheme, MO, NO, TH, MW>;
    static PnnpPerDevice lds_once;
    if (pnnp_allow_lds(lds_once, kern, Cfg::LDS_BYTES) != PNNP_OK) return PNNP_E_LAUNCH;
    const int blocks = (a.M / (32 * MO)) * (a.N / (32 * NO)) * a.Z;
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(NTHR), Cfg::LDS_BYTES, s, a);
    return pnnp_launch_status();
}

// the configuration for (M, N): output tile 64 x 64 / 64 x 32 / 32 x 64 / 32 x 32 (what the channel counts allow) at the scheme's pixel-tile height
template <class Scheme>
int ws_th(int M, int N) { return (M % 64 == 0) ? ((N % 64 == 0) ? Scheme::TH22 : Scheme::TH21) : ((N % 64 == 0) ? Scheme::TH12 : Scheme::TH11); }

template <class Scheme>
int ws_launch(const WsArgs& a, hipStream_t s) {
    if ((int64_t)a.M * a.N * 9 >= (1ll << 31)) return PNNP_E_UNSUPPORTED;      // the kernel indexes one slab with 32 bits
    if (a.M % 64 == 0) return a.N % 64 == 0 ? ws_launch_tile<Scheme, 2, 2, Scheme::TH22, Scheme::MW2 ? 2 : 1>(a, s) : ws_launch_tile<Scheme, 2, 1, Scheme::TH21>(a, s);
    return a.N % 64 == 0 ? ws_launch_tile<Scheme, 1, 2, Scheme::TH12>(a, s) : ws_launch_tile<Scheme, 1, 1, Scheme::TH11>(a, s);
}

}  // namespace

// 3x3 convolution (forward / backward-data) on the low-precision matrix cores, float32 operands split into pieces on the fly: ONE kernel text for both split
// schemes.  What a scheme is comes from the `Scheme` of csrc/conv_x3s.hip (bf16x3, exact three-way split) or csrc/conv_h2s.hip (fp16x2, two scaled pieces);
// those files also hold the thin __global__ wrappers (igemm_x3s_kernel / igemm_h2s_kernel: the names the profiles and tools know) and the dispatch.
//
// This file: constants, SCfg, the launcher and the host validation.  The kernel text itself is csrc/conv_s_body.h, which a wrapper includes as its body after
// `using Scheme = ...` (BN, EK and the argument `ha` are the wrapper's).  It is an included text and not a __device__ __forceinline__ function on purpose: as a
// function the compiler optimises it on its own first -- without the kernel's launch bounds and without knowing that `ha` is the kernel-argument segment -- and
// inlines the result, and all fifteen fp16x2 instruction streams then differ from the kernel they had as one function (the producers' out-of-range selects become
// branches or the reverse, and igemm_h2s_kernel<64, EK_BWDU> spills a register).  Included, they are identical to it, instruction for instruction.
//
// A workgroup has SPECIALISED waves (round 4; why: the header of csrc/conv_x3s.hip), a 16-row x 32-px pixel tile x BN = 32 / 64 channels:
//   8 CONSUMER waves (two per SIMD, 2 pixel rows x BN channels each): ds_read_b128 + MFMA only inside the K loop (Scheme::mfma_item), and the epilogue
//     straight from the accumulators (weights as the MFMA's first operand: a lane holds 4 consecutive channels of one pixel);
//   4 PRODUCER waves (one per SIMD): the halo tile of a later 16-channel chunk (fp32 NHWC global -> one of NSETS register sets -> Scheme::split -> the
//     other of two LDS images) and the weights of a later work item (LDS-DMA into a ring of NSTAGE stages, AHEAD items ahead).
// A chunk of K is Scheme::ITEMS work items (bf16x3: its three filter rows; fp16x2: the whole chunk), one s_barrier per item, all 12 waves.  A workgroup walks
// tiles t, t + G, ... (persistent grid, XCD-aware order); stores drain while the next tile starts.
//
// A Scheme provides
//   halo image    PIECES per value (image = [piece][k-octet 2][pixel, plane padded to 624] 16-byte words), split() of two values into their pieces, ZERO_PAD:
//                 whether the padding words of the hi planes are zeroed in the prologue;
//   weight pack   WBLK: bytes of one item of one 32-column block, contiguous in the pack (csrc/pack_jobs.hip) and in an LDS stage, fetched as 1 KB pieces;
//   work items    ITEMS per chunk, nstage(BN) / ahead(BN), SLOTS: staging slots (of the 5 per producer thread) split per item, NSETS producer register sets;
//   matrix work   mfma_item<BN>(acc, xs, wsb, wave, lane, item, stage, image): the scheme's own MFMA schedule;
//   SCALED        power-of-two operand scales from the tensors' amax slots (scale_exps()), undone in the epilogue, and max |stored value| into amax slots;
//   BITS          sign bits of the forward output written / read back as the act' mask;
//   has(EK, BN)   the epilogues the scheme's dispatch launches.
#pragma once
#include "h2.h"

namespace {

constexpr int NCW = 8, NPW = 4, NTHR = 64 * (NCW + NPW);           // consumer / producer waves
constexpr int MT = 2, TH = NCW * MT, HR = TH + 2, HC = 34, NPIX = HR * HC;     // 16-row x 32-px tile, 612 halo pixels
constexpr int NPIXP = (NPIX + 15) / 16 * 16;                       // 624: a plane of the halo image, padded to a multiple of 16 words
#define XS_PLANE(piece, oct) (((piece) * 2 + (oct)) * NPIXP)
constexpr int XS_PIECE_STRIDE = 2 * NPIXP;
constexpr int PTHR = 64 * NPW;                                     // producer threads
constexpr int NSLOT = (2 * NPIX + PTHR - 1) / PTHR;                // halo staging slots per producer thread: 1224 (pixel, octet) pairs / 256 -> 5
constexpr unsigned OOB = 0x80000000u;
#define CS_VMCNT(N) (0x0f70 | ((N) & 15) | (((N) >> 4) << 14))     // s_waitcnt vmcnt(N) alone
// The item barrier as assembly (LDS operations of this wave done, then s_barrier; "memory": the compiler moves nothing across it).  Through
// __syncthreads() -- a workgroup fence + barrier -- the compiler waits for EVERY LDS-DMA a wave has in flight (vmcnt(0): it cannot know which
// stage the reads behind the barrier touch), i.e. for the weights requested a moment ago for the item after next.
#define CS_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")
#ifndef CONVS_STORE_AUX
#define CONVS_STORE_AUX 2            // cache-policy bits of the epilogue's full-resolution stores: 2 = nt (non-temporal: +0.3-0.5 % on the step, three
                                   // alternating same-box pairs, profiles/r4/ab_store_policy.txt); 0 = default, 1 = sc0, 3 = sc0 + nt measured too
#endif
#ifdef CONVS_STAMPS               // debug build: cycle sums per wave, dumped into dst[0] (tools/x3s_stamps.py, tools/h2s_stamps.py)
#define CS_T(v) { const long long now_ = clock64(); v += now_ - tlast_; tlast_ = now_; }
#else
#define CS_T(v)
#endif

// the epilogue a kernel carries (one straight-line path each): forward (no mask, no accumulation, no residual; writes sign bits when asked),
// masked backward-data with float32 masks / with bit masks, the general one, forward + MaxPool2d(2)
enum { EK_FWD = 0, EK_BWD = 1, EK_GEN = 2, EK_POOL = 3, EK_BWDB = 4, EK_HEAD = 5, EK_RES = 6, EK_BWDU = 7 };
// EK_BWDU (round 7): EK_BWDB for ONE destination that is the input of a MaxPool2d(2) as well as a skip connection (archs/Unet.py: conv1_2 .. conv4_2) -- the
// bit-masked backward-data value + the un-pooled gradient of the pooled map, which csrc/misc.hip maxpool_bwd_codes_kernel used to add in a pass of its own
// (a read-modify-write of the full-resolution map).  In the order of EK_RES: trade, add, track, store.  After the trade a lane's two stores are 4 consecutive
// channels of one pixel each, so the pooled gradient is one 16-byte word and the codes one dword per store address, shared by the wave's two rows (a wave owns
// rows 2 w, 2 w + 1: one window row).  Same float operations in the same order as the pass (t + ((k == argmax) ? g d : 0), the add ALSO when the term is
// zero); the amax slot sees only what is stored (pixels outside the map are zeroed in front of the trade), as the pass's did: bit-identical, slot included.
// EK_RES (round 6): a plain layer + a residual tensor of the destination's geometry, no activation, no mask (ResUnet: the second convolution of every
// ResidualBlock, forward `conv + bias + shortcut` and backward-data `dgrad + g`, archs/modules.py:176-197) -- the general epilogue took 3.2 x the
// forward epilogue's cycles for them (16-pixel x 64-byte stores, three loads per block: profiles/r6/gen_epilogue_stamps.txt).  Here: the residual
// words are requested up front in the full-line pattern the stores use and added BEHIND the line trade; scale + bias in one fma (bias from LDS).
// ((v 2^dexp + bias) + res in this order, as the general epilogue computes it: bit-identical.)
// EK_HEAD (32-column kernel only): the forward epilogue + the network's 1x1 head (archs/Unet.py:94: conv10_1, 32 -> 4 channels, no activation) computed from
// the activated accumulators -- a lane holds 8 of a pixel's 32 channels, the 4 lanes of a pixel add their partial sums through two butterfly exchanges --
// and written as the NCHW output planes (+ the `res` networks' input residual).  The 32-channel map itself is stored only when the caller asks for it
// (a training forward: backward needs it); an eval forward never writes or re-reads it.

// Element types of the activations (csrc/conv_h1s.hip H1a): a scheme with SRC16 reads its K segments as fp16 NHWC tensors (one 16-byte load per staging slot,
// the word goes into the halo image as loaded: no split, no scale), one with DST16 stores dst[0] and the pooled map as fp16 (one round to nearest even of the
// float32 value the epilogue would store).  A scheme that names neither has float32 on both sides.
template <class S, class = void> struct SElem { static constexpr bool SRC16 = false, DST16 = false; };
template <class S> struct SElem<S, std::void_t<decltype(S::SRC16), decltype(S::DST16)>> { static constexpr bool SRC16 = S::SRC16, DST16 = S::DST16; };

constexpr int HEAD_LDS_FLOATS = 256;                               // (EK_HEAD) [4][32] head weights + [4] biases, padded
template <class Scheme, int BN> struct SCfg {
    static constexpr int NT = BN / 32;
    static constexpr int XS_F4 = Scheme::PIECES * 2 * NPIXP, XS_BYTES = XS_F4 * 16;      // one halo image: 59904 (3 pieces) / 39936 bytes (2)
    static constexpr int WS_STAGE = NT * Scheme::WBLK;             // one item's weights
    static constexpr int NP1 = Scheme::WBLK / 1024;                // 1 KB LDS-DMA pieces per item and 32-column block
    static constexpr int NDMA = WS_STAGE / 1024;                   // ... per stage
    static constexpr int DPW = (NDMA + NPW - 1) / NPW;             // LDS-DMA instructions per producer wave and item
    static constexpr int NSTAGE = Scheme::nstage(BN), AHEAD = Scheme::ahead(BN);
    static constexpr int BIAS_MAX = 1024;                          // the layer's bias vector lives in LDS: at most this many output channels (the launcher checks)
    static constexpr int LDS_BYTES = 2 * XS_BYTES + NSTAGE * WS_STAGE + (BIAS_MAX + 64) * 4 + (Scheme::has(EK_HEAD, BN) ? HEAD_LDS_FLOATS * 4 : 0);
    static_assert(Scheme::WBLK % 1024 == 0 && AHEAD >= 1 && AHEAD < NSTAGE && AHEAD <= Scheme::ITEMS, "the weight ring");
    static_assert(LDS_BYTES <= 160 * 1024, "a workgroup's LDS");
};

__device__ __forceinline__ int xcd_remap(int id, int n) {
    const int q = n >> 3, r = n & 7, x = id & 7, k = id >> 3;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + k;
}

template <class Scheme, int BN, int EK, void (*KERN)(const H2Args)>
int conv_s_launch(const H2Args& a, hipStream_t s) {
    using Cfg = SCfg<Scheme, BN>;
    static PnnpPerDevice lds_once;
    if (pnnp_allow_lds(lds_once, KERN, Cfg::LDS_BYTES) != PNNP_OK) return PNNP_E_LAUNCH;
    const int tiles = ((a.g.DW + 31) / 32) * ((a.g.DH + TH - 1) / TH) * a.g.B * ((a.g.Ntot + BN - 1) / BN) * (EK == EK_GEN && a.ksplit > 1 ? a.ksplit : 1);
    if (tiles <= 0) return PNNP_OK;
    const int wgs = pnnp_persistent_grid(tiles);
    hipLaunchKernelGGL(KERN, dim3(wgs), dim3(NTHR), Cfg::LDS_BYTES, s, a);
    return pnnp_launch_status();
}

// ---- host: what both families' launch entries check before they dispatch.  a.w: the scheme's pack of csrc/pack_jobs.hip (kind 2 / 4), `pack_chunk` bytes per
// 32-column block and 16-channel chunk.  chan_per_seg: channels each K segment contributes (multiple of 8; of 16 when there are several segments).  Only
// what the 3x3 / stride-1 layers need: in_mul = out_mul = 1, no sub-pixel N.  PNNP_OK: `b` is `a` with the chunk counts filled in.
// src_es / dst_es: bytes per element of the K segments / of dst[0] (2: an fp16 map -- 16-byte words are then 8 channels, and the 2 GB limit of one image is
// counted in 2-byte elements)
inline int conv_s_validate(const IgemmArgs& a, int chan_per_seg, int pack_chunk, IgemmArgs& b, int src_es = 4, int dst_es = 4) {
    const int src_q = 16 / src_es - 1, dst_q = 16 / dst_es - 1;      // channel strides in whole 16-byte words
    if (a.nseg < 1 || a.nseg > 2 || chan_per_seg <= 0 || (chan_per_seg & 7) || (a.nseg > 1 && (chan_per_seg & 15)) || a.Ntot <= 0) return PNNP_E_INVALID;
    if (a.Ntot > 1024) return PNNP_E_UNSUPPORTED;                     // (the bias vector lives in LDS: SCfg::BIAS_MAX columns)
    if ((a.Ntot & 31) || a.in_mul != 1 || a.out_mul != 1 || a.n_sub || a.out_yoff || a.out_xoff) return PNNP_E_UNSUPPORTED;
    if (a.dst[1] && (a.n_split & 31)) return PNNP_E_UNSUPPORTED;
    if (a.addsrc && a.accum[0]) return PNNP_E_UNSUPPORTED;
    if ((a.dst_cs[0] & dst_q) || (a.dst[1] && (a.dst_cs[1] & 3))) return PNNP_E_UNSUPPORTED;
    if (dst_es != 4 && a.dst[1]) return PNNP_E_UNSUPPORTED;
    if ((((uintptr_t)a.dst[0]) | ((uintptr_t)a.dst[1]) | ((uintptr_t)a.bias) | ((uintptr_t)a.mask[0]) | ((uintptr_t)a.mask[1]) |
         ((uintptr_t)a.addsrc) | ((uintptr_t)a.w)) & 15) return PNNP_E_INVALID;
    for (int i = 0; i < a.nseg; ++i) {
        if (a.seg[i].yoff || a.seg[i].xoff || (a.seg[i].cstride & src_q) || (src_es != 4 && (a.seg[i].coff & src_q)) || (((uintptr_t)a.seg[i].ptr) & 15)) return PNNP_E_UNSUPPORTED;
        if (((int64_t)a.IH + 4) * a.IW * a.seg[i].cstride * src_es >= (1ll << 31)) return PNNP_E_UNSUPPORTED;     // 32-bit offsets inside one image
    }
    for (int d = 0; d < 2; ++d)
        if (a.dst[d] && (int64_t)a.OH * a.OW * a.dst_cs[d] * (d ? 4 : dst_es) >= (1ll << 31)) return PNNP_E_UNSUPPORTED;
    b = a;
    b.chunks_per_seg = (chan_per_seg + 15) / 16;
    b.seg_channels = chan_per_seg;
    if ((int64_t)((a.Ntot + 31) / 32) * b.nseg * b.chunks_per_seg * pack_chunk >= (1ll << 31)) return PNNP_E_UNSUPPORTED;      // 32-bit offsets inside the pack
    return PNNP_OK;
}
// ... and of a launch with a MaxPool2d(2) in its epilogue, forward (the pooled map and the codes are written) or backward-data (EK_BWDU: the pooled map's
// gradient and the codes are read): one destination, no residual / accumulation, even sizes, the whole map
inline int conv_s_validate_pool(const IgemmArgs& a, const void* map, const void* codes, int es = 4) {
    if (!map || !codes || a.dst[1] || a.accum[0] || a.addsrc || (a.OH & 1) || (a.OW & 1) || a.OH != a.DH || a.OW != a.DW || (a.pool_cs & (16 / es - 1)) ||
        a.pool_cs < a.Ntot || ((uintptr_t)map & 15) || ((uintptr_t)codes & 3))
        return PNNP_E_UNSUPPORTED;
    if ((int64_t)(a.OH / 2) * (a.OW / 2) * a.pool_cs * es >= (1ll << 31)) return PNNP_E_UNSUPPORTED;
    return PNNP_OK;
}

}  // namespace

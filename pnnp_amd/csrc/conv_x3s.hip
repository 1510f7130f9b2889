// 3x3 convolution (forward / backward-data) on the bf16 matrix cores, fp32 operands split into three bf16 pieces -- the scheme, the LDS
// images, the weight pack and the tile of rounds 2-3's kernel (git history: igemm_x3_kernel; DESIGN Appendix A.1) -- with the workgroup's waves SPECIALISED (round 4):
//
//   8 CONSUMER waves (two per SIMD, 2 pixel rows x BN channels each): ds_read_b128 + v_mfma_f32_16x16x32_bf16 only, and the epilogue;
//   4 PRODUCER waves (one per SIMD): everything else -- the halo tile of the next chunk (fp32 NHWC global -> registers -> hi / mid / lo
//     split -> LDS image) and the weights of the next filter rows (LDS-DMA).
//
// Why (tools/ubench/mfma_valu_coissue.hip, profiles/r4/mfma_valu_coissue.txt): VALU instructions of a wave do NOT run under that wave's own
// MFMAs -- a wave that interleaves k vector instructions per MFMA needs (MFMA time + k x 4 cycles) per MFMA, exactly additive, and two
// such waves per SIMD only partly cover for each other (4 staging units per 8 MFMAs: 33 cycles per MFMA and SIMD instead of 13.5) -- but
// VALU instructions of ANOTHER wave of the SIMD do: two MFMA-only waves keep their 13.5 cycles per MFMA whatever a third, VALU-only wave
// does beside them.  That kernel's waves each staged 1/8 of the next halo between their own MFMAs (filter row 2 of every chunk: 146 vector
// instructions per 144 MFMAs, measured 5100 cycles against 2850 for the staging-free rows 0 and 1); moving the staging between the waves of
// a SIMD ("complementary pairing", X3_FILLMODE) changed nothing because every wave still paid for its own share.  Here the consumers never
// issue a vector-ALU or vector-memory instruction inside the K loop.
//
// Synchronisation: one s_barrier per work item (filter row of a 16-channel chunk), all 12 waves.  Between barrier i and i + 1 the consumers
// run item i (halo image c & 1 of chunk c, weight stage i % NSTAGE); the producers request the weights of item i + AHEAD into the stage
// item i - 1 has just left, split a share of chunk c + 1's halo into the other image, and wait (exact vmcnt) for the weights of item i + 1
// before they arrive at barrier i + 1.  Epilogue: straight from the accumulators (weights as the MFMA's first operand: a lane holds 4
// consecutive channels of one pixel), stores drain while the next tile starts -- the consumers have nothing else in flight to wait for.
#include "conv_s.h"
#include "x3.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

int pnnp_igemm_x3_launch(const IgemmArgs& a, int chan_per_seg, hipStream_t s);

namespace {

struct X3s {
    // halo image: 3 pieces x 2 octets x 624 px x 16 B = 58.5 KB; no word outside the 612 pixels is read
    static constexpr int PIECES = 3;
    static constexpr bool ZERO_PAD = false;
    static __device__ __forceinline__ void split(float a0, float a1, float, unsigned (&p)[3]) { split2(a0, a1, p[0], p[1], p[2]); }
    // weights of one filter row of one 32-channel block: [tap 3][octet 2][piece 3][32][16 B] = 9216 bytes (9 pieces); the rows of a chunk follow each other
    static constexpr int WBLK = 3 * 2 * 3 * 32 * 16;
    // Two images and a chunk's 27 KB of weights per 32 columns do not fit twice: the work item is a FILTER ROW of a chunk.  Weight ring: BN = 64 two stages,
    // one item ahead (an item is 72 MFMAs per consumer wave, > 2 us); BN = 32 three stages (filter row r lives in stage r), two items ahead.  The staging
    // slots of the next chunk's halo are dealt over the rows: {0, 1}, {2, 3}, {4}; one register set, requested again behind the last split
    static constexpr int ITEMS = 3, SLOTS = 2;
    static constexpr int nstage(int BN) { return BN == 32 ? 3 : 2; }
    static constexpr int ahead(int BN) { return nstage(BN) - 1; }
    static constexpr int NSETS = 1;
    static constexpr bool SCALED = false, BITS = false;
    static constexpr bool has(int EK, int) { return EK == EK_FWD || EK == EK_BWD || EK == EK_GEN || EK == EK_POOL; }
    // MFMAs of filter row tr (halo image img, weight stage st).  Order per tap: pass j (16 output channels) x pixel block mb x the three
    // products, smallest terms first.  The 8 pixel words of the tap stay in registers for all passes and are refreshed IN PLACE for the next
    // tap during the last pass; the 3 weight words of a pass are read one pass ahead into the other of two register sets.
    template <int BN>
    static __device__ __forceinline__ void mfma_item(f32x4 (&acc)[2 * MT][BN / 16], const u32x4* xs, const char* wsb, int wave, int lane, int tr, int st, int img) {
        constexpr int MB = 2 * MT, NB = BN / 16, WS_STAGE = (BN / 32) * WBLK, XS_F4 = PIECES * 2 * NPIXP;
        // lane bases, from the lane number itself: the compiler computes them once, in front of the K loop.  (From an opaque copy per item, as fp16x2 derives its
        // own per chunk, the consumers run a dozen vector instructions per filter row, which add to their MFMA time: every layer 1.5-2 % slower, forward and
        // backward-data, profiles/r7/ab_conv_one_source.txt part 0.)
        const int r16 = lane & 15, q16 = lane >> 4, oct16 = q16 & 1, ps16 = q16 >> 1;
        // operand forms (two pieces concatenated along K = 32): pixels  0 = [hi | mid], 1 = [hi | lo];  weights 0 = [hi' | hi'], 1 = [mid' | mid'],
        // 2 = [lo' | hi']:  P1 W2 = hi lo' + lo hi',  P0 W1 = hi mid' + mid mid',  P0 W0 = hi hi' + mid hi'  -- the six products of the scheme
        const int aoff0 = XS_PLANE(ps16 ? 1 : 0, oct16) + r16, aoff1 = XS_PLANE(ps16 ? 2 : 0, oct16) + r16;            // 16-byte words
        const int boff0 = ((oct16 * 3 + 0) * 32 + r16) * 16, boff1 = ((oct16 * 3 + 1) * 32 + r16) * 16,
                  boff2 = ((oct16 * 3 + (ps16 ? 0 : 2)) * 32 + r16) * 16;                                            // bytes inside one tap
        constexpr int GT = NB * MB * 3;                             // MFMAs per tap
        const char* wst = wsb + st * WS_STAGE;
        const u32x4* xim = xs + img * XS_F4;
        u32x4 A[MB][2], Bv[2][3];
        auto a_read = [&](int tp, int mb, int f) {
            A[mb][f] = xim[(f ? aoff1 : aoff0) + (wave * MT + (mb >> 1) + tr) * HC + tp + 16 * (mb & 1)];
        };
        auto b_read = [&](int tp, int j, int f, int buf) {
            Bv[buf][f] = *reinterpret_cast<const u32x4*>(wst + (j >> 1) * WBLK + tp * 3072 + (f == 0 ? boff0 : (f == 1 ? boff1 : boff2)) + (j & 1) * 256);
        };
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) { a_read(0, mb, 1); a_read(0, mb, 0); }
#pragma unroll
        for (int f = 0; f < 3; ++f) b_read(0, 0, 2 - f, 0);
        __builtin_amdgcn_sched_barrier(0);
        static_for<0, 3 * GT>([&](auto Gc) {
            constexpr int gi = decltype(Gc)::value;
            constexpr int tp = gi / GT, gt = gi % GT, j = gt / (MB * 3), w = gt % (MB * 3), mb = w / 3, sp = w % 3;
            constexpr int pass = tp * NB + j, buf = pass & 1;
#define X3S_MFMA(FA, FB) acc[mb][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, Bv[buf][FB]), __builtin_bit_cast(bf16x8, A[mb][FA]), \
                                                                         acc[mb][j], 0, 0, 0)
            if constexpr (sp == 0) X3S_MFMA(1, 2);                  // hi lo' + lo hi'
            else if constexpr (sp == 1) X3S_MFMA(0, 1);             // hi mid' + mid mid'
            else X3S_MFMA(0, 0);                                    // hi hi' + mid hi'
#undef X3S_MFMA
            if constexpr (w < 3 && pass + 1 < 3 * NB) b_read((pass + 1) / NB, (pass + 1) % NB, 2 - w, buf ^ 1);
            if constexpr (j == NB - 1 && tp < 2) {
                if constexpr (sp == 0) a_read(tp + 1, mb, 1);
                if constexpr (sp == 2) a_read(tp + 1, mb, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        });
    }
};

template <int BN, int EK>
__global__ void __launch_bounds__(NTHR, 1)
igemm_x3s_kernel(const H2Args ha) {
    using Scheme = std::enable_if_t<BN != 0, X3s>;                       // (a dependent name: the body's `if constexpr (Scheme::...)` then discards)
#include "conv_s_body.h"
}

template <int BN, int EK>
int launch_x3s(const H2Args& a, hipStream_t s) { return conv_s_launch<X3s, BN, EK, igemm_x3s_kernel<BN, EK>>(a, s); }

}  // namespace

// a.w: the x3 pack of csrc/pack_jobs.hip (kind 2); validation shared with pnnp_igemm_h2s_launch (csrc/conv_s.h).  The kernel takes the fp16x2 family's argument
// struct with every field of that family null or zero.
int pnnp_igemm_x3_launch(const IgemmArgs& a, int chan_per_seg, hipStream_t s) {
    H2Args b = {};
    if (const int rc = conv_s_validate(a, chan_per_seg, X3s::ITEMS * X3s::WBLK, b.g); rc != PNNP_OK) return rc;
    b.ksplit = 1;
    // 64-column tiles unless they leave CUs idle: the fp16x2 family's rule (pnnp_conv3_tile_columns, csrc/igemm.h; exported as pnnp_h2_tile_columns)
    if (a.pool_dst || a.pool_codes) {
        // fused MaxPool2d(2): plain forward layers only (one destination, no mask / residual / accumulate), even sizes
        if (conv_s_validate_pool(a, a.pool_dst, a.pool_codes) != PNNP_OK || a.mask_mode[0]) return PNNP_E_UNSUPPORTED;
        return pnnp_conv3_tile_columns(a.B, a.DH, a.DW, a.Ntot, 1) == 64 ? launch_x3s<64, EK_POOL>(b, s) : launch_x3s<32, EK_POOL>(b, s);
    }
    const bool wide = pnnp_conv3_tile_columns(a.B, a.DH, a.DW, a.Ntot, 0) == 64;
    const bool two = a.dst[1] != nullptr;
    const bool plain = !a.addsrc && !a.accum[0] && !(two && a.accum[1]);
    const bool any_mask = a.mask_mode[0] || (two && a.mask_mode[1]);
    if (plain && !any_mask) return wide ? launch_x3s<64, EK_FWD>(b, s) : launch_x3s<32, EK_FWD>(b, s);
    if (plain && !a.act && !a.bias) return wide ? launch_x3s<64, EK_BWD>(b, s) : launch_x3s<32, EK_BWD>(b, s);
    return wide ? launch_x3s<64, EK_GEN>(b, s) : launch_x3s<32, EK_GEN>(b, s);
}

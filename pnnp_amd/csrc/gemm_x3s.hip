// Pointwise convolutions on the bf16 matrix cores with SPECIALISED waves (round 4): the kernel of csrc/gemm_s.h on the exact bf16x3 split of csrc/x3.h --
// what csrc/gemm_x3.hip validates and hands over.
//
// Why specialised waves: without a halo a staged activation feeds only the tile's N columns, so round 3's waves -- each splitting its share of the next
// item between its own MFMAs -- spent more time on the split than on the matrix pipe (cycle stamps: 4300-5400 cycles per item for 3072 MFMA cycles, matrix
// pipe busy 0.2-0.4; profiles/r4/gemm_x3_stamps_before.txt) and then 11-16 thousand cycles per tile in an epilogue that went through an LDS patch.
// An item is 16 channels: hi / mid / lo pieces, SIX piece products as three v_mfma_f32_16x16x32_bf16 (two pieces concatenated along K), weights
// [octet 2][piece 3][32][8] bf16 = 3072 bytes per item and 32-column block.  Why A = 6 on the 256-pixel tiles (3 on the 512-pixel ones, whose register
// sets are twice as large): an item is only 1536 matrix-pipe cycles, and with two items of flight time (first version) the kernel ran at the memory
// latency, not at the matrix pipe (busy 0.43 at K = 512).
// Tiles: 256 px x 128 columns (4 x 2 consumer waves of 64 px x 64), 512 px x 64 (8 x 1), 256 px x 64 (4 x 2 waves of 64 px x 32: small layers), 512 px x 32.
#include "x3.h"
#include "gemm_s.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

int pnnp_gemm_x3s_launch(const IgemmArgs& a, hipStream_t s);

namespace {

struct X3s {
    using Args = IgemmArgs;
    static __host__ __device__ const IgemmArgs& g(const IgemmArgs& a) { return a; }
    static constexpr int CH = 16, PIECES = 3, NAF = 2, NPROD = 3;
    static constexpr bool SCALED = false, BITS = false;
    static constexpr bool gen_lean(int BN, int WN) { return BN == 64 && WN == 32; }      // (csrc/gemm_s.h: slower on the wide tiles, an occupancy step on this one)
    static constexpr int nwm(int BN, int WN) { return NCW / (BN / WN); }      // every consumer wave computes: 512 pixels where a wave takes the tile's whole width
    static constexpr int lookahead(int PT) { return PT == 256 ? 6 : 3; }
    static __device__ __forceinline__ void split(float a0, float a1, float, unsigned (&p)[3]) { split2(a0, a1, p[0], p[1], p[2]); }
    // operand forms as in csrc/conv_x3s.hip (k-group q16 of an instruction = octet q16 & 1 of the form's half q16 >> 1):
    // pixels 0 = [hi | mid], 1 = [hi | lo]; weights 0 = [hi' | hi'], 1 = [mid' | mid'], 2 = [lo' | hi'].  As coefficients (csrc/gemm_s.h): image plane = AH half + AC + octet,
    // weight row = WH half + WC + WO octet
    static constexpr int AH[2] = {2, 4}, AC[2] = {0, 0};            // images [piece 3][octet 2]: (hi, mid) / (hi, lo)
    static constexpr int WH[3] = {0, 0, -2}, WC[3] = {0, 1, 2}, WO = 3;      // weights [octet 2][piece 3]: hi' twice / mid' twice / (lo', hi')
    // hi lo' + lo hi', then hi mid' + mid mid', then hi hi' + mid hi'
    static constexpr int fa(int sp) { return sp == 0 ? 1 : 0; }
    static constexpr int fb(int sp) { return 2 - sp; }
    static __device__ __forceinline__ f32x4 mfma(u32x4 b, u32x4 a, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, b), __builtin_bit_cast(bf16x8, a), c, 0, 0, 0);
    }
};

}  // namespace

// `b`: validated by pnnp_gemm_x3_launch (csrc/gemm_x3.hip), with chunks_per_seg = 16-channel items per K segment.
int pnnp_gemm_x3s_launch(const IgemmArgs& b, hipStream_t s) {
    if (b.amax_out[1]) return PNNP_E_UNSUPPORTED;                   // (amax of the first destination only: what ConvTranspose2d needs)
    int cus = pnnp_device_cus();
    if (cus < 1) cus = 256;
    // the widest tile that still gives 3/4 of the CUs a tile: 256 px x 128, 512 px x 64, 256 px x 64; N = 32 (mod 64): 512 px x 32
    const int64_t rows8 = (int64_t)((b.DW + 31) / 32) * ((b.DH + 7) / 8) * b.B, rows16 = (int64_t)((b.DW + 31) / 32) * ((b.DH + 15) / 16) * b.B;
    if (b.Ntot % 128 == 0 && rows8 * (b.Ntot / 128) * 4 >= (int64_t)cus * 3) return launch_gs_ek<X3s, 128, 64>(b, s);
    if (b.Ntot % 64 == 0) return rows16 * (b.Ntot / 64) * 4 >= (int64_t)cus * 3 ? launch_gs_ek<X3s, 64, 64>(b, s) : launch_gs_ek<X3s, 64, 32>(b, s);
    return launch_gs_ek<X3s, 32, 32>(b, s);
}

// Weight gradient of a 3x3 / stride 1 / pad 1 convolution on the bf16 matrix cores: the kernel of csrc/wgrad_s.h on the bf16x3 scheme of csrc/x3.h (round 4;
// `set_policy(h2=False)`).  Both operands are split exactly into THREE bf16 pieces hi / mid / lo on the way into LDS, unscaled; SIX
// v_mfma_f32_32x32x16_bf16 per (16-pixel k-step, tap).
#include "x3.h"
#include "wgrad_s.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

namespace {

struct Wx3s {
    static constexpr int PIECES = 3, MFMAS = 6;
    // ROLL and the G loads' cache policy stay at round 4's behaviour (stage a whole tile, then request the tile after next; default policy): the fp16x2
    // settings were measured on that scheme only
    static constexpr bool SCALED = false, ROLL = false;
    static constexpr int G_AUX = 0;
    static constexpr bool MW2 = false;                                // 96 accumulator registers + 3-piece operands do not fit 128 registers
    static constexpr int TH22 = 2, TH21 = 3, TH12 = 2, TH11 = 4;      // what the LDS holds twice at three planes per operand
    // smallest terms first: (hi,lo) (lo,hi) (mid,mid) (hi,mid) (mid,hi) (hi,hi)
    static constexpr int pa(int G) { return G == 0 ? 0 : (G == 1 ? 2 : (G == 2 ? 1 : (G == 3 ? 0 : (G == 4 ? 1 : 0)))); }
    static constexpr int pb(int G) { return G == 0 ? 2 : (G == 1 ? 0 : (G == 2 ? 1 : (G == 3 ? 1 : (G == 4 ? 0 : 0)))); }
    static __device__ __forceinline__ f32x16 mfma(u32x4 a, u32x4 b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    }
    static __device__ __forceinline__ float unscale(float v, int) { return v; }
    static __device__ __forceinline__ void split(f32x4 v, float, unsigned (&p)[3][2]) {
        split2(v.x, v.y, p[0][0], p[1][0], p[2][0]);
        split2(v.z, v.w, p[0][1], p[1][1], p[2][1]);
    }
};

}  // namespace

int pnnp_wx3s_th(int M, int N) { return ws_th<Wx3s>(M, N); }
int pnnp_wx3s_launch(const WsArgs& a, hipStream_t s) { return ws_launch<Wx3s>(a, s); }

// sRGB -> packed raw on the device: the reference's Brooks-style unprocessing, data_process/unprocess.py:79-121 and 199-207
// (inverse_smoothstep, gamma_expansion, apply_ccm, safe_invert_gains, the final clamp), and its Bayer gathers mosaic / mosaic_GBRG (:123-167).
//
// One streaming pass: 12 B (float32) or 3 B (uint8) read per pixel, 12 B (the un-mosaicked RGB) and / or 4 B (the packed raw) written; no LDS, no
// atomics.  A lane owns 4 consecutive pixels of one row, the rows of all images are walked by a grid-stride loop over a grid of at most 2048
// workgroups.  With W % 4 == 0 and 16-byte aligned arrays the lane's 48 input bytes are three 16-byte non-temporal loads (HWC) or one per plane
// (CHW), 12 input bytes are three dwords (uint8), the RGB output is three 16-byte stores and the packed output one 8-byte store into each of the
// row's two Bayer planes (a 16-byte packed store would take 8 pixels per lane and double the 12 unrolled copies of the transcendental chain).
// Otherwise (W = 2 mod 4: a 12-byte pixel then leaves row starts 4-byte aligned only) every lane takes the scalar path: same arithmetic, element accesses.
//
// Arithmetic: float32, every operation rounded on its own (this file is built with -ffp-contract=off), in the reference's operand order, except
// the tone curve.  The reference's 0.5 - sin(asin(1 - 2x) / 3) cancels near x = 0 (below x ~ 6e-8 it returns the 1e-8 floor); here the same root
// s of 3 s^2 - 2 s^3 = x is taken without a difference of near-equal terms: with h = asin(sqrt x) / 3,
//     1 - 2x = cos(2 asin sqrt x),   s = sin(pi/6) - sin(pi/6 - 2h) = sin h (sqrt 3 cos h + sin h),
// on the lower half only (x > 0.5 goes through the curve's symmetry s(x) = 1 - s(1 - x), where 1 - x is exact: next to x = 1 asin multiplies the
// half ulp of sqrt x without bound), then polished by one Newton step whose residual 3 s^2 - 2 s^3 - x is formed in float64.  s is then within
// an ulp of the float64 value for every x (0.75 ulp over 2e6 evenly spaced x in a float32 emulation; 5.4 ulp without the step), which is what
// the tests ask (tests/_unprocess_ref.py).
// Every clamp and the maximum are written as comparisons that a NaN fails, so a NaN goes through as torch.clamp / torch.max pass it: one NaN
// channel makes all three channels of its pixel NaN through the matrix.
#include "common.h"

namespace {

constexpr int UNP_THREADS = 256;
constexpr int UNP_MAX_BLOCKS = 2048;
typedef float f32x2 __attribute__((ext_vector_type(2)));

struct UnpArgs {
    const void* in;
    const float* rows;                                           // [B][PNNP_UNP_NPARAM]: rgb2cam[9] row-major, gains[3], 4 unused
    float* out_rgb;                                              // the input's layout, or null
    float* out_packed;                                           // [B][4][H/2][W/2], or null
    int64_t items;                                               // B * H * W4
    int H, W, W4, gbrg, vec;
};

__device__ __forceinline__ float unp_max(float a, float b) { return (a > b || a != a) ? a : b; }   // torch.max: a NaN on either side comes out

// inverse_smoothstep on x in [0,1] (or NaN): the root of 3 s^2 - 2 s^3 = x in [0,1]
__device__ __forceinline__ float unp_inverse_smoothstep(float x) {
    const bool upper = x > 0.5f;                                 // the curve's symmetry: the lower half only (asin is ill-conditioned next to 1)
    const float u = upper ? 1.f - x : x;                         // exact for x in [0.5, 1]
    const float h = asinf(sqrtf(u)) / 3.f;                       // [0, pi/12]
    const float h2 = h * h;
    // Taylor sums, good on [0, pi/6]: the first terms left out are h^11 / 11! (4e-11 of sin h) and h^12 / 12! (1e-12)
    const float p = fmaf(h2, fmaf(h2, fmaf(h2, 2.7557319e-6f, -1.9841270e-4f), 8.3333333e-3f), -1.6666667e-1f);
    const float q = fmaf(h2, fmaf(h2, fmaf(h2, fmaf(h2, -2.7557319e-7f, 2.4801587e-5f), -1.3888889e-3f), 4.1666667e-2f), -0.5f);
    const float sn = fmaf(h * h2, p, h), cs = fmaf(h2, q, 1.f);
    const float s0 = sn * fmaf(1.7320508f, cs, sn);              // [0, 0.5]
    const double sd = (double)s0;
    const float r = (float)(sd * sd * (3.0 - 2.0 * sd) - (double)u);
    const float d = 6.f * s0 * (1.f - s0);                       // the curve's slope: 0 only at s0 = 0, which is exact
    const float s = d > 0.f ? s0 - r / d : s0;
    return upper ? 1.f - s : s;
}

// unprocess.py:79-121 on one pixel: v[3] in -> c[3] after the matrix, and the three safe gains
__device__ __forceinline__ void unp_pixel(const float v[3], const float m[9], const float g[3], float c[3], float safe[3]) {
    float l[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float s = unp_inverse_smoothstep(pnnp_clampf(v[j], 0.f, 1.f));
        l[j] = powf(s < 1e-8f ? 1e-8f : s, 2.2f);                // gamma_expansion
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) c[i] = (l[0] * m[3 * i] + l[1] * m[3 * i + 1]) + l[2] * m[3 * i + 2];
    const float gray = ((c[0] + c[1]) + c[2]) / 3.f;
    float t = gray - 0.9f;
    t = t < 0.f ? 0.f : t;
    t = t / (float)(1.0 - 0.9);
    const float mask = t * t;
#pragma unroll
    for (int i = 0; i < 3; ++i) safe[i] = unp_max(mask + (1.f - mask) * g[i], g[i]);
}

template <int KIND>
__global__ void __launch_bounds__(UNP_THREADS) unprocess_kernel(UnpArgs a) {
    const int64_t plane = (int64_t)a.H * a.W;
    const int h2 = a.H / 2, w2 = a.W / 2;
    for (int64_t item = (int64_t)blockIdx.x * UNP_THREADS + threadIdx.x; item < a.items; item += (int64_t)gridDim.x * UNP_THREADS) {
        const int64_t row = item / a.W4;                         // img * H + y
        const int x0 = (int)(item - row * a.W4) * 4;
        const int64_t img = row / a.H;
        const int y = (int)(row - img * a.H);
        const int n = a.W - x0 < 4 ? a.W - x0 : 4;               // pixels of this lane (< 4 only at the end of a row with W % 4 != 0)
        const int64_t pix = row * a.W + x0;                      // HWC pixel index over the batch
        const int64_t chw = img * 3 * plane + (int64_t)y * a.W + x0;

        float v[4][3];
        if constexpr (KIND == PNNP_UNP_IN_HWC_F32) {
            const float* src = (const float*)a.in + 3 * pix;
            if (a.vec) {
                const f32x4 t0 = __builtin_nontemporal_load((const f32x4*)src), t1 = __builtin_nontemporal_load((const f32x4*)src + 1);
                const f32x4 t2 = __builtin_nontemporal_load((const f32x4*)src + 2);
                v[0][0] = t0.x; v[0][1] = t0.y; v[0][2] = t0.z; v[1][0] = t0.w; v[1][1] = t1.x; v[1][2] = t1.y;
                v[2][0] = t1.z; v[2][1] = t1.w; v[2][2] = t2.x; v[3][0] = t2.y; v[3][1] = t2.z; v[3][2] = t2.w;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int c = 0; c < 3; ++c) v[i][c] = i < n ? src[3 * i + c] : 0.f;
            }
        } else if constexpr (KIND == PNNP_UNP_IN_CHW_F32) {
            const float* src = (const float*)a.in + chw;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (a.vec) {
                    const f32x4 t = __builtin_nontemporal_load((const f32x4*)(src + c * plane));
                    v[0][c] = t.x; v[1][c] = t.y; v[2][c] = t.z; v[3][c] = t.w;
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[i][c] = i < n ? src[c * plane + i] : 0.f;
                }
            }
        } else {
            const unsigned char* src = (const unsigned char*)a.in + 3 * pix;
            unsigned by[12];
            if (a.vec) {
                const unsigned* s4 = (const unsigned*)src;       // 3 * pix bytes with pix % 4 == 0: dword aligned
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    const unsigned t = __builtin_nontemporal_load(s4 + d);
                    by[4 * d] = t & 255u; by[4 * d + 1] = (t >> 8) & 255u; by[4 * d + 2] = (t >> 16) & 255u; by[4 * d + 3] = t >> 24;
                }
            } else {
#pragma unroll
                for (int k = 0; k < 12; ++k) by[k] = k < 3 * n ? src[k] : 0u;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int c = 0; c < 3; ++c) v[i][c] = (float)by[3 * i + c] / 255.f;
        }

        const float* P = a.rows + img * PNNP_UNP_NPARAM;
        float m[9], g[3];
#pragma unroll
        for (int k = 0; k < 9; ++k) m[k] = P[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) g[k] = P[9 + k];

        // the Bayer channel of this row's even and odd columns, and the packed plane each goes to (unprocess.py:137-141, 160-164)
        const int odd = y & 1;
        const int ce = a.gbrg ? (odd ? 0 : 1) : (odd ? 1 : 0), co = a.gbrg ? (odd ? 1 : 2) : (odd ? 2 : 1);
        const int pe = a.gbrg ? (odd ? 0 : 2) : (odd ? 3 : 0), po = a.gbrg ? (odd ? 1 : 3) : (odd ? 2 : 1);

        float o[4][3], pk[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float c[3], safe[3];
            unp_pixel(v[i], m, g, c, safe);
            const int ch = (i & 1) ? co : ce;
            if (a.out_rgb) {
#pragma unroll
                for (int k = 0; k < 3; ++k) o[i][k] = pnnp_clampf(c[k] * safe[k], 0.f, 1.f);
                pk[i] = ch == 0 ? o[i][0] : (ch == 1 ? o[i][1] : o[i][2]);
            } else {                                             // packed only: the gain and the clamp on the pixel's Bayer channel alone
                const float cc = ch == 0 ? c[0] : (ch == 1 ? c[1] : c[2]), ss = ch == 0 ? safe[0] : (ch == 1 ? safe[1] : safe[2]);
                pk[i] = pnnp_clampf(cc * ss, 0.f, 1.f);
            }
        }

        if (a.out_rgb) {
            if constexpr (KIND == PNNP_UNP_IN_CHW_F32) {
                float* dst = a.out_rgb + chw;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    if (a.vec) {
                        f32x4 t;
                        t.x = o[0][c]; t.y = o[1][c]; t.z = o[2][c]; t.w = o[3][c];
                        *(f32x4*)(dst + c * plane) = t;
                    } else {
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            if (i < n) dst[c * plane + i] = o[i][c];
                    }
                }
            } else {
                float* dst = a.out_rgb + 3 * pix;
                if (a.vec) {
                    f32x4 t0, t1, t2;
                    t0.x = o[0][0]; t0.y = o[0][1]; t0.z = o[0][2]; t0.w = o[1][0]; t1.x = o[1][1]; t1.y = o[1][2];
                    t1.z = o[2][0]; t1.w = o[2][1]; t2.x = o[2][2]; t2.y = o[3][0]; t2.z = o[3][1]; t2.w = o[3][2];
                    ((f32x4*)dst)[0] = t0; ((f32x4*)dst)[1] = t1; ((f32x4*)dst)[2] = t2;
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int c = 0; c < 3; ++c)
                            if (i < n) dst[3 * i + c] = o[i][c];
                }
            }
        }
        if (a.out_packed) {                                      // H and W are even here: n is 2 or 4
            const int64_t pp = (int64_t)h2 * w2;
            float* de = a.out_packed + (img * 4 + pe) * pp + (int64_t)(y >> 1) * w2 + (x0 >> 1);
            float* dq = a.out_packed + (img * 4 + po) * pp + (int64_t)(y >> 1) * w2 + (x0 >> 1);
            if (a.vec) {
                f32x2 te, tq;
                te.x = pk[0]; te.y = pk[2]; tq.x = pk[1]; tq.y = pk[3];
                *(f32x2*)de = te; *(f32x2*)dq = tq;
            } else {
                de[0] = pk[0]; dq[0] = pk[1];
                if (n == 4) { de[1] = pk[2]; dq[1] = pk[3]; }
            }
        }
    }
}

inline bool unp_aligned(const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) == 0; }

}  // namespace

extern "C" {

int pnnp_unprocess_f32(const void* in, int in_kind, int B, int H, int W, const float* rows, unsigned flags, float* out_rgb, float* out_packed,
                       void* stream) {
    if (!in || !rows || (!out_rgb && !out_packed) || B < 1 || H < 1 || W < 1) return PNNP_E_INVALID;
    if (in_kind != PNNP_UNP_IN_HWC_F32 && in_kind != PNNP_UNP_IN_CHW_F32 && in_kind != PNNP_UNP_IN_HWC_U8) return PNNP_E_INVALID;
    if (flags & ~PNNP_UNP_GBRG) return PNNP_E_INVALID;
    if (out_packed && ((H | W) & 1)) return PNNP_E_INVALID;      // the reference's torch.stack of the four gathers fails on an odd size
    const uintptr_t elem = in_kind == PNNP_UNP_IN_HWC_U8 ? 0 : 3;
    if (!unp_aligned(in, elem) || !unp_aligned(rows, 3) || !unp_aligned(out_rgb, 3) || !unp_aligned(out_packed, 3)) return PNNP_E_INVALID;
    const int W4 = (W + 3) / 4;
    const int64_t items = (int64_t)B * H * W4;
    if ((int64_t)B * H * W >= (1ll << 40)) return PNNP_E_INVALID;
    UnpArgs a{};
    a.in = in; a.rows = rows; a.out_rgb = out_rgb; a.out_packed = out_packed;
    a.items = items; a.H = H; a.W = W; a.W4 = W4; a.gbrg = (flags & PNNP_UNP_GBRG) ? 1 : 0;
    a.vec = W % 4 == 0 && unp_aligned(in, in_kind == PNNP_UNP_IN_HWC_U8 ? 3 : 15) && unp_aligned(out_rgb, 15) && unp_aligned(out_packed, 15);
    const int64_t want = (items + UNP_THREADS - 1) / UNP_THREADS;
    const dim3 grid((unsigned)(want < UNP_MAX_BLOCKS ? want : UNP_MAX_BLOCKS)), block(UNP_THREADS);
    if (in_kind == PNNP_UNP_IN_HWC_F32) hipLaunchKernelGGL(unprocess_kernel<PNNP_UNP_IN_HWC_F32>, grid, block, 0, as_stream(stream), a);
    else if (in_kind == PNNP_UNP_IN_CHW_F32) hipLaunchKernelGGL(unprocess_kernel<PNNP_UNP_IN_CHW_F32>, grid, block, 0, as_stream(stream), a);
    else hipLaunchKernelGGL(unprocess_kernel<PNNP_UNP_IN_HWC_U8>, grid, block, 0, as_stream(stream), a);
    return pnnp_launch_status();
}

}  // extern "C"

// Packed raw -> sRGB on the device: the reference's pure-tensor ISP, data_process/process.py:104-184 (apply_gains, raw2LRGB,
// apply_ccms, gamma_compression, process, raw2rgb_v2), and the trainers' per-epoch preview strip (trainer_SID.py:150-158, trainer_NF_SID.py:166-180).
//
// One streaming pass: 16 B read and 3 B (uint8) and / or 12 B (float planes) written per pixel; no LDS, no atomics.  A lane owns 4 consecutive pixels
// of a row: one 16-byte non-temporal load per plane (the input is read once), the 12 output bytes packed into three dwords, one 16-byte store per
// float plane.  blockIdx.y is the image (the panel of a preview), so the parameter row is uniform over the workgroup.  When W % 4 != 0 (rows
// then start at any element) or an array is not 16-byte aligned, every lane takes the scalar path: same arithmetic, element accesses.
//
// Arithmetic: float32, every operation rounded on its own (this file is built with -ffp-contract=off), in the reference's order; the operand order
// of the matrix row, (r c0 + g c1) + b c2, is what torch.sum gives and decides saturated highlights: with all channels at 1 a row of the Sony
// matrix sums to 1 or to 1 - 2^-24, and 1 - 2^-23 would already render as 254.  The power x ^ float32(1/2.2) is evaluated in float64 as
// exp(e log x) on the float32 operands (relative error about 1e-15, nine orders below a float32 ulp) and rounded once to float32: the correctly
// rounded float32 power except where the exact value lies within 1e-15 of a rounding tie.  torch's own float32 pow is within one ulp of it.
// Only values next to a quantisation threshold pay for it: see isp_level.
#include "common.h"

namespace {

constexpr int ISP_THREADS = 256;
enum { ISP_PROCESS = 0, ISP_GAMMA = 1, ISP_PREVIEW = 2 };
constexpr float ISP_EXPONENT = (float)(1.0 / 2.2);               // torch (and numpy on a float32 array) raise to the float32 exponent

struct IspArgs {
    const float *src0, *src1, *src2;                             // the input (process, gamma) or the three panels (preview)
    const float* mid;                                            // preview: added to panel 1 after a clip to [0,1], or null
    const float* rows;                                           // process: [B][PNNP_ISP_NPARAM]
    float* outf;
    unsigned char* out8;
    float wb0, wb2;                                              // preview gains of channels 0 and 2
    int H, W, W4, bgr, vec;
};

// gamma_compression: clamp(min=1e-8) ** (1/2.2), (x * 255).int(), clamp(0, 255).  A NaN falls through every select and renders as 0.
//
// The float64 power is the whole cost of the kernel (it is issue-bound on it, profiles/r7/isp_render.txt), and the level it yields can differ from
// a cheap estimate only next to a quantisation threshold.  So every value first takes the hardware's float32 log2 / exp2 (1 ulp each):
//   y = e log2 m: |log2 m| <= 26.6 (m >= 1e-8), so the log's ulp is 2^-19 = 1.9e-6, times e = 8.7e-7, plus the product's half ulp 4.8e-7;
//   2^y is then off by ln 2 * 1.35e-6 + 1.2e-7 (its own ulp) = 1.05e-6 relative, and s = 255 * 2^y by at most 2.7e-4 + 1.5e-5 (the product);
//   the exact path's own s is within 2.3e-5 of the real value.  Together under 3.1e-4.
// A value whose estimate lies further than ISP_MARGIN = 2e-3 (6 times that) from every integer truncates to the same level on both paths and
// keeps the estimate; the others (0.4 % of uniformly spread values) take the float64 path.  m = 1 (clamped highlights) is 255 exactly; an
// estimate below 0.5 is level 0 on both paths; a NaN fails every comparison and renders as 0.
constexpr float ISP_MARGIN = 2e-3f;

__device__ __forceinline__ float isp_scaled_exact(float m) { return (float)exp((double)ISP_EXPONENT * log((double)m)) * 255.f; }

template <bool FLOOR>
__device__ __forceinline__ int isp_level(float v) {
    const float m = FLOOR ? (v < 1e-8f ? 1e-8f : v) : v;
    if (m == 1.f) return 255;
    float s = __builtin_amdgcn_exp2f(ISP_EXPONENT * __builtin_amdgcn_logf(m)) * 255.f;   // v_exp_f32, v_log_f32
    const float r = rintf(s);
    if (fabsf(s - r) < ISP_MARGIN && r >= 1.f && r <= 255.f) s = isp_scaled_exact(m);
    return s >= 1.f ? (s >= 255.f ? 255 : (int)s) : 0;
}

template <int MODE>
__global__ void __launch_bounds__(ISP_THREADS) isp_render_kernel(IspArgs a) {
    constexpr int NIN = MODE == ISP_PROCESS ? 4 : 3;             // planes read
    constexpr int NPL = MODE == ISP_GAMMA ? 3 : 4;               // planes of an input image
    const int q = blockIdx.x * ISP_THREADS + threadIdx.x;
    if (q >= a.H * a.W4) return;
    const int img = blockIdx.y;
    const int y = q / a.W4, x0 = (q - y * a.W4) * 4;
    const int n = a.W - x0 < 4 ? a.W - x0 : 4;                   // pixels of this lane (< 4 only at the end of a row with W % 4 != 0)
    const int64_t plane = (int64_t)a.H * a.W, pix = (int64_t)y * a.W + x0;
    const float* src = MODE == ISP_PREVIEW ? (img == 0 ? a.src0 : (img == 1 ? a.src1 : a.src2)) : a.src0 + (int64_t)img * NPL * plane;

    float v[NIN][4];
    if (a.vec) {
#pragma unroll
        for (int c = 0; c < NIN; ++c) {
            const f32x4 t = __builtin_nontemporal_load((const f32x4*)(src + c * plane + pix));
            v[c][0] = t.x; v[c][1] = t.y; v[c][2] = t.z; v[c][3] = t.w;
        }
    } else {
#pragma unroll
        for (int c = 0; c < NIN; ++c)
#pragma unroll
            for (int i = 0; i < 4; ++i) v[c][i] = i < n ? src[c * plane + pix + i] : 0.f;
    }

    int k[3][4];
    if constexpr (MODE == ISP_PROCESS) {
        const float* P = a.rows + (int64_t)img * PNNP_ISP_NPARAM;
        float wb[4], m[9];
#pragma unroll
        for (int c = 0; c < 4; ++c) wb[c] = P[c];
#pragma unroll
        for (int c = 0; c < 9; ++c) m[c] = P[4 + c];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float r = pnnp_clampf(v[0][i] * wb[0], 0.f, 1.f), g1 = pnnp_clampf(v[1][i] * wb[1], 0.f, 1.f);
            const float b = pnnp_clampf(v[2][i] * wb[2], 0.f, 1.f), g2 = pnnp_clampf(v[3][i] * wb[3], 0.f, 1.f);
            const float g = (g1 + g2) / 2.f;                                                   // torch.mean over the two greens
#pragma unroll
            for (int c = 0; c < 3; ++c)
                k[c][i] = isp_level<true>(pnnp_clampf((r * m[3 * c] + g * m[3 * c + 1]) + b * m[3 * c + 2], 0.f, 1.f));
        }
    } else if constexpr (MODE == ISP_GAMMA) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int i = 0; i < 4; ++i) k[c][i] = isp_level<true>(v[c][i]);
    } else {
        if (img == 0) {                                                                        // inputs.clip(0, 1)
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int i = 0; i < 4; ++i) v[c][i] = pnnp_clampf(v[c][i], 0.f, 1.f);
        } else if (img == 1 && a.mid) {                                                        // sample + inputs.clip(0, 1)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float o[4];
                if (a.vec) {
                    const f32x4 t = __builtin_nontemporal_load((const f32x4*)(a.mid + c * plane + pix));
                    o[0] = t.x; o[1] = t.y; o[2] = t.z; o[3] = t.w;
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) o[i] = i < n ? a.mid[c * plane + pix + i] : 0.f;
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) v[c][i] = v[c][i] + pnnp_clampf(o[i], 0.f, 1.f);
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            k[0][i] = isp_level<false>(pnnp_clampf(v[0][i] * a.wb0, 0.f, 1.f));
            k[1][i] = isp_level<false>(pnnp_clampf(v[1][i], 0.f, 1.f));
            k[2][i] = isp_level<false>(pnnp_clampf(v[2][i] * a.wb2, 0.f, 1.f));
        }
    }

    if (a.out8) {
        // process: [B][H][W][3]; preview: [H][3W][3], panel `img` at column img * W
        const int64_t opix = MODE == ISP_PREVIEW ? (int64_t)y * 3 * a.W + (int64_t)img * a.W + x0 : (int64_t)img * plane + pix;
        unsigned char* o = a.out8 + 3 * opix;
        const int c0 = a.bgr ? 2 : 0, c2 = a.bgr ? 0 : 2;
        if (a.vec) {
            unsigned by[12];
#pragma unroll
            for (int i = 0; i < 4; ++i) { by[3 * i] = (unsigned)k[c0][i]; by[3 * i + 1] = (unsigned)k[1][i]; by[3 * i + 2] = (unsigned)k[c2][i]; }
            unsigned* o4 = (unsigned*)o;                                                       // 3 * opix bytes with opix % 4 == 0: dword aligned
#pragma unroll
            for (int d = 0; d < 3; ++d) o4[d] = by[4 * d] | (by[4 * d + 1] << 8) | (by[4 * d + 2] << 16) | (by[4 * d + 3] << 24);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i < n) { o[3 * i] = (unsigned char)k[c0][i]; o[3 * i + 1] = (unsigned char)k[1][i]; o[3 * i + 2] = (unsigned char)k[c2][i]; }
        }
    }
    if (MODE != ISP_PREVIEW && a.outf) {
        float* o = a.outf + (int64_t)img * 3 * plane + pix;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (a.vec) {
                f32x4 t;
                t.x = (float)k[c][0] / 255.f; t.y = (float)k[c][1] / 255.f; t.z = (float)k[c][2] / 255.f; t.w = (float)k[c][3] / 255.f;
                *(f32x4*)(o + c * plane) = t;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (i < n) o[c * plane + i] = (float)k[c][i] / 255.f;
            }
        }
    }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// PNNP_OK and the grid, or PNNP_E_INVALID
int isp_grid(int images, int H, int W, dim3* grid) {
    if (images < 1 || images > 65535 || H < 1 || W < 1) return PNNP_E_INVALID;
    const int64_t quads = (int64_t)H * ((W + 3) / 4);
    if (quads >= (1ll << 31) - ISP_THREADS) return PNNP_E_INVALID;
    *grid = dim3((unsigned)((quads + ISP_THREADS - 1) / ISP_THREADS), (unsigned)images);
    return PNNP_OK;
}

}  // namespace

extern "C" {

int pnnp_isp_process_f32(const float* in, int B, int H, int W, const float* rows, unsigned flags, float* out_f32, uint8_t* out_u8, void* stream) {
    const bool gamma_only = flags & PNNP_ISP_GAMMA_ONLY;
    if (!in || (!out_f32 && !out_u8) || (!gamma_only && !rows)) return PNNP_E_INVALID;
    dim3 grid;
    if (isp_grid(B, H, W, &grid) != PNNP_OK) return PNNP_E_INVALID;
    IspArgs a{};
    a.src0 = in; a.rows = rows; a.outf = out_f32; a.out8 = out_u8;
    a.H = H; a.W = W; a.W4 = (W + 3) / 4; a.bgr = (flags & PNNP_ISP_BGR) ? 1 : 0;
    a.vec = W % 4 == 0 && aligned16(in) && aligned16(out_f32) && aligned16(out_u8);
    if (gamma_only) hipLaunchKernelGGL(isp_render_kernel<ISP_GAMMA>, grid, dim3(ISP_THREADS), 0, as_stream(stream), a);
    else hipLaunchKernelGGL(isp_render_kernel<ISP_PROCESS>, grid, dim3(ISP_THREADS), 0, as_stream(stream), a);
    return pnnp_launch_status();
}

int pnnp_isp_preview_f32(const float* inputs, const float* output, const float* target, const float* mid_offset, int H, int W,
                         const float* wb, uint8_t* out_u8, void* stream) {
    if (!inputs || !output || !target || !wb || !out_u8) return PNNP_E_INVALID;
    dim3 grid;
    if (isp_grid(3, H, W, &grid) != PNNP_OK) return PNNP_E_INVALID;
    IspArgs a{};
    a.src0 = inputs; a.src1 = output; a.src2 = target; a.mid = mid_offset; a.out8 = out_u8;
    a.wb0 = wb[0]; a.wb2 = wb[2];
    a.H = H; a.W = W; a.W4 = (W + 3) / 4; a.bgr = 1;
    a.vec = W % 4 == 0 && aligned16(inputs) && aligned16(output) && aligned16(target) && aligned16(mid_offset) && aligned16(out_u8);
    hipLaunchKernelGGL(isp_render_kernel<ISP_PREVIEW>, grid, dim3(ISP_THREADS), 0, as_stream(stream), a);
    return pnnp_launch_status();
}

}  // extern "C"

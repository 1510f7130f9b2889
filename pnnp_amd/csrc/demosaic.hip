// Full-resolution render on the device: the reference's FastISP, utils/isp_ops.py:134-158, with its one outside call,
// cv2.cvtColor(COLOR_BAYER_BG2RGB_EA), replaced by the edge-aware integer demosaic defined in include/pnnp_hip.h (parity with an OpenCV
// build is not a goal: its vector and scalar loops round differently from each other).
//
// One launch: front (gained mosaic, clip, 14-bit truncation), stencil, tail (/ 16383, colour matrix, clip, gamma 2.2 in float64).  A
// workgroup stages the uint16 mosaic of its 16 x 64 tile plus one mosaic pixel of halo in LDS, so the front runs once per element
// (1188 for 1024 outputs); a lane then owns 4 consecutive output pixels of a row and stores three dwords of bytes and / or one 16-byte
// piece per float plane.  Border pixels evaluate the interior formula at the clamped coordinate: no dependence between lanes.  When
// W % 4 != 0 or an output is not 16-byte aligned, every lane stores element by element: same arithmetic.
//
// Arithmetic.  Front: float32, every operation rounded on its own (this file is built with -ffp-contract=off).  Tail: float64 as numpy
// does it, (v0 m0 + v1 m1) + v2 m2 being the order of np.sum over three elements.  The power y = v^(1/2.2) is the root of y^11 = v^5:
// the hardware's float32 log2 / exp2 give y0 (relative error e0 <= 1.1e-6 for v >= 1e-6, <= 4.1e-6 down to v = 1e-30: the budget of
// csrc/isp.hip plus the rounding of v to float32), and one Newton step in float64, y1 = y0 (1 + (v^5 / y0^11 - 1) / 11), leaves
// 5 e0^2 <= 8.4e-11 relative (6e-12 for v >= 1e-6), four orders below a float32 ulp: the float planes are float32(y1).  A level
// floor(255 y1) is final unless 255 y1 lies within 1e-6 of an integer >= 1 (2 values in a million, 700 times the step's error); those take
// exp(log(v) / 2.2) (relative error about 1e-14; numpy's own pow is within one float64 ulp of it), as do values below 1e-30.
// Both outputs of a launch come from the same y1, so the bytes do not depend on whether the float planes are asked for.
#include "common.h"

namespace {

constexpr int DM_THREADS = 256, DM_TW = 64, DM_TH = 16;          // the tile in output pixels: 16 lanes of 4 pixels x 16 rows
constexpr int DM_LW = DM_TW + 2, DM_LH = DM_TH + 2;              // ... and in LDS, with one mosaic pixel of halo
constexpr double DM_EXPONENT = 1.0 / 2.2;
constexpr float DM_EXPONENT_F = (float)(1.0 / 2.2);
constexpr double DM_MARGIN = 1e-6;
// the reference's default matrix (utils/isp_ops.py:151-153) is a float64 constant that no float32 table can carry
__constant__ double DM_SONY[9] = {1.9712269, -0.6789218, -0.29230508, -0.29104823, 1.748401, -0.45735288, 0.02051281, -0.5380369, 1.5175241};

struct DmArgs {
    const void* src;                                             // u16 [B][H][W] (stencil alone) or f32 [B][4][H/2][W/2]
    const float* rows;
    float* outf;
    unsigned char* out8;
    unsigned short* out16;
    int H, W, tiles_x, bgr, vec, sony;
};

// the uint16 mosaic element (Y, X) of image `img`: the front of FastISP, or the source itself
template <bool RAW16>
__device__ __forceinline__ unsigned short dm_element(const DmArgs& a, int img, int Y, int X, float wb0, float wb2) {
    if constexpr (RAW16) {
        return ((const unsigned short*)a.src)[((int64_t)img * a.H + Y) * a.W + X];
    } else {
        const int h = a.H >> 1, w = a.W >> 1;
        const int plane = (Y & 1) ? ((X & 1) ? 2 : 3) : (X & 1);                              // R G1 / G2 B
        float v = ((const float*)a.src)[(((int64_t)img * 4 + plane) * h + (Y >> 1)) * w + (X >> 1)];
        if (plane == 0) v = v * wb0;
        if (plane == 2) v = v * wb2;
        const float s = pnnp_clampf(v, 0.f, 1.f) * 16383.0f;
        return s == s ? (unsigned short)s : (unsigned short)0;                                // a NaN is 0
    }
}

// the stencil at the interior pixel (cy, cx); t points at its element in the LDS tile
__device__ __forceinline__ void dm_pixel(const unsigned short* t, int cy, int cx, unsigned& R, unsigned& G, unsigned& B) {
    const int c = t[0], l = t[-1], r = t[1], u = t[-DM_LW], d = t[DM_LW];
    const unsigned hz = (unsigned)(l + r + 1) >> 1, vt = (unsigned)(u + d + 1) >> 1;
    if (((cy ^ cx) & 1) == 0) {                                                               // an R or a B site
        const int dh = l > r ? l - r : r - l, dv = u > d ? u - d : d - u;
        G = dh > dv ? vt : hz;                                                                // a tie takes the horizontal pair
        const unsigned o = ((unsigned)t[-DM_LW - 1] + t[-DM_LW + 1] + t[DM_LW - 1] + t[DM_LW + 1] + 2u) >> 2;
        if (cy & 1) { B = (unsigned)c; R = o; } else { R = (unsigned)c; B = o; }
    } else {
        G = (unsigned)c;
        if (cy & 1) { B = hz; R = vt; } else { R = hz; B = vt; }
    }
}

// D / 16383 in float64, correctly rounded, without the division's reciprocal and fix-up sequence: the product with RN(1 / 16383) and one
// residual correction, both fused.  Equal to the IEEE quotient for every uint16 D (all 65 536 checked on the host, where fma rounds the same).
__device__ __forceinline__ double dm_unit(unsigned D) {
    constexpr double y = 1.0 / 16383.0;
    const double a = (double)D, q = a * y;
    return __builtin_fma(__builtin_fma(-q, 16383.0, a), y, q);
}

// v in [0, 1] -> v^(1/2.2) in float64 and its level floor(255 v^(1/2.2)): see the head of the file
__device__ __forceinline__ double dm_gamma(double v, int& level) {
    const bool tiny = !(v >= 1e-30);                             // 0 (every clipped shadow) and cancellation residue
    const double vs = tiny ? 1.0 : v;
    const double y0 = (double)__builtin_amdgcn_exp2f(DM_EXPONENT_F * __builtin_amdgcn_logf((float)vs));   // v_exp_f32, v_log_f32
    const double y2 = y0 * y0, y4 = y2 * y2, y8 = y4 * y4, y11 = (y8 * y2) * y0;                          // >= 1e-150
    const double v2 = vs * vs, v5 = (v2 * v2) * vs;
    double r = __builtin_amdgcn_rcp(y11);                        // v_rcp_f64, then two Newton steps: 1 / y11 to float64 accuracy whatever its own
    r = __builtin_fma(__builtin_fma(-y11, r, 1.0), r, r);
    r = __builtin_fma(__builtin_fma(-y11, r, 1.0), r, r);
    double y = __builtin_fma(y0, __builtin_fma(v5, r, -1.0) * (1.0 / 11.0), y0);
    double s = 255.0 * y;
    const double near = rint(s);
    if (tiny ? v > 0.0 : (fabs(s - near) < DM_MARGIN && near >= 1.0 && v < 1.0)) {
        y = exp(DM_EXPONENT * log(v));
        s = 255.0 * y;
    }
    if (tiny && !(v > 0.0)) { y = 0.0; s = 0.0; }
    level = (int)s;
    return y;
}

enum { DM_RAW16 = 0, DM_FASTISP = 1 };                           // the stencil alone; front, stencil and tail

template <int MODE>
__global__ void __launch_bounds__(DM_THREADS) demosaic_kernel(DmArgs a) {
    __shared__ unsigned short tile[DM_LH * DM_LW];
    const int img = blockIdx.y;
    const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
    const int y0 = ty * DM_TH, x0t = tx * DM_TW;
    float wb0 = 0.f, wb2 = 0.f;
    if constexpr (MODE != DM_RAW16) { wb0 = a.rows[(int64_t)img * PNNP_ISP_NPARAM]; wb2 = a.rows[(int64_t)img * PNNP_ISP_NPARAM + 2]; }
    for (int i = threadIdx.x; i < DM_LH * DM_LW; i += DM_THREADS) {
        const int ly = i / DM_LW, lx = i - ly * DM_LW;
        int Y = y0 - 1 + ly, X = x0t - 1 + lx;                   // clamped into the frame: what lies outside is never read by an output
        Y = Y < 0 ? 0 : (Y > a.H - 1 ? a.H - 1 : Y);
        X = X < 0 ? 0 : (X > a.W - 1 ? a.W - 1 : X);
        tile[i] = dm_element<MODE == DM_RAW16>(a, img, Y, X, wb0, wb2);
    }
    __syncthreads();

    const int y = y0 + (threadIdx.x >> 4), x0 = x0t + (threadIdx.x & 15) * 4;
    if (y >= a.H || x0 >= a.W) return;
    const int n = a.W - x0 < 4 ? a.W - x0 : 4;
    const int cy = y < 1 ? 1 : (y > a.H - 2 ? a.H - 2 : y);
    unsigned rgb[3][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int x = x0 + i < a.W ? x0 + i : a.W - 1;
        const int cx = x < 1 ? 1 : (x > a.W - 2 ? a.W - 2 : x);
        dm_pixel(tile + (cy - y0 + 1) * DM_LW + (cx - x0t + 1), cy, cx, rgb[0][i], rgb[1][i], rgb[2][i]);
    }
    const int64_t plane = (int64_t)a.H * a.W, pix = (int64_t)y * a.W + x0;

    if constexpr (MODE == DM_RAW16) {
        unsigned short* o = a.out16 + ((int64_t)img * plane + pix) * 3;
        if (a.vec) {                                             // 24 bytes, 8-byte aligned: pix % 4 == 0
            unsigned hw[12];
#pragma unroll
            for (int i = 0; i < 4; ++i) { hw[3 * i] = rgb[0][i]; hw[3 * i + 1] = rgb[1][i]; hw[3 * i + 2] = rgb[2][i]; }
            u32x2* o2 = (u32x2*)o;
#pragma unroll
            for (int d = 0; d < 3; ++d) { u32x2 t; t.x = hw[4 * d] | (hw[4 * d + 1] << 16); t.y = hw[4 * d + 2] | (hw[4 * d + 3] << 16); o2[d] = t; }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i < n) { o[3 * i] = (unsigned short)rgb[0][i]; o[3 * i + 1] = (unsigned short)rgb[1][i]; o[3 * i + 2] = (unsigned short)rgb[2][i]; }
        }
    } else {
        double m[9];
#pragma unroll
        for (int c = 0; c < 9; ++c) m[c] = a.sony ? DM_SONY[c] : (double)a.rows[(int64_t)img * PNNP_ISP_NPARAM + 4 + c];
        int k[3][4];
        float p[3][4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const double v0 = dm_unit(rgb[0][i]), v1 = dm_unit(rgb[1][i]), v2 = dm_unit(rgb[2][i]);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                double lin = (v0 * m[3 * c] + v1 * m[3 * c + 1]) + v2 * m[3 * c + 2];
                lin = lin < 0.0 ? 0.0 : (lin > 1.0 ? 1.0 : lin);
                p[c][i] = (float)dm_gamma(lin, k[c][i]);
            }
        }
        if (a.out8) {
            unsigned char* o = a.out8 + ((int64_t)img * plane + pix) * 3;
            const int c0 = a.bgr ? 2 : 0, c2 = a.bgr ? 0 : 2;
            if (a.vec) {
                unsigned by[12];
#pragma unroll
                for (int i = 0; i < 4; ++i) { by[3 * i] = (unsigned)k[c0][i]; by[3 * i + 1] = (unsigned)k[1][i]; by[3 * i + 2] = (unsigned)k[c2][i]; }
                unsigned* o4 = (unsigned*)o;
#pragma unroll
                for (int d = 0; d < 3; ++d) o4[d] = by[4 * d] | (by[4 * d + 1] << 8) | (by[4 * d + 2] << 16) | (by[4 * d + 3] << 24);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (i < n) { o[3 * i] = (unsigned char)k[c0][i]; o[3 * i + 1] = (unsigned char)k[1][i]; o[3 * i + 2] = (unsigned char)k[c2][i]; }
            }
        }
        if (a.outf) {
            float* o = a.outf + (int64_t)img * 3 * plane + pix;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (a.vec) {
                    f32x4 t;
                    t.x = p[c][0]; t.y = p[c][1]; t.z = p[c][2]; t.w = p[c][3];
                    *(f32x4*)(o + c * plane) = t;
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (i < n) o[c * plane + i] = p[c][i];
                }
            }
        }
    }
}

inline bool dm_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// PNNP_OK and the grid, or PNNP_E_INVALID: a Bayer frame (even sides) of at least 4 x 4 whose 3 H W output elements of one image index below
// 2^31.  Even sides also keep the clamped coordinate of a partial tile's pixels inside the tile's halo (an odd W could leave a tile one column).
int dm_grid(int images, int H, int W, dim3* grid, int* tiles_x) {
    if (images < 1 || images > 65535 || H < 4 || W < 4 || (H & 1) || (W & 1)) return PNNP_E_INVALID;
    if (3 * (int64_t)H * W >= (1ll << 31)) return PNNP_E_INVALID;
    *tiles_x = (W + DM_TW - 1) / DM_TW;
    const int64_t tiles = (int64_t)*tiles_x * ((H + DM_TH - 1) / DM_TH);
    *grid = dim3((unsigned)tiles, (unsigned)images);
    return PNNP_OK;
}

}  // namespace

extern "C" {

int pnnp_demosaic_ea_u16(const uint16_t* src, int B, int H, int W, uint16_t* dst, void* stream) {
    if (!src || !dst) return PNNP_E_INVALID;
    DmArgs a{};
    dim3 grid;
    if (dm_grid(B, H, W, &grid, &a.tiles_x) != PNNP_OK) return PNNP_E_INVALID;
    a.src = src; a.out16 = dst; a.H = H; a.W = W;
    a.vec = W % 4 == 0 && dm_aligned16(dst);
    hipLaunchKernelGGL(demosaic_kernel<DM_RAW16>, grid, dim3(DM_THREADS), 0, as_stream(stream), a);
    return pnnp_launch_status();
}

int pnnp_fastisp_f32(const float* in, int B, int h, int w, const float* rows, unsigned flags, float* out_f32, uint8_t* out_u8, void* stream) {
    if (!in || !rows || (!out_f32 && !out_u8) || h < 2 || w < 2 || h > (1 << 29) || w > (1 << 29)) return PNNP_E_INVALID;
    DmArgs a{};
    dim3 grid;
    if (dm_grid(B, 2 * h, 2 * w, &grid, &a.tiles_x) != PNNP_OK) return PNNP_E_INVALID;
    a.src = in; a.rows = rows; a.outf = out_f32; a.out8 = out_u8; a.H = 2 * h; a.W = 2 * w;
    a.bgr = (flags & PNNP_ISP_BGR) ? 1 : 0; a.sony = (flags & PNNP_FASTISP_SONY_CCM) ? 1 : 0;
    a.vec = a.W % 4 == 0 && dm_aligned16(out_f32) && dm_aligned16(out_u8);
    hipLaunchKernelGGL(demosaic_kernel<DM_FASTISP>, grid, dim3(DM_THREADS), 0, as_stream(stream), a);
    return pnnp_launch_status();
}

}  // extern "C"

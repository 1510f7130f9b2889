// The reference's classical raw toolbox on the device: utils/isp_algos.py (VST / inverse_VST, stdfilt, GuidedFilter,
// FastGuidedFilter) and the two OpenCV-backed helpers of utils/isp_ops.py (bayer2gray :70-74, repair_bad_pixels :115-123).  The OpenCV
// calls (boxFilter, blur, resize, filter2D, medianBlur) are replaced by the definitions in include/pnnp_hip.h; parity with an OpenCV build
// is not a goal.
//
// The box mean.  A workgroup of 256 threads owns a tile of TH x 64 outputs of one plane (TH = 16, or 32 from d = 17 on, where the halo of
// 2r rows would otherwise outweigh the tile).  It stages the tile's sources plus r pixels of halo in LDS as float32 -- the border rule, the
// plane's strides and, in half mode, the 0.5x bilinear resize are applied there, once per element -- and then takes one quantity at a time
// (p, I, I*I, I*p for guided_ab): every thread sums d staged values of a row in float64 into a row-sum array in LDS, a barrier, and every
// thread sums d row sums of its column for each of its TH / 4 outputs, multiplies by the float64 constant 1 / d^2 and rounds once to
// float32.  Every sum starts at its first term and adds the others in order: no running sum is carried from one output to the next, so a
// NaN or an inf reaches exactly the outputs whose window holds it.  Products are rounded to float32 before they are widened, and everything
// after the means is float32, one rounding per operation (this file is built with -ffp-contract=off).  Accesses are 4-byte vector loads
// and stores, consecutive lanes on consecutive pixels.
#include "common.h"

namespace {

constexpr int BX_THREADS = 256, BX_TW = 64;
constexpr int BX_MAX_D = 51;
enum { BX_AB = 0, BX_AB_SELF = 1, BX_APPLY = 2, BX_MEANS = 3, BX_STD = 4 };

struct BxArgs {
    const float *s0, *s1;        // the boxed sources: (p, I), (I, -), (a, b), (x, -)
    const float* g;              // BX_APPLY: the guide
    float *o0, *o1;
    int64_t sp, sr, sx;          // element strides (plane, row, pixel) of the sources, of the guide, of the outputs
    int64_t gp, gr, gx;
    int64_t op, orow, ox;
    int H, W;                    // the size at which the box runs (half mode: half the sources' size)
    int r, reflect, half, tiles_x;
    float eps;
    double inv;                  // 1.0 / (d * d)
};

// the coordinate c of a line of n pixels under the border rule, then clamped: what a partial tile stages beyond the frame's own halo is
// never read by an output that is stored, and stays inside the plane
__device__ __forceinline__ int bx_map(int c, int n, int reflect) {
    if (reflect) c = c < 0 ? -c : (c >= n ? 2 * (n - 1) - c : c);
    return c < 0 ? 0 : (c > n - 1 ? n - 1 : c);
}

__device__ __forceinline__ float bx_read(const float* s, const BxArgs& a, int y, int x) {
    if (a.half) {                // cv2.resize(fx = fy = 0.5, INTER_LINEAR): the 2 x 2 block's mean, horizontal pairs first (the products are exact)
        const float* q = s + (int64_t)(2 * y) * a.sr + (int64_t)(2 * x) * a.sx;
        const float x00 = q[0], x01 = q[a.sx], x10 = q[a.sr], x11 = q[a.sr + a.sx];
        return (x00 + x01) * 0.25f + (x10 + x11) * 0.25f;
    }
    return s[(int64_t)y * a.sr + (int64_t)x * a.sx];
}

// np.maximum(t, 0): a NaN stays, -0.0 stays (it compares >= 0)
__device__ __forceinline__ float np_max0(float t) { return (t >= 0.f || t != t) ? t : 0.f; }

template <int MODE, int TH>
__global__ void __launch_bounds__(BX_THREADS) box_kernel(BxArgs a) {
    extern __shared__ __align__(16) unsigned char bx_lds[];
    constexpr int NSRC = (MODE == BX_AB_SELF || MODE == BX_STD) ? 1 : 2;
    constexpr int NQ = MODE == BX_AB ? 4 : 2;
    constexpr int RPT = TH / 4;                                  // outputs per thread: rows tr, tr + 4, ...
    const int r = a.r, d = 2 * r + 1, LH = TH + 2 * r, LW = BX_TW + 2 * r;
    double* R = (double*)bx_lds;                                 // [LH][64] row sums of the current quantity
    float* S0 = (float*)(R + LH * BX_TW);                        // [LH][LW] staged sources
    float* S1 = S0 + LH * LW;
    const int plane = blockIdx.y;
    const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
    const int y0 = ty * TH, x0 = tx * BX_TW;
    const float* s0 = a.s0 + (int64_t)plane * a.sp;
    const float* s1 = NSRC == 2 ? a.s1 + (int64_t)plane * a.sp : nullptr;

    for (int i = threadIdx.x; i < LH * LW; i += BX_THREADS) {
        const int ly = i / LW, lx = i - ly * LW;
        const int Y = bx_map(y0 - r + ly, a.H, a.reflect), X = bx_map(x0 - r + lx, a.W, a.reflect);
        S0[i] = bx_read(s0, a, Y, X);
        if constexpr (NSRC == 2) S1[i] = bx_read(s1, a, Y, X);
    }
    __syncthreads();

    const int lx = threadIdx.x & 63, tr = threadIdx.x >> 6;
    float m[NQ][RPT];
    static_for<0, NQ>([&](auto qc) {
        constexpr int q = decltype(qc)::value;
        auto term = [&](int at) -> double {                      // the quantity's float32 value at a staged element, widened
            if constexpr (q == 0) return (double)S0[at];
            else if constexpr (MODE == BX_AB) return q == 1 ? (double)S1[at] : (q == 2 ? (double)(S1[at] * S1[at]) : (double)(S1[at] * S0[at]));
            else if constexpr (NSRC == 1) return (double)(S0[at] * S0[at]);
            else return (double)S1[at];
        };
        for (int e = threadIdx.x; e < LH * BX_TW; e += BX_THREADS) {
            const int at = (e >> 6) * LW + (e & 63);
            double acc = term(at);
            for (int k = 1; k < d; ++k) acc += term(at + k);
            R[e] = acc;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < RPT; ++j) {
            const double* c = R + (tr + 4 * j) * BX_TW + lx;
            double acc = c[0];
            for (int k = 1; k < d; ++k) acc += c[k * BX_TW];
            m[q][j] = (float)(acc * a.inv);
        }
        __syncthreads();
    });

    const int X = x0 + lx;
    if (X >= a.W) return;
#pragma unroll
    for (int j = 0; j < RPT; ++j) {
        const int Y = y0 + tr + 4 * j;
        if (Y >= a.H) continue;
        const int64_t o = (int64_t)plane * a.op + (int64_t)Y * a.orow + (int64_t)X * a.ox;
        if constexpr (MODE == BX_AB || MODE == BX_AB_SELF) {
            const float mu_p = m[0][j], mu_I = MODE == BX_AB ? m[1][j] : m[0][j];
            const float II = MODE == BX_AB ? m[2][j] : m[1][j], Ip = MODE == BX_AB ? m[3][j] : m[1][j];
            const float var = II - mu_I * mu_I, cov = Ip - mu_I * mu_p;
            const float av = cov / (var + a.eps);                // IEEE division (hipcc's default for float32)
            a.o0[o] = av;
            a.o1[o] = mu_p - av * mu_I;
        } else if constexpr (MODE == BX_APPLY) {
            const float gv = a.g[(int64_t)plane * a.gp + (int64_t)Y * a.gr + (int64_t)X * a.gx];
            a.o0[o] = m[0][j] * gv + m[1][j];
        } else if constexpr (MODE == BX_MEANS) {
            a.o0[o] = m[0][j];
            a.o1[o] = m[1][j];
        } else {
            a.o0[o] = sqrtf(np_max0(m[1][j] - m[0][j] * m[0][j]));
        }
    }
}

template <int MODE, int TH>
int bx_launch_th(BxArgs a, int N, hipStream_t st) {
    static PnnpPerDevice once;
    constexpr int NSRC = (MODE == BX_AB_SELF || MODE == BX_STD) ? 1 : 2;
    const int LH = TH + 2 * a.r, LW = BX_TW + 2 * a.r;
    const int bytes = LH * BX_TW * 8 + NSRC * LH * LW * 4;
    // the limit is raised once per device, so to this instantiation's largest request: r = 7 on the 16-row tile (below 64 KB: nothing to
    // raise), r = 25 on the 32-row tile (116 768 B with two sources, 79 376 B with one)
    constexpr int RMAX = TH == 16 ? 7 : BX_MAX_D / 2;
    constexpr int MAX_BYTES = (TH + 2 * RMAX) * (BX_TW * 8 + NSRC * (BX_TW + 2 * RMAX) * 4);
    if (bytes > MAX_BYTES || pnnp_allow_lds(once, box_kernel<MODE, TH>, MAX_BYTES) != PNNP_OK) return PNNP_E_LAUNCH;
    a.tiles_x = (a.W + BX_TW - 1) / BX_TW;
    const int64_t tiles = (int64_t)a.tiles_x * ((a.H + TH - 1) / TH);
    hipLaunchKernelGGL((box_kernel<MODE, TH>), dim3((unsigned)tiles, (unsigned)N), dim3(BX_THREADS), bytes, st, a);
    return pnnp_launch_status();
}

template <int MODE>
int bx_launch(const BxArgs& a, int N, hipStream_t st) {
    return a.r >= 8 ? bx_launch_th<MODE, 32>(a, N, st) : bx_launch_th<MODE, 16>(a, N, st);
}

// what every box entry refuses: the window, the plane count, the size, and REFLECT_101 with a window that reaches past the frame's mirror
bool bx_valid(int N, int H, int W, int d, int reflect) {
    if (N < 1 || N > 65535 || H < 1 || W < 1 || H > (1 << 24) || W > (1 << 24)) return false;
    if (d < 1 || d > BX_MAX_D || !(d & 1)) return false;
    if ((int64_t)((W + BX_TW - 1) / BX_TW) * ((H + 15) / 16) >= (1ll << 31)) return false;
    if (reflect && d / 2 >= (H < W ? H : W)) return false;
    return true;
}

bool bx_strides(const int64_t* s) { return s && s[0] >= 0 && s[1] >= 1 && s[2] >= 1; }

// FastGuidedFilter's tail: the low-resolution means upsampled by 2 with INTER_LINEAR's rule (source coordinate (x + 0.5) / 2 - 0.5: weights
// 0.75 / 0.25, 0 where the neighbour would lie outside), horizontal pass first, each pass s0 (1 - w) + s1 w in float32; then mu_a I + mu_b
struct UpArgs {
    const float *ma, *mb, *g;
    float* out;
    int64_t gp, gr, gx, op, orow, ox;
    int H, W, h, w;
};

__device__ __forceinline__ void up_coord(int X, int n, int& i0, int& i1, float& w1) {
    i0 = (X & 1) ? (X >> 1) : (X >> 1) - 1;
    w1 = (X & 1) ? 0.25f : 0.75f;
    if (i0 < 0) { i0 = 0; w1 = 0.f; }
    if (i0 >= n - 1) { i0 = n - 1; w1 = 0.f; }
    i1 = i0 + 1 < n ? i0 + 1 : n - 1;
}

__device__ __forceinline__ float up_sample(const float* s, int w, int ya, int yb, float wy, int xa, int xb, float wx) {
    const float ha = s[(int64_t)ya * w + xa] * (1.f - wx) + s[(int64_t)ya * w + xb] * wx;
    const float hb = s[(int64_t)yb * w + xa] * (1.f - wx) + s[(int64_t)yb * w + xb] * wx;
    return ha * (1.f - wy) + hb * wy;
}

__global__ void __launch_bounds__(BX_THREADS) up_apply_kernel(UpArgs a) {
    const int64_t idx = (int64_t)blockIdx.x * BX_THREADS + threadIdx.x;
    if (idx >= (int64_t)a.H * a.W) return;
    const int Y = (int)(idx / a.W), X = (int)(idx - (int64_t)Y * a.W), plane = blockIdx.y;
    int ya, yb, xa, xb;
    float wy, wx;
    up_coord(Y, a.h, ya, yb, wy);
    up_coord(X, a.w, xa, xb, wx);
    const int64_t lo = (int64_t)plane * a.h * a.w;
    const float mu_a = up_sample(a.ma + lo, a.w, ya, yb, wy, xa, xb, wx), mu_b = up_sample(a.mb + lo, a.w, ya, yb, wy, xa, xb, wx);
    const float gv = a.g[(int64_t)plane * a.gp + (int64_t)Y * a.gr + (int64_t)X * a.gx];
    a.out[(int64_t)plane * a.op + (int64_t)Y * a.orow + (int64_t)X * a.ox] = mu_a * gv + mu_b;
}

// ---------------------------------------------------------------- VST / inverse_VST (utils/isp_algos.py:4-18), elementwise
struct VstArgs {
    const float* x;
    float* out;
    const float* scale;          // optional, one value per `group` elements: forward takes x * scale, inverse returns result / scale
    int64_t n, group;
    float c[5];                  // forward: gain, c1, c2, c3, 2 / gain; inverse: 3/8, sigma^2 / gain^2, gain
    float wp;
    int inverse, vec;
};

__device__ __forceinline__ float vst_one(const VstArgs& a, float x, float s) {
    if (!a.inverse) {
        if (a.scale) x = x * s;
        const float t = ((a.c[0] * x + a.c[1]) + a.c[2]) - a.c[3];
        const float y = sqrtf(np_max0(t)) / a.wp;
        return a.c[4] * y;
    }
    x = x * a.wp;
    const float hx = x / 2.0f;
    float y = (hx * hx - a.c[0]) - a.c[1];
    y = (y * a.c[2]) / a.wp;
    return a.scale ? y / s : y;
}

__global__ void __launch_bounds__(BX_THREADS) vst_kernel(VstArgs a) {
    const int64_t i = ((int64_t)blockIdx.x * BX_THREADS + threadIdx.x) * 4;
    if (i >= a.n) return;
    if (a.vec && i + 4 <= a.n) {                                 // group % 4 == 0: the four elements share a scale
        const f32x4 v = *(const f32x4*)(a.x + i);
        const float s = a.scale ? a.scale[i / a.group] : 1.f;
        f32x4 o;
        o.x = vst_one(a, v.x, s); o.y = vst_one(a, v.y, s); o.z = vst_one(a, v.z, s); o.w = vst_one(a, v.w, s);
        *(f32x4*)(a.out + i) = o;
    } else {
        for (int64_t k = i; k < i + 4 && k < a.n; ++k) a.out[k] = vst_one(a, a.x[k], a.scale ? a.scale[k / a.group] : 1.f);
    }
}

// ---------------------------------------------------------------- bayer2gray (utils/isp_ops.py:70-74)
// filter2D with [1 2 1; 2 4 2; 1 2 1] / 16 and BORDER_REFLECT (cba|abc|cba): the nine products are exact in float64, their sum in
// row-major order is rounded once
__global__ void __launch_bounds__(BX_THREADS) gray_kernel(const float* src, float* dst, int H, int W) {
    const int64_t idx = (int64_t)blockIdx.x * BX_THREADS + threadIdx.x;
    if (idx >= (int64_t)H * W) return;
    const int y = (int)(idx / W), x = (int)(idx - (int64_t)y * W);
    const float* s = src + (int64_t)blockIdx.y * H * W;
    double acc = 0.0;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
        int Y = y + dy;
        Y = Y < 0 ? 0 : (Y > H - 1 ? H - 1 : Y);                 // BORDER_REFLECT one pixel out is the edge pixel
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            int X = x + dx;
            X = X < 0 ? 0 : (X > W - 1 ? W - 1 : X);
            const double wgt = (dy == 0 ? 2.0 : 1.0) * (dx == 0 ? 2.0 : 1.0) / 16.0;
            const double t = (double)s[(int64_t)Y * W + X] * wgt;
            acc = (dy == -1 && dx == -1) ? t : acc + t;
        }
    }
    dst[(int64_t)blockIdx.y * H * W + idx] = (float)acc;
}

// ---------------------------------------------------------------- repair_bad_pixels (utils/isp_ops.py:115-123)
// Two launches: every point's median of the 3 x 3 neighbourhood in its own colour plane (stride 2 in the mosaic, REPLICATE at the plane's
// border) is taken from the unmodified frame into `tmp`; the second launch writes them.  Duplicates write the same value.
template <typename T>
__device__ __forceinline__ void med_cs(T& x, T& y) { const T lo = x < y ? x : y, hi = x < y ? y : x; x = lo; y = hi; }

template <typename T>
__global__ void __launch_bounds__(BX_THREADS) median_kernel(const T* raw, int H, int W, const int* pts, int n, T* tmp) {
    const int i = blockIdx.x * BX_THREADS + threadIdx.x;
    if (i >= n) return;
    const int y = pts[2 * i], x = pts[2 * i + 1];
    if (y < 0 || y >= H || x < 0 || x >= W) return;              // refused on the host; never an access outside the frame
    const int py = y & 1, px = x & 1, h = H >> 1, w = W >> 1, cy = y >> 1, cx = x >> 1;
    T v[9];
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            int Y = cy + dy, X = cx + dx;
            Y = Y < 0 ? 0 : (Y > h - 1 ? h - 1 : Y);
            X = X < 0 ? 0 : (X > w - 1 ? w - 1 : X);
            v[(dy + 1) * 3 + dx + 1] = raw[(int64_t)(2 * Y + py) * W + 2 * X + px];
        }
    // the 19-exchange median-of-9 network
    med_cs(v[1], v[2]); med_cs(v[4], v[5]); med_cs(v[7], v[8]); med_cs(v[0], v[1]); med_cs(v[3], v[4]); med_cs(v[6], v[7]);
    med_cs(v[1], v[2]); med_cs(v[4], v[5]); med_cs(v[7], v[8]); med_cs(v[0], v[3]); med_cs(v[5], v[8]); med_cs(v[4], v[7]);
    med_cs(v[3], v[6]); med_cs(v[1], v[4]); med_cs(v[2], v[5]); med_cs(v[4], v[7]); med_cs(v[4], v[2]); med_cs(v[6], v[4]);
    med_cs(v[4], v[2]);
    tmp[i] = v[4];
}

template <typename T>
__global__ void __launch_bounds__(BX_THREADS) repair_kernel(T* raw, int H, int W, const int* pts, int n, const T* tmp) {
    const int i = blockIdx.x * BX_THREADS + threadIdx.x;
    if (i >= n) return;
    const int y = pts[2 * i], x = pts[2 * i + 1];
    if (y < 0 || y >= H || x < 0 || x >= W) return;
    raw[(int64_t)y * W + x] = tmp[i];
}

template <typename T>
int repair_launch(void* raw, int H, int W, const int* pts, int n, void* tmp, hipStream_t st) {
    const dim3 grid((unsigned)((n + BX_THREADS - 1) / BX_THREADS));
    hipLaunchKernelGGL(median_kernel<T>, grid, dim3(BX_THREADS), 0, st, (const T*)raw, H, W, pts, n, (T*)tmp);
    if (pnnp_launch_status() != PNNP_OK) return PNNP_E_LAUNCH;
    hipLaunchKernelGGL(repair_kernel<T>, grid, dim3(BX_THREADS), 0, st, (T*)raw, H, W, pts, n, (const T*)tmp);
    return pnnp_launch_status();
}

inline bool al4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }
inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" {

int pnnp_guided_ab_f32(const float* p, const float* I, int N, int H, int W, const int64_t* strides, int d, float eps, unsigned flags,
                       float* a_out, float* b_out, void* stream) {
    if (!p || !I || !a_out || !b_out || !al4(p) || !al4(I) || !al4(a_out) || !al4(b_out) || !bx_strides(strides)) return PNNP_E_INVALID;
    if (flags & ~(PNNP_BOX_REFLECT_101 | PNNP_BOX_HALF)) return PNNP_E_INVALID;
    const int half = (flags & PNNP_BOX_HALF) ? 1 : 0, reflect = (half || (flags & PNNP_BOX_REFLECT_101)) ? 1 : 0;
    if (half && (H < 2 || W < 2 || (H & 1) || (W & 1))) return PNNP_E_INVALID;
    const int h = half ? H / 2 : H, w = half ? W / 2 : W;
    if (!bx_valid(N, h, w, d, reflect) || !(eps == eps)) return PNNP_E_INVALID;
    BxArgs a{};
    a.s0 = p; a.s1 = I; a.o0 = a_out; a.o1 = b_out;
    a.sp = strides[0]; a.sr = strides[1]; a.sx = strides[2];
    a.op = (int64_t)h * w; a.orow = w; a.ox = 1;
    a.H = h; a.W = w; a.r = d / 2; a.reflect = reflect; a.half = half; a.eps = eps; a.inv = 1.0 / ((double)d * d);
    if (p == I) { a.s0 = I; a.s1 = nullptr; return bx_launch<BX_AB_SELF>(a, N, as_stream(stream)); }
    return bx_launch<BX_AB>(a, N, as_stream(stream));
}

int pnnp_guided_apply_f32(const float* a_in, const float* b_in, const float* I, int N, int H, int W, const int64_t* i_strides, int d,
                          unsigned flags, float* workspace, float* out, const int64_t* out_strides, void* stream) {
    if (!a_in || !b_in || !I || !out || !al4(a_in) || !al4(b_in) || !al4(I) || !al4(out) || !bx_strides(i_strides) || !bx_strides(out_strides))
        return PNNP_E_INVALID;
    if (flags & ~(PNNP_BOX_REFLECT_101 | PNNP_BOX_HALF)) return PNNP_E_INVALID;
    const int half = (flags & PNNP_BOX_HALF) ? 1 : 0, reflect = (half || (flags & PNNP_BOX_REFLECT_101)) ? 1 : 0;
    if (half && (H < 2 || W < 2 || (H & 1) || (W & 1) || !workspace || !al4(workspace))) return PNNP_E_INVALID;
    const int h = half ? H / 2 : H, w = half ? W / 2 : W;
    if (!bx_valid(N, h, w, d, reflect)) return PNNP_E_INVALID;
    if (half && (int64_t)((int64_t)H * W + BX_THREADS - 1) / BX_THREADS >= (1ll << 31)) return PNNP_E_INVALID;
    BxArgs a{};
    a.s0 = a_in; a.s1 = b_in;
    a.sp = (int64_t)h * w; a.sr = w; a.sx = 1;
    a.H = h; a.W = w; a.r = d / 2; a.reflect = reflect; a.inv = 1.0 / ((double)d * d);
    if (!half) {
        a.g = I; a.gp = i_strides[0]; a.gr = i_strides[1]; a.gx = i_strides[2];
        a.o0 = out; a.op = out_strides[0]; a.orow = out_strides[1]; a.ox = out_strides[2];
        return bx_launch<BX_APPLY>(a, N, as_stream(stream));
    }
    a.o0 = workspace; a.o1 = workspace + (int64_t)N * h * w;
    a.op = (int64_t)h * w; a.orow = w; a.ox = 1;
    const int rc = bx_launch<BX_MEANS>(a, N, as_stream(stream));
    if (rc != PNNP_OK) return rc;
    UpArgs u{};
    u.ma = a.o0; u.mb = a.o1; u.g = I; u.out = out;
    u.gp = i_strides[0]; u.gr = i_strides[1]; u.gx = i_strides[2];
    u.op = out_strides[0]; u.orow = out_strides[1]; u.ox = out_strides[2];
    u.H = H; u.W = W; u.h = h; u.w = w;
    const dim3 grid((unsigned)(((int64_t)H * W + BX_THREADS - 1) / BX_THREADS), (unsigned)N);
    hipLaunchKernelGGL(up_apply_kernel, grid, dim3(BX_THREADS), 0, as_stream(stream), u);
    return pnnp_launch_status();
}

int pnnp_stdfilt_f32(const float* x, int N, int H, int W, const int64_t* strides, int k, float* out, const int64_t* out_strides, void* stream) {
    if (!x || !out || !al4(x) || !al4(out) || !bx_strides(strides) || !bx_strides(out_strides)) return PNNP_E_INVALID;
    if (!bx_valid(N, H, W, k, 1)) return PNNP_E_INVALID;
    BxArgs a{};
    a.s0 = x; a.o0 = out;
    a.sp = strides[0]; a.sr = strides[1]; a.sx = strides[2];
    a.op = out_strides[0]; a.orow = out_strides[1]; a.ox = out_strides[2];
    a.H = H; a.W = W; a.r = k / 2; a.reflect = 1; a.inv = 1.0 / ((double)k * k);
    return bx_launch<BX_STD>(a, N, as_stream(stream));
}

int pnnp_vst_f32(const float* x, int64_t n, int inverse, double sigma, double mu, double gain, double wp, const float* scale, int64_t group,
                 float* out, void* stream) {
    if (!x || !out || !al4(x) || !al4(out) || n < 1 || n >= (1ll << 40) || (inverse != 0 && inverse != 1)) return PNNP_E_INVALID;
    if (scale && (!al4(scale) || group < 1)) return PNNP_E_INVALID;
    if (!(gain == gain) || !(sigma == sigma) || !(mu == mu) || !(wp == wp) || gain == 0.0 || wp == 0.0) return PNNP_E_INVALID;
    VstArgs a{};
    a.x = x; a.out = out; a.scale = scale; a.n = n; a.group = scale ? group : 1; a.inverse = inverse; a.wp = (float)wp;
    if (!inverse) {
        a.c[0] = (float)gain; a.c[1] = (float)(gain * gain * 3.0 / 8.0); a.c[2] = (float)(sigma * sigma); a.c[3] = (float)(gain * mu);
        a.c[4] = (float)(2.0 / gain);
    } else {
        a.c[0] = 0.375f; a.c[1] = (float)(sigma * sigma / (gain * gain)); a.c[2] = (float)gain;
    }
    a.vec = al16(x) && al16(out) && (!scale || group % 4 == 0);
    const int64_t blocks = ((n + 3) / 4 + BX_THREADS - 1) / BX_THREADS;
    hipLaunchKernelGGL(vst_kernel, dim3((unsigned)blocks), dim3(BX_THREADS), 0, as_stream(stream), a);
    return pnnp_launch_status();
}

int pnnp_bayer2gray_f32(const float* src, int B, int H, int W, float* dst, void* stream) {
    if (!src || !dst || src == dst || !al4(src) || !al4(dst) || B < 1 || B > 65535 || H < 1 || W < 1) return PNNP_E_INVALID;
    if (((int64_t)H * W + BX_THREADS - 1) / BX_THREADS >= (1ll << 31)) return PNNP_E_INVALID;
    const dim3 grid((unsigned)(((int64_t)H * W + BX_THREADS - 1) / BX_THREADS), (unsigned)B);
    hipLaunchKernelGGL(gray_kernel, grid, dim3(BX_THREADS), 0, as_stream(stream), src, dst, H, W);
    return pnnp_launch_status();
}

int pnnp_repair_bad_pixels(void* raw, int elem_size, int H, int W, const int32_t* points, int n, void* tmp, void* stream) {
    if (!raw || (elem_size != 2 && elem_size != 4) || H < 2 || W < 2 || (H & 1) || (W & 1) || n < 0) return PNNP_E_INVALID;
    if ((reinterpret_cast<uintptr_t>(raw) & (uintptr_t)(elem_size - 1)) != 0) return PNNP_E_INVALID;
    if (n == 0) return PNNP_OK;
    if (!points || !tmp || !al4(points) || (reinterpret_cast<uintptr_t>(tmp) & (uintptr_t)(elem_size - 1)) != 0) return PNNP_E_INVALID;
    return elem_size == 2 ? repair_launch<unsigned short>(raw, H, W, points, n, tmp, as_stream(stream))
                          : repair_launch<float>(raw, H, W, points, n, tmp, as_stream(stream));
}

}  // extern "C"

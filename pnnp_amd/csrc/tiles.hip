// A frame as overlapping tiles and back: the two gathers of SynBase_Dataset.eval_crop / eval_merge (data_process/syn_datasets.py:109-159),
// the reference's only inference entry point (trainer_SID.py:345-360 `predict`) and its eval loop's fallback for frames that do not fit (:209-218).
//
//   d = base / 2, l = P - base, nh = H / l + 1, nw = W / l + 1, tile (i, j) = number i * nw + j.
//   crop:  tile row i, local row r reads padded row (i < nh - 1 ? i * l : H - l) + r; padded p is frame row reflect(p - d) (-k -> k, H-1+k -> H-1-k).
//   merge: the interior [d, d + l) of tile row i lands on frame rows (i < nh - 1 ? i * l : H - l) + ry; the reference writes body tiles, then the
//          edge strips, then the corner, so a row y >= H - l belongs to the LAST tile row: a thread stores only where its tile owns the destination.
//          Every frame element therefore has one writer whatever chunk of tiles a launch covers (no read-modify-write).
//   Columns alike.
//
// Both kernels stream.  A workgroup takes 256 / G whole rows of tiles at a time (G: the lanes a row needs), rows are walked with a grid-stride loop
// and every element offset is 64-bit (a frame may pass 2^31 bytes).  A lane moves V = 4 neighbouring columns with 16-byte loads and stores where
// P, base / 2, P - base and W are multiples of 4 and the arrays are 16-byte aligned (then a group of 4 never straddles a reflection or an ownership
// boundary), else V = 1.  The write side is contiguous along the lanes: NCHW rows, and neighbouring float4s of the engines' [P][pitch][Cp] layout.
#include "common.h"

namespace {

__device__ __forceinline__ int reflect_index(int q, int n) { return q < 0 ? -q : (q >= n ? 2 * n - 2 - q : q); }

// the rows a workgroup takes per trip and this lane's place in them: (rows per block, row of the lane [>= rows per block: idle], first group, group step)
struct RowLanes { int rpb, rsub, g0, gstep; };
__device__ __forceinline__ RowLanes row_lanes(int G) {
    RowLanes m;
    m.rpb = G < 256 ? 256 / G : 1;
    m.rsub = m.rpb > 1 ? (int)threadIdx.x / G : 0;
    m.g0 = m.rpb > 1 ? (int)threadIdx.x % G : (int)threadIdx.x;
    m.gstep = m.rpb > 1 ? G : 256;
    return m;
}

// frame [C][H][W] -> tiles t0 .. t0 + nt as NCHW [nt][C][P][P] (the public eval_crop): a lane moves V columns of every channel
template <int V>
__global__ void __launch_bounds__(256)
tile_crop_kernel(const float* __restrict__ frame, float* __restrict__ nchw, int C, int H, int W, int P, int d, int l, int nh, int nw, int t0, int nt,
                 unsigned* __restrict__ amax) {
    float amx = 0.f;                                                  // max |element| (csrc/h2.h)
    const int64_t hw = (int64_t)H * W, pp = (int64_t)P * P;
    const int64_t rows = (int64_t)nt * P;
    const int G = P / V;
    const RowLanes m = row_lanes(G);
    for (int64_t row = (int64_t)blockIdx.x * m.rpb + m.rsub; m.rsub < m.rpb && row < rows; row += (int64_t)gridDim.x * m.rpb) {
        const int k = (int)(row / P), r = (int)(row % P);
        const int t = t0 + k, i = t / nw, j = t % nw;
        const int y = reflect_index((i < nh - 1 ? i * l : H - l) + r - d, H);
        const int c0 = j < nw - 1 ? j * l : W - l;
        const float* src = frame + (int64_t)y * W;
        float* dst = nchw + (int64_t)k * C * pp + (int64_t)r * P;
        for (int g = m.g0; g < G; g += m.gstep) {
            const int c = g * V, q = c0 + c - d;
            if constexpr (V == 4) {
                const bool vec = q >= 0 && q + 3 < W;                 // the whole group inside the frame: one aligned 16-byte load per channel
                const int x0 = reflect_index(q, W), x1 = reflect_index(q + 1, W), x2 = reflect_index(q + 2, W), x3 = reflect_index(q + 3, W);
                for (int ch = 0; ch < C; ++ch) {
                    const float* s = src + ch * hw;
                    const float4 f = vec ? *reinterpret_cast<const float4*>(s + q) : make_float4(s[x0], s[x1], s[x2], s[x3]);
                    *reinterpret_cast<float4*>(dst + ch * pp + c) = f;
                    amx = fmaxf(fmaxf(amx, fmaxf(fabsf(f.x), fabsf(f.y))), fmaxf(fabsf(f.z), fabsf(f.w)));
                }
            } else {
                const int x = reflect_index(q, W);
                for (int ch = 0; ch < C; ++ch) {
                    const float f = src[ch * hw + x];
                    dst[ch * pp + c] = f;
                    amx = fmaxf(amx, fabsf(f));
                }
            }
        }
    }
    if (amax) pnnp_amax_commit_block(amx, amax);
}

// ... as the engines' first-layer input [nt][P][pitch][Cp] (channels >= C zero-filled, Cp % 4 == 0), like nchw_to_nhwc_kernel (csrc/misc.hip): a lane
// gathers four channels of one pixel and stores one float4, neighbouring lanes neighbouring float4s; the NCHW tiles (a `res` network's residual) on the side
__global__ void __launch_bounds__(256)
tile_crop_nhwc_kernel(const float* __restrict__ frame, float* __restrict__ nchw, float* __restrict__ nhwc, int C, int H, int W, int P, int d, int l,
                      int nh, int nw, int t0, int nt, int pitch, int Cp, unsigned* __restrict__ amax) {
    float amx = 0.f;
    const int64_t hw = (int64_t)H * W, pp = (int64_t)P * P;
    const int64_t rows = (int64_t)nt * P;
    const int Q = Cp / 4, G = P * Q;
    const RowLanes m = row_lanes(G);
    for (int64_t row = (int64_t)blockIdx.x * m.rpb + m.rsub; m.rsub < m.rpb && row < rows; row += (int64_t)gridDim.x * m.rpb) {
        const int k = (int)(row / P), r = (int)(row % P);
        const int t = t0 + k, i = t / nw, j = t % nw;
        const int y = reflect_index((i < nh - 1 ? i * l : H - l) + r - d, H);
        const int c0 = j < nw - 1 ? j * l : W - l;
        const float* src = frame + (int64_t)y * W;
        float* o8 = nhwc + ((int64_t)k * P + r) * pitch * Cp;
        for (int g = m.g0; g < G; g += m.gstep) {
            const int c = g / Q, cq = g % Q;
            const int x = reflect_index(c0 + c - d, W);
            float v[4];
#pragma unroll
            for (int qc = 0; qc < 4; ++qc) {
                const int ch = 4 * cq + qc;
                v[qc] = ch < C ? src[ch * hw + x] : 0.f;
                if (nchw && ch < C) nchw[((int64_t)k * C + ch) * pp + (int64_t)r * P + c] = v[qc];
            }
            *reinterpret_cast<float4*>(o8 + (int64_t)c * Cp + 4 * cq) = make_float4(v[0], v[1], v[2], v[3]);
            amx = fmaxf(fmaxf(amx, fmaxf(fabsf(v[0]), fabsf(v[1]))), fmaxf(fabsf(v[2]), fabsf(v[3])));
        }
    }
    if (amax) pnnp_amax_commit_block(amx, amax);
}

// tiles t0 .. t0 + nt as NCHW [nt][C][P][P] -> frame [C][H][W]: every owned interior element, (x ratio, clamp to [0, 1]) on the way
template <int V>
__global__ void __launch_bounds__(256)
tile_merge_kernel(const float* __restrict__ tiles, float* __restrict__ frame, int C, int H, int W, int P, int d, int l, int nh, int nw,
                  int t0, int nt, float ratio_host, const float* __restrict__ ratio_dev, int clamp) {
    const float ratio = ratio_dev ? ratio_dev[0] : ratio_host;
    const int64_t rows = (int64_t)nt * C * l;
    const int G = l / V;
    const RowLanes m = row_lanes(G);
    for (int64_t row = (int64_t)blockIdx.x * m.rpb + m.rsub; m.rsub < m.rpb && row < rows; row += (int64_t)gridDim.x * m.rpb) {
        const int ry = (int)(row % l);
        const int64_t kc = row / l;                                   // k * C + ch
        const int ch = (int)(kc % C), t = t0 + (int)(kc / C), i = t / nw, j = t % nw;
        const int y = (i < nh - 1 ? i * l : H - l) + ry;
        if (i < nh - 1 && y >= H - l) continue;                       // the last tile row owns this frame row
        const int x0 = j < nw - 1 ? j * l : W - l;
        const float* src = tiles + (kc * P + d + ry) * P + d;
        float* dst = frame + ((int64_t)ch * H + y) * W + x0;
        const int lim = j < nw - 1 ? min(l, W - l - x0) : l;          // columns from W - l on belong to the last tile column
        for (int g = m.g0; g * V < lim; g += m.gstep) {
            // (tile * ratio).clamp(0, 1): one rounding for the product, a NaN falls through both selects of pnnp_clampf like torch.clamp
            if constexpr (V == 4) {
                float4 f = *reinterpret_cast<const float4*>(src + 4 * g);
                f.x *= ratio; f.y *= ratio; f.z *= ratio; f.w *= ratio;
                if (clamp) f = make_float4(pnnp_clampf(f.x, 0.f, 1.f), pnnp_clampf(f.y, 0.f, 1.f), pnnp_clampf(f.z, 0.f, 1.f), pnnp_clampf(f.w, 0.f, 1.f));
                *reinterpret_cast<float4*>(dst + 4 * g) = f;
            } else {
                const float v = src[g] * ratio;
                dst[g] = clamp ? pnnp_clampf(v, 0.f, 1.f) : v;
            }
        }
    }
}

// what both entries refuse: the geometry rules of pnnp_amd/tiles.py (TileGrid), a tile range outside the grid
bool tile_args_ok(int C, int H, int W, int P, int base, int t0, int nt) {
    if (C <= 0 || H <= 0 || W <= 0 || P <= 0 || base <= 0 || (base & 1) || base >= P || t0 < 0 || nt < 0) return false;
    const int d = base / 2, l = P - base;
    if (H < l || W < l || d >= H || d >= W) return false;
    const int64_t T = (int64_t)(H / l + 1) * (W / l + 1);
    return T < (1 << 30) && (int64_t)t0 + nt <= T && (int64_t)C * H * W < ((int64_t)1 << 40);
}

// G lanes per row: 256 / G rows per workgroup and trip
int tile_grid_blocks(int64_t rows, int G) {
    const int rpb = G < 256 ? 256 / G : 1;
    const int64_t b = (rows + rpb - 1) / rpb;
    return (int)(b < 1 ? 1 : (b > 256 * 16 ? 256 * 16 : b));
}

// 16-byte lanes: every row start, tile origin, interior and ownership boundary is a multiple of 4 floats
bool tile_vec4(int W, int P, int base, const void* a, const void* b) {
    return !(W & 3) && !(P & 3) && !((base / 2) & 3) && !((P - base) & 3) && !(reinterpret_cast<uintptr_t>(a) & 15) && !(reinterpret_cast<uintptr_t>(b) & 15);
}

}  // namespace

extern "C" {

int pnnp_tile_crop_f32(const float* frame, int C, int H, int W, int P, int base, int t0, int nt, float* nchw, float* nhwc, int pitch, int Cp,
                       unsigned* amax, void* stream) {
    if (!frame || (!nchw && !nhwc) || !tile_args_ok(C, H, W, P, base, t0, nt)) return PNNP_E_INVALID;
    if (nhwc && (Cp < C || (Cp & 3) || pitch < P || (reinterpret_cast<uintptr_t>(nhwc) & 15))) return PNNP_E_INVALID;
    if (nt == 0) return PNNP_OK;
    const int l = P - base;
    const int d = base / 2, nh = H / l + 1, nw = W / l + 1;
    const int64_t rows = (int64_t)nt * P;
    if (nhwc)
        hipLaunchKernelGGL(tile_crop_nhwc_kernel, dim3(tile_grid_blocks(rows, P * (Cp / 4))), dim3(256), 0, as_stream(stream), frame, nchw, nhwc, C, H, W, P,
                           d, l, nh, nw, t0, nt, pitch, Cp, amax);
    else if (tile_vec4(W, P, base, frame, nchw))
        hipLaunchKernelGGL(tile_crop_kernel<4>, dim3(tile_grid_blocks(rows, P / 4)), dim3(256), 0, as_stream(stream), frame, nchw, C, H, W, P, d, l, nh, nw,
                           t0, nt, amax);
    else
        hipLaunchKernelGGL(tile_crop_kernel<1>, dim3(tile_grid_blocks(rows, P)), dim3(256), 0, as_stream(stream), frame, nchw, C, H, W, P, d, l, nh, nw,
                           t0, nt, amax);
    return pnnp_launch_status();
}

int pnnp_tile_merge_f32(const float* tiles, float* frame, int C, int H, int W, int P, int base, int t0, int nt, float ratio, const float* ratio_dev,
                        int clamp, void* stream) {
    if (!tiles || !frame || !tile_args_ok(C, H, W, P, base, t0, nt)) return PNNP_E_INVALID;
    if (nt == 0) return PNNP_OK;
    const int l = P - base;
    if (tile_vec4(W, P, base, tiles, frame))
        hipLaunchKernelGGL(tile_merge_kernel<4>, dim3(tile_grid_blocks((int64_t)nt * C * l, l / 4)), dim3(256), 0, as_stream(stream), tiles, frame, C, H, W, P,
                           base / 2, l, H / l + 1, W / l + 1, t0, nt, ratio, ratio_dev, clamp);
    else
        hipLaunchKernelGGL(tile_merge_kernel<1>, dim3(tile_grid_blocks((int64_t)nt * C * l, l)), dim3(256), 0, as_stream(stream), tiles, frame, C, H, W, P,
                           base / 2, l, H / l + 1, W / l + 1, t0, nt, ratio, ratio_dev, clamp);
    return pnnp_launch_status();
}

}  // extern "C"

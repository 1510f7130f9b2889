// The byte mover the render kernel is measured against (tools/isp_render_bench.py): the grid and the accesses of csrc/isp.hip's vector path --
// per lane four 16-byte non-temporal loads (one per plane of [B][4][H][W]), three dwords stored to [B][H][W][3] bytes and, when asked, three
// 16-byte stores to [B][3][H][W] floats -- with no arithmetic but what keeps the loads alive.  W % 4 == 0, arrays 16-byte aligned.
//   hipcc --offload-arch=gfx950 -O3 -shared -fPIC -o libisp_roof.so isp_roof.hip
#include <hip/hip_runtime.h>
#include <stdint.h>
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
__global__ void __launch_bounds__(256) isp_roof_kernel(const float* __restrict__ in, float* __restrict__ outf, unsigned* __restrict__ out8, int H, int W4) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= H * W4) return;
    const int img = blockIdx.y, y = q / W4, x0 = (q - y * W4) * 4, W = 4 * W4;
    const int64_t plane = (int64_t)H * W, pix = (int64_t)y * W + x0;
    const float* src = in + (int64_t)img * 4 * plane + pix;
    f32x4 v[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = __builtin_nontemporal_load((const f32x4*)(src + c * plane));
    if (out8) {
        unsigned* o = out8 + 3 * (((int64_t)img * plane + pix) >> 2);
        const u32x4 a = __builtin_bit_cast(u32x4, v[0]), b = __builtin_bit_cast(u32x4, v[1]), c = __builtin_bit_cast(u32x4, v[2]), d = __builtin_bit_cast(u32x4, v[3]);
        o[0] = a.x ^ b.y ^ c.z ^ d.w; o[1] = a.y ^ b.z ^ c.w ^ d.x; o[2] = a.z ^ b.w ^ c.x ^ d.y;
    }
    if (outf) {
        float* o = outf + (int64_t)img * 3 * plane + pix;
        *(f32x4*)o = v[0]; *(f32x4*)(o + plane) = v[1] + v[3]; *(f32x4*)(o + 2 * plane) = v[2];
    }
}
extern "C" int isp_roof_launch(const float* in, int B, int H, int W, float* outf, unsigned char* out8, void* stream) {
    if (!in || B < 1 || B > 65535 || H < 1 || W < 4 || W % 4 || (int64_t)H * (W / 4) >= (1ll << 31) - 256) return -1;
    if (((uintptr_t)in | (uintptr_t)outf | (uintptr_t)out8) & 15) return -1;
    const int W4 = W / 4;
    hipLaunchKernelGGL(isp_roof_kernel, dim3((unsigned)(((int64_t)H * W4 + 255) / 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream, in, outf, (unsigned*)out8, H, W4);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

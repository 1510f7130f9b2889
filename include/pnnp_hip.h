/*
 * pnnp_hip.h -- C ABI of libpnnp_hip.so, the MI355X (gfx950) implementation of the
 * PNNP data-parallel hot path.
 *
 * The reference (fenghansen/PNNP) is pure Python: it has no FFI of its own.  Its
 * "operator interface" for this path is a set of Python callables; each entry point
 * below is what a ctypes binding of that callable binds to (INTEGRATION.md shows the
 * reference-side stub).  Citations are file:line under the reference tree.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch types.
 *   - every pointer is a DEVICE pointer owned by the caller unless marked [host].
 *   - `stream` is a hipStream_t passed as void*; kernels are enqueued on it; the
 *     library never synchronises, allocates or frees device memory.
 *   - return value: 0 = ok, negative = error (pnnp_error_string()).
 *   - activations between layers are NHWC fp32 ("pixel-major": [B][H][W][C]);
 *     network input/output at the boundary are NCHW fp32 like the reference's tensors.
 */
#ifndef PNNP_HIP_H
#define PNNP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PNNP_OK 0
#define PNNP_E_INVALID (-1)     /* bad argument (shape, alignment, null)              */
#define PNNP_E_UNSUPPORTED (-2) /* valid request this build has no kernel for          */
#define PNNP_E_LAUNCH (-3)      /* hipLaunchKernel reported an error                   */
#define PNNP_E_WORKSPACE (-4)   /* caller-provided workspace too small                 */

int pnnp_version(void);
const char* pnnp_error_string(int code);
/* ABI version: bumped whenever a struct of this header changes its layout or an entry point its meaning (history: INTEGRATION.md, "Upgrade
 * notes").  A binding written against this header compares pnnp_abi_version() with the PNNP_ABI_VERSION it was compiled / written with and
 * pnnp_pack_job_bytes() with its own sizeof(PnnpPackJob) before it passes a job table (pnnp_amd/ops.py does, on first use).
 *   6 (round 6): PnnpPackJob carries a trailing `amax` pointer since round 5 (an older caller's job ARRAY would be read with the wrong stride);
 *                pnnp_x3_supported refuses more than 1024 output channels (PNNP_E_UNSUPPORTED from the pnnp_conv3x3_x3_* entries beyond it). */
#define PNNP_ABI_VERSION 9
int pnnp_abi_version(void);
int pnnp_pack_job_bytes(void);
/* Number of compute units etc. of the current device (0 on failure). */
int pnnp_device_cus(void);
/* Workgroups per CU of the persistent forward / backward-data convolution kernels (default 1: one per CU with an equal static share of
 * the tiles).  n > 1 launches n per CU with 1/n share each; the surplus waits in the hardware dispatcher and goes to whichever CU frees up
 * first, so a kernel resident on some CUs beside the convolution (an RCCL collective overlapping the backward pass: replaces what
 * nn.DataParallel's reduce did behind autograd, base_trainer.py:115-118) stretches a layer by ~CUs / (CUs - k) instead of doubling it.
 * Process-wide setting, 1 <= n <= 16: the ONE deliberate exception to "no global mutable state"  -- it changes grid sizes, never a
 * result bit (tests/test_gpu_overlap.py), and a per-launch argument would have to thread through every convolution entry point.  Callers
 * scope it: HipTrainStep sets it around the backward pass of a step whose all-reduce overlaps and restores the previous value. */
void pnnp_set_persistent_split(int n);
int pnnp_get_persistent_split(void);

/* ---------------------------------------------------------------- Bayer pack / unpack
 * raw2bayer  utils/isp_ops.py:84-96     u16|f32 [B][H][W] -> f32 [B][4][H/2][W/2]
 *   plane order R,G1,B,G2 = Bayer offsets (0,0),(0,1),(1,1),(1,0).
 *   norm: (x - black[c]) / (wp - black[c]) evaluated in float64 and rounded to
 *   float32 once (numpy promotion of the reference); clip: clamp to [0,1].
 *   black [host] = bias[c] + bl.  Bit-exact with the reference.
 */
int pnnp_pack_bayer_u16(const uint16_t* src, int B, int H, int W, int64_t src_row_stride,
                        int64_t src_batch_stride, float* dst, const double* black4 /*[host]*/,
                        double wp, int norm, int clip, void* stream);
int pnnp_pack_bayer_f32(const float* src, int B, int H, int W, int64_t src_row_stride,
                        int64_t src_batch_stride, float* dst, const double* black4 /*[host]*/,
                        double wp, int norm, int clip, void* stream);
/* pack_raw_bayer  data_process/process.py:40-64: CFA-pattern-aware pack.  pos4 [host] = Bayer offset
 *   (dy<<1|dx) of the R, G1, B, G2 sites; black4 [host] per-channel black level; float32 arithmetic. */
int pnnp_pack_bayer_pattern(const void* src, int is_f32, int B, int H, int W, int64_t src_row_stride,
                            int64_t src_batch_stride, float* dst, const double* black4 /*[host]*/,
                            double wp, int clip, const int* pos4 /*[host]*/, void* stream);
/* bayer2raw  utils/isp_ops.py:98-112    f32 [B][4][h][w] -> u16 [B][2h][2w]
 *   clamp(x,0,1) * (wp-bl) + bl in float32 (two roundings), C-cast truncation.        */
int pnnp_unpack_bayer_u16(const float* src, int B, int h, int w, uint16_t* dst,
                          int wp, int bl, void* stream);
/* bayer2rggb / rggb2bayer  utils/isp_ops.py:57-63 ; bayer2rows / rows2bayer :65-81
 *   pure index moves on elements of `elem_bytes` (2, 4 or 8).                         */
int pnnp_bayer_to_rggb(const void* src, void* dst, int H, int W, int elem_bytes, void* stream);
int pnnp_rggb_to_bayer(const void* src, void* dst, int h, int w, int elem_bytes, void* stream);
int pnnp_bayer_to_rows(const void* src, void* dst, int H, int W, int elem_bytes, void* stream);
int pnnp_rows_to_bayer(const void* src, void* dst, int h, int W, int elem_bytes, void* stream);

/* ---------------------------------------------------------------- noise sampler
 * generate_noisy_obs   data_process/process.py:591-631  (PNNP_NOISE_MODE_OBS)
 * generate_noisy_torch data_process/process.py:634-673  (PNNP_NOISE_MODE_TORCH)
 *   y, out: f32 [B][C][H][W];  params: f32 [B][PNNP_NPARAM] (device), one row per crop.
 *   Counter-based RNG: Philox4x32-10, key = seed, counter = (element, crop_base+b,
 *   draw slot, offset) -- results do not depend on B, grid or GPU count.
 *   Specification of the sampler = oracle/pnnp_oracle.c (pnnp_oracle_noise_sample).
 */
enum {
    PNNP_P_K = 0, PNNP_P_SIGGS, PNNP_P_SIGTL, PNNP_P_LAM, PNNP_P_SIGR, PNNP_P_Q,
    PNNP_P_RATIO, PNNP_P_WP, PNNP_P_BL, PNNP_P_BIAS0, PNNP_P_BIAS1, PNNP_P_BIAS2,
    PNNP_P_BIAS3, PNNP_NPARAM = 16
};
#define PNNP_NOISE_P 0x01u      /* 'p' Poisson shot noise                             */
#define PNNP_NOISE_G 0x02u      /* 'g' Tukey-lambda read noise (else Gaussian)        */
#define PNNP_NOISE_R 0x04u      /* 'r' row noise, one draw per (channel,row)          */
#define PNNP_NOISE_Q 0x08u      /* 'q' quantisation noise                             */
#define PNNP_NOISE_D 0x10u      /* 'd' dark bias per channel                          */
#define PNNP_NOISE_B 0x20u      /* 'b' black frame: no read noise                     */
#define PNNP_NOISE_ORI 0x100u   /* ori=True: do not multiply by ratio                 */
#define PNNP_NOISE_CLIP 0x200u  /* clip=True: clamp to [0,1] instead of [-bl/wp,1]    */
#define PNNP_NOISE_MODE_TORCH 0x1000u /* quirks of generate_noisy_torch (else _obs)   */
#define PNNP_NOISE_POST_MAX1 0x2000u  /* then min(z,1): Trainer.preprocess clamp, trainer_SID.py:481-485 */
#define PNNP_NOISE_POST_MIN0 0x4000u  /* then max(z,0) (clip other than HALF_CLIP)     */
#define PNNP_NOISE_TORCH_TUKEY 0x8000u /* extension: allow 'g' in TORCH mode with the Tukey-lambda
                                          read noise of generate_noisy_obs (process.py:611) instead of the
                                          NotImplementedError of process.py:654 */
int pnnp_noise_sample_f32(const float* y, float* out, int B, int C, int H, int W,
                          const float* params, unsigned flags, float mfm /* sqrt(MultiFrameMean) */,
                          uint64_t seed, uint64_t offset, uint32_t crop_base, void* stream);

/* ---------------------------------------------------------------- denoiser layers (NHWC fp32)
 * What the archs/ modules of the reference do through torch.nn (archs/Unet.py:16-99,
 * archs/ResUnet.py:15-88, archs/modules.py:130-197).  Arithmetic: fp32 operands and fp32
 * accumulation on the matrix cores (v_mfma_f32_32x32x2_f32 == an fmaf chain), so results
 * differ from the reference only by summation order.
 *
 * Weights are consumed in a packed, kernel-friendly order produced on the device from the
 * parameter tensors (which keep the reference's state_dict layout):
 *   Conv2d  [Cout][Cin][k][k] -> fwd   [taps][Cin/4][Cout][4]   (Cin*taps*Cout floats)
 *                             -> dgrad [taps][Cout/4][Cin][4]   (flipped taps)
 *   ConvTranspose2d [Cin][Cout][2][2] -> fwd 4 x [Cin/4][Cout][4], dgrad [(4*Cout)/4][Cin][4]
 * Channel counts must be multiples of 4 (weights, gradients) / 8 (activations read as K).
 */
int pnnp_pack_conv_weight_f32(const float* w, float* fwd /*or null*/, float* dgrad /*or null*/,
                              int Cout, int Cin, int taps, int Cin_pad, int Cout_pad, void* stream);
int pnnp_pack_convt_weight_f32(const float* w, float* fwd /*or null*/, float* dgrad /*or null*/,
                               int Cin, int Cout, void* stream);

/* y = act(conv(cat[x1,x2]) + bias (+ residual)); taps 9 (3x3, pad 1) or 1 (1x1); x2 null when
 * there is no concat (the cat of archs/Unet.py:75,80,85,90 is never materialised).
 * act: 0 none, 1 LeakyReLU(0.2), 2 ReLU. */
int pnnp_conv_fwd_f32(const float* x1, int C1, const float* x2, int C2, const float* w_packed,
                      const float* bias, const float* residual, float* y, int B, int H, int W,
                      int Cout, int taps, int act, void* stream);
/* backward-data: g = dL/d(pre-activation output) -> dx1 (and dx2 for a concat layer).
 * mask_i/mode_i: multiply by the activation derivative of the tensor that produced x_i
 * (mask = that saved activation; mode 1 LeakyReLU', 2 ReLU', 0/null none); accum_i: dx_i +=. */
int pnnp_conv_bwd_data_f32(const float* g, int Cout, const float* w_dgrad,
                           float* dx1, int C1, const float* mask1, int mode1, int accum1,
                           float* dx2, int C2, const float* mask2, int mode2, int accum2,
                           int B, int H, int W, int taps, void* stream);
/* The same two operators for 3x3 / stride 1 / pad 1 layers through Winograd F(2x2,3x3) (2.25x fewer MFMA passes;
 * results differ from the direct form by fp32 rounding of the transforms, ~1e-6 relative).  Weights are packed by
 * pnnp_pack_conv_weight_wino_f32 into U = G g G^T, 16*Cout*Cin floats each; supported when the channels read are a
 * multiple of 8 and the channels written a multiple of 64 (pnnp_wino_supported).
 * Limits (PNNP_E_UNSUPPORTED, nothing is launched): byte offsets inside one image are 32-bit, so H * W * cs * 4 < 2^31 for the widest
 * of the tensors read AND written (cs = channels per pixel of x1, x2 / g and of y / dx1, dx2; mask and addsrc share the destination's
 * geometry), and B * H * W * cs < 2^31 for the tensors read.  Destinations, bias, masks and addsrc are 16-byte aligned and the
 * destinations' channel counts multiples of 4 (PNNP_E_INVALID); dx1 is a multiple of 32 channels when dx2 follows it.
 * Non-finite values: a tile's 4x4 input patch is mixed by the transforms, so one NaN or inf in x (forward) or g (backward-data)
 * makes non-finite every output that the direct form makes non-finite, and at most the outputs -- in every channel -- of the 2x2
 * output tiles (tiles start at even rows and columns) whose 4x4 patch (one pixel of border around the tile) holds that pixel; every
 * other output is unaffected.  Backward-weight: an inf of g gives a bias gradient of inf in its channel as the plain sum does, leaves
 * the other channels' dbias and dW rows finite, and makes that channel's dW row non-finite wherever the direct form is. */
int64_t pnnp_wino_weight_floats(int Cout, int Cin);
int pnnp_wino_supported(int K_read, int N_written);
int pnnp_pack_conv_weight_wino_f32(const float* w, float* fwd /*or null*/, float* dgrad /*or null*/, int Cout, int Cin, void* stream);
int pnnp_conv3x3_wino_fwd_f32(const float* x1, int C1, const float* x2, int C2, const float* u_fwd, const float* bias,
                              const float* residual /*or null*/, float* y, int B, int H, int W, int Cout, int act, void* stream);
int pnnp_conv3x3_wino_bwd_data_res_f32(const float* g, int Cout, const float* u_dgrad, float* dx, int C1,
                                       const float* addsrc, const float* mask, int mode, int B, int H, int W, void* stream);
int pnnp_conv3x3_wino_bwd_data_f32(const float* g, int Cout, const float* u_dgrad,
                                   float* dx1, int C1, const float* mask1, int mode1, int accum1,
                                   float* dx2, int C2, const float* mask2, int mode2, int accum2,
                                   int B, int H, int W, void* stream);
/* ---------------------------------------------------------------- weight re-packing, batched (csrc/pack_jobs.hip)
 * The optimiser moves every weight every step (trainer_SID.py:101), so every layer's packed images are rebuilt every step.  A job
 * is one such rebuild; pnnp_pack_jobs_f32 runs a HOST array of jobs in ceil(n / 32) launches.  The builders append the jobs of one
 * layer (the same ones pnnp_pack_conv_weight_f32 / pnnp_pack_convt_weight_f32 / pnnp_pack_conv_weight_wino_f32 run): build the
 * table once, run it once per step.  kind 0 = strided gather, kind 1 = Winograd filter transform (K = Cout, N = Cin, T = dgrad). */
typedef struct PnnpPackJob {
    const float* src; float* dst;
    int kind, T, K, N;
    int64_t sk, sn, st, off;
    int flip, Kvalid, Ndst, n_off;
    const unsigned* amax;            /* kind 4 (fp16x2 pack): the weight tensor's amax slot */
} PnnpPackJob;
int pnnp_pack_jobs_f32(const PnnpPackJob* jobs /*[host]*/, int n, void* stream);
int pnnp_pack_jobs_add_conv(PnnpPackJob* jobs, int* n, int cap, const float* w, float* fwd /*or null*/, float* dgrad /*or null*/,
                            int Cout, int Cin, int taps, int Cin_pad, int Cout_pad);
int pnnp_pack_jobs_add_convt(PnnpPackJob* jobs, int* n, int cap, const float* w, float* fwd /*or null*/, float* dgrad /*or null*/,
                             int Cin, int Cout);
int pnnp_pack_jobs_add_wino(PnnpPackJob* jobs, int* n, int cap, const float* w, float* fwd /*or null*/, float* dgrad /*or null*/,
                            int Cout, int Cin);
int pnnp_pack_jobs_add_conv3x3s2_dgrad(PnnpPackJob* jobs, int* n, int cap, const float* w, float* dst, int Cout, int Cin);

/* ---- Conv2d 3x3 / stride 1 / pad 1 on the bf16 matrix cores with float32 operands split into three bf16 pieces
 * (csrc/conv_x3s.hip: a = hi + mid + lo exactly, six of the nine piece products kept, fp32 accumulation -- float32-accurate
 * results at 6/16 of the fp32-MFMA time).  Same contracts as pnnp_conv_fwd_f32 / pnnp_conv_bwd_data_f32 /
 * pnnp_conv_bwd_data_res_f32 with taps = 9 (archs/Unet.py:16-52,54-92; archs/modules.py:176-197); the weights are x3 packs:
 * kind-2 jobs of the pack table, pnnp_x3_weight_bytes(K, N) bytes each (K = channels reduced over, N = channels written). */
int pnnp_x3_supported(int K, int N);
/* size limit of the convolution kernels (bf16x3 AND fp32-MFMA families: all address one image through a buffer resource): one
 * image [H][W][cstride] of every map they touch must fit a 32-bit byte offset ((H + 4) W cstride 4 < 2^31); beyond it the launchers
 * return PNNP_E_UNSUPPORTED -- ask first and tile the frame (the Python engines refuse such a frame before launching anything).
 * bf16x3 dynamic range: a piece is a bf16, which has float32's exponent range, so for 2^-110 (7.7e-34) <= |a| <= float32 max all
 * three pieces are normal numbers and hi + mid + lo == a exactly; below that the lo (then mid) piece becomes a bf16 subnormal and
 * may be flushed by the matrix core: accuracy degrades gracefully to 16 (8) significand bits, never to garbage
 * (tests/test_gpu_x3.py::test_x3_dynamic_range, ::test_x3_below_the_supported_range_degrades_gracefully).  Products and sums are
 * float32 and obey float32's own range. */
int pnnp_x3_image_fits(int H, int W, int cstride);
int64_t pnnp_x3_weight_bytes(int K, int N);
int pnnp_pack_jobs_add_x3(PnnpPackJob* jobs, int* n, int cap, const float* w, void* fwd /*or null*/, void* dgrad /*or null*/,
                          int Cout, int Cin, int Cin_pad);
int pnnp_conv3x3_x3_fwd_f32(const float* x1, int C1, const float* x2, int C2, const void* w_x3, const float* bias,
                            const float* residual, float* y, int B, int H, int W, int Cout, int act, void* stream);
/* the same layer with the MaxPool2d(2) behind it (archs/Unet.py:35,41,47,53) fused into its epilogue: y as above, pooled
 * [B][H/2][W/2][Cout] and codes exactly as pnnp_maxpool2_fwd_codes_f32 would produce from y (H, W even). */
int pnnp_conv3x3_x3_fwd_pool_f32(const float* x1, int C1, const float* x2, int C2, const void* w_x3, const float* bias, float* y,
                                 float* pooled, unsigned char* codes, int B, int H, int W, int Cout, int act, void* stream);
int pnnp_conv3x3_x3_bwd_data_f32(const float* g, int Cout, const void* w_x3_dgrad,
                                 float* dx1, int C1, const float* mask1, int mode1, int accum1,
                                 float* dx2 /*or null*/, int C2, const float* mask2, int mode2, int accum2,
                                 int B, int H, int W, void* stream);
int pnnp_conv3x3_x3_bwd_data_res_f32(const float* g, int Cout, const void* w_x3_dgrad, float* dx, int C1,
                                     const float* addsrc, const float* mask, int mode, int B, int H, int W, void* stream);
/* ---- the same layers on the fp16 matrix cores with float32 operands split into TWO scaled fp16 pieces ("h2": csrc/conv_h2s.hip, csrc/h2.h):
 * hi = f16(s a), lo = f16(s a - hi), a b = hi hi' + hi lo' + lo hi' -- three fp16 products per multiply where bf16x3 needs six, fp32
 * accumulation; s = the power of two that brings the TENSOR's largest magnitude into [2^14, 2^15).  That maximum travels in a 4-byte "amax
 * slot" beside every tensor the kernels split: the bit pattern of max |element| (non-negative floats order like unsigned integers), zeroed by
 * the caller once per pass and raised with atomicMax by whichever kernel writes the tensor (amax_y / amax_dx arguments here;
 * pnnp_amax_f32 for a tensor from elsewhere).  A slot may over-estimate (costs range at the small end), never under-estimate.
 * Supported range: every float32 tensor whose elements of interest lie within 2^-18 of its maximum keeps 22 significand bits per operand;
 * smaller elements carry an absolute error of 2^-40 of the maximum (tests/test_gpu_h2.py runs the float64 yardsticks of the bf16x3 family).
 * Sign bits: a forward layer can store (activated output > 0) as one bit per element (bits_y: pnnp_h2_bits_words(B, H, W, Cout) words, a
 * tile-private order that only pnnp_conv3x3_h2_bwd_data_f32 reads back) -- the LeakyReLU' / ReLU' mask of the backward pass at 1/32 of the
 * float32 activation's traffic (archs/Unet.py:52,57-69).  Weights: kind-4 packs of pnnp_h2_weight_bytes(K, N) bytes, scaled with the
 * weight tensor's own slot (pnnp_pack_jobs_add_amax in an earlier launch of the pack table, then pnnp_pack_jobs_add_h2). */
int pnnp_h2_supported(int K, int N);
/* GEMM columns (output channels) per workgroup tile that pnnp_conv3x3_h2_* picks for a [B][H][W] map with N channels written: 64, or 32 when N < 64
 * or 64-column tiles would leave CUs idle (the rule the launcher itself uses).  The 32-column tiles are the HBM-bound instantiations of the
 * 512 x 512 level (bench.py reports them against the HBM roofline).  pool != 0: the forward + MaxPool2d(2) entry. */
int pnnp_h2_tile_columns(int B, int H, int W, int N, int pool);
int64_t pnnp_h2_weight_bytes(int K, int N);
int64_t pnnp_h2_bits_words(int B, int H, int W, int C);
int pnnp_amax_f32(const float* x, int64_t count, unsigned* slot, void* stream);
int pnnp_pack_jobs_add_amax(PnnpPackJob* jobs, int* n, int cap, const float* x, int64_t count, unsigned* slot);
int pnnp_pack_jobs_add_h2(PnnpPackJob* jobs, int* n, int cap, const float* w, void* fwd /*or null*/, void* dgrad /*or null*/,
                          int Cout, int Cin, int Cin_pad, const unsigned* amax_w);
int pnnp_conv3x3_h2_fwd_f32(const float* x1, int C1, const unsigned* amax_x1, const float* x2 /*or null*/, int C2, const unsigned* amax_x2,
                            const void* w_h2, const unsigned* amax_w, const float* bias, const float* residual, float* y,
                            unsigned* amax_y /*or null*/, unsigned* bits_y /*or null*/, int B, int H, int W, int Cout, int act, void* stream);
/* Split-K for small grids (round 6; an eval forward on ONE 512 x 512 crop gives the deep layers 16-32 output tiles for 256 CUs): pnnp_h2_splitk returns the
 * number of K slices for a layer with `chunks` = segments x ceil(C / 16) chunks of K (1 = launch as usual); with ksplit > 1 the kernel writes raw partial
 * sums into ws ([ksplit][B][H][W][Cout] floats) and a reduce kernel adds them in a fixed order (deterministic), then bias, activation, amax_y and the sign
 * bits exactly as pnnp_conv3x3_h2_fwd_f32 would have.  Another partition of the K sum: results differ from the unsplit launch by float32 rounding only.
 * With ksplit > 1 the reduce kernel reads the slabs and the bias and writes y as float4: y, bias and ws must be 16-byte aligned and amax_y 4-byte aligned, else
 * PNNP_E_INVALID and nothing is launched (the rule of the _h1_ twin below; until the two entries shared one body this entry did not check it). */
int pnnp_h2_splitk(int B, int H, int W, int chunks, int N);
int pnnp_conv3x3_h2_fwd_splitk_f32(const float* x1, int C1, const unsigned* amax_x1, const float* x2 /*or null*/, int C2, const unsigned* amax_x2,
                                   const void* w_h2, const unsigned* amax_w, const float* bias, float* y, unsigned* amax_y, unsigned* bits_y,
                                   int B, int H, int W, int Cout, int act, int ksplit, float* ws, int64_t ws_floats, void* stream);
/* The last 3x3 layer + LeakyReLU + the 1x1 head conv10_1 (archs/Unet.py:93-94; ResUnet: archs/ResUnet.py conv_out) in ONE kernel (round 6): Cout == 32
 * (one workgroup tile holds every channel of a pixel), head_w [4][32] / head_b [4] are the parameters as they are, head_out NCHW [B][4][H][W] float32
 * (+ head_res, NCHW like head_out: the `res` networks' input, or null).  y (the 32-channel map, with amax_y / bits_y as in pnnp_conv3x3_h2_fwd_f32) may be
 * NULL: an eval forward neither writes nor re-reads it; a training forward passes it (backward needs it: pnnp_head_bwd_f32).  The head's sums run in
 * float32 on the vector ALUs over the ACTIVATED float32 accumulators (the same arithmetic as pnnp_head_fwd_f32, another summation order). */
int pnnp_conv3x3_h2_fwd_head_f32(const float* x1, int C1, const unsigned* amax_x1, const float* x2 /*or null*/, int C2, const unsigned* amax_x2,
                                 const void* w_h2, const unsigned* amax_w, const float* bias, float* y /*or null*/, unsigned* amax_y, unsigned* bits_y,
                                 const float* head_w, const float* head_b /*or null*/, const float* head_res /*or null*/, float* head_out,
                                 int B, int H, int W, int Cout, int act, void* stream);
int pnnp_conv3x3_h2_fwd_pool_f32(const float* x1, int C1, const unsigned* amax_x1, const float* x2 /*or null*/, int C2, const unsigned* amax_x2,
                                 const void* w_h2, const unsigned* amax_w, const float* bias, float* y, float* pooled, unsigned char* codes,
                                 unsigned* amax_y /*or null*/, unsigned* bits_y /*or null*/, int B, int H, int W, int Cout, int act, void* stream);
/* ---- the fp16x1 ("h1") family: the same stride-1 3x3 FORWARD layers with ONE scaled fp16 piece per float32 operand (csrc/conv_h1s.hip): hi = f16(a 2^se),
 * se from the tensor's amax slot as above; one fp16 rounding per operand (relative 2^-11), products exact, float32 accumulation -- outputs at about 1e-3
 * relative to the activations' scale.  EVAL FORWARD ONLY and opt-in (ConvPolicy.h1_eval): no sign bits, no backward entries; five matrix instructions per
 * chunk and block where the fp16x2 kernel issues fourteen.  Each entry has the argument list of its h2 twin minus bits_y, the same tile rule
 * (pnnp_h2_tile_columns), split-K policy (pnnp_h2_splitk) and amax contract.  Weights: kind-7 packs of pnnp_h1_weight_bytes(K, N) bytes
 * ([N/32][K16][tap 10][octet 2][32][8] fp16, the tenth tap and the padded K rows zero), scaled with the weight tensor's slot like the h2 pack.  Every pointer
 * the kernels touch with vector accesses must be 16-byte aligned (x1, x2, w_h1, bias, residual, y, pooled, ws), slots and head tensors 4-byte: PNNP_E_INVALID /
 * PNNP_E_UNSUPPORTED otherwise, nothing launched. */
int pnnp_h1_supported(int K, int N);
int64_t pnnp_h1_weight_bytes(int K, int N);
int pnnp_pack_jobs_add_h1(PnnpPackJob* jobs, int* n, int cap, const float* w, void* fwd, int Cout, int Cin, int Cin_pad, const unsigned* amax_w);
int pnnp_conv3x3_h1_fwd_f32(const float* x1, int C1, const unsigned* amax_x1, const float* x2 /*or null*/, int C2, const unsigned* amax_x2,
                            const void* w_h1, const unsigned* amax_w, const float* bias, const float* residual, float* y,
                            unsigned* amax_y /*or null*/, int B, int H, int W, int Cout, int act, void* stream);
int pnnp_conv3x3_h1_fwd_splitk_f32(const float* x1, int C1, const unsigned* amax_x1, const float* x2 /*or null*/, int C2, const unsigned* amax_x2,
                                   const void* w_h1, const unsigned* amax_w, const float* bias, float* y, unsigned* amax_y,
                                   int B, int H, int W, int Cout, int act, int ksplit, float* ws, int64_t ws_floats, void* stream);
int pnnp_conv3x3_h1_fwd_head_f32(const float* x1, int C1, const unsigned* amax_x1, const float* x2 /*or null*/, int C2, const unsigned* amax_x2,
                                 const void* w_h1, const unsigned* amax_w, const float* bias, float* y /*or null*/, unsigned* amax_y,
                                 const float* head_w, const float* head_b /*or null*/, const float* head_res /*or null*/, float* head_out,
                                 int B, int H, int W, int Cout, int act, void* stream);
int pnnp_conv3x3_h1_fwd_pool_f32(const float* x1, int C1, const unsigned* amax_x1, const float* x2 /*or null*/, int C2, const unsigned* amax_x2,
                                 const void* w_h1, const unsigned* amax_w, const float* bias, float* y, float* pooled, unsigned char* codes,
                                 unsigned* amax_y /*or null*/, int B, int H, int W, int Cout, int act, void* stream);
/* ---- ... with fp16 ACTIVATIONS ("h1a", csrc/conv_h1s.hip H1a): each entry is its _f32 twin above with an element type per side.
 *   src_f16 != 0: x1 / x2 are fp16 NHWC tensors (both: a float32 segment beside an fp16 one cannot be asked for).  Their halves are the matrix operands as they
 *     are -- unscaled (se_x = 0), subnormals kept; the amax slots of x1 / x2 are not read and may be null.  Fed x16 where the _f32 twin is fed float(x16) the
 *     outputs agree bit for bit whenever max |x16| < 2^15 (the twin's scaled rounding is then exact).  C1 in multiples of 8; 16-byte aligned.
 *   dst_f16 != 0: y (and the pooled map) are fp16: float16(v) of the float32 value v the _f32 twin stores -- ONE round to nearest even, unscaled, subnormals kept,
 *     NOT saturated (|v| > 65504 becomes inf; NaN stays NaN).  amax_y still records max |v| BEFORE the rounding.  Codes are the twin's.
 *   One image of a map must stay below 2 GB in ITS element size (pnnp_image_fits_es).  No residual; the split-K slabs (ws) stay float32; the head entry stores
 *   nothing but head_out (float32 NCHW); the pool entry takes fp16 on both sides.  Everything else: PNNP_E_UNSUPPORTED /
 *   PNNP_E_INVALID as for the twins, nothing launched, outputs untouched.  src_f16 = dst_f16 = 0: the twin itself. */
int pnnp_image_fits_es(int H, int W, int cstride, int elem_bytes /*2 or 4*/);
/* MaxPool2d(2) of an fp16 NHWC map (a pooled layer that ran split-K has no pool in its epilogue): H, W even, C in multiples of 8, 16-byte aligned */
int pnnp_maxpool2_fwd_f16(const void* x, void* y, int B, int H, int W, int C, void* stream);
int pnnp_conv3x3_h1_fwd_et(const void* x1, int C1, const unsigned* amax_x1, const void* x2 /*or null*/, int C2, const unsigned* amax_x2, const void* w_h1,
                           const unsigned* amax_w, const float* bias, void* y, unsigned* amax_y /*or null*/, int src_f16, int dst_f16,
                           int B, int H, int W, int Cout, int act, void* stream);
int pnnp_conv3x3_h1_fwd_splitk_et(const void* x1, int C1, const unsigned* amax_x1, const void* x2 /*or null*/, int C2, const unsigned* amax_x2, const void* w_h1,
                                  const unsigned* amax_w, const float* bias, void* y, unsigned* amax_y, int src_f16, int dst_f16,
                                  int B, int H, int W, int Cout, int act, int ksplit, float* ws, int64_t ws_floats, void* stream);
int pnnp_conv3x3_h1_fwd_head_et(const void* x1, int C1, const unsigned* amax_x1, const void* x2 /*or null*/, int C2, const unsigned* amax_x2, const void* w_h1,
                                const unsigned* amax_w, const float* bias, const float* head_w, const float* head_b /*or null*/, const float* head_res /*or null*/,
                                float* head_out, int src_f16, int B, int H, int W, int Cout, int act, void* stream);
int pnnp_conv3x3_h1_fwd_pool_et(const void* x1, int C1, const unsigned* amax_x1, const void* x2 /*or null*/, int C2, const unsigned* amax_x2, const void* w_h1,
                                const unsigned* amax_w, const float* bias, void* y, void* pooled, unsigned char* codes, unsigned* amax_y /*or null*/,
                                int src_f16, int dst_f16, int B, int H, int W, int Cout, int act, void* stream);
/* ConvTranspose2d(k2, s2) in the same sense (pnnp_convt_h1_fwd_f32's contract, kind-8 pack): x and y both fp16 (1, 1) or the twin (0, 0); a mixed pair is
 * PNNP_E_UNSUPPORTED.  One image of x / y must stay below 2 GB in 2-byte elements. */
int pnnp_convt_h1_fwd_et(const void* x, int Cin, const unsigned* amax_x /*or null for fp16*/, const void* w_h1, const unsigned* amax_w, const float* bias /*or null*/,
                         void* y, unsigned* amax_y /*or null*/, int src_f16, int dst_f16, int B, int H, int W, int Cout, void* stream);
/* ---- ... and the layers only ResUnet has, with fp16 on EVERY side (ConvPolicy.h1_act16_res; the same storage contract):
 *   pnnp_conv3x3_h1_fwd_res_et: pnnp_conv3x3_h1_fwd_f32 with a residual: y16 = float16((acc 2^dexp + bias) + float(r16)), the sum made in float32 in that order
 *     and rounded ONCE; amax_y records the float32 sum.  residual: an fp16 NHWC tensor with y's geometry.  Offered for src_f16 = res_f16 = dst_f16 = 1 (and
 *     all three 0: the _f32 twin); any other triple, or act != 0: PNNP_E_UNSUPPORTED.  A null residual: PNNP_E_INVALID.
 *   pnnp_conv_s2_h1_fwd_et / pnnp_conv1x1_h1_fwd_et: the stride-2 3x3 layer and the 1x1 layer on cat([x1, x2]) (kind-8 packs) with x and y both fp16 (1, 1) or
 *     the twin (0, 0); a mixed pair is PNNP_E_UNSUPPORTED.  An fp16 source has no amax slot (null allowed).  The fp16 1x1 layer takes no residual (PNNP_E_UNSUPPORTED).  Channel
 *     strides in multiples of 8; one image of a map below 2 GB in 2-byte elements. */
int pnnp_conv3x3_h1_fwd_res_et(const void* x1, int C1, const unsigned* amax_x1, const void* x2 /*or null*/, int C2, const unsigned* amax_x2, const void* w_h1,
                               const unsigned* amax_w, const float* bias /*or null*/, const void* residual, void* y, unsigned* amax_y /*or null*/,
                               int src_f16, int res_f16, int dst_f16, int B, int H, int W, int Cout, int act, void* stream);
int pnnp_conv_s2_h1_fwd_et(const void* x, int Cin, const unsigned* amax_x /*or null for fp16*/, const void* w_h1, const unsigned* amax_w, const float* bias /*or null*/,
                           void* y, unsigned* amax_y /*or null*/, int src_f16, int dst_f16, int B, int H, int W, int Cout, int act, void* stream);
int pnnp_conv1x1_h1_fwd_et(const void* x1, int C1, const unsigned* amax_x1, const void* x2 /*or null*/, int C2, const unsigned* amax_x2, const void* w_h1,
                           const unsigned* amax_w, const float* bias /*or null*/, const float* residual /*null with fp16*/, void* y, unsigned* amax_y /*or null*/,
                           int src_f16, int dst_f16, int B, int H, int W, int Cout, int act, void* stream);
int pnnp_conv3x3_h2_bwd_data_f32(const float* g, int Cout, const unsigned* amax_g, const void* w_h2_dgrad, const unsigned* amax_w,
                                 float* dx1, int C1, const float* mask1, const unsigned* bits1, int mode1, int accum1, unsigned* amax_dx1,
                                 float* dx2 /*or null*/, int C2, const float* mask2, const unsigned* bits2, int mode2, int accum2, unsigned* amax_dx2,
                                 int B, int H, int W, void* stream);
/* A COLUMN RANGE of that layer into one destination, optionally with the backward pass of MaxPool2d(2) folded into the store (round 7).  The backward-data pack
 * is column-block-major, so columns [col0, col0 + C) of a pack with `cols` columns (both multiples of 32, the range inside the pack: else PNNP_E_INVALID) are
 * the same kernel on an offset pack pointer: dx [B][H][W][C] = act'(bits) x dgrad (bits null: no mask; accum as above).  A two-destination launch of
 * pnnp_conv3x3_h2_bwd_data_f32 equals the two launches over [0, C1) and [C1, C1 + C2) bit for bit (same tiles, same sums).
 * gp / codes given: dx is ALSO the input of a MaxPool2d(2) (archs/Unet.py: conv1_2 .. conv4_2, skip connection + pool); gp [B][H/2][W/2][gp_cs] is the pooled
 * map's gradient (its first C channels are used; gp_cs >= C, a multiple of 4; 16-byte aligned), codes the bytes pnnp_maxpool2_fwd_codes_f32 /
 * pnnp_conv3x3_h2_fwd_pool_f32 wrote (4-byte aligned, same geometry).  The kernel stores  act'(bits) x dgrad + unpool(gp, codes)  and raises amax_dx with
 * max |stored value|.  BIT-EXACTNESS CONTRACT: dx and amax_dx are bit-identical to this entry without gp / codes followed by
 * pnnp_maxpool2_bwd_codes_amax_f32(codes, gp, dx, B, H, W, C, mode, 1, amax_dx') -- the same float32 operations in the same order (t + ((k == argmax) ?
 * g x (sign_k ? 1 : slope) : 0), the addition also where the term is zero), amax_dx == amax_dx' -- without the pass's read-modify-write of the full-resolution
 * map.  Requires bits and mode != 0, accum == 0, even H and W; anything else returns PNNP_E_UNSUPPORTED and launches nothing. */
int pnnp_conv3x3_h2_bwd_data_unpool_f32(const float* g, int Cout, const unsigned* amax_g, const void* w_h2_dgrad, const unsigned* amax_w, int col0, int cols,
                                        float* dx, int C, const unsigned* bits /*or null*/, int mode, int accum, unsigned* amax_dx /*or null*/,
                                        const float* gp /*or null*/, int gp_cs, const unsigned char* codes /*or null*/, int B, int H, int W, void* stream);
/* backward-weight: both operands are split on the fly; same workspace (pnnp_x3_wgrad_workspace_floats), supported shapes
 * (pnnp_x3_wgrad_supported, pnnp_x3_wgrad_fits) and contract as pnnp_conv3x3_x3_bwd_weight_f32 */
int pnnp_conv3x3_h2_bwd_weight_f32(const float* g, int g_cs, int Cout, const unsigned* amax_g, const float* x1, int x1_cs, int C1, const unsigned* amax_x1,
                                   const float* x2 /*or null*/, int x2_cs, int C2, const unsigned* amax_x2, float* dW, float* dbias /*or null*/,
                                   int B, int H, int W, int accumulate, float* workspace, int64_t workspace_floats, void* stream);
int pnnp_conv3x3_h2_bwd_data_res_f32(const float* g, int Cout, const unsigned* amax_g, const void* w_h2_dgrad, const unsigned* amax_w,
                                     float* dx, int C1, const float* addsrc, const float* mask, int mode, unsigned* amax_dx,
                                     int B, int H, int W, void* stream);
/* The same pointwise layers on the fp16 matrix cores (csrc/gemm_s.h on the scheme of csrc/gemm_h2s.hip; round 5): the fp16x2 scheme of the 3x3 kernels (csrc/h2.h) -- per-tensor
 * power-of-two scale from 4-byte amax slots, two fp16 pieces per operand, three products per multiply instead of bf16x3's six.  Contracts of the
 * _x3_ entries below + the slots: amax_x / amax_g of the tensor that is split on the fly, amax_w of the weight tensor (the kind-6 packs of
 * pnnp_pack_jobs_add_h2_convt / _1x1 / _s2 were scaled with it; pnnp_h2mat_bytes(K, N) bytes), amax_y / amax_dx (or null) raised to max |stored|.
 * K (channels per segment) % 32 == 0, N (GEMM columns: 4 Cout for ConvTranspose2d forward) % 32 == 0 (round 6; was 64): pnnp_gemm_h2_supported. */
int pnnp_gemm_h2_supported(int K, int N);
int64_t pnnp_h2mat_bytes(int K, int N);
int pnnp_pack_jobs_add_h2_convt(PnnpPackJob* jobs, int* n, int cap, const float* w, void* fwd /*or null*/, void* dgrad /*or null*/, int Cin, int Cout, const unsigned* amax);
int pnnp_pack_jobs_add_h2_1x1(PnnpPackJob* jobs, int* n, int cap, const float* w, void* fwd /*or null*/, void* dgrad /*or null*/, int Cout, int Cin, const unsigned* amax);
int pnnp_pack_jobs_add_h2_s2(PnnpPackJob* jobs, int* n, int cap, const float* w, void* fwd /*or null*/, void* dgrad /*or null: 9 x pnnp_h2mat_bytes(Cout, Cin)*/, int Cout, int Cin, const unsigned* amax);
int pnnp_conv3x3s2_h2_fwd_f32(const float* x, int Cin, const unsigned* amax_x, const void* w_h2, const unsigned* amax_w, const float* bias /*or null*/, float* y,
                              unsigned* amax_y /*or null*/, int B, int H, int W, int Cout, int act, void* stream);
int pnnp_conv3x3s2_h2_bwd_data_f32(const float* g, int Cout, const unsigned* amax_g, const void* w_h2_s2dgrad, const unsigned* amax_w, float* dx, int Cin,
                                   const float* mask /*or null*/, int mode, int accum, unsigned* amax_dx /*or null*/, int B, int H, int W, void* stream);
/* ... and their backward-weights (csrc/wgrad_h2g.hip: the kernel of csrc/wgrad_g.h on this scheme): contracts of the _x3_ entries + the amax slots of the two tensors that are split; shapes and
 * workspace: pnnp_h2g_wgrad_supported / _workspace_floats (kind as pnnp_x3g_wgrad_supported: everything it takes, and stride-2 with Cout % 64 == 0) */
int pnnp_h2g_wgrad_supported(int kind, int M, int N);
int64_t pnnp_h2g_wgrad_workspace_floats(int kind, int B, int UH, int UW, int M, int N);
int pnnp_convt2x2_h2_bwd_weight_f32(const float* x, int Cin, const unsigned* amax_x, const float* g, int Cout, const unsigned* amax_g, float* dW, float* dbias /*or null*/,
                                    int B, int H, int W, int accumulate, float* workspace, int64_t workspace_floats, void* stream);
int pnnp_conv3x3s2_h2_bwd_weight_f32(const float* g, int Cout, const unsigned* amax_g, const float* x, int Cin, const unsigned* amax_x, float* dW, float* dbias /*or null*/,
                                     int B, int H, int W, int accumulate, float* workspace, int64_t workspace_floats, void* stream);
int pnnp_conv1x1_h2_bwd_weight_f32(const float* g, int g_cs, int Cout, const unsigned* amax_g, const float* x1, int x1_cs, int C1, const unsigned* amax_x1,
                                   const float* x2 /*or null*/, int x2_cs, int C2, const unsigned* amax_x2, float* dW, float* dbias /*or null*/,
                                   int B, int H, int W, int accumulate, float* workspace, int64_t workspace_floats, void* stream);
int pnnp_convt2x2_h2_fwd_f32(const float* x, int Cin, const unsigned* amax_x, const void* w_h2, const unsigned* amax_w, const float* bias /*or null*/, float* y,
                             unsigned* amax_y /*or null*/, int B, int H, int W, int Cout, void* stream);
int pnnp_convt2x2_h2_bwd_data_f32(const float* g, int Cout, const unsigned* amax_g, const void* w_h2_dgrad, const unsigned* amax_w, float* dx, int Cin,
                                  const float* mask /*or null*/, int mode, unsigned* amax_dx /*or null*/, int B, int H, int W, void* stream);
/* ... with the act' mask as the SIGN BITS pnnp_conv3x3_h2_fwd_f32 / _fwd_pool_f32 stored for the layer's input map (round 6: the float32 activation is not read:
 * 503 MB per UNet step); bits: pnnp_h2_bits_words(B, H, W, Cin) words, Cin % 32 == 0, mode 1 LeakyReLU(0.2)' / 2 ReLU'.  Bit-identical to the float32-mask entry. */
int pnnp_convt2x2_h2_bwd_data_bits_f32(const float* g, int Cout, const unsigned* amax_g, const void* w_h2_dgrad, const unsigned* amax_w, float* dx, int Cin,
                                       const unsigned* bits, int mode, unsigned* amax_dx, int B, int H, int W, void* stream);
int pnnp_conv1x1_h2_fwd_f32(const float* x1, int C1, const unsigned* amax_x1, const float* x2 /*or null*/, int C2, const unsigned* amax_x2, const void* w_h2,
                            const unsigned* amax_w, const float* bias /*or null*/, const float* residual /*or null*/, float* y, unsigned* amax_y /*or null*/,
                            int B, int H, int W, int Cout, int act, void* stream);
int pnnp_conv1x1_h2_bwd_data_f32(const float* g, int Cout, const unsigned* amax_g, const void* w_h2_dgrad, const unsigned* amax_w,
                                 float* dx1, int C1, const float* mask1, int mode1, int accum1, unsigned* amax_dx1 /*or null*/,
                                 float* dx2 /*or null*/, int C2, const float* mask2, int mode2, int accum2, int B, int H, int W, void* stream);
/* ---- the fp16x1 ("h1") pointwise layers: the three FORWARD entries above with ONE scaled fp16 piece per float32 operand (csrc/gemm_s.h on the scheme of
 * csrc/gemm_h1s.hip): one matrix instruction per 32 channels and 16 x 16 block where fp16x2 issues three; error as for pnnp_conv3x3_h1_fwd_f32 (one fp16 rounding
 * per operand, float32 accumulation).  EVAL FORWARD ONLY and opt-in (ConvPolicy.h1_pointwise): no backward entries; the launcher answers PNNP_E_UNSUPPORTED to
 * masks, bit images, accumulating or second destinations.  Argument lists, amax contract and tile set of the _h2_ twins; shapes: pnnp_h1_pointwise_supported
 * (= pnnp_gemm_h2_supported: K % 32 == 0, N % 32 == 0).  Weights: kind-8 packs of pnnp_h1_pointwise_weight_bytes(K, N) = 2 K N bytes with the forward GEMM's
 * K and N (ConvTranspose2d: Cin, 4 Cout; 1x1: C1 + C2, Cout; stride 2: 9 Cin, Cout) -- the kind-6 layout [N/32][K/32][octet 4][32][8] fp16 without its lo'
 * plane, hi' = f16(w 2^se) with the weight tensor's amax slot; zero-fill the buffer first, as for the h2 packs.  Every tensor pointer 16-byte aligned, slots
 * 4-byte: PNNP_E_INVALID otherwise. */
int pnnp_h1_pointwise_supported(int K, int N);
int64_t pnnp_h1_pointwise_weight_bytes(int K, int N);
int pnnp_pack_jobs_add_h1_convt(PnnpPackJob* jobs, int* n, int cap, const float* w, void* fwd, int Cin, int Cout, const unsigned* amax);
int pnnp_pack_jobs_add_h1_1x1(PnnpPackJob* jobs, int* n, int cap, const float* w, void* fwd, int Cout, int Cin, const unsigned* amax);
int pnnp_pack_jobs_add_h1_s2(PnnpPackJob* jobs, int* n, int cap, const float* w, void* fwd, int Cout, int Cin, const unsigned* amax);
int pnnp_convt_h1_fwd_f32(const float* x, int Cin, const unsigned* amax_x, const void* w_h1, const unsigned* amax_w, const float* bias /*or null*/, float* y,
                          unsigned* amax_y /*or null*/, int B, int H, int W, int Cout, void* stream);
int pnnp_conv1x1_h1_fwd_f32(const float* x1, int C1, const unsigned* amax_x1, const float* x2 /*or null*/, int C2, const unsigned* amax_x2, const void* w_h1,
                            const unsigned* amax_w, const float* bias /*or null*/, const float* residual /*or null*/, float* y, unsigned* amax_y /*or null*/,
                            int B, int H, int W, int Cout, int act, void* stream);
int pnnp_conv_s2_h1_fwd_f32(const float* x, int Cin, const unsigned* amax_x, const void* w_h1, const unsigned* amax_w, const float* bias /*or null*/, float* y,
                            unsigned* amax_y /*or null*/, int B, int H, int W, int Cout, int act, void* stream);
/* pointwise layers on the bf16 matrix cores (csrc/gemm_x3.hip): ConvTranspose2d k2 s2 (archs/Unet.py:35-47), Conv2d 1x1 (ResidualBlock
 * shortcuts, archs/modules.py:176-197), Conv2d 3x3 stride 2 (archs/modules.py:130-138); same contracts as pnnp_convt2x2_* /
 * pnnp_conv_fwd_f32 + pnnp_conv_bwd_data_f32 with taps = 1 / pnnp_conv3x3s2_*; channel counts in multiples of 32; the weights are
 * kind-3 packs of pnnp_x3mat_bytes(K, N) bytes (stride-2 backward-data: 9 x pnnp_x3mat_bytes(Cout, Cin)). */
int pnnp_gemm_x3_supported(int K, int N);
int64_t pnnp_x3mat_bytes(int K, int N);
int pnnp_pack_jobs_add_x3_convt(PnnpPackJob* jobs, int* n, int cap, const float* w, void* fwd /*or null*/, void* dgrad /*or null*/, int Cin, int Cout);
int pnnp_pack_jobs_add_x3_1x1(PnnpPackJob* jobs, int* n, int cap, const float* w, void* fwd /*or null*/, void* dgrad /*or null*/, int Cout, int Cin);
int pnnp_pack_jobs_add_x3_s2(PnnpPackJob* jobs, int* n, int cap, const float* w, void* fwd /*or null*/, void* dgrad /*or null*/, int Cout, int Cin);
int pnnp_convt2x2_x3_fwd_f32(const float* x, int Cin, const void* w_x3, const float* bias, float* y, int B, int H, int W, int Cout, void* stream);
int pnnp_convt2x2_x3_bwd_data_f32(const float* g, int Cout, const void* w_x3_dgrad, float* dx, int Cin, const float* mask, int mode,
                                  int B, int H, int W, void* stream);
/* ... the same two with max |output| raised into an amax slot of the fp16x2 family (see pnnp_conv3x3_h2_fwd_f32) */
int pnnp_convt2x2_x3_fwd_amax_f32(const float* x, int Cin, const void* w_x3, const float* bias, float* y, unsigned* amax_y /*or null*/,
                                  int B, int H, int W, int Cout, void* stream);
int pnnp_convt2x2_x3_bwd_data_amax_f32(const float* g, int Cout, const void* w_x3_dgrad, float* dx, int Cin, const float* mask, int mode,
                                       unsigned* amax_dx /*or null*/, int B, int H, int W, void* stream);
int pnnp_conv1x1_x3_fwd_f32(const float* x1, int C1, const float* x2 /*or null*/, int C2, const void* w_x3, const float* bias, const float* residual,
                            float* y, int B, int H, int W, int Cout, int act, void* stream);
int pnnp_conv1x1_x3_bwd_data_f32(const float* g, int Cout, const void* w_x3_dgrad, float* dx1, int C1, const float* mask1, int mode1, int accum1,
                                 float* dx2 /*or null*/, int C2, const float* mask2, int mode2, int accum2, int B, int H, int W, void* stream);
int pnnp_conv3x3s2_x3_fwd_f32(const float* x, int Cin, const void* w_x3, const float* bias, float* y, int B, int H, int W, int Cout, int act, void* stream);
int pnnp_conv3x3s2_x3_bwd_data_f32(const float* g, int Cout, const void* w_x3_s2dgrad, float* dx, int Cin, const float* mask, int mode, int accum,
                                   int B, int H, int W, void* stream);
int pnnp_conv3x3s2_x3_fwd_amax_f32(const float* x, int Cin, const void* w_x3, const float* bias, float* y, unsigned* amax_y /*or null*/,
                                   int B, int H, int W, int Cout, int act, void* stream);
int pnnp_conv3x3s2_x3_bwd_data_amax_f32(const float* g, int Cout, const void* w_x3_s2dgrad, float* dx, int Cin, const float* mask, int mode, int accum,
                                        unsigned* amax_dx /*or null*/, int B, int H, int W, void* stream);
/* backward-weight of the same layers (csrc/wgrad_x3.hip; pixel-major LDS images read with ds_read_b64_tr_b16): same contract
 * as pnnp_conv_bwd_weight_f32 with taps = 9; channel counts in multiples of 32; workspace from the query.  A layer with 9 Cout Cin >= 2^31
 * (8 GB per slab: no workspace holds it) is PNNP_E_UNSUPPORTED: the kernel indexes one slab with 32 bits. */
int pnnp_x3_wgrad_supported(int H, int W, int Cout, int C1, int C2);
/* its size limit: the WHOLE batch of a map [B][H][W][cstride] must fit a 32-bit byte offset ((B H + 2) W cstride 4 < 2^31) */
int pnnp_x3_wgrad_fits(int B, int H, int W, int cstride);
int64_t pnnp_x3_wgrad_workspace_floats(int B, int H, int W, int Cout, int Cin);
int pnnp_conv3x3_x3_bwd_weight_f32(const float* g, int g_cs, int Cout, const float* x1, int x1_cs, int C1,
                                   const float* x2 /*or null*/, int x2_cs, int C2, float* dW, float* dbias /*or null*/,
                                   int B, int H, int W, int accumulate, float* workspace, int64_t workspace_floats, void* stream);

/* backward-weight of the POINTWISE / STRIDED layers on the same scheme (csrc/wgrad_x3g.hip; geometries, tiles, staging layout: csrc/wgrad_g.h; round 4; they ran on the fp32 matrix cores
 * before): kind 0 = Conv2d 1x1 (M = Cout, N = C1 + C2; replaces pnnp_conv_bwd_weight_f32 with taps = 1, archs/modules.py:184-187),
 * 1 = ConvTranspose2d 2x2 stride 2 (M = Cin, N = Cout; replaces pnnp_convt2x2_bwd_weight_f32, archs/Unet.py:35-47),
 * 2 = Conv2d 3x3 stride 2 (M = Cout, N = Cin; replaces pnnp_conv3x3s2_bwd_weight_f32, archs/ResUnet.py:18-27).  Same contracts as
 * the entries they replace; `supported` says whether (M, N) has a tile configuration (otherwise use the fp32 entry); the workspace
 * query takes the LOW-resolution map (the layer input of the ConvTranspose2d, the output of the stride-2 convolution). */
int pnnp_x3g_wgrad_supported(int kind, int M, int N);
int64_t pnnp_x3g_wgrad_workspace_floats(int kind, int B, int UH, int UW, int M, int N);
int pnnp_convt2x2_x3_bwd_weight_f32(const float* x, int Cin, const float* g, int Cout, float* dW, float* dbias /*or null*/,
                                    int B, int H, int W, int accumulate, float* workspace, int64_t workspace_floats, void* stream);
int pnnp_conv3x3s2_x3_bwd_weight_f32(const float* g, int Cout, const float* x, int Cin, float* dW, float* dbias /*or null*/,
                                     int B, int H, int W, int accumulate, float* workspace, int64_t workspace_floats, void* stream);
int pnnp_conv1x1_x3_bwd_weight_f32(const float* g, int g_cs, int Cout, const float* x1, int x1_cs, int C1,
                                   const float* x2 /*or null*/, int x2_cs, int C2, float* dW, float* dbias /*or null*/,
                                   int B, int H, int W, int accumulate, float* workspace, int64_t workspace_floats, void* stream);

/* (The Winograd kernel's cycle-stamp hook `pnnp_wino_set_debug` exists only in profiling builds, -DPNNP_WINO_DEBUG=1: the shipped
 * library exports no debug hook, reads no environment variable and keeps no state between calls besides idempotent per-device
 * caches of device facts and the persistent-split setting above.) */
/* Winograd backward-weight (dg = G^T [sum_tiles (A dY A^T) (.) (B^T d B)] G): same contract as
 * pnnp_conv_bwd_weight_f32 with taps = 9; needs H % 4 == 0, W % 8 == 0 and Cout, C1, C2 multiples of 64.
 * Limits (PNNP_E_UNSUPPORTED, nothing is launched): B * H * W * cs < 2^31 elements and, byte offsets inside one image being 32-bit,
 * (H * W + W + 1) * cs * 4 < 2^31 for the widest pixel stride cs of g_cs, x1_cs, x2_cs. */
int pnnp_wino_wgrad_supported(int H, int W, int Cout, int C1, int C2);
int64_t pnnp_wino_wgrad_workspace_floats(int B, int H, int W, int Cout, int Cin);
int pnnp_conv3x3_wino_bwd_weight_f32(const float* g, int g_cs, int Cout, const float* x1, int x1_cs, int C1,
                                     const float* x2, int x2_cs, int C2, float* dW, float* dbias /*or null*/,
                                     int B, int H, int W, int accumulate, float* workspace, int64_t workspace_floats,
                                     void* stream);
/* backward-weight: dW [Cout][C1+C2][taps] (+ dbias [Cout]); workspace from the query below. */
int64_t pnnp_wgrad_workspace_floats(int B, int H, int W, int M, int N, int taps);
int pnnp_wgrad_splits(int B, int H, int W, int M, int N, int taps);
/* backward-data through an identity shortcut: dx = (conv_bwd_data(g) + addsrc) * act'(mask)
 * (ResidualBlock, archs/modules.py:193-197). */
int pnnp_conv_bwd_data_res_f32(const float* g, int Cout, const float* w_dgrad, float* dx, int C1,
                               const float* addsrc, const float* mask, int mode, int B, int H, int W,
                               int taps, void* stream);
/* *_cs = channels per pixel of that tensor (>= the channels used: the 4-channel boundary
 * tensors travel zero-padded to 8 channels). */
int pnnp_conv_bwd_weight_f32(const float* g, int g_cs, int Cout, const float* x1, int x1_cs, int C1,
                             const float* x2, int x2_cs, int C2,
                             float* dW, float* dbias /*or null*/, int B, int H, int W, int taps,
                             int accumulate, float* workspace, int64_t workspace_floats, void* stream);
/* ConvTranspose2d(Cin, Cout, 2, stride=2): x [B][H][W][Cin] <-> y [B][2H][2W][Cout]. */
int pnnp_convt2x2_fwd_f32(const float* x, int Cin, const float* w_packed, const float* bias, float* y,
                          int B, int H, int W, int Cout, void* stream);
int pnnp_convt2x2_bwd_data_f32(const float* g, int Cout, const float* w_dgrad, float* dx, int Cin,
                               const float* mask, int mode, int B, int H, int W, void* stream);
int pnnp_convt2x2_bwd_weight_f32(const float* x, int Cin, const float* g, int Cout, float* dW,
                                 float* dbias /*[Cout] = channel sums of g, or null*/, int B, int H, int W, int accumulate,
                                 float* workspace, int64_t workspace_floats, void* stream);
/* Conv2d 3x3 stride 2 pad 1 (ResUnet down-sampling `conv3x3`, archs/modules.py:130-138,
 * archs/ResUnet.py:18-27): x [B][H][W][Cin] <-> y [B][H/2][W/2][Cout].  forward takes the ordinary
 * forward pack; backward-data its own pack (9*Cout*Cin floats); backward-weight workspace is
 * pnnp_wgrad_workspace_floats(B, H/2, W/2, Cout, Cin, 18). */
int pnnp_conv3x3s2_fwd_f32(const float* x, int Cin, const float* w_packed, const float* bias, float* y,
                           int B, int H, int W, int Cout, int act, void* stream);
int pnnp_pack_conv3x3s2_dgrad_f32(const float* w, float* dst, int Cout, int Cin, void* stream);
int pnnp_conv3x3s2_bwd_data_f32(const float* g, int Cout, const float* w_s2dgrad, float* dx, int Cin,
                                const float* mask, int mode, int accum, int B, int H, int W, void* stream);
int pnnp_conv3x3s2_bwd_weight_f32(const float* g, int Cout, const float* x, int Cin, float* dW,
                                  float* dbias /*or null*/, int B, int H, int W, int accumulate,
                                  float* workspace, int64_t workspace_floats, void* stream);
/* MaxPool2d(2) (archs/Unet.py:57-69); backward routes to the first maximum of each window,
 * multiplies by act'(x) and optionally accumulates into gx (skip-connection gradient).
 * Semantics of a window (a, b, c, d) = positions (0,0) (0,1) (1,0) (1,1), shared bit for bit by all four implementations -- pnnp_maxpool2_fwd_f32,
 * pnnp_maxpool2_fwd_codes_f32 and the epilogues of pnnp_conv3x3_x3_fwd_pool_f32 / pnnp_conv3x3_h2_fwd_pool_f32 (tests/test_gpu_misc.py):
 *   value   fmaxf(fmaxf(a, b), fmaxf(c, d)).  On finite data and infinities this is F.max_pool2d.  A NaN beside a number is DROPPED (fmaxf returns
 *           the other operand): the pooled value is NaN only if all four elements are, where F.max_pool2d returns NaN for any.  (The skip connection
 *           carries the same NaN to the loss, which does propagate it.)  Of +0.0 and -0.0 either may be returned.
 *   argmax  a scan from position 0 that moves to position k only on x[k] > x[arg]: the FIRST maximum wins a tie (+0.0 and -0.0 tie), and a comparison
 *           against a NaN is false, so a NaN at position 0 keeps the argmax and a later NaN never takes it.
 *   sign    x > 0: 0 for +0.0, -0.0 and NaN. */
int pnnp_maxpool2_fwd_f32(const float* x, float* y, int B, int H, int W, int C, void* stream);
int pnnp_maxpool2_bwd_f32(const float* x, const float* gy, float* gx, int B, int H, int W, int C,
                          int act_mode, int accumulate, void* stream);
/* The same pair with a one-byte code per pooled element (bits 0-1: first maximum of the window, bits 2-5: sign of its four
 * elements) written by the forward pass, so that the backward pass needs gy and the codes only (no second read of x). */
int pnnp_maxpool2_fwd_codes_f32(const float* x, float* y, unsigned char* codes /*[B][H/2][W/2][C]*/, int B, int H, int W, int C, void* stream);
int pnnp_maxpool2_bwd_codes_f32(const unsigned char* codes, const float* gy, float* gx, int B, int H, int W, int C, int act_mode,
                                int accumulate, void* stream);
/* ... and max |gx| (of the sums it stored, when accumulating) into an amax slot of the fp16x2 family (see pnnp_conv3x3_h2_fwd_f32) */
int pnnp_maxpool2_bwd_codes_amax_f32(const unsigned char* codes, const float* gy, float* gx, int B, int H, int W, int C, int act_mode,
                                     int accumulate, unsigned* amax_gx /*or null*/, void* stream);
/* ---------------------------------------------------------------- the thin ends of the networks (csrc/thin.hip)
 * The 1x1 head conv10_1 (archs/Unet.py:80,93: nf -> out_nc, no activation) and the first 3x3 convolution's weight gradient
 * (archs/Unet.py:31 conv1_1, in_nc -> nf).  With 4 channels on one side these are HBM streams over the full-resolution
 * nf-channel map, done in float32 on the vector ALUs; weights are read in the torch layout (no packed copy).
 *   head forward:  out NCHW [B][cout][H][W] = bias + x W^T (+ residual NCHW)   -- replaces the 1x1 GEMM + pnnp_nhwc_to_nchw_f32
 *   head backward: gx = (g W) * act'(x) [mode 0 none / 1 LeakyReLU(0.2) / 2 ReLU; x is the activation output],
 *                  dW [cout][cin] and dbias [cout] (+)= in the same pass over x and g (g: first cout of gcs >= 4 channels)
 *   first forward: y [B][H][W][ycs] = act(conv3x3(x) + bias), the 4 input channels NOT padded to a GEMM chunk
 *   first backward-weight: dW [cout][cin][3][3], dbias (+)=; x [B][H][W][xcs] must be ZERO in channels cin .. 3.
 * *_supported() say whether these kernels take the layer (else use pnnp_conv_* with taps 1 / 9); ws >= *_workspace_floats(). */
int pnnp_head_supported(int cin, int cout, int64_t npix);
int64_t pnnp_head_bwd_workspace_floats(int cin);
int pnnp_head_fwd_f32(const float* x, int xcs, int cin, const float* w /*[cout][cin]*/, const float* bias, const float* residual /*or null*/,
                      float* out, int B, int H, int W, int cout, void* stream);
int pnnp_head_bwd_f32(const float* g, int gcs, const float* x, int xcs, int cin, const float* w, float* gx, int gxcs, int mode,
                      float* dW, float* dbias /*or null*/, int B, int H, int W, int cout, int accumulate, float* ws, int64_t ws_floats,
                      void* stream);
int pnnp_head_bwd_amax_f32(const float* g, int gcs, const float* x, int xcs, int cin, const float* w, float* gx, int gxcs, int mode,
                           float* dW, float* dbias /*or null*/, int B, int H, int W, int cout, int accumulate, float* ws, int64_t ws_floats,
                           unsigned* amax_gx /*or null: max |gx| into an amax slot of the fp16x2 family*/, void* stream);
int pnnp_first_wgrad_supported(int cin, int cout, int H, int W);
int64_t pnnp_first_wgrad_workspace_floats(int cout);
int pnnp_first_fwd_f32(const float* x, int xcs, int cin, const float* w /*[cout][cin][3][3]*/, const float* bias /*or null*/, float* y, int ycs,
                       int B, int H, int W, int cout, int act /*0 none, 1 LeakyReLU(0.2), 2 ReLU*/, void* stream);
int pnnp_first_fwd_amax_f32(const float* x, int xcs, int cin, const float* w, const float* bias /*or null*/, float* y, int ycs,
                            int B, int H, int W, int cout, int act, unsigned* amax_y /*or null: max |y| into an amax slot*/, void* stream);
int pnnp_first_bwd_weight_f32(const float* g, int gcs, int cout, const float* x, int xcs, int cin, float* dW, float* dbias /*or null*/,
                              int B, int H, int W, int accumulate, float* ws, int64_t ws_floats, void* stream);
/* ... with an element type on the side that faces the network (the fp16-storage eval forward of ResUnet, ConvPolicy.h1_act16_res):
 *   first forward, dst_f16 != 0: y is an fp16 NHWC tensor = float16(v) of the float32 value v the _f32 twin stores -- one round to nearest even, unscaled,
 *     not saturated; amax_y still max |v|.  x stays float32.
 *   head forward, src_f16 != 0: x is an fp16 NHWC tensor (8-byte aligned, xcs in multiples of 4), widened exactly; fed x16 where the twin is fed float(x16)
 *     the outputs agree bit for bit.  w, bias, residual, out stay float32.
 * dst_f16 / src_f16 = 0: the twin itself. */
int pnnp_first_fwd_amax_et(const float* x, int xcs, int cin, const float* w, const float* bias /*or null*/, void* y, int ycs,
                           int B, int H, int W, int cout, int act, unsigned* amax_y /*or null*/, int dst_f16, void* stream);
int pnnp_head_fwd_et(const void* x, int xcs, int cin, const float* w /*[cout][cin]*/, const float* bias, const float* residual /*or null*/,
                     float* out, int src_f16, int B, int H, int W, int cout, void* stream);
/* boundary layout changes: NCHW [B][C][H][W] <-> NHWC [B][H][W][Cp] (Cp >= C, zero padded);
 * the NCHW result can add a residual (arch 'res' flag, archs/Unet.py:95-98). */
int pnnp_nchw_to_nhwc_f32(const float* src, float* dst, int B, int C, int H, int W, int Cp, void* stream);
/* the same into a frame that is reflect-padded by `pad` pixels on every side, dst [B][H+2pad][W+2pad][Cp]: the eval loop's
 * F.pad(imgs_lr, (4,4,4,4), mode='reflect') for frames whose width is not a multiple of 16 (trainer_SID.py:221-226), folded into the
 * layout change the network input goes through anyway */
int pnnp_nchw_to_nhwc_reflect_f32(const float* src, float* dst, int B, int C, int H, int W, int Cp, int pad, void* stream);
/* ... with max |element| raised into an amax slot of the fp16x2 family (the network input's scale: conv1_1 on pnnp_conv3x3_h2_fwd_f32) */
int pnnp_nchw_to_nhwc_reflect_amax_f32(const float* src, float* dst, int B, int C, int H, int W, int Cp, int pad, unsigned* amax /*or null*/, void* stream);
int pnnp_nhwc_to_nchw_f32(const float* src, const float* residual /*or null*/, float* dst,
                          int B, int C, int H, int W, int Cp, void* stream);
/* out[c] (+)= sum over pixels (bias gradient of a ConvTranspose2d); workspace >= 1024*C floats */
int pnnp_channel_sum_f32(const float* x, float* out, int64_t npix, int C, int accumulate,
                         float* workspace, void* stream);
/* loss = mean|clamp(pred,0,1) - hr| (trainer_SID.py:99, losses/base_loss.py:92-107) on NCHW
 * tensors; loss_out[0] = loss, loss_out[1+b] = sum_b (clamp(pred)-clamp(hr))^2 for PSNR_Loss
 * (losses/__init__.py:4-15); grad_nhwc (or null) = dL/dpred as [B][H][W][Cp].
 * workspace >= 128*B floats. */
int pnnp_l1_clamp_loss_f32(const float* pred, const float* hr, float* grad_nhwc, float* loss_out,
                           int B, int C, int H, int W, int Cp, float* workspace, void* stream);
/* the same with the `ori` branch of the train loop (trainer_SID.py:97-99: pred = pred * ratio before the loss):
 * scale [B] (device, or null = 1) multiplies crop b's prediction first; loss, SSE and dL/dpred (x scale[b]) follow. */
/* pnnp_l1_clamp_loss_scaled_f32 with the TARGET clamped to [0,1] inside the kernel when clamp_target != 0 (preprocess's
 * `imgs_hr.clamp(0, 1)` under dst.clip, trainer_SID.py:485, without an elementwise pass of its own) */
int pnnp_l1_clamp_loss_tc_f32(const float* pred, const float* hr, const float* scale /*[B] or null*/, float* grad_nhwc, float* loss_out,
                              int B, int C, int H, int W, int Cp, float* workspace, int clamp_target, void* stream);
int pnnp_l1_clamp_loss_scaled_f32(const float* pred, const float* hr, const float* scale /*[B] or null*/, float* grad_nhwc,
                                  float* loss_out, int B, int C, int H, int W, int Cp, float* workspace, void* stream);
/* pnnp_l1_clamp_loss_tc_f32 with dL/dpred multiplied by grad_weight: the weight B_local world / B_global of a rank's mean gradient when one
 * global batch is split unevenly over the data-parallel ranks (base_trainer.py:115-118 scatters the batch the same way); loss and SSE unweighted. */
int pnnp_l1_clamp_loss_w_f32(const float* pred, const float* hr, const float* scale /*[B] or null*/, float* grad_nhwc, float* loss_out,
                             int B, int C, int H, int W, int Cp, float* workspace, int clamp_target, float grad_weight, void* stream);
/* Unet_Loss (losses/base_loss.py:33-107) and its gradient (csrc/unet_loss.hip; an entry added under ABI version 9, as the tile entries were):
 *   recon = f-mean of d = low - high, f = |d| or, with `charbonnier`, sqrt(d^2 + 1e-6); with `pyramid` the 4-level AvgPool2d(2,2) pyramid
 *           (((t0 + t1/2) + t2/4) + t3/8) / 1.875 of the level means t_l, the levels pooled successively as Pyramid_Sample does;
 *   total = recon + grad_lambda * grad_loss(low, high)   (the Sobel edge term, :15-31, :80-84; grad_lambda = 0: not computed).
 * low = pred * scale[b], clamped to [0,1] when clamp_pred (the trainer's pred.clamp(0,1), trainer_SID.py:99; 0 = the bare module); high = hr,
 * clamped when clamp_target.  Otherwise the terms of pnnp_l1_clamp_loss_w_f32: grad_weight scales the gradient only, the clamp passes gradient on
 * the closed interval, a NaN prediction gives a NaN loss, and with charbonnier = pyramid = 0, grad_lambda = 0, clamp_pred = 1 loss, SSE and
 * gradient are that entry's bits.
 *   loss_out [1 + B]: total, then the per-crop SSE of the clamped pair at full resolution;  terms [5] (or null): the four level means before
 *   weighting (levels 1-3 zero without `pyramid`) and the Sobel term;  grad_nhwc [B][H][W][Cp] (or null; Cp 4 or 8, padding channels zero) and /
 *   or grad_nchw [B][C][H][W] (or null): dtotal/dpred.  recon = 0: only grad_lambda * the Sobel term and its gradient (SSE and terms[0..3] zero).
 * workspace: pnnp_unet_loss_workspace_floats(B) floats, 8-byte aligned.  Deterministic: per-block partials, a one-wave finish in a fixed order.
 * PNNP_E_INVALID before any launch, no output touched: null pred / hr / loss_out / workspace, B < 1 or > 2^20, C outside 1..8, H or W < 1,
 * Cp < C or not 4 / 8 or grad_nhwc off a 16-byte boundary, a flag that is not 0 / 1, grad_lambda negative or not finite, recon = 0 without
 * grad_lambda > 0, pyramid with grad_lambda > 0 (the reference never defines it), pyramid with H % 8 or W % 8 (deviation: the reference floors odd
 * sizes; the networks need multiples of 16) or pred / hr / grad_nchw off a 16-byte boundary.  PNNP_E_WORKSPACE: workspace_floats too small. */
int64_t pnnp_unet_loss_workspace_floats(int B);
int pnnp_unet_loss_f32(const float* pred, const float* hr, const float* scale /*[B] or null*/, float* grad_nhwc /*or null*/, float* grad_nchw /*or null*/,
                       float* loss_out, float* terms /*[5] or null*/, int B, int C, int H, int W, int Cp, float* workspace, int64_t workspace_floats,
                       int clamp_target, int clamp_pred, float grad_weight, int charbonnier, int pyramid, float grad_lambda, int recon, void* stream);
/* torch.optim.Adam step (trainer_SID.py:44,101) over a flat parameter buffer; step is 1-based;
 * grad_scale is applied to g first (1/world_size after a sum all-reduce). */
int pnnp_adam_step_f32(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
                       float beta2, float eps, int step, float grad_scale, void* stream);

/* ---------------------------------------------------------------- NoiseFlow.sample
 * archs/noise_flow.py:173-188: z ~ N(0,I) pushed through the reversed bijector chain
 * 8 x [AffineCoupling^-1, Conv2d1x1^-1] (+ GainISO^-1 after the 4th pair, SignalDependantISO^-1
 * at the end).  NCHW fp32 [B][4][H][W].  `step` [host] = 317 floats (struct NfStep in csrc/nf.hip):
 * conv2d_1 w[4][2][9] b[4], BN1 scale[4] offset[4], conv2d_2 w[4][4] b[4], BN2 scale[4] offset[4],
 * conv2d_3 w[4][5][9] b[4], exp(3*logs)[4], scale, W^-1[4][4] (x ISO gain where it applies). */
int pnnp_normal_fill_f32(float* out, int64_t n, uint64_t seed, uint64_t offset, void* stream);
int pnnp_nf_step_f32(const float* x, float* y, int B, int H, int W, const float* step /*[host]*/,
                     const float* clean /*or null*/, float sdn_a, float sdn_b, float out_mul, void* stream);
/* the same step with the trainer's preprocess around sample() fused in (trainer_SID.py:463-472,481-485; trainer_LRID.py:419-427):
 * the clean crop is divided by clean_div[b] (or clean_div_s) where it enters the signal-dependent scale (`clean = imgs_hr / ratio`);
 * with mix_base the result is clamp(mix_base + (sample * mix_mul[b] or mix_mul_s), clamp_lo, clamp_hi) (`imgs_lr = imgs_hr + noise *
 * ratio; imgs_lr.clamp(lb, 1)`); flag (device int, or null): bit 0 is set when the scale a*clean + b is negative anywhere -- the
 * reference's `assert scale >= 0` (signal_dependant.py:50) without a host round trip per step. */
int pnnp_nf_step_mix_f32(const float* x, float* y, int B, int H, int W, const float* step /*[host]*/,
                         const float* clean /*or null*/, float sdn_a, float sdn_b, float out_mul,
                         const float* clean_div /*[B] or null*/, float clean_div_s, const float* mix_base /*or null*/,
                         const float* mix_mul /*[B] or null*/, float mix_mul_s, float clamp_lo, float clamp_hi, int* flag /*or null*/,
                         const float* bn_stats /*device [24] or null*/, void* stream);
/* training-mode sampling (trainer_LRID.py:34-39,420-427: the proxy is never put in eval mode): with bn_stats = the batch statistics
 * pnnp_nf_train_stats_f32 left on the device, the step's BatchNorm slots hold weight / bias and scale = gamma rstd, offset =
 * beta - (mean + conv bias) scale are formed in the kernel; pnnp_nf_bn_update_f32 moves the running buffers of the coupling's two
 * BatchNorm2d layers as nn.BatchNorm2d does (momentum 0.1, unbiased variance, num_batches_tracked += 1; n = B H W).  No host round trip. */
int pnnp_nf_bn_update_f32(const float* bn_stats, const float* conv_bias1, const float* conv_bias2, float* running_mean1,
                          float* running_var1, float* running_mean2, float* running_var2, long long* batches1 /*or null*/,
                          long long* batches2 /*or null*/, double n, void* stream);
/* One [Conv2d1x1, AffineCoupling] pair of the forward (density) chain, NoiseFlow.forward (archs/noise_flow.py:113-130);
 * partial [B][ceil(H/32)*ceil(W/32)] receives the per-workgroup sums of the pixel-wise log-det terms. */
int pnnp_nf_fwd_step_f32(const float* x, float* y, float* partial, int B, int H, int W, const float* step /*[host]*/,
                         const float* clean, float sdn_a, float sdn_b, void* stream);

/* ---------------------------------------------------------------- NoiseFlow NLL fitting (csrc/nf_train.hip)
 * net.train(); nll, _ = net.loss(noise=, clean=, iso=); nll.backward()  (trainer_NF_SID.py:102,116-126; archs/noise_flow.py:113-165):
 * one [SignalDependantISO | GainISO, Conv2d1x1, AffineCoupling] pair of the forward chain with BatchNorm in training mode
 * (batch statistics, affine_coupling.py:257-264), and its backward.  All pointers are DEVICE pointers (parameters are read
 * from the device so that a step needs no host round trip):
 *   wm [4][4]   the Conv2d1x1 matrix W = P L U (conv2d1x1.py:58-65), divided by the GainISO scale where that layer precedes it
 *   ab {a, b}   SignalDependantISO scale sqrt(a*clean + b), a = beta1/gain, b = beta2 (signal_dependant.py:37-51); with clean, first pair
 *   prm [301]   W1[4][2][9] B1[4] G1[4] BE1[4] W2[4][4] B2[4] G2[4] BE2[4] W3[4][5][9] B3[4] LOGS[4] SCALE  (G/BE = BatchNorm weight/bias)
 *   bn [24]     out: mean1[4] rstd1[4] var1[4] mean2[4] rstd2[4] var2[4] (biased variances; eps 1e-5; means of the BIAS-FREE conv outputs)
 *   h1, h2, out3 [B][4][H][W]  saved conv2d_1 / conv2d_2 outputs (pre-BatchNorm, without their biases, which a batch-statistics
 *               BatchNorm cancels exactly) and conv2d_3 output * exp(3 logs)
 *   ldpart [tiles][2]  per-workgroup (sum of the pixel log-det terms, sum z^2), tiles = pnnp_nf_train_tiles(B,H,W), crop-major
 *   part        scratch: max(tiles*197, pblocks*28) floats covers both calls (pblocks = pnnp_nf_train_pblocks) */
int pnnp_nf_train_tiles(int B, int H, int W);
int pnnp_nf_train_pblocks(int B, int H, int W);
int pnnp_nf_train_fwd_pair_f32(const float* x, const float* clean /*or null*/, const float* ab, const float* wm, const float* prm,
                               float* bn, float* h1, float* h2, float* out3, float* z, float* ldpart, float* part, int B, int H, int W,
                               void* stream);
/* Backward of the pair: dz = gradient of its output (times dzmul; the last pair passes z and dzmul = -dL/dF / B for the N(0,I)
 * prior), cobj = dL/d(objective) per crop.  dx: gradient of its input.  sums [319] (deterministic reductions):
 *   dW3[180] dB3[4] dLOGS[4] dSCALE dBE2[4] dG2[4] | dW2[16] dB2[4] dBE1[4] dG1[4] | dW1[72] dB1[4] dWm[16] da db
 * dy2, dy1 [B][4][H][W] and dv23 [B][2][H][W] are scratch. */
int pnnp_nf_train_bwd_pair_f32(const float* x, const float* clean /*or null*/, const float* ab, const float* wm, const float* prm,
                               const float* bn, const float* h1, const float* h2, const float* out3, const float* dz, float dzmul,
                               float cobj, float* dx, float* sums, float* dy2, float* dy1, float* dv23, float* part, int B, int H,
                               int W, void* stream);
/* batch statistics of a coupling's two BatchNorm layers for training-mode SAMPLING (trainer_LRID.py:34-39,420-427: the proxy is
 * sampled without .eval()): u [B][4][H][W] feeds the coupling network with its first two planes; ident = device 4x4 identity;
 * bn [24] as above; h1, h2 scratch [B][4][H][W]; part scratch max(tiles, pblocks) * 8 floats. */
int pnnp_nf_train_stats_f32(const float* u, const float* ident, const float* prm, float* bn, float* h1, float* h2, float* part,
                            int B, int H, int W, void* stream);

/* ---------------------------------------------------------------- NoiseFlow.sample backward (csrc/nf_sample_bwd.hip)
 * The vector-Jacobian product of one [AffineCoupling^-1, Conv2d1x1^-1] pair of the reversed chain that pnnp_nf_step(_mix)_f32 runs:
 *   out = (Winv [u0, u1, (u2 - shift_a) exp(-ls_a), (u3 - shift_b) exp(-ls_b)]) * s,   (shift, ls) = coupling_net(u[0:2]),
 *   s = sqrt(a*clean + b) with clean (last pair), else 1.
 * All pointers are DEVICE pointers.  The caller keeps each pair's input u; the hidden maps are recomputed here.
 *   u, dout     [B][4][H][W] the pair's input and the gradient of its output;  du: gradient of its input (aliases neither)
 *   winv [4][4] the Conv2d1x1 inverse (x the GainISO scalar where it applies);  ab {a, b};  prm [301] as for pnnp_nf_train_*
 *   bn [24]     mean1[4] rstd1[4] -[4] mean2[4] rstd2[4] -[4] of the BIAS-FREE conv outputs.  bn_batch = 1: the batch statistics
 *               pnnp_nf_train_stats_f32 left for the forward (training mode; the BatchNorm-backward statistics terms are carried);
 *               bn_batch = 0: a fixed affine, mean = running_mean - conv bias, rstd = 1/sqrt(running_var + eps) (eval mode)
 *   gprm [301]  gradient of prm, same layout;  dwinv [16];  dab [2] (required with clean, else unused)
 *   scratch     h1, h2, out3, dy2, dy1 [B][4][H][W] each;  sums [319];  part [pnnp_nf_sample_bwd_part_floats(B,H,W)]
 * Deterministic (no float atomics): per-workgroup partial rows, then a column reduction in double. */
int64_t pnnp_nf_sample_bwd_part_floats(int B, int H, int W);
int pnnp_nf_sample_bwd_pair_f32(const float* u, const float* clean /*or null*/, const float* ab, const float* winv, const float* prm,
                                const float* bn, int bn_batch, const float* dout, float* du, float* gprm, float* dwinv,
                                float* dab /*or null*/, float* h1, float* h2, float* out3, float* dy2, float* dy1, float* sums,
                                float* part, int B, int H, int W, void* stream);

/* SNA_torch (data_process/process.py:562-588): shot-noise augmentation under a white-balance gain change.
 * gt [C][H][W] -> dn (the extra Poisson noise, / (wp-bl), x ratio unless ori) and dy (the signal change); aug_wb4 is a
 * HOST array of the four plane gains.  Counter-based RNG as in pnnp_noise_sample_f32. */
int pnnp_sna_f32(const float* gt, float* dn, float* dy, int C, int H, int W, const float* aug_wb4, float K, float wp, float bl,
                 float ratio, int black_lr, int ori, uint64_t seed, uint64_t offset, uint32_t crop, void* stream);

/* The paired-data branch of Trainer.preprocess (trainer_SID.py:430-447,481-485; trainer_LRID.py:367-397,436-439: datasets Mix_Dataset,
 * IMX686_Mix_Dataset, IMX686_SFRN_Raw_Dataset) in ONE launch over a batch: per crop i the digital gain on lr, SNA_torch on hr, the two
 * adds and the trainer's clamp.  lr, hr, lr_out, hr_out: f32 [B][4][H][W] (device); an output may alias ITS OWN input (every element is
 * read and written by one thread).  rows: f32 [B][PNNP_SNA_NPARAM] (device), one row per crop; nothing is read back.  Per element of
 * plane c, in float32, every operation rounded on its own:
 *   l = ori ? lr : lr*ratio
 *   if active:  g = hr*(wp-bl)/ratio;  y = g*aug[c];  n = Poisson(y/K)*K;  if black_lr: y -= g;  y = y*ratio/(wp-bl);  n = n/(wp-bl);
 *               if !ori: n *= ratio;   l += n;   if add_dy: hr += y
 *   PNNP_SNA_CLIP_MAX1: l = min(l,1), hr = clamp(hr,0,1);  PNNP_SNA_CLIP_MIN0 (with MAX1): l = max(l,0)
 * The Poisson draw of element t of global crop crop_base+i is pnnp_sna_f32's (same Philox block, same sampler): a batched call is
 * bit-equal to that entry followed by the adds, and independent of batch size, grid and rank.  An active row needs K > 0 and
 * ratio > 0 (the caller's duty: rows live on the device).  PNNP_E_INVALID: null pointers, 4*H*W >= 2^32, B >= 2^24. */
enum {
    PNNP_SNA_AUG0 = 0, PNNP_SNA_AUG1, PNNP_SNA_AUG2, PNNP_SNA_AUG3, PNNP_SNA_K, PNNP_SNA_WP, PNNP_SNA_BL, PNNP_SNA_RATIO,
    PNNP_SNA_ACTIVE, PNNP_SNA_BLACK_LR, PNNP_SNA_ADD_DY, PNNP_SNA_NPARAM = 12
};
#define PNNP_SNA_ORI 0x1u        /* dst.ori: lr is not multiplied by the ratio, nor is the noise */
#define PNNP_SNA_CLIP_MAX1 0x2u  /* dst.clip set: lr <= 1, hr in [0,1] */
#define PNNP_SNA_CLIP_MIN0 0x4u  /* dst.clip other than HALF_CLIP: lr >= 0 as well */
int pnnp_sna_batch_f32(const float* lr, const float* hr, float* lr_out, float* hr_out, int B, int H, int W, const float* rows,
                       unsigned flags, uint64_t seed, uint64_t offset, uint32_t crop_base, void* stream);

/* HighBitRecovery.map (data_process/process.py:718-751): pixels whose rounded value x lies in [low, high) are re-drawn
 * inside their quantisation bin, d' = ppf(cdf[x-low] + u*range[x-low]) + (d - x); d = data*in_mul; the result is
 * divided by out_div (norm=True) or, if out_div == 0, shifted by out_add (norm=False).  cdf/range: float64 device LUTs of
 * the host-side HB2LB_LUT; rand: optional float64 uniforms (else the counter RNG). */
int pnnp_hbr_map_f32(const float* data, float* out, int64_t n, const double* cdf, const double* range, int low, int high,
                     int dist /* 0 normal, 1 Tukey-lambda */, double loc, double scale, double lam, const double* rand,
                     float in_mul, float out_div, float out_add, int keep_delta, uint64_t seed, uint64_t offset, void* stream);

/* ---------------------------------------------------------------- dataset-side crop / augment
 * init_random_crop_point + random_crop + data_aug (data_process/syn_datasets.py:69-107,162-173; the 4-way
 * variant real_datasets.py:98-137), fused behind raw2bayer (utils/isp_ops.py:84-96), the linear dark-shading
 * subtraction (real_datasets.py:360-368) and the random_gains white-balance augmentation
 * (syn_datasets.py:313-322).  desc [device, n x 4 int32] = {h0, w0, rot90 k, flip}; gains [device, n x 3 f64]
 * = {rgb, red, blue} or NULL; dark [device, H x W] f32/f64 or NULL. */
int pnnp_crop_pack_bayer_u16(const uint16_t* frame, int H, int W, const void* dark, int dark_is_f64, double dark_add,
                             float* dst /* [n][4][ps][ps] */, int n, int ps, const int* desc, const double* gains,
                             const double* black4, double wp, int norm, int clip, int post_clip, void* stream);
int pnnp_crop_aug_f32(const float* img /* [C][h][w] */, int C, int h, int w, float* dst /* [n][C][ps][ps] */,
                      int n, int ps, const int* desc, const double* gains, int post_clip, void* stream);

/* ---------------------------------------------------------------- eval epilogue
 * IlluminanceCorrect.correct (data_process/__init__.py:165-175) and the raw-domain PSNR / SSIM of
 * quality_assess(tensor2im(.), tensor2im(.), data_range=255) (utils/visualization.py:9-31). */
int pnnp_illuminance_correct_f32(const float* pred, const float* src, float* out, int64_t n,
                                 double* workspace /* >= 512 doubles */, void* stream);
/* The elementwise tail of one eval iteration in one pass (trainer_SID.py:226-235: crop the reflect-padded output back, the input residual
 * of a `res` network, `ori`: x ratio, both frames clamped to [0,1]): dn = clamp((net_out[crop] (+ lr_in)) * ratio, 0, 1),
 * lr_out (or null) = clamp(lr_in * ratio, 0, 1).  net_out [C][HP][WP] holds the frame at (pad, pad); the others are [C][H][W]. */
int pnnp_eval_post_f32(const float* net_out, const float* lr_in, float* dn, float* lr_out /*or null*/, int C, int H, int W, int HP, int WP,
                       int pad, float ratio, const float* ratio_dev /*device scalar overriding ratio, or null*/, int add_residual, void* stream);
int pnnp_psnr_ssim_f32(const float* a, const float* b, float* out2 /* {psnr, ssim} */, int C, int H, int W,
                       double* workspace /* >= 2*C*ceil(H/32)*ceil(W/32) doubles */, void* stream);

/* ---------------------------------------------------------------- a frame as overlapping tiles and back (csrc/tiles.hip)
 * SynBase_Dataset.eval_crop / eval_merge (data_process/syn_datasets.py:109-159): d = base / 2, l = P - base, nh = H / l + 1, nw = W / l + 1,
 * tile (i, j) = number i * nw + j.  Crop: tile row i, local row r reads row (i < nh - 1 ? i * l : H - l) + r of the frame reflect-padded by d
 * (-k -> k, H-1+k -> H-1-k); the padded frame is never stored.  Merge: the interior [d, d + l) of every tile goes back to the frame; where
 * interiors overlap, the last tile row / column owns the element (the reference's write order), and a launch stores only what its tiles own, so
 * any partition of the tiles into launches fills the frame exactly once.  Columns alike.  Both take the tiles t0 .. t0 + nt of the grid.
 * PNNP_E_INVALID: null pointers, base odd / <= 0 / >= P, H < l or W < l, d >= H or d >= W, a tile range outside the grid, C H W >= 2^40;
 * crop with nhwc: Cp < C, Cp % 4 != 0, pitch < P, nhwc off a 16-byte boundary. */
/* frame [C][H][W] -> nchw [nt][C][P][P] and / or nhwc [nt][P][pitch][Cp] (channels >= C zero-filled; the layout of pnnp_nchw_to_nhwc_f32, float4
 * stores); amax (or null): max |element| raised into an amax slot of the fp16x2 family, as pnnp_nchw_to_nhwc_reflect_amax_f32 does. */
int pnnp_tile_crop_f32(const float* frame, int C, int H, int W, int P, int base, int t0, int nt, float* nchw /*or null*/, float* nhwc /*or null*/,
                       int pitch, int Cp, unsigned* amax /*or null*/, void* stream);
/* tiles [nt][C][P][P] -> frame [C][H][W], with the eval tail on the way: frame = tile * ratio, then clamp to [0, 1] if `clamp` (a NaN stays a NaN,
 * as in pnnp_eval_post_f32).  ratio 1 and clamp 0: the plain gather, bit for bit. */
int pnnp_tile_merge_f32(const float* tiles, float* frame, int C, int H, int W, int P, int base, int t0, int nt, float ratio,
                        const float* ratio_dev /*device scalar overriding ratio, or null*/, int clamp, void* stream);

/* ---------------------------------------------------------------- range census of the fp16x2 family (csrc/range_census.hip)
 * Per job (a tensor an fp16x2 kernel split and the amax slot it took the scale from): an integer histogram of
 * k = floor(log2 A) - floor(log2 |x|) over the finite non-zero elements (A: the float whose bits the slot holds; bins 0 .. 46, bin 47 = k >= 47)
 * and the counters zero, nonfinite and over (|x| > A: the slot contract says never).  The split keeps max(0, min(22, 39 - k)) significand
 * bits of an element in bin k.  `table` (device, 16-byte aligned, pnnp_census_table_words(rows) words, zeroed by the caller, word 0 = the first
 * "low-bit" bin) holds one row of PNNP_CENSUS_ROW_WORDS per job `row`: the running counters since the caller last zeroed the table, the
 * largest per-census low-bit share (share of the finite non-zero elements in bins >= word 0, as float bits) with the `step` of that census, the
 * latest share, the slot's bits and the number of censuses; words PNNP_CENSUS_SCRATCH .. of a row are the census's own 32-bit counts (zero
 * between launches).  `jobs`: a DEVICE array (16-byte aligned) of `njobs` <= PNNP_CENSUS_MAX_JOBS jobs with distinct rows, `x` 16-byte aligned,
 * n < 2^32.  Two launches (count, then summary); integer atomics only, so the table is bitwise reproducible. */
#define PNNP_CENSUS_BINS 48
#define PNNP_CENSUS_ZERO 48
#define PNNP_CENSUS_NONFINITE 49
#define PNNP_CENSUS_OVER 50
#define PNNP_CENSUS_COUNTERS 51         /* words 0 .. 50 of a row: bins, zero, nonfinite, over */
#define PNNP_CENSUS_WORST 51            /* float bits of the largest per-census low-bit share */
#define PNNP_CENSUS_WORST_STEP 52
#define PNNP_CENSUS_LAST 53             /* float bits of the latest census's share */
#define PNNP_CENSUS_AMAX 54             /* the slot's bits at the latest census */
#define PNNP_CENSUS_CENSUSES 55
#define PNNP_CENSUS_SCRATCH 64
#define PNNP_CENSUS_ROW_WORDS 128
#define PNNP_CENSUS_HDR_WORDS 64        /* header: [0] first low-bit bin (set by the caller), [1] censuses run, [2] step of the latest */
#define PNNP_CENSUS_MAX_JOBS 512
typedef struct PnnpCensusJob {
    const float* x; int64_t n;          /* the tensor's elements */
    const unsigned* slot;               /* its amax slot */
    int row, reserved;                  /* output row of the table; reserved = 0 */
} PnnpCensusJob;
int pnnp_census_job_bytes(void);
int64_t pnnp_census_table_words(int rows);
int pnnp_range_census_f32(const PnnpCensusJob* jobs /*[device]*/, int njobs, uint64_t* table, long long step, void* stream);

/* ---------------------------------------------------------------- score of a noise model (csrc/noise_score.hip)
 * kl_div_norm with bl given (utils/kld_div.py:163-200): the integer-DN histogram KL divergence of two sample sets, with the reference's float
 * edges (a key k = clip(rint(v (+ bl)), 0, wp) is counted in the bin np.histogram gives float32(k) / float32(wp) against
 * np.arange(0, 1 + 1/wp, 1/wp): `lut`, int32 [wp + 1], -1 = in no bin; depends on wp alone, built on the host with numpy), its shift rule
 * (p += bl, q += bl iff min(p) < 0 under numpy's NaN-propagating min) and n = every sample, NaNs included.  The caller's arrays are NOT
 * modified (the reference adds bl in place).
 *   pnnp_kl_div_norm_f32     p, q: [ncrops][n] float32 DN values, any element alignment.
 *   pnnp_noise_score_f32     trainer_NF_SID.py:165-172: clean, real, sampled_noise [ncrops][n]; inputs = clip(clean, 0, 1), output = sampled_noise +
 *                            inputs, p = rint((real - inputs) s), q = rint((output - inputs) s) in float32, s = float32(wp_data - bl_data); also the
 *                            population std of real and of output (float64 shifted sums).  bl, wp are kl_div_norm's own (defaults 512, 16383).
 * hist [ncrops][2][nbins] float64: y_p, y_q = counts / n.  result [ncrops][PNNP_NOISE_SCORE_ROW] float64: kl_fwd, kl_inv, kl_sym, gt_std, out_std,
 * diff_p = 100 (gt_std - out_std) / gt_std (the three zero in DN mode), flags of p (1: some p < 0, 2: some NaN; the shift is on iff flags == 1), 0.
 * ws: 16-byte aligned, pnnp_noise_score_ws_bytes(ncrops, n) bytes, need not be zeroed.  Behind one memset: pair mode one pass over the images
 * (p, q are integers there: it counts a window index from which the key with and without the shift follows) + a finishing launch; DN mode a
 * flags pass, a count pass and the finishing launch.  No synchronisation; 32-bit integer atomics and fixed-order float64 sums: bitwise
 * reproducible.  PNNP_E_UNSUPPORTED before anything is launched: n >= 2^32, wp > PNNP_NOISE_SCORE_MAX_WP, nbins > wp_max + 1, and in pair
 * mode a bl that is not an integer in [0, 512] (the window).  The bl=None branch of the reference (data-dependent edges) is pnnp_hist_edges_f64's, below. */
#define PNNP_NOISE_SCORE_MAX_WP 16383
#define PNNP_NOISE_SCORE_ROW 8
int64_t pnnp_noise_score_ws_bytes(int ncrops, int64_t n);
int pnnp_kl_div_norm_f32(const float* p, const float* q, int ncrops, int64_t n, float bl, int wp, const int* lut, int nbins,
                         void* ws, double* hist, double* result, void* stream);
int pnnp_noise_score_f32(const float* clean, const float* real, const float* sampled_noise, int ncrops, int64_t n, float s, float bl, int wp,
                         const int* lut, int nbins, void* ws, double* hist, double* result, void* stream);

/* ---------------------------------------------------------------- histogram KL over float edges (csrc/hist_kl.hip)
 * get_histogram / kl_div_3_data (utils/kld_div.py:145-161, :202-210) and the bl=None branch of kl_div_norm (:166-169): np.histogram's rule
 * for an array of float64 edges e[0..nbins] -- a sample x with e[0] <= x <= e[nbins] is counted in the largest bin i <= nbins - 1 with
 * e[i] <= x (half-open bins, the last one closed, equal neighbours give an empty bin); a smaller or larger x and a NaN are in no bin and count
 * in n only.  The comparison is exact: a float32 sample is widened to float64.  y = counts / n, each array by its own n; over the bins where
 * both are > 0: kl_fwd = sum yp (log yp - log yq), kl_inv = sum yq (log yq - log yp), kl_sym = (kl_fwd + kl_inv) / 2.
 *   pnnp_hist_edges_f64   p: [ncrops][n_p], q: [ncrops][n_q] or null; float32 (elem_f64 = 0) or float64 (1), aligned to their element, any
 *                         length.  edges: [nbins + 1] float64 on the device; PRECONDITION: finite and non-decreasing (the caller checks: the
 *                         values live on the device).  hint_scale = 0: a binary search per sample; > 0: the edges came from arange, the guess
 *                         int((x - hint_e0) hint_scale) is corrected against the table until the rule holds (a bad hint costs time only).
 *                         With q: hist [ncrops][2][nbins], kl [ncrops][3].  Without: hist [ncrops][nbins], kl is not written (may be null).
 *                         ws: 16-byte aligned, pnnp_hist_edges_ws_bytes(ncrops, nbins) bytes, need not be zeroed.
 *   pnnp_minmax_f         out: 6 doubles -- min p, max p, min q, max q over the FINITE samples (p's twice without a q; -0.0 reads as 0.0), then
 *                         1.0 if some sample is a NaN or an inf (else 0.0), then 0.  float32 values are exact in the doubles.
 * One memset, a count pass and a finishing launch (the range pass: three launches); no synchronisation; 32-bit integer atomics, integer min /
 * max atomics and fixed-order float64 sums: bitwise reproducible.  PNNP_E_UNSUPPORTED before anything is launched: nbins >
 * PNNP_HIST_EDGES_MAX_BINS, n_p or n_q >= 2^32.  PNNP_E_INVALID: null or misaligned pointers, ncrops outside 1..65535, n < 1, nbins < 1, a
 * negative or non-finite hint_scale. */
#define PNNP_HIST_EDGES_MAX_BINS 16384
int64_t pnnp_hist_edges_ws_bytes(int ncrops, int nbins);
int pnnp_hist_edges_f64(const void* p, const void* q, int elem_f64, int ncrops, int64_t n_p, int64_t n_q, const double* edges, int nbins,
                        double hint_e0, double hint_scale, void* ws, double* hist, double* kl, void* stream);
int pnnp_minmax_f(const void* p, const void* q, int elem_f64, int64_t n_p, int64_t n_q, void* out, void* stream);

/* ---------------------------------------------------------------- differentiable distribution losses (csrc/ddl.hip)
 * The linearly interpolated empirical CDF of a sample set at ascending points and the losses built on it, with the gradient with respect to
 * the samples, in streaming passes: no sort.  Per point k: xc = clamp(x[k], min d, max d), c = #{d < xc}, hi = min{d >= xc}, lo = max{d < xc}
 * (-inf if none), cdf[k] = ((float(c + 1) - (hi - xc) / (hi - lo)) - 1) / float(n - 1) in float32 in this order: bit for bit what
 * CDFPPF.get_cdf computes on the CPU.  float32 only; 2 <= n < 2^31; 1 <= k <= PNNP_DDL_MAX_K (the KLD: k >= 2); anything else is
 * PNNP_E_UNSUPPORTED before a launch.  PRECONDITION: x ascending (not checked).  NaN samples are not supported.  Among equal samples the LOWEST
 * index is the bracket (and receives the gradient).  Arrays may start at any element.  No synchronisation, nothing allocated; integer
 * atomics and fixed-order float64 sums only: bitwise reproducible.
 *   pnnp_ddl_ws_bytes   the workspace of a call with nops (1 or 2) operands and k points; ws is 16-byte aligned and need not be zeroed.
 *   pnnp_ecdf_f32       utils/kld_div.py:21-46 (CDFPPF: sort, inf padding, searchsorted, interpolation): cdf [k]; brackets [2k + 2] int32 =
 *                       arg hi [k], arg lo [k] (-1: none), arg min, arg max -- the state the backward needs.
 *   pnnp_ecdf_bwd_f32   the backward of :30-46 through sort / searchsorted / gather / clamp: grad [n] (zeroed here) of sum_k g[k] cdf[k]
 *                       (g times scale[0] when scale, a device pointer, is given), evaluated term by term like ATen (0 where lo = -inf).
 *   pnnp_cdf_loss_f32   :56-60 (CDFLoss): loss [1] = mean_k |cdf_output - cdf_gt|.
 *   pnnp_kld_loss_f32   :62-78 (KLD, cdf2pdf): q, p = max(|cdf[k] - cdf[k+1]|, float32(1e-9)) of output, gt, both divided by the (detached)
 *                       larger sum; loss [1] = sum p (log p - log q), float64 inside.
 *                       Both: output [n_output], gt [n_gt]; cdf [2][k], brackets [2][2k + 2], dcdf [2][k] = dL/dcdf (output, gt): what
 *                       pnnp_ecdf_bwd_f32 takes as g, with the upstream scalar as scale. */
#define PNNP_DDL_MAX_K 4096
int64_t pnnp_ddl_ws_bytes(int nops, int k);
int pnnp_ecdf_f32(const float* data, int64_t n, const float* x, int k, void* ws, float* cdf, int* brackets, void* stream);
int pnnp_ecdf_bwd_f32(const float* data, int64_t n, const float* x, int k, const int* brackets, const float* g, const float* scale /*[device], may be NULL*/,
                      float* grad, void* stream);
int pnnp_cdf_loss_f32(const float* output, int64_t n_output, const float* gt, int64_t n_gt, const float* x, int k, void* ws,
                      float* cdf, int* brackets, float* loss, float* dcdf, void* stream);
int pnnp_kld_loss_f32(const float* output, int64_t n_output, const float* gt, int64_t n_gt, const float* x, int k, void* ws,
                      float* cdf, int* brackets, float* loss, float* dcdf, void* stream);

/* ---------------------------------------------------------------- QuantileLoss (csrc/quantile.hip; utils/kld_div.py:49-53)
 * torch.quantile(..., dim=-1, interpolation='linear') of `rows` rows of n float32 samples at k probabilities q, the L1 loss between the
 * quantiles of two operands and the gradient with respect to the samples, by an exact multi-rank select: no sort.  Per probability, in float32
 * on the device:  pos = q * float(n - 1);  lo = floor(pos);  hi = ceil(pos);  w = pos - floor(pos)  (lo, hi clamped into [0, n - 1]);
 * value = w < 0.5 ? a + w * (b - a) : b - (b - a) * (1 - w)  with a = s[lo], b = s[hi] of the row sorted ascending, unfused.  The order
 * statistics are exact for any finite or infinite input (-0.0 orders as +0.0); among equal samples the LOWEST index holds an order statistic
 * (and receives its gradient).  q need not be ascending and may repeat; it is not validated.  NaN samples are not supported (no index leaves
 * [0, n)).  float32 only; 1 <= n < 2^31; 1 <= k <= PNNP_QUANTILE_MAX_K; rows >= 1; anything else is PNNP_E_UNSUPPORTED before a launch.
 * Three passes over the samples whatever they hold (range, census, gather); no synchronisation, nothing allocated; integer atomics and
 * fixed-order float64 sums only: bitwise reproducible.  Arrays may start at any element; rows are contiguous ([rows][n]).
 *   pnnp_quantile_ws_bytes   the workspace of a call on operands of n_a and n_b samples per row (n_b = 0: one operand); ws is 16-byte aligned
 *                            and need not be zeroed.  It holds 8 bytes per sample (the worst case of the gather: all samples equal).
 *   pnnp_quantile_f32        values [k][rows] (the layout torch.quantile returns); arg [2][rows][k] int32 = the element of its row that holds
 *                            s[lo], then s[hi]; w [k].
 *   pnnp_quantile_bwd_f32    grad [rows][n] (zeroed here) of sum g[k][r] value[k][r]: g (1 - w) to arg lo, g w to arg hi (g times scale[0] when
 *                            scale, a device pointer, is given); contributions that meet on an element are summed in float64 in a fixed
 *                            order and rounded once.
 *   pnnp_quantile_loss_f32   QuantileLoss: loss [1] = mean over k, rows of |value_output - value_gt|; values [2][k][rows], arg [2][2][rows][k],
 *                            w [2][k] (output, gt: their n may differ), dq [2][k][rows] = dL/dvalue = +-sign(difference) / (k rows), 0 at 0:
 *                            what pnnp_quantile_bwd_f32 takes as g, with the upstream scalar as scale.
 * These entries were added under ABI version 9 (entries only): a binding finds an older library by the missing symbol. */
#define PNNP_QUANTILE_MAX_K 1024
int64_t pnnp_quantile_ws_bytes(int rows, int64_t n_a, int64_t n_b, int k);
int pnnp_quantile_f32(const float* data, int rows, int64_t n, const float* q, int k, void* ws, float* values, int* arg, float* w, void* stream);
int pnnp_quantile_bwd_f32(int rows, int64_t n, int k, const int* arg, const float* w, const float* g, const float* scale /*[device], may be NULL*/,
                          float* grad, void* stream);
int pnnp_quantile_loss_f32(const float* output, int64_t n_output, const float* gt, int64_t n_gt, int rows, const float* q, int k, void* ws,
                           float* values, int* arg, float* w, float* loss, float* dq, void* stream);

/* ---------------------------------------------------------------- packed raw -> sRGB (csrc/isp.hip; data_process/process.py:104-184)
 * The reference's pure-tensor ISP `process()` and the trainers' per-epoch preview strip, one streaming pass per pixel, one launch per call.
 *   pnnp_isp_process_f32   in: f32 [B][4][H][W] packed RGBG (planes R, G1, B, G2), device.  rows: f32 [B][PNNP_ISP_NPARAM], device, one row per
 *                          image: 4 white-balance gains, then the 3x3 colour matrix row-major (out[r] = sum_c ccm[r][c] in[c]).  Per pixel, in
 *                          float32, every operation rounded on its own, in the reference's order:
 *                            x * wb;  clamp [0,1];  g = (g1 + g2) / 2;  (r c0 + g c1) + b c2 per matrix row;  clamp [0,1];
 *                            p = max(v, 1e-8) ^ float32(1/2.2)  (evaluated in float64 on the float32 operands, rounded once to float32; a value
 *                            whose float32 estimate of 255 p lies further than 2e-3 from every integer keeps the estimate: the same level);
 *                            level = clamp(int(p * 255), 0, 255)
 *                          With PNNP_ISP_GAMMA_ONLY `in` is f32 [B][3][H][W], rows is not read (may be NULL) and only the last two lines run
 *                          (the reference's gamma_compression).  Outputs, each optional (NULL skips it, one is required): out_f32
 *                          f32 [B][3][H][W] = level / 255 (the reference's result); out_u8 [B][H][W][3] = level, RGB or, with PNNP_ISP_BGR, BGR.
 *                          A NaN renders as level 0 (the reference's int() of it is undefined).
 *   pnnp_isp_preview_f32   trainer_SID.py:150-158 / trainer_NF_SID.py:166-180: inputs, output, target: f32 [4][H][W] (device; plane 3 is not
 *                          read); wb: 4 gains, HOST pointer; mid_offset: f32 [4][H][W] device or NULL.  out_u8 [H][3W][3] BGR: panel 0 is
 *                          clip(inputs, 0, 1), panel 1 output (+ clip(mid_offset, 0, 1) when given), panel 2 target; channel 0 times wb[0],
 *                          channel 2 times wb[2]; clip [0,1]; ^ float32(1/2.2) as above (no 1e-8 floor: 0 stays 0); uint8(v * 255).  Always
 *                          clips before the power (trainer_NF_SID does; trainer_SID does not and writes NaN bytes outside [0,1]).
 * Vector path (16 B per lane and plane, three dwords of bytes per lane) when W % 4 == 0 and every array starts 16-byte aligned; otherwise the same
 * arithmetic with scalar accesses.  PNNP_E_INVALID: null input, no output, B, H or W < 1, B > 65535, H * ceil(W / 4) >= 2^31.
 * These entries were added under ABI version 9 (entries only): a binding finds an older library by the missing symbol. */
#define PNNP_ISP_NPARAM 16       /* wb[4], ccm[9], 3 unused */
#define PNNP_ISP_BGR 0x1u        /* out_u8 in B, G, R order */
#define PNNP_ISP_GAMMA_ONLY 0x2u /* three planes in: gamma_compression alone */
int pnnp_isp_process_f32(const float* in, int B, int H, int W, const float* rows, unsigned flags, float* out_f32, uint8_t* out_u8, void* stream);
int pnnp_isp_preview_f32(const float* inputs, const float* output, const float* target, const float* mid_offset, int H, int W,
                         const float* wb /*[host, 4]*/, uint8_t* out_u8, void* stream);

/* ---------------------------------------------------------------- full-resolution render (csrc/demosaic.hip; utils/isp_ops.py:134-158, FastISP)
 * The reference's FastISP with its one outside call, cv2.cvtColor(COLOR_BAYER_BG2RGB_EA), replaced by the demosaic DEFINED here (parity
 * with an OpenCV build is not a goal).  Pattern RGGB, output order R, G, B, integer arithmetic on the mosaic S [H][W], H and W even, >= 4.
 *   Interior, 1 <= y <= H-2, 1 <= x <= W-2:
 *     R or B site (own colour C, other colour O):  C = S[y][x];
 *         G = (S[y-1][x] + S[y+1][x] + 1) >> 1  if |S[y][x-1] - S[y][x+1]| > |S[y-1][x] - S[y+1][x]|,
 *             (S[y][x-1] + S[y][x+1] + 1) >> 1  otherwise (a tie takes the horizontal pair);
 *         O = (S[y-1][x-1] + S[y-1][x+1] + S[y+1][x-1] + S[y+1][x+1] + 2) >> 2
 *     G site:  G = S[y][x];  the horizontal neighbours' colour = (S[y][x-1] + S[y][x+1] + 1) >> 1, the vertical neighbours' colour =
 *         (S[y-1][x] + S[y+1][x] + 1) >> 1: on even rows horizontal is R and vertical B, on odd rows the reverse
 *   Border:  out[y][x] = out[clamp(y, 1, H-2)][clamp(x, 1, W-2)], the interior formula evaluated at the clamped coordinate.
 *   pnnp_demosaic_ea_u16   the stencil alone: src u16 [B][H][W] -> dst u16 [B][H][W][3], both device; full-range inputs (sums in 32 bits).
 *   pnnp_fastisp_f32       one launch of front, stencil and tail.  in: f32 [B][4][h][w] packed planes R, G1, B, G2, device; H = 2h, W = 2w.
 *                          rows: f32 [B][PNNP_ISP_NPARAM] as for pnnp_isp_process_f32: gains 0 and 2 and the nine matrix entries are read.
 *                          Front, float32, every operation rounded on its own:  S[2i][2j] = R wb0, S[2i][2j+1] = G1, S[2i+1][2j+1] = B wb2,
 *                            S[2i+1][2j] = G2;  clamp [0,1];  * 16383.0f;  truncate to uint16.  A NaN gives 0 (DEVIATION: the reference's
 *                            cast of a NaN is undefined).
 *                          Tail, float64 as numpy does it in the reference:  v = D / 16383;  (v0 m[r][0] + v1 m[r][1]) + v2 m[r][2] per matrix
 *                            row r, the matrix entries widened to float64;  clamp [0,1];  ^ (1 / 2.2), evaluated to 1e-10 relative (a float32
 *                            estimate and one float64 Newton step on y^11 = v^5) and, where 255 y lies within 1e-6 of an integer, as
 *                            exp(log(v) / 2.2) to 1e-14.
 *                            With PNNP_FASTISP_SONY_CCM the matrix is the reference's default (isp_ops.py:151-153), a float64 constant
 *                            that the float32 table cannot carry, and the table's matrix entries are not read.
 *                          Outputs, each optional (NULL skips it, one is required): out_f32 f32 [B][3][H][W] = float32(v64) (DEVIATION: the
 *                            reference returns float64); out_u8 [B][H][W][3] = floor(255 v64), RGB or, with PNNP_ISP_BGR, BGR.  Both
 *                            come from the same float64 value: the bytes do not depend on whether the planes are asked for.
 * Vector stores (16 B per lane and float plane, three dwords of bytes, 24 B of uint16) when W % 4 == 0 and every output starts 16-byte aligned;
 * otherwise the same arithmetic with element stores.  PNNP_E_INVALID: a null input, rows or (every) output, B < 1, B > 65535, h < 2 or w < 2
 * (H < 4, W < 4 or an odd side for the stencil alone), 3 H W >= 2^31; a refusal leaves the outputs untouched.
 * Added under ABI version 9 (entries only): a binding finds an older library by the missing symbol. */
#define PNNP_FASTISP_SONY_CCM 0x4u /* the tail's matrix is the reference's float64 default */
int pnnp_demosaic_ea_u16(const uint16_t* src, int B, int H, int W, uint16_t* dst, void* stream);
int pnnp_fastisp_f32(const float* in, int B, int h, int w, const float* rows, unsigned flags, float* out_f32, uint8_t* out_u8, void* stream);

/* ---------------------------------------------------------------- sRGB -> packed raw(csrc/unprocess.hip; data_process/unprocess.py:79-167, 199-207)
 * The reference's `unprocess()` arithmetic and its `mosaic` / `mosaic_GBRG` gathers, one streaming pass per pixel, one launch per call.
 *   in        device; in_kind says what it holds:  PNNP_UNP_IN_HWC_F32  f32 [B][H][W][3] (the reference's layout: apply_ccm and safe_invert_gains
 *             work on the last axis);  PNNP_UNP_IN_CHW_F32  f32 [B][3][H][W] planes;  PNNP_UNP_IN_HWC_U8  uint8 [B][H][W][3], taken as
 *             float32(v) / 255 (an EXTENSION: the reference has no 8-bit input).
 *   rows      f32 [B][PNNP_UNP_NPARAM], device, one row per image: rgb2cam row-major (c[i] = sum_j l[j] rgb2cam[i][j]), then the three gains
 *             (1/red, 1, 1/blue) / rgb_gain as the reference's float32 tensor ops give them (safe_invert_gains :111), 4 unused.
 *   Per pixel, in float32, every operation rounded on its own, in the reference's order:
 *             x = clamp(in, 0, 1);  s = 0.5 - sin(asin(1 - 2x) / 3);  l = max(s, 1e-8) ^ 2.2;  c[i] = (l0 m[i][0] + l1 m[i][1]) + l2 m[i][2];
 *             gray = ((c0 + c1) + c2) / 3;  mask = (max(gray - 0.9, 0) / float32(1 - 0.9))^2;  safe[i] = max(mask + (1 - mask) gains[i], gains[i]);
 *             out[i] = clamp(c[i] safe[i], 0, 1)
 *             DEVIATION: s is the same root of 3 s^2 - 2 s^3 = x taken without the reference's cancellation (it returns the 1e-8 floor below
 *             x ~ 6e-8; x > 0.5 through the curve's symmetry) and polished by one Newton step with a float64 residual: within an ulp of
 *             the float64 value for every x.
 *             A NaN passes every clamp and the maximum as in torch: one NaN channel makes the pixel's three channels NaN.
 *   out_rgb   f32 in the INPUT's layout ([B][H][W][3], or [B][3][H][W] for CHW_F32): what `unprocess()` returns.  NULL skips it.
 *   out_packed  f32 [B][4][H/2][W/2], the gather of out_rgb.  NULL skips it; one output is required.  Plane order without flags (`mosaic`):
 *             R (0::2,0::2), Gr (0::2,1::2), B (1::2,1::2), Gb (1::2,0::2), the RGBG order of raw2bayer above.  With PNNP_UNP_GBRG
 *             (`mosaic_GBRG`, whose plane order differs): R (1::2,0::2), Gr (1::2,1::2), Gb (0::2,0::2), B (0::2,1::2).  Bitwise the gather of
 *             out_rgb of the same launch; with out_rgb NULL a pixel applies the gain to its Bayer channel alone.
 * Vector path (16-byte loads and RGB stores, 8-byte packed stores) when W % 4 == 0 and every array starts 16-byte aligned (uint8 input: 4);
 * otherwise the same arithmetic with element accesses.  PNNP_E_INVALID: null in or rows, no output, an unknown in_kind or flag, B, H or W < 1,
 * odd H or W with out_packed (the reference's torch.stack fails there), a float array that is not 4-byte aligned, B H W >= 2^40.
 * Added under ABI version 9 (an entry only): a binding finds an older library by the missing symbol. */
#define PNNP_UNP_NPARAM 16       /* rgb2cam[9], gains[3], 4 unused */
#define PNNP_UNP_IN_HWC_F32 0
#define PNNP_UNP_IN_CHW_F32 1
#define PNNP_UNP_IN_HWC_U8 2
#define PNNP_UNP_GBRG 0x1u       /* out_packed in mosaic_GBRG's pattern and plane order */
int pnnp_unprocess_f32(const void* in, int in_kind, int B, int H, int W, const float* rows, unsigned flags, float* out_rgb /*or NULL*/,
                       float* out_packed /*or NULL*/, void* stream);

/* ---------------------------------------------------------------- classical raw filters (csrc/isp_algos.hip; utils/isp_algos.py, isp_ops.py:70-74,115-123)
 * The reference's VST / inverse_VST, GuidedFilter, FastGuidedFilter, stdfilt, bayer2gray and repair_bad_pixels.  Their OpenCV calls are
 * replaced by the definitions below (parity with an OpenCV build is not a goal).  Images are N planes of H x W float32 addressed by element
 * strides {plane, row, pixel} (row and pixel >= 1): contiguous planes are {H W, W, 1}, channel-last data [H][W][C] is {1, W C, C}.
 *   BOX MEAN  window d x d, d odd, 1 <= d <= 51, anchor at the centre; border REPLICATE (aaa|abc|ccc, the default) or, with
 *             PNNP_BOX_REFLECT_101, cb|abc|cb, which needs d / 2 < min(H, W).  The d^2 values are summed in float64 (row sums first, each
 *             sum started at its first term, no running sums), multiplied by the float64 constant 1.0 / (d d) and rounded once to float32.
 *             Products (I I, I p, x x) are rounded to float32 before they are widened.  Everything after the means is float32, every
 *             operation rounded on its own, division and square root IEEE.
 *   pnnp_guided_ab_f32     mu_p, mu_I, II = box(I I), Ip = box(I p);  var = II - mu_I mu_I;  cov = Ip - mu_I mu_p;  a = cov / (var + eps);
 *                          b = mu_p - a mu_I.  a, b: contiguous planes [N][H][W].  p == I (the same pointer) skips the duplicate means,
 *                          bitwise the same result.  With PNNP_BOX_HALF (H and W even; the border is REFLECT_101) p and I are read through
 *                          the 0.5x bilinear resize, the mean f32(f32(x00 + x01) 0.25f + f32(x10 + x11) 0.25f) of each 2 x 2 block, and a, b are [N][H/2][W/2].
 *   pnnp_guided_apply_f32  out = box(a) I + box(b), out addressed by its own strides.  With PNNP_BOX_HALF a, b are [N][H/2][W/2]; their
 *                          means (REFLECT_101) go to `workspace` (2 N H/2 W/2 floats, device; NULL otherwise) and are upsampled by 2
 *                          with INTER_LINEAR's rule: source coordinate (x + 0.5) / 2 - 0.5, weights 0.75 / 0.25, at both ends the weight
 *                          of the missing neighbour is 0; horizontal pass first; each pass s0 (1 - w) + s1 w in float32.
 *   pnnp_stdfilt_f32       sqrt(max(box(x x) - box(x)^2, 0)) with REFLECT_101 (a NaN stays a NaN).
 *   pnnp_vst_f32           n contiguous elements.  inverse = 0 (the generalised Anscombe transform as the reference writes it, `wp` only
 *                          divides):  t = ((f32(gain) x + f32(gain^2 3 / 8)) + f32(sigma^2)) - f32(gain mu);  y = sqrt(max(t, 0)) / f32(wp);
 *                          out = f32(2 / gain) y.  inverse = 1:  x = x f32(wp);  y = ((x / 2)^2 - 0.375f) - f32(sigma^2 / gain^2);
 *                          out = (y f32(gain)) / f32(wp); mu is not added back, as in the reference.  The constants are formed in double.
 *                          scale (device, NULL: none): one float per `group` consecutive elements; forward transforms f32(x scale),
 *                          inverse returns f32(out / scale).
 *   pnnp_bayer2gray_f32    src f32 [B][H][W] -> dst: the 3 x 3 filter [1 2 1; 2 4 2; 1 2 1] / 16 with BORDER_REFLECT (cba|abc|cba): nine exact
 *                          float64 products summed in row-major order, rounded once.
 *   pnnp_repair_bad_pixels raw: one mosaic [H][W] (both even) of elem_size 2 (uint16) or 4 (float32), repaired IN PLACE at the n points
 *                          (row, col), int32 [n][2] on the device: the median of the 3 x 3 neighbourhood in the point's own colour plane
 *                          (stride 2 in the mosaic, REPLICATE at the plane's border), every median taken from the unmodified frame (two
 *                          launches through `tmp`, n elements of elem_size, device).  Duplicates allowed; n = 0 launches nothing.  A point
 *                          outside the frame is the caller's to refuse (the kernels skip it).  A NaN in a float32 neighbourhood is not
 *                          supported: the compare-exchange network does not put it last as a sort does, and the median is then unspecified.
 * PNNP_E_INVALID before any launch, outputs untouched: a null or misaligned pointer, N or B outside 1..65535, H or W < 1 or > 2^24, d even or
 * outside 1..51, REFLECT_101 with d / 2 >= min(H, W), odd H or W with PNNP_BOX_HALF (or for the repair), an unknown flag, a NaN eps, gain or wp 0.
 * All kernels are scratch-free and use vector accesses only.  Added under ABI version 9 (entries only). */
#define PNNP_BOX_REFLECT_101 0x1u /* border cb|abc|cb instead of aaa|abc|ccc */
#define PNNP_BOX_HALF 0x2u        /* FastGuidedFilter: a, b at half resolution */
int pnnp_guided_ab_f32(const float* p, const float* I, int N, int H, int W, const int64_t* strides /*[host, 3]*/, int d, float eps, unsigned flags,
                       float* a_out, float* b_out, void* stream);
int pnnp_guided_apply_f32(const float* a_in, const float* b_in, const float* I, int N, int H, int W, const int64_t* i_strides /*[host, 3]*/, int d,
                          unsigned flags, float* workspace /*or NULL*/, float* out, const int64_t* out_strides /*[host, 3]*/, void* stream);
int pnnp_stdfilt_f32(const float* x, int N, int H, int W, const int64_t* strides /*[host, 3]*/, int k, float* out,
                     const int64_t* out_strides /*[host, 3]*/, void* stream);
int pnnp_vst_f32(const float* x, int64_t n, int inverse, double sigma, double mu, double gain, double wp, const float* scale /*or NULL*/,
                 int64_t group, float* out, void* stream);
int pnnp_bayer2gray_f32(const float* src, int B, int H, int W, float* dst, void* stream);
int pnnp_repair_bad_pixels(void* raw, int elem_size, int H, int W, const int32_t* points, int n, void* tmp, void* stream);

/* ---------------------------------------------------------------- dark-frame calibration (csrc/calib.hip; pnnp_amd/calibrate.py)
 * The two streaming passes over a stack of dark (bias) frames from which pnnp_amd/calibrate.py estimates a camera's noise table, and the
 * row means that row_denoise needs.  frames: uint16 [n][H][W], a contiguous Bayer mosaic on the device: one chunk of the stack.
 *   pnnp_calib_accum_u16     one read of the chunk, three exact integer results:
 *                              sum[y][x]   += sum_f v            int32 [H][W], read and written: the caller zeroes it before the first chunk
 *                              sumsq[y][x] += sum_f v v          int64 [H][W], likewise
 *                              rowsum[f][y][c] = sum over x with (x & 1) == c of v     int32 [n][H][2], this chunk's slice, written (never read)
 *                            A chunk of more than 1024 frames runs as several launches.  The caller keeps the stack's total at or below
 *                            32768 frames (32768 * 65535 < 2^31, the int32 sum); the entry refuses n > 32768.
 *   pnnp_calib_residual_u16  out[f][y][x] = (float(v) - ds[y][x]) - rowoff[f][y][x & 1]: two float32 subtractions in that order, each
 *                            rounded on its own.  ds f32 [H][W], rowoff f32 [n][H][2], out f32 [n][H][W].
 *   pnnp_calib_rowmean_f32   out[y] = (sum_x map[y][x]) / W in float64, map f32 [H][W], out f64 [H]; one workgroup per row, a fixed order
 *                            (thread t adds x = t, t + 256, ... in order; the 256 partial sums fold in halves).
 * 16-byte accesses when W % 8 == 0 and frames, sum, sumsq (ds, out) start 16-byte aligned; otherwise the same arithmetic with element
 * accesses.  PNNP_E_INVALID before any launch, outputs untouched: a null or misaligned pointer, n outside 1..32768, H or W odd or below 2
 * (rowmean: below 1), W > 65536 (the int32 row sum), H > 2^24.  All kernels are scratch-free and use vector accesses only.
 *
 * THE 1-D BILATERAL FILTER of row_denoise (the stand-in for cv2.bilateralFilter on a 1 x n row; parity with an OpenCV build is not a
 * goal), float64 on the host over the n row means m:
 *     out[i] = sum_k w_k m[clamp(i + k, 0, n - 1)] / sum_k w_k,   k = -12 .. 12 (window 25, border REPLICATE),
 *     w_k = exp(-k^2 / (2 ss^2)) exp(-(m[clamp(i + k)] - m[i])^2 / (2 sc^2)),   sc = 10,  ss = 1 + iso / 200,
 * the terms added in the order k = -12 .. 12.
 * Added under ABI version 9 (entries only): a binding finds an older library by the missing symbol. */
int pnnp_calib_accum_u16(const uint16_t* frames, int n, int H, int W, int32_t* sum_i32, int64_t* sumsq_i64, int32_t* rowsum_i32, void* stream);
int pnnp_calib_residual_u16(const uint16_t* frames, int n, int H, int W, const float* ds_f32, const float* rowoff_f32, float* out_f32, void* stream);
int pnnp_calib_rowmean_f32(const float* map, int H, int W, double* out_f64, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PNNP_HIP_H */

// The bf16x3 ("x3") family's operand split: a float32 value as the sum of three bf16 pieces hi + mid + lo (round to nearest even each; the residuals
// are exact in float32), two values per register (csrc/conv_x3s.hip).
#pragma once
#include "common.h"

__device__ __forceinline__ unsigned cvt_pk_bf16(float a, float b) {      // RNE, low half = a
    unsigned r; asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r;
}
__device__ __forceinline__ void split2(float a0, float a1, unsigned& h, unsigned& m, unsigned& l) {
    h = cvt_pk_bf16(a0, a1);
    const float r0 = a0 - __uint_as_float(h << 16), r1 = a1 - __uint_as_float(h & 0xffff0000u);
    m = cvt_pk_bf16(r0, r1);
    const float s0 = r0 - __uint_as_float(m << 16), s1 = r1 - __uint_as_float(m & 0xffff0000u);
    l = cvt_pk_bf16(s0, s1);
}

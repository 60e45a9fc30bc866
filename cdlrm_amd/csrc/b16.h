// The bf16 operand conversions of the matrix-core modes: the one rounding of "bf16" and the two-plane split of "bf16x3" (DESIGN.md
// 4.1, 4.2), shared by the MLP GEMMs (gemm_bf16.h) and the extra-wide interaction (interact_xwide_b16.hip).
#pragma once
#include "common.h"

typedef __bf16 b16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 b16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2v __attribute__((ext_vector_type(2)));

// two fp32 -> packed bf16 pair (lo in bits 0-15): the plain cast, v_cvt_pk_bf16_f32 (round-to-nearest-even, NaN-preserving)
__device__ __forceinline__ unsigned b16_pack(float lo, float hi) {
    const b16x2 v = __builtin_convertvector((f32x2v){lo, hi}, b16x2);
    return __builtin_bit_cast(unsigned, v);
}

// the two planes of a pair: hi = the plain cast, lo = the cast of the (exact) remainder, 0 where hi is Inf or NaN -- a NaN or an
// overflow then lives in the hi plane alone and reaches the outputs of its own row / column only
__device__ __forceinline__ void b16_split(float x0, float x1, unsigned& hi, unsigned& lo) {
    hi = b16_pack(x0, x1);
    const float r0 = x0 - __uint_as_float(hi << 16), r1 = x1 - __uint_as_float(hi & 0xffff0000u);
    lo = b16_pack((hi & 0x7f80u) != 0x7f80u ? r0 : 0.f, (hi & 0x7f800000u) != 0x7f800000u ? r1 : 0.f);
}

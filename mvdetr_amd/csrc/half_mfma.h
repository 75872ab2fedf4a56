// What the MFMA kernels share -- gfx950 (MI355X): the 32x32 accumulator layout (the fp32 kernels of attention.hip and
// deform_conv.hip too), and for the 16-bit kernels (attention_half.hip, deform_conv_half.hip) the 32x32x16 product, the packed
// conversions and the hi / lo split of an fp32 operand.
#pragma once
#include "half_types.h"

#include <type_traits>

namespace mvdetr {

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef float floatx2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

// v_mfma_f32_32x32x*: lane (r = lane & 31, h = lane >> 5) holds D[mfma_crow(e, h)][r] in accumulator register e
__device__ __forceinline__ int mfma_crow(int e, int h) { return (e & 3) + 8 * (e >> 2) + 4 * h; }

// v_mfma_f32_32x32x16_{f16,bf16}: eight 16-bit values of A and of B per lane
template <typename Conv> __device__ __forceinline__ floatx16 mfma16(const uint4 &a, const uint4 &b, const floatx16 &c)
{
    if constexpr (std::is_same<Conv, F16>::value)
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// two fp32 values -> one word of two 16-bit values, round to nearest even (the lower address first).  bfloat16 takes the
// hardware's packed conversion (v_cvt_pk_bf16_f32) where BF16::down spends ~6 integer ops per value; for values that are never
// NaN (probabilities; column values unless the input is).
template <typename Conv> __device__ __forceinline__ uint32_t pack2(float a, float b)
{
    const floatx2 f = {a, b};
    if constexpr (std::is_same<Conv, F16>::value)
        return __builtin_bit_cast(uint32_t, __builtin_convertvector(f, f16x2));
    else
        return __builtin_bit_cast(uint32_t, __builtin_convertvector(f, bf16x2));
}

constexpr float HALF_LO_SCALE = 2048.f;                      // 2^11: the fp16 lo term
constexpr float HALF_MIN = 6.103515625e-05f;                 // 2^-14, the smallest normal half

// An fp32 operand as two 16-bit terms, two values at a time: hi = rn16(x), lo = rn16(x - hi) (the difference is exact), one MFMA
// each.  fp16: nothing depends on what the MFMA does with subnormal operands -- a hi below 2^-14 is sent to 0 (lo then carries
// the value whole) and lo is scaled by HALF_LO_SCALE (the caller keeps it in an accumulator of its own).  SIGNED: x may be
// negative (column values; probabilities are not, and their kernel was tuned on the plain comparison).
template <typename Conv, bool SIGNED> __device__ __forceinline__ void split2(float x0, float x1, uint32_t &hi, uint32_t &lo)
{
    float h0, h1;
    if constexpr (std::is_same<Conv, F16>::value) {
        const bool s0 = (SIGNED ? fabsf(x0) : x0) < HALF_MIN, s1 = (SIGNED ? fabsf(x1) : x1) < HALF_MIN;
        hi = pack2<Conv>(s0 ? 0.f : x0, s1 ? 0.f : x1);
        up2<Conv>(hi, h0, h1);
        lo = pack2<Conv>((x0 - h0) * HALF_LO_SCALE, (x1 - h1) * HALF_LO_SCALE);
    } else {
        hi = pack2<Conv>(x0, x1);
        up2<Conv>(hi, h0, h1);
        lo = pack2<Conv>(x0 - h0, x1 - h1);
    }
}

}  // namespace mvdetr

// 16-bit storage types of the inference kernels (float16 / bfloat16) -- gfx950 (MI355X).
//
// The house style of every 16-bit kernel here: tensors are READ and WRITTEN as raw 16-bit words, every arithmetic step
// is fp32, and a result is rounded once, to nearest-even, on the way out.  A kernel is templated on one of the two
// converters below; Raw<VEC> is VEC such words as one 2 / 4 / 8 / 16-byte access.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mvdetr {

struct F16 {
    static __device__ __forceinline__ float up(uint16_t h)
    {
        _Float16 x;
        __builtin_memcpy(&x, &h, 2);
        return (float)x;
    }
    static __device__ __forceinline__ uint16_t down(float f)
    {
        const _Float16 x = (_Float16)f;                   // v_cvt_f16_f32: round to nearest even
        uint16_t h;
        __builtin_memcpy(&h, &x, 2);
        return h;
    }
};

struct BF16 {
    static __device__ __forceinline__ float up(uint16_t h) { return __uint_as_float((uint32_t)h << 16); }
    static __device__ __forceinline__ uint16_t down(float f)
    {
        const uint32_t u = __float_as_uint(f);
        if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);      // quiet NaN
        return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);                      // round to nearest even
    }
};

template <int VEC> struct Raw;                            // VEC 16-bit values as one access
template <> struct Raw<1> { uint16_t v[1]; };
template <> struct alignas(4) Raw<2> { uint16_t v[2]; };
template <> struct alignas(8) Raw<4> { uint16_t v[4]; };
template <> struct alignas(16) Raw<8> { uint16_t v[8]; };

// The two values of one 32-bit word (the lower address first), and back.
template <typename C> __device__ __forceinline__ void up2(uint32_t w, float &lo, float &hi)
{
    lo = C::up((uint16_t)(w & 0xffffu));
    hi = C::up((uint16_t)(w >> 16));
}
template <typename C> __device__ __forceinline__ uint32_t down2(float lo, float hi)
{
    return (uint32_t)C::down(lo) | ((uint32_t)C::down(hi) << 16);
}

// Eight values (16 bytes) as four words in registers: a uint4 stays in VGPRs where an indexed array of halves may not.
// `ok` false: zeros, without a branch and without touching `p` (the address is replaced by `safe`, any readable one).
__device__ __forceinline__ uint4 load8_or_zero(const uint16_t *p, bool ok, const uint16_t *safe)
{
    const uint4 v = *reinterpret_cast<const uint4 *>(ok ? p : safe);
    return make_uint4(ok ? v.x : 0u, ok ? v.y : 0u, ok ? v.z : 0u, ok ? v.w : 0u);
}
template <typename C> __device__ __forceinline__ void up8(const uint4 &r, float (&f)[8])
{
    up2<C>(r.x, f[0], f[1]);
    up2<C>(r.y, f[2], f[3]);
    up2<C>(r.z, f[4], f[5]);
    up2<C>(r.w, f[6], f[7]);
}
template <typename C> __device__ __forceinline__ uint4 down8(const float (&f)[8])
{
    return make_uint4(down2<C>(f[0], f[1]), down2<C>(f[2], f[3]), down2<C>(f[4], f[5]), down2<C>(f[6], f[7]));
}

}  // namespace mvdetr

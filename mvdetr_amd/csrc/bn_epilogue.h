// The inference BatchNorm epilogue  act( x*s[c] + t[c]  [+ q]  [+ q*s2[c] + t2[c]] )  as the kernels that apply it share
// it: the pass of its own (trunk_epilogue.hip) and the Winograd convolution's output store (conv_winograd.hip).  One
// text for the fold and for the finishing step, compiled under the same flags in both, so that the convolution's fused
// store gives the bits of the convolution followed by the pass.
//     s = gamma / sqrt(var + eps),  t = beta - mean * s        formed in the kernel on every call (nothing cached)
#pragma once
#include <hip/hip_runtime.h>

namespace mvdetr {

struct BnVectors {
    const float *mean, *var, *gamma, *beta;                   // [C]; gamma / beta may be null (1 / 0)
    float eps;
};

__device__ __forceinline__ float bn_scale(float g, float v, float eps) { return g / sqrtf(v + eps); }
// Every multiply-add below is ONE fused operation, written as such: left to -ffp-contract the compiler fuses where the
// product and the sum meet in one basic block and not elsewhere, which differs from kernel to kernel.
__device__ __forceinline__ float bn_shift(float b, float m, float s) { return __builtin_fmaf(-m, s, b); }     // b - m*s

// scale and shift of one channel
__device__ __forceinline__ void bn_fold1(const BnVectors &bn, int c, float &s, float &t)
{
    const float m = bn.mean[c], v = bn.var[c];
    const float g = bn.gamma ? bn.gamma[c] : 1.f;
    const float b = bn.beta ? bn.beta[c] : 0.f;
    s = bn_scale(g, v, bn.eps);
    t = bn_shift(b, m, s);
}

// scale and shift of four consecutive channels
__device__ __forceinline__ void bn_fold4(const BnVectors &bn, int c, float4 &s, float4 &t)
{
    const float4 m = *reinterpret_cast<const float4 *>(bn.mean + c);
    const float4 v = *reinterpret_cast<const float4 *>(bn.var + c);
    const float4 g = bn.gamma ? *reinterpret_cast<const float4 *>(bn.gamma + c) : make_float4(1.f, 1.f, 1.f, 1.f);
    const float4 b = bn.beta ? *reinterpret_cast<const float4 *>(bn.beta + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    s = make_float4(bn_scale(g.x, v.x, bn.eps), bn_scale(g.y, v.y, bn.eps), bn_scale(g.z, v.z, bn.eps), bn_scale(g.w, v.w, bn.eps));
    t = make_float4(bn_shift(b.x, m.x, s.x), bn_shift(b.y, m.y, s.y), bn_shift(b.z, m.z, s.z), bn_shift(b.w, m.w, s.w));
}

__device__ __forceinline__ float relu_nan(float z) { return z < 0.f ? 0.f : z; }              // NaN stays NaN

__device__ __forceinline__ float bn_apply(float x, float s, float t) { return __builtin_fmaf(x, s, t); }

// What follows z = bn_apply(x, s, t).  RES 0: no residual; 1: + q; 2: + (q*s2 + t2), t already holding t + t2.
template <int RES, bool RELU>
__device__ __forceinline__ float bn_finish(float z, float q, float s2)
{
    if (RES == 1) z = z + q;
    if (RES == 2) z = __builtin_fmaf(q, s2, z);
    if (RELU) z = relu_nan(z);
    return z;
}

}  // namespace mvdetr

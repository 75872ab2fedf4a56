// The ONE keep decision of attention dropout, shared by the device kernels (attention.hip), the host path and the
// mask-materialising entry point (host_path.cpp): element (b, h, i, j) of the [B, H, Sq, Sk] probabilities is KEPT iff
//   mvdetr_attn_hash(seed, ((b * H + h) * Sq + i) * Sk + j) >= threshold,   threshold = mvdetr_attn_threshold(p) ~ p * 2^32.
// Stateless and counter-based: no generator state on the device, the same mask in the forward and the backward and in every
// work decomposition.  The hash is the splitmix64 finaliser over idx * golden-ratio + seed; its upper 32 bits are compared.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MVDETR_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define MVDETR_HD inline
#endif

MVDETR_HD uint32_t mvdetr_attn_hash(uint64_t seed, uint64_t idx)
{
    uint64_t x = idx * 0x9E3779B97F4A7C15ull + seed;
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return (uint32_t)(x >> 32);
}

// p in [0, 1) -> the 32-bit threshold below which an element is dropped
inline uint32_t mvdetr_attn_threshold(double p)
{
    const double t = p * 4294967296.0;
    return t <= 0.0 ? 0u : (t >= 4294967295.0 ? 4294967295u : (uint32_t)t);
}

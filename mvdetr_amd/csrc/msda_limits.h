// Shape limits of the LDS-tiled MSDA kernels that host-side dispatch needs as well.  Plain C++ (no HIP): the one definition both
// the kernels (through msda_tile.h / msda_backward_sampling.hip) and the route headers (msda_forward_route.h,
// msda_backward_route.h) read.
#pragma once
#include <stdint.h>

namespace mvdetr {

constexpr int TILE_MAX_LEVELS = 16;     // 64-bit miss mask = L * P bits with P == 4
constexpr int TILE_P = 4;
// msda_bwd_sampling_resident: head width, and the levels whose value windows stay in LDS together
constexpr int RS_D = 16, RS_MAXL = 7;

// the LDS-tiled encoder kernels, forward and backward.  queries = tokens of levels [ql0, ql1) (0, L: all, the plain encoder
// call, which needs Lq == S)
inline bool msda_tile_supported(int B, int S, int M, int D, int L, int Lq, int P, bool aligned16, int ql0, int ql1)
{
    if (!aligned16 || P != TILE_P || L > TILE_MAX_LEVELS || B < 1) return false;
    // the LDS-DMA window copies (msda_forward_group.hip, msda_backward_sampling.hip) address one batch element's value
    // tokens through a 32-bit buffer descriptor whose out-of-range sentinel is offset 2^31: a per-batch value tensor of
    // 2 GiB or more would alias it.  Such calls take the gather / lane-group kernels (64-bit addressing).
    if ((int64_t)S * M * D * 4 >= 0x7fffffffLL) return false;
    const bool all_levels = ql0 == 0 && ql1 == L;
    if (ql0 < 0 || ql1 <= ql0 || ql1 > L || (all_levels ? Lq != S : Lq > S)) return false;
    return (D == 16 && M % 2 == 0) || D == 32;
}

// mvdetr_msda_fused_train_supported(): every deformable-encoder shape the LDS-tiled kernels take: up to 16 levels (of equal
// shape: the caller's promise), 16- or 32-channel heads, 4 points, queries = tokens
inline bool msda_fused_train_supported(int B, int S, int M, int D, int L, int Lq, int P)
{
    if (!msda_tile_supported(B, S, M, D, L, Lq, P, true, 0, L)) return false;
    // (the whole raw tensor, all batch elements, in 32-bit float offsets: msda_group_fits; one element's in 2^29 for the backward)
    if ((int64_t)S * M * L * P * 3 >= ((int64_t)1 << 29)) return false;
    return (int64_t)B * S * M * L * P * 3 < ((int64_t)1 << 30);
}

}  // namespace mvdetr

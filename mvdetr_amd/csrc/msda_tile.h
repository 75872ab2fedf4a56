// Shared configuration of the LDS-tiled MSDA kernels (forward: msda_forward_tile.hip, backward:
// msda_backward_*.hip).  Internal, not part of the C ABI.
#pragma once
#include "common.h"
#include "msda_forward_route.h"

namespace mvdetr {

// R_: halo in x (and in y unless RY_ is given).  The LDS-DMA window copies start every window row at a wave-uniform LDS
// base; rows of WW * SLICE * 4 bytes that are not multiples of 512 bytes (WW = 26 at R = 5) fault on gfx950, so a narrower
// halo is only available in y.
template <int D_, int SLICE_, int TH_, int TW_, int R_, int THREADS_ = TH_ * TW_ * 2, int RY_ = R_> struct TileCfg {
    static constexpr int D = D_, TH = TH_, TW = TW_, R = R_, RY = RY_;
    static constexpr int SLICE = SLICE_;              // floats of a token row staged per workgroup (32 = 128 B, 16 = 64 B)
    static constexpr int SUBS = 2;                    // lanes per query, each owning half a slice
    static constexpr int NV = SLICE / SUBS / 4;       // 16-byte chunks (float4 accumulators) per lane
    static constexpr int PARTS = SLICE / 4;           // float4 per token in LDS
    static constexpr int WH = TH + 2 * RY, WW = TW + 2 * R;
    static constexpr int THREADS = THREADS_;          // >= TH*TW*SUBS compute lanes; the surplus only helps the window copy
    static_assert(THREADS_ >= TH_ * TW_ * 2 && THREADS_ % 64 == 0, "whole waves covering the tile");
    static constexpr int COLSLOTS = THREADS / PARTS;  // window columns a copy pass covers ...
    static constexpr int ROWS_PER_PASS = COLSLOTS / WW;   // ... i.e. this many whole rows
    static constexpr int NSTAGE = (WH + ROWS_PER_PASS - 1) / ROWS_PER_PASS;   // float4 per lane per window
    static constexpr int LDS_BYTES = WH * WW * SLICE * 4;
    static constexpr int TOK_PER_BANKROW = 256 / (SLICE * 4);                 // tokens per 256-byte LDS bank row
    // workgroups per CU the LDS admits; the register allocation is capped to match (waves per SIMD)
    static constexpr int WGS_PER_CU = (160 * 1024) / LDS_BYTES;
    static constexpr int WAVES_PER_SIMD = WGS_PER_CU * (THREADS / 64) / 4;
#ifndef MVDETR_TAP_FENCE
#define MVDETR_TAP_FENCE 1
#endif
    static constexpr bool TAP_FENCE = MVDETR_TAP_FENCE;
    static_assert(SLICE == 16 || SLICE == 32, "64- or 128-byte slices");
    static_assert(D % (SLICE / SUBS) == 0, "a lane's channels must lie inside one head");
    static_assert(ROWS_PER_PASS >= 1, "window copy: one pass must cover at least one row");
};

// 128-byte slices: 71.7 KB window, 2 workgroups / CU.  64-byte slices: 35.8 KB, 4 workgroups / CU (twice the
// waves to hide LDS and global latency behind, at the price of duplicating the per-tap address math).
using CfgWide16 = TileCfg<16, 32, 8, 16, 6>;
using CfgWide32 = TileCfg<32, 32, 8, 16, 6>;

// Where element (query, head, level) of the sampling locations / weights starts, in floats:
//     query * q + (head / hps) * s + (head % hps) * h + level * l
// hps > 1 groups the heads whose channels one workgroup stages together (a 128-byte slice of the token row): the
// fused path's slice-interleaved layout keeps everything ONE workgroup reads for a (query, level) -- offsets and
// logits of its hps heads -- in one contiguous run, so that a 128-byte line is not fetched for a quarter of its
// bytes.  Plain layouts have hps = 1, s = h.  Covers the reference layout [.., Lq, M, L, P(, 2)] and the fused path's
// level-major, column-block and slice-interleaved layouts; filled in by the host.
// Reference points: query * r_q + level * r_l (+ 2 * point when there is one per point).
struct SamplingLayout {
    int q_l, h_l, l_l;      // locations (or raw offsets)
    int q_w, h_w, l_w;      // weights (or raw logits)
    int hps, s_l, s_w;      // head grouping (see above)
    int r_q, r_l;           // reference points
    __host__ __device__ int head_l(int head) const { return (head / hps) * s_l + (head % hps) * h_l; }
    __host__ __device__ int head_w(int head) const { return (head / hps) * s_w + (head % hps) * h_w; }
};
inline SamplingLayout plain_layout(int q_l, int h_l, int l_l, int q_w, int h_w, int l_w, int r_q = 0, int r_l = 0)
{
    return SamplingLayout{q_l, h_l, l_l, q_w, h_w, l_w, 1, h_l, h_w, r_q, r_l};
}

// Which levels' tokens are the queries of a call: [begin, end) of the L levels, Lq tokens in all.
struct QueryLevels {
    int begin, end, Lq;
};

// The fused entries' layout bits (msda_forward_route.h) as a SamplingLayout.  q_l, q_w: the query strides of offsets and logits.
inline SamplingLayout fused_layout(int layout, int q_l, int q_w, int M, int D, int L, int Lq)
{
    const int P = TILE_P;
    // reference points: [.., Lq, L, P, 2], [.., Lq, L, 2] (shared_ref) or [.., L, Lq, 2] (shared_ref + ref_level_major)
    const int r_q = msda_fused_ref_query_stride(layout, L);
    const int r_l = (layout & 8) ? Lq * 2 : ((layout & 2) ? 2 : P * 2);
    if (layout & 4) {
        // one tensor [.., Lq, M / hps, L, (hps x P x 2 offsets | hps x P logits)]: what the workgroup of a 128-byte
        // slice reads for a (query, level) is one contiguous run of hps * 12 floats; `logits` = `offsets` + hps * 8
        // Bit 4: the level is the OUTER index, [.., Lq, L, M / hps, run] -- a (query, level)'s runs of all slices are then
        // M / hps * chunk * 4 = 384 contiguous bytes = three whole 128-byte lines (at D = 16, M = 8), shared by the four
        // slice jobs of a tile, which run at the same time on one XCD (one L2); with the slice outermost a run shares its
        // lines with the same slice's NEXT level, i.e. with a later phase of the same job, by when the line has left L2.
        const int hps = 32 / D, chunk = hps * P * 3;
        if (layout & 16) return SamplingLayout{q_l, P * 2, (M / hps) * chunk, q_w, P, (M / hps) * chunk, hps, chunk, chunk, r_q, r_l};
        return SamplingLayout{q_l, P * 2, chunk, q_w, P, chunk, hps, L * chunk, L * chunk, r_q, r_l};
    }
    if (layout & 1) return plain_layout(q_l, P * 2, M * P * 2, q_w, P, M * P, r_q, r_l);              // [.., Lq, L, M, P(, 2)]
    return plain_layout(q_l, L * P * 2, P * 2, q_w, L * P, P, r_q, r_l);                              // [.., Lq, M, L, P(, 2)]
}

// Tile count of one level, recomputed by every workgroup from the device-side shapes (uniform ->
// scalar registers).
template <typename Cfg>
__device__ __forceinline__ int tiles_of_level(const int64_t *shapes, int l)
{
    const int H = (int)shapes[2 * l], W = (int)shapes[2 * l + 1];
    return ((H + Cfg::TH - 1) / Cfg::TH) * ((W + Cfg::TW - 1) / Cfg::TW);
}

}  // namespace mvdetr

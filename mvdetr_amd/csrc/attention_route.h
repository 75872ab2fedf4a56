// Which kernel a fused-attention call runs: the one decision every C ABI entry of attention.hip and attention_half.hip switches
// on, with the limits that both the decision and the kernels need.  Plain C++ (no HIP include), so a host compiler alone can
// print the table (tests/test_attention_route.py).  A call is refused here, before anything is enqueued.
#pragma once
#include "attention_hash.h"
#include <stdint.h>

namespace mvdetr {

constexpr int ATTN_GD = 256;                // largest head dimension of the generic kernels
constexpr int ATTN_TQ = 128;                // queries (or keys, in the dK / dV kernel) per workgroup of the fp32 MFMA kernels
constexpr int64_t ATTN_MAX_GRID = 1 << 20;  // workgroups of the grid-stride kernels (attn_delta and the generic ones)

// B H S rows of one token each (sizes, none negative), saturating
inline int64_t attn_rows(int B, int H, int S)
{
    int64_t n;
    return __builtin_mul_overflow((int64_t)B * H, (int64_t)S, &n) ? INT64_MAX : n;
}

// the C ABI entries: fp32 / fp64 forward and backward, the 16-bit forward
enum class AttnEntry { forward, backward, forward_half };

// One call as the route sees it.  Pointers the entry does not have are ignored.
struct AttnQuery {
    AttnEntry entry;
    int elem_size;                          // 2 (float16 / bfloat16), 4, 8
    int B, H, Sq, Sk, D;
    double dropout_p;                       // (the 16-bit entry has none)
    int forced_tile;                        // mvdetr_attn_half_set_query_tile: 0 (by the shape), 64 or 128
    bool has_strides;
    // every stride the entry tests is a multiple of 4 elements (fp32: 4 tensors forward, 8 backward) or of 8 (16-bit: 12 strides)
    bool strides_ok;
    bool has_q, has_k, has_v, has_out, has_lse;                 // non-null
    bool has_go, has_work, has_gq, has_gk, has_gv;              // the backward's grad_out, workspace, grad_q, grad_k, grad_v
    // every pointer the entry tests is 16-byte aligned (q, k, v, out; the backward: grad_out, q, k, v, grad_q, grad_k, grad_v)
    bool ptrs16;
};

enum class AttnStatus { ok, empty /* success, nothing to launch */, invalid_value, not_supported };

// the kernels of the same names (bwd_mfma: attn_bwd_dq_mfma + attn_bwd_dkv_mfma; bwd_generic: attn_bwd_dq_generic +
// attn_bwd_dkv_generic; both after attn_delta)
enum class AttnKind { fwd_generic, fwd_mfma, fwd_mfma_half, bwd_generic, bwd_mfma };

struct AttnGrid {
    unsigned x, y, z;
};

struct AttnRoute {
    AttnStatus status;
    AttnKind kind;
    const char *name;           // what mvdetr_attention_last_kernel reports from this call on
    int D;                      // the MFMA kernels' instantiation: 16 or 32 (0: a generic kernel)
    bool drop;                  // the dropout instantiation
    int tile;                   // queries per workgroup of the MFMA forwards: 128 (fp32), 64 or 128 (16-bit)
    bool with_dq;               // backward: there are queries, so attn_delta and the dQ kernel run (else dK / dV alone, zeros)
    AttnGrid grid, grid_kv;     // the forward or dQ kernel; the dK / dV kernel
    unsigned grid_delta;        // attn_delta
};

// Oddities of the table, kept as they are: no key (Sk < 1) or no channel (D < 1) is invalid_value in the fp32 / fp64 entries and
// not_supported in the 16-bit one, which also says not_supported before it says empty or looks at a pointer; a backward without
// queries still refuses D > 256 and reports attn_bwd_generic for its one kernel.
inline AttnRoute attn_route(const AttnQuery &q)
{
    using K = AttnKind;
    using S = AttnStatus;
    AttnRoute r{S::ok, K::fwd_generic, nullptr, 0, false, 0, false, {1, 1, 1}, {1, 1, 1}, 0};
    auto refuse = [&r](S s) { r.status = s; return r; };
    auto launch = [&r](K kind, const char *name) { r.kind = kind; r.name = name; return r; };
    auto capped = [](int64_t n, int per) { const int64_t g = n / per + (n % per != 0); return (unsigned)(g < ATTN_MAX_GRID ? g : ATTN_MAX_GRID); };
    auto tiles = [&q](int S_, int tile) { return AttnGrid{(unsigned)(((int64_t)S_ + tile - 1) / tile), (unsigned)q.H, (unsigned)q.B}; };
    const int B = q.B, H = q.H, Sq = q.Sq, Sk = q.Sk, D = q.D;
    const bool mfma_shape = (D == 16 || D == 32) && H <= 65535 && B <= 65535;          // (heads and batch are grid.y and grid.z)

    if (q.entry == AttnEntry::forward_half) {
        if (!q.has_strides || B < 0 || H < 0 || Sq < 0) return refuse(S::invalid_value);
        if (!mfma_shape || Sk < 1 || !q.strides_ok) return refuse(S::not_supported);
        if (attn_rows(B, H, Sq) == 0) return refuse(S::empty);
        if (!q.has_q || !q.has_k || !q.has_v || !q.has_out) return refuse(S::invalid_value);
        if (!q.ptrs16) return refuse(S::not_supported);
        // 128 queries per workgroup unless one 64-query workgroup holds every query
        r.D = D, r.tile = q.forced_tile ? q.forced_tile : Sq <= 64 ? 64 : 128;
        r.grid = tiles(Sq, r.tile);
        return launch(K::fwd_mfma_half, "attn_fwd_mfma_half");
    }

    if (!q.has_strides || B < 0 || H < 0 || Sq < 0 || Sk < 1 || D < 1 || !(q.dropout_p >= 0.0) || !(q.dropout_p < 1.0))
        return refuse(S::invalid_value);
    const int64_t rows = attn_rows(B, H, Sq), krows = attn_rows(B, H, Sk);
    r.drop = mvdetr_attn_threshold(q.dropout_p) != 0;
    // the MFMA route: fp32, D 16 or 32, float4 access to every row, a grid that fits
    const bool fast = q.elem_size == 4 && mfma_shape && q.ptrs16 && q.strides_ok;

    if (q.entry == AttnEntry::forward) {
        if (rows == 0) return refuse(S::empty);
        if (!q.has_q || !q.has_k || !q.has_v || !q.has_out || !q.has_lse) return refuse(S::invalid_value);
        if (fast) {
            r.D = D, r.tile = ATTN_TQ, r.grid = tiles(Sq, ATTN_TQ);
            return launch(K::fwd_mfma, "attn_fwd_mfma");
        }
        if (D > ATTN_GD) return refuse(S::invalid_value);
        r.grid = {capped(rows, 4), 1, 1};
        return launch(K::fwd_generic, "attn_fwd_generic");
    }

    if ((int64_t)B * H == 0) return refuse(S::empty);
    r.with_dq = rows != 0;
    if (!q.has_k || !q.has_v || !q.has_gk || !q.has_gv ||
        (r.with_dq && (!q.has_go || !q.has_q || !q.has_out || !q.has_lse || !q.has_gq || !q.has_work)))
        return refuse(S::invalid_value);
    r.grid_delta = capped(rows, 256);
    if (r.with_dq && fast) {
        r.D = D, r.tile = ATTN_TQ, r.grid = tiles(Sq, ATTN_TQ), r.grid_kv = tiles(Sk, ATTN_TQ);
        return launch(K::bwd_mfma, "attn_bwd_mfma");
    }
    if (D > ATTN_GD) return refuse(S::invalid_value);
    r.grid = {capped(rows, 4), 1, 1}, r.grid_kv = {capped(krows, 4), 1, 1};
    return launch(K::bwd_generic, "attn_bwd_generic");
}

}  // namespace mvdetr

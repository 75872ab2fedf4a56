// Which kernels a multi-scale deformable attention forward runs: the one decision the fp32 / fp64 entries of msda_forward.hip
// switch on.  Plain C++ (no HIP include), so a host compiler alone can print the table (tests/test_msda_forward_route.py).  A
// call is refused here, before anything is enqueued.
#pragma once
#include "msda_limits.h"
#include <stdint.h>
#include <string.h>

namespace mvdetr {

// ---- what the kernels take -------------------------------------------------------------------------------------------------

// the camera-grouped kernels: MVDeTr's camera counts (msda_fwd_group2: 6 / 7, msda_fwd_group: 9..16), unless MVDETR_MSDA_GROUP=0
inline bool msda_group_supported(int D, int L, bool group_enabled)
{
    return group_enabled && (D == 16 || D == 32) && (L == 6 || L == 7 || (L >= 9 && L <= 16));
}

// their per-lane addresses are 32-bit float offsets from per-batch, per-camera bases: one batch element's reference points and
// output must each stay below 2^32 bytes -- and the WHOLE sampling tensors (all B elements), because msda_fwd_group2 folds the
// batch index into the 32-bit scalar offset of one whole-tensor buffer descriptor (per-batch descriptors cost the headline
// instantiation its zero-scratch build: ADVICE r04).  Anything larger runs the tile kernel: 64-bit addresses.
// row: floats of a token (M * D); q_l, q_w, r_q: the query strides of SamplingLayout (msda_tile.h)
inline bool msda_group_fits(int B, int S, int row, int q_l, int q_w, int r_q)
{
    const int64_t lim = (int64_t)1 << 30;                   // floats
    return (int64_t)B * S * q_l < lim && (int64_t)B * S * q_w < lim && (int64_t)S * r_q < lim && (int64_t)S * row < lim;
}

// The fused entries' layout bits: bit 0 level-major raw tensors, bit 1 one reference point per (query, level), bit 2
// slice-interleaved raw tensor (offsets and logits in one run per (query, slice, level); excludes bit 0), bit 3 level-major
// reference points [.., L, Lq, 2] (needs bit 1), bit 4 the slice-interleaved tensor with the LEVEL outermost,
// [.., Lq, L, M/g, run] (needs bit 2)
inline bool msda_fused_layout_valid(int layout)
{
    return !((layout & ~31) || ((layout & 4) && (layout & 1)) || ((layout & 8) && !(layout & 2)) || ((layout & 16) && !(layout & 4)));
}
// reference points: [.., Lq, L, P, 2], [.., Lq, L, 2] (bit 1) or [.., L, Lq, 2] (bits 1 and 3) -- floats from one query to the next
inline int msda_fused_ref_query_stride(int layout, int L)
{
    return (layout & 8) ? 2 : L * ((layout & 2) ? 2 : TILE_P * 2);
}

// ---- the route -------------------------------------------------------------------------------------------------------------

enum class MsdaFwdEntry { public_f32, public_f64, fused, fused_train };

// MVDETR_MSDA_FWD_IMPL / mvdetr_msda_set_forward_impl(); anything else counts as automatic
enum class MsdaFwdKnob { automatic, gather, tile };
inline MsdaFwdKnob msda_forward_parse_knob(const char *e)
{
    if (!e) return MsdaFwdKnob::automatic;
    return !strcmp(e, "gather") ? MsdaFwdKnob::gather : !strcmp(e, "tile") ? MsdaFwdKnob::tile : MsdaFwdKnob::automatic;
}

enum class MsdaFwdStatus { ok, empty /* success, nothing to launch */, invalid_value, not_supported };

// The kernel sequence.  Public entries:
//   gather            msda_fwd_gather<T, gather_vec>
//   tile              [msda_locality_probe ->] msda_fwd_tile<Cfg, 0>
//   group2            msda_fwd_group2<Cfg, L, 0> (stands down job by job under `auto`: no probe)
//   group_many        [msda_locality_probe ->] msda_fwd_group<Cfg, L, .., 0, 4>
// Fused entries (ref_mode 1: a reference point per (query, level, point), 2: per (query, level)):
//   fused_tile        msda_fwd_tile<Cfg, 1|2> [-> msda_softmax_stats_kernel]
//   fused_group2      msda_fwd_group2<Cfg, L, 1|2> (writes the training entry's statistics itself)
//   fused_group_many  msda_fwd_group<Cfg, L, .., 1|2, 4, DMA> (likewise)
// A kernel that takes the probe's verdict runs the gather formulation in the same launch when the taps are far from their cells;
// the grouped kernels run the tile kernel's body in the same launch when the levels' shapes turn out unequal on the device.
enum class MsdaFwdKind { none, gather, tile, group2, group_many, fused_tile, fused_group2, fused_group_many };
inline const char *msda_forward_route_name(MsdaFwdKind k)
{
    static const char *const names[] = {"none", "gather", "tile", "group2", "group-many", "fused-tile", "fused-group2", "fused-group-many"};
    return names[(int)k];
}

struct MsdaFwdRoute {
    MsdaFwdStatus status;
    MsdaFwdKind kind;
    bool probe;             // allocate and launch the locality probe in front of the kernel
    bool standdown;         // GROUP_OPT_STANDDOWN
    bool stats_pass;        // msda_softmax_stats follows the kernel
    int ref_mode;           // the launchers' `fused` template argument: 0 public contract, 1 / 2 see above
    int gather_vec;         // channels per lane of msda_fwd_gather
    int q_l, q_w, r_q;      // query strides of locations / offsets, weights / logits and reference points, in floats
};

// One forward call as the route sees it.  layout, qstride_l / qstride_w (0: dense), ql0 / ql1, logits_follow_offsets and
// want_stats matter to the fused entries only.
struct MsdaFwdQuery {
    MsdaFwdEntry entry;
    int B, S, M, D, L, Lq, P;
    int layout, qstride_l, qstride_w;
    int ql0, ql1;                   // the query levels [ql0, ql1) (public entries: 0, L)
    bool logits_follow_offsets;     // slice-interleaved layouts: `logits` points behind the first slice's offsets in one tensor
    bool all16;                     // every tensor pointer is 16-byte aligned (fused: and ref_bstride a multiple of 2 with one
                                    // reference point per (query, level), of 4 otherwise)
    bool a16;                       // `value` and `out` are
    MsdaFwdKnob knob;
    bool group_enabled;             // MVDETR_MSDA_GROUP is not 0
    bool want_stats;                // the training entry
};

// Oddities of the table, kept as they are: the fused entries have no `empty` status -- B == 0 is not_supported, S == Lq == 0
// with B >= 1 launches over nothing; the knob does not reach the fused entries; the training entry refuses what
// msda_fused_train_supported() does not take before it looks at its strides.
inline MsdaFwdRoute msda_forward_route(const MsdaFwdQuery &c)
{
    using K = MsdaFwdKind;
    auto refuse = [](MsdaFwdStatus s) { return MsdaFwdRoute{s, K::none, false, false, false, 0, 0, 0, 0, 0}; };
    const int B = c.B, S = c.S, M = c.M, D = c.D, L = c.L, Lq = c.Lq, P = c.P;
    const bool bad_dims = B < 0 || S < 0 || M <= 0 || D <= 0 || L <= 0 || Lq < 0 || P <= 0;
    MsdaFwdRoute r = refuse(MsdaFwdStatus::ok);

    if (c.entry == MsdaFwdEntry::public_f32 || c.entry == MsdaFwdEntry::public_f64) {
        if (bad_dims) return refuse(MsdaFwdStatus::invalid_value);
        if ((int64_t)B * Lq == 0) return refuse(MsdaFwdStatus::empty);
        // encoder-shaped fp32 calls have the LDS-window kernels; everything else, and everything under `gather`, the gather
        // kernel: 16-byte accesses (4 floats / 2 doubles per lane) where alignment and head width allow
        if (c.entry == MsdaFwdEntry::public_f64 || c.knob == MsdaFwdKnob::gather || !msda_tile_supported(B, S, M, D, L, Lq, P, c.all16, 0, L)) {
            const int wide = c.entry == MsdaFwdEntry::public_f64 ? 2 : 4;
            r.kind = K::gather;
            r.gather_vec = c.a16 && D % wide == 0 ? wide : 1;
            return r;
        }
        r.q_l = M * L * TILE_P * 2;                                   // [.., Lq, M, L, P, 2]
        r.q_w = M * L * TILE_P;
        // camera-grouped kernel also for the public (unfused) contract: 188 vs 197 us at Wildtrack size -- the
        // reference layout re-touches every sampling_loc line in 4 level iterations, so the gain is small
        const bool grouped = msda_group_supported(D, L, c.group_enabled) && msda_group_fits(B, S, M * D, r.q_l, r.q_w, r.r_q);
        r.kind = !grouped ? K::tile : L <= 7 ? K::group2 : K::group_many;
        // `auto`: a device-side probe (stream-ordered scratch, no host sync) tells the kernel whether the sampling locations are
        // near the queries' cells; if not, the same launch runs the gather formulation.  A forced `tile` skips the probe (the
        // kernel is then measured as it is).  msda_fwd_group2 looks at every tile's own taps and stands down job by job instead:
        // no probe kernel, no scratch allocation in front of the forward
        r.probe = c.knob == MsdaFwdKnob::automatic && r.kind != K::group2;
        r.standdown = c.knob == MsdaFwdKnob::automatic && grouped;
        return r;
    }

    if (c.entry == MsdaFwdEntry::fused_train && !msda_fused_train_supported(B, S, M, D, L, Lq, P)) return refuse(MsdaFwdStatus::not_supported);
    const int dense_l = M * L * P * 2, dense_w = M * L * P;
    r.q_l = c.qstride_l ? c.qstride_l : dense_l;
    r.q_w = c.qstride_w ? c.qstride_w : dense_w;
    if (r.q_l < dense_l || r.q_w < dense_w || r.q_l % 4 || r.q_w % 4) return refuse(MsdaFwdStatus::invalid_value);
    if (bad_dims) return refuse(MsdaFwdStatus::invalid_value);
    if (c.ql0 < 0 || c.ql1 <= c.ql0 || c.ql1 > L) return refuse(MsdaFwdStatus::invalid_value);
    if (!msda_fused_layout_valid(c.layout)) return refuse(MsdaFwdStatus::invalid_value);
    // slice-interleaved: the two pointers address one tensor, the logits start behind the slice's offsets
    if ((c.layout & 4) && ((D != 16 && D != 32) || !c.logits_follow_offsets || r.q_l != r.q_w || r.q_l < dense_l + dense_w))
        return refuse(MsdaFwdStatus::invalid_value);
    if (!msda_tile_supported(B, S, M, D, L, Lq, P, c.all16, c.ql0, c.ql1)) return refuse(MsdaFwdStatus::not_supported);
    r.r_q = msda_fused_ref_query_stride(c.layout, L);
    r.ref_mode = (c.layout & 2) ? 2 : 1;
    // MVDeTr's camera counts: the camera-grouped kernels.  A query-sharded call (a rank's own cameras as queries,
    // mvdetr_amd/dist.py) has too few query levels per window to amortise the grouped staging and runs the tile kernel.
    const bool grouped = c.ql0 == 0 && c.ql1 == L && msda_group_supported(D, L, c.group_enabled) && msda_group_fits(B, S, M * D, r.q_l, r.q_w, r.r_q);
    r.kind = !grouped ? K::fused_tile : L <= 7 ? K::fused_group2 : K::fused_group_many;
    // the training entry's statistics: the camera-grouped kernels write them themselves; the tile kernel runs as it does for
    // inference and a small pass over the logits follows
    r.stats_pass = c.want_stats && !grouped;
    return r;
}

}  // namespace mvdetr

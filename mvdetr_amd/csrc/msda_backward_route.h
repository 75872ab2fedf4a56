// Which kernels a multi-scale deformable attention backward runs: the one decision both entries of msda_backward.hip switch on.
// Plain C++ (no HIP include), so a host compiler alone can print the table (tests/test_msda_backward_route.py).  A call is
// refused here, before anything is enqueued.
#pragma once
#include "msda_limits.h"
#include <stdint.h>
#include <string.h>

namespace mvdetr {

// ---- what the kernels take -------------------------------------------------------------------------------------------------

// msda_bwd_value_tok addresses one batch element's tensors with 32-bit byte offsets (q_floats: floats of one query's locations,
// or the fused entry's raw query stride): larger calls keep the generic kernel
inline bool msda_backward_value_tok_fits(int S, int M, int D, int64_t q_floats)
{
    const int64_t lim = (int64_t)1 << 32;
    return (D == 16 || D == 32) && (int64_t)S * q_floats * 4 < lim && (int64_t)S * M * D * 4 < lim;
}

// msda_bwd_onepass: 16-channel heads; one batch element's tensors addressed with 32-bit byte offsets
inline bool msda_backward_onepass_supported(int S, int M, int D, int L, int64_t q_floats)
{
    const int64_t lim = (int64_t)1 << 31;
    return D == 16 && L <= TILE_MAX_LEVELS && (int64_t)S * M * D * 4 < lim && (int64_t)S * q_floats * 4 < lim;
}

// msda_bwd_onepass<DET> (an element's sum stays below 2^38 x the taps that can land on it: 2^24 of them leave a factor two to int64)
inline bool msda_backward_deterministic_supported(int S, int M, int D, int L, int64_t q_floats)
{
    return msda_backward_onepass_supported(S, M, D, L, q_floats) && (int64_t)S * L * TILE_P < ((int64_t)1 << 24);
}

// ---- the route -------------------------------------------------------------------------------------------------------------

enum class MsdaBwdEntry { public_f32, public_f64, fused };

// MVDETR_MSDA_BWD_IMPL; anything else counts as unset
enum class MsdaBwdKnob { unset, twopass, split, onepass, atomic };
inline MsdaBwdKnob msda_backward_parse_knob(const char *e)
{
    if (!e) return MsdaBwdKnob::unset;
    return !strcmp(e, "twopass") ? MsdaBwdKnob::twopass : !strcmp(e, "split") ? MsdaBwdKnob::split
         : !strcmp(e, "onepass") ? MsdaBwdKnob::onepass : !strcmp(e, "atomic") ? MsdaBwdKnob::atomic : MsdaBwdKnob::unset;
}

enum class MsdaBwdStatus { ok, empty /* success, nothing to launch */, invalid_value, not_supported };

// The kernel sequence.  Public entry:
//   twopass        msda_locality_probe -> msda_bwd_value_tok<D> -> sampling kernel (with the probe's verdict)
//   split          msda_bwd_onepass<DOTS = 0> (stand-down on) -> sampling kernel (no probe)
//   onepass        msda_bwd_onepass<DOTS = 1> (stand-down on)
//   atomic         msda_bwd_lanes<T, lanes_vec, lanes_g>, or msda_bwd_serial<T> when lanes_g == 0
//   deterministic  msda_det_absmax -> msda_bwd_onepass<DET> -> msda_det_finish
// Fused entry:
//   fused_split    msda_bwd_onepass<fused, DOTS = 0> -> msda_bwd_fused_sampling<NG = L>
//   fused_twopass  msda_bwd_value_tok<16, fused> -> msda_bwd_fused_sampling<NG = L>
//   fused_onepass  msda_bwd_onepass<fused>
//   fused_groups   msda_bwd_value_tok<32, fused> -> msda_bwd_sampling_groups<32, 3, fused>
//   fused_deterministic  as deterministic, on the raw tensor
enum class MsdaBwdKind {
    none, twopass, split, onepass, atomic, deterministic, fused_split, fused_twopass, fused_onepass, fused_groups, fused_deterministic
};
inline const char *msda_backward_route_name(MsdaBwdKind k)
{
    static const char *const names[] = {"none", "twopass", "split", "onepass", "atomic", "deterministic", "fused-split",
                                        "fused-twopass", "fused-onepass", "fused-groups", "fused-deterministic"};
    return names[(int)k];
}

// the sampling kernel of a two-kernel route: msda_bwd_sampling_resident (16-channel heads, up to RS_MAXL levels),
// msda_bwd_sampling_groups<16, 7> / <32, 3> (more levels, 32-channel heads), msda_bwd_fused_sampling
enum class MsdaBwdSampling { none, resident, groups, fused };

struct MsdaBwdRoute {
    MsdaBwdStatus status;
    MsdaBwdKind kind;
    MsdaBwdSampling sampling;
    int lanes_vec, lanes_g;
};

// all16: every tensor pointer of the call is 16-byte aligned (fused entry: also reference points and statistics 8-byte aligned
// and an even ref_bstride); a16: `value` and `grad_out` are.  raw_q: the fused entry's raw query stride (public entries: 0).
inline MsdaBwdRoute msda_backward_route(MsdaBwdEntry entry, int B, int S, int M, int D, int L, int Lq, int P, int raw_q, bool all16,
                                        bool a16, MsdaBwdKnob knob, bool deterministic)
{
    using K = MsdaBwdKind;
    using Smp = MsdaBwdSampling;
    auto refuse = [](MsdaBwdStatus s) { return MsdaBwdRoute{s, K::none, Smp::none, 0, 0}; };
    auto route = [](K k, Smp s = Smp::none) { return MsdaBwdRoute{MsdaBwdStatus::ok, k, s, 0, 0}; };
    if (B < 0 || S < 0 || M <= 0 || D <= 0 || L <= 0 || Lq < 0 || P <= 0) return refuse(MsdaBwdStatus::invalid_value);
    if ((int64_t)B * Lq == 0) return refuse(MsdaBwdStatus::empty);

    if (entry == MsdaBwdEntry::fused) {
        if (!msda_fused_train_supported(B, S, M, D, L, S, P)) return refuse(MsdaBwdStatus::not_supported);
        if (raw_q < M * L * P * 3 || raw_q % 4) return refuse(MsdaBwdStatus::invalid_value);
        // the kernels address one batch element's raw tensor (and its gradient) with 32-bit offsets of the CALLER's query stride,
        // which may be wider than the dense width msda_fused_train_supported() bounds (a column block of a wider GEMM)
        if ((int64_t)S * raw_q >= ((int64_t)1 << 29)) return refuse(MsdaBwdStatus::not_supported);
        if (!all16) return refuse(MsdaBwdStatus::not_supported);
        // (the checks above imply msda_backward_onepass_supported() for 16-channel heads and msda_backward_value_tok_fits() for all)
        if (deterministic)
            return msda_backward_deterministic_supported(S, M, D, L, raw_q) ? route(K::fused_deterministic) : refuse(MsdaBwdStatus::not_supported);
        // 32-channel heads: msda_bwd_value_tok<32, fused> + the level-groups sampling kernel on the raw tensor
        if (D != 16) return route(K::fused_groups, Smp::groups);
        // 16-channel heads: 6 / 7 levels (MVDeTr's own) have msda_bwd_fused_sampling; every other level count the one-pass kernel.
        // Measured (profiles/r06_bwd_ab.txt): Wildtrack 549 us split, 564 twopass, 706 onepass; MultiviewX 386 / 404 / 493.
        if (knob == MsdaBwdKnob::onepass || (L != 6 && L != 7)) return route(K::fused_onepass);
        return route(knob == MsdaBwdKnob::twopass ? K::fused_twopass : K::fused_split, Smp::fused);
    }

    if (entry == MsdaBwdEntry::public_f64 && deterministic) return refuse(MsdaBwdStatus::not_supported);
    // Encoder-shaped fp32 calls (the shapes the forward tile kernels take) have the LDS-window kernels; `atomic` keeps everything
    // on the direct-atomics kernel.  The default is the measured one (profiles/r06_bwd_ab.txt, realistic / uniform input):
    // Wildtrack 625 / 3,383 us twopass, 642 / 3,607 split, 671 / 3,960 onepass; MultiviewX 458 / 2,316, 458 / 2,360, 506 / 2,527
    // -- round 5 had made `split` the default to save the 6-us probe launch; it moves 2.4 x the bytes and is not faster.
    if (entry == MsdaBwdEntry::public_f32) {
        const int64_t q_floats = (int64_t)M * L * P * 2;
        const bool tile_shapes = knob != MsdaBwdKnob::atomic && msda_tile_supported(B, S, M, D, L, Lq, P, all16, 0, L);
        const bool op_ok = tile_shapes && msda_backward_onepass_supported(S, M, D, L, q_floats);
        // (tile_shapes bounds the value tensor of a batch element below 2^31 bytes, which the resident kernel needs)
        const Smp smp = D == RS_D && L <= RS_MAXL ? Smp::resident : Smp::groups;
        // one kernel does the deterministic mode; calls it does not take are refused, not served by a kernel that is not
        if (deterministic)
            return tile_shapes && msda_backward_deterministic_supported(S, M, D, L, q_floats) ? route(K::deterministic)
                                                                                              : refuse(MsdaBwdStatus::not_supported);
        if (op_ok && knob == MsdaBwdKnob::onepass) return route(K::onepass);
        if (op_ok && knob == MsdaBwdKnob::split) return route(K::split, smp);
        if (tile_shapes && msda_backward_value_tok_fits(S, M, D, q_floats)) return route(K::twopass, smp);
    }
    // One channel per lane (G = D lanes per head): a wave's atomic instruction then covers whole 4*D-byte head segments, which
    // the memory-side atomic units take as ONE request each, instead of four partial ones with 16-byte-per-lane vectors
    // (measured at Wildtrack size: 3.15 ms vs 12.7 ms -- the kernel is bound by atomic requests, ~21 G/s, not by bytes).
    MsdaBwdRoute r = route(K::atomic);
    const int wide = entry == MsdaBwdEntry::public_f64 ? 2 : 4;
    auto pow2_to_64 = [](int g) { return g >= 1 && g <= 64 && (g & (g - 1)) == 0; };
    if (pow2_to_64(D)) { r.lanes_vec = 1; r.lanes_g = D; }
    else if (a16 && D % wide == 0 && pow2_to_64(D / wide)) { r.lanes_vec = wide; r.lanes_g = D / wide; }
    return r;
}

}  // namespace mvdetr

// Which kernel a perspective-warp call runs: the one decision every C ABI entry of warp_perspective.hip switches on, with the
// tile constants, the gather backward's plan layout and its shape limits that both the decision and the kernels need.  Plain
// C++ (no HIP include), so a host compiler alone can print the table (tests/test_warp_route.py).  A call is refused here, before
// anything is enqueued.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

namespace mvdetr {

// ---- what the kernels take -------------------------------------------------------------------------------------------------

constexpr int WARP_PIX = 64;      // pixels per block (one per lane)
constexpr int WARP_CH = 64;       // channels per block
constexpr int WARP_SUB = 4;       // waves per block; each owns WARP_CH / WARP_SUB channels

// Block id -> (view, 8x8 destination tile, channel group).  The world grid is not aligned with the image
// axes (a ground-plane row is a slanted, perspective-foreshortened line in the camera image), so 64
// consecutive pixels of one destination ROW gather from ~30 different source cache lines per load
// instruction (measured: 66 M L1 accesses per launch, i.e. the kernel ran at the texture-address rate, and
// neither fewer bytes nor a different XCD assignment changed its 100 us).  An 8x8 destination tile maps to
// a compact source patch instead: a handful of lines per load.
// (round 4 re-measured the tile shape at Wildtrack size, NCHW -> NCHW: 8 x 8 90 us, 4 x 16 102, 2 x 32 105, 16 x 4 149)
constexpr int WARP_TW = 8, WARP_TH = 8;
static_assert(WARP_TW * WARP_TH == WARP_PIX, "one lane per tile pixel");

// warp_fwd_nchw_patch (warp_forward.hip): destination tile, channels per workgroup, LDS floats
#ifndef MVDETR_WARP_PP_CH
#define MVDETR_WARP_PP_CH 32
#endif
#ifndef MVDETR_WARP_PP_FLOATS
#define MVDETR_WARP_PP_FLOATS 8192          // 32 KB of LDS: 5 workgroups per CU
#endif
constexpr int WARP_PP_TH = 8, WARP_PP_TW = 32, WARP_PP_CH = MVDETR_WARP_PP_CH, WARP_PP_FLOATS = MVDETR_WARP_PP_FLOATS;
static_assert(WARP_PP_TH * WARP_PP_TW == 256, "one lane per tile pixel, four waves");

constexpr int WARP_CL_THREADS = 256;        // the channel-last kernels
// warp_fwd_cl_nchw: destination tile = 2 rows x 32 columns; channels in groups of 128
constexpr int WARP_NC_TW = 32, WARP_NC_TH = 2, WARP_NC_CG = 128, WARP_NC_LD = WARP_NC_CG + 4;

constexpr int WARP_SCAN_THREADS = 64;
constexpr int WARP_ODD_SEGS = 1024;     // workgroups (= list segments) that look for pixels kornia does not divide
constexpr int WARP_HEAVY = 128;         // blocks with more candidates than this get a whole workgroup
constexpr int WARP_HEAVY_WGS = 2048;

constexpr int64_t WARP_INT_MAX = 0x7fffffffLL;     // grids, and the element offsets the channel-last kernels keep in an int

// a product of sizes (none negative), saturating: every caller compares it with a limit far below
inline int64_t warp_prod(int64_t a, int64_t b, int64_t c = 1, int64_t d = 1)
{
    int64_t p;
    if (__builtin_mul_overflow(a, b, &p) || __builtin_mul_overflow(p, c, &p) || __builtin_mul_overflow(p, d, &p)) return INT64_MAX;
    return p;
}
inline int64_t warp_tiles(int size, int tile) { return ((int64_t)size + tile - 1) / tile; }

inline int64_t warp_grid(int N, int H, int W, int groups)
{
    return warp_prod(N, warp_tiles(H, WARP_TH), warp_tiles(W, WARP_TW), groups);
}

// ---- the gather backward's plan ---------------------------------------------------------------------------------------------

struct WarpScan {
    int u0, u1;                  // lines u0..u1 (inclusive); empty when u1 < u0
    int len;                     // candidates per line
    int swap;                    // 0: lines are destination rows (u = i, v = j); 1: lines are columns (u = j, v = i)
    double a, s, uc;             // line u starts at v = ceil(a + s * (u - uc))
};

// Layout of the gather backward's geometry ("plan"): [counts: heavy, odd, odd per segment | scans: 2 per 2 x 2 block | heavy-
// block list | odd-pixel list].  It depends on the matrices and the shapes only, not on the gradient.
struct WarpPlanLayout {
    size_t count_bytes, scan_bytes, heavy_bytes, odd_bytes;
    int64_t nblk, npix;
    size_t total() const { return count_bytes + scan_bytes + heavy_bytes + odd_bytes; }
};
inline WarpPlanLayout warp_plan_layout(int N, int h, int w, int H, int W)
{
    WarpPlanLayout L;
    L.nblk = warp_prod(N, warp_tiles(h, 2), warp_tiles(w, 2));
    L.npix = warp_prod(N, H, W);
    L.count_bytes = ((2 + WARP_ODD_SEGS) * sizeof(int) + 15) / 16 * 16;
    L.scan_bytes = (size_t)L.nblk * 2 * sizeof(WarpScan);
    L.heavy_bytes = ((size_t)L.nblk * sizeof(int) + 15) / 16 * 16;
    const int64_t odd_per = (L.npix + WARP_ODD_SEGS - 1) / WARP_ODD_SEGS;
    L.odd_bytes = (size_t)odd_per * WARP_ODD_SEGS * sizeof(int);
    return L;
}

// the four sections of a plan buffer: what the geometry pass writes and the gather reads
struct WarpPlanParts {
    int *counts;
    WarpScan *scans;
    int *heavy_list, *odd_list;
};
inline WarpPlanParts warp_plan_parts(char *plan, const WarpPlanLayout &L)
{
    char *const scans = plan + L.count_bytes, *const heavy = scans + L.scan_bytes;
    return {reinterpret_cast<int *>(plan), reinterpret_cast<WarpScan *>(scans), reinterpret_cast<int *>(heavy),
            reinterpret_cast<int *>(heavy + L.heavy_bytes)};
}

// does the gather take these shapes?  (lgG / cgroups: lanes per hit stream, channel groups per block; wgs: its light workgroups)
inline bool warp_gather_shapes(int elem_size, int N, int C, int h, int w, int H, int W, int &lgG, int &cgroups, int64_t &wgs)
{
    const int VEC = 16 / elem_size;
    if (C <= 0 || C % VEC) return false;
    const int chunks = C / VEC;
    lgG = 0;
    while ((1 << lgG) < chunks && lgG < 6) ++lgG;
    const int G = 1 << lgG;
    cgroups = (chunks + G - 1) / G;
    const int64_t items = warp_prod(N, warp_tiles(h, 2), warp_tiles(w, 2), cgroups);       // (2 x 2 block, channel group)
    wgs = items / 4 + (items % 4 != 0);
    return wgs <= WARP_INT_MAX && warp_prod(N, H, W, C) <= WARP_INT_MAX;
}

// ---- the route -------------------------------------------------------------------------------------------------------------

// the C ABI entries: fp32 / fp64 forward and backward (the tagged backward included), the 16-bit forward, and the two-step
// gradient's mvdetr_warp_backward_plan_bytes, mvdetr_warp_backward_plan_* and mvdetr_warp_perspective_backward_planned_*
enum class WarpEntry { forward, backward, forward_half, plan_bytes, plan, planned };

// The environment knobs.  Anything but the words below counts as unset.
struct WarpKnobs {
    bool scatter;           // MVDETR_WARP_BWD_IMPL=scatter: the atomic kernels, kept for comparison (default: the gather)
    bool force_clip;        // MVDETR_WARP_BWD_GEOMETRY=clip: the clipping path for every block (a test knob)
    bool heavy_set;         // MVDETR_WARP_BWD_HEAVY is set ...
    int heavy_above;        // ... to this many candidates (0: every block with candidates is "heavy"); default WARP_HEAVY
    int heavy_wgs;          // MVDETR_WARP_BWD_HEAVY_WGS (at least 1); default WARP_HEAVY_WGS
    bool fwd_nchw_gather;   // MVDETR_WARP_FWD_NCHW=gather: warp_fwd<NCHW> where warp_fwd_nchw_patch would run
    // what a plan's contents depend on, as the scratch cache keys it
    int64_t plan_key() const { return (int64_t)force_clip | ((heavy_set ? (int64_t)heavy_above + 1 : 0) * 256); }
};
inline WarpKnobs warp_parse_knobs(const char *bwd_impl, const char *bwd_geometry, const char *bwd_heavy, const char *bwd_heavy_wgs,
                                  const char *fwd_nchw)
{
    WarpKnobs k;
    k.scatter = bwd_impl && !strcmp(bwd_impl, "scatter");
    k.force_clip = bwd_geometry && !strcmp(bwd_geometry, "clip");
    k.heavy_set = bwd_heavy != nullptr;
    k.heavy_above = bwd_heavy ? atoi(bwd_heavy) : WARP_HEAVY;
    k.heavy_wgs = bwd_heavy_wgs ? (atoi(bwd_heavy_wgs) > 0 ? atoi(bwd_heavy_wgs) : 1) : WARP_HEAVY_WGS;
    k.fwd_nchw_gather = fwd_nchw && !strcmp(fwd_nchw, "gather");
    return k;
}

// One call as the route sees it.  `in` is the source (forward) or grad_dst (backward, planned), `out` the destination or
// grad_src; the plan-bytes entry has no pointers, the plan entry no `in` / `out`.
struct WarpQuery {
    WarpEntry entry;
    int elem_size;                          // 2 (float16 / bfloat16), 4, 8; the plan-bytes entry passes its caller's number on
    int N, C, h, w, H, W;
    int layout_nhwc;                        // as the caller gave it: bit 0 destination, bit 1 source channel-last, bit 2 nearest
    bool has_in, has_M, has_out, has_plan;  // non-null
    bool in16, out16, plan16;               // 16-byte aligned
    WarpKnobs knobs;
};

enum class WarpStatus { ok, empty /* success, nothing to launch */, invalid_value, not_supported };

// none: success without a launch (a backward whose grad_src has no elements); zero_fill: grad_src is zeroed and nothing else
// runs (a backward without destination pixels); plan: the geometry pass warp_bwd_scans (the plan-bytes entry: nothing runs, the
// route carries the answer); the others are the kernels of warp_forward.hip and warp_backward.hip of the same names.
enum class WarpKind { none, zero_fill, fwd, fwd_nchw_patch, fwd_cl, fwd_cl_nchw, fwd_half, fwd_cl_half, bwd, bwd_cl, bwd_gather, plan };

struct WarpRoute {
    WarpStatus status;
    WarpKind kind;
    const char *name;           // what mvdetr_warp_last_kernel reports from this call on; null: left as it is
    bool src_nhwc, dst_nhwc;    // the decoded layout bits
    int nearest;
    bool zero_first;            // grad_src is zeroed in front of the kernel (the scatter kernels add into it)
    int64_t grid;               // workgroups of the kernel (<= WARP_INT_MAX; the gather: wgs + heavy_wgs, below 2^32)
    int lgG, cgroups;           // the gather's lanes per hit stream (log2), channel groups per block ...
    int64_t wgs;                // ... and light workgroups
    int64_t plan_bytes;         // the gather and the plan kinds: size of the plan
};

// Oddities of the table, kept as they are: the 16-bit entry alone refuses h * w beyond an int; a channel-last source that is
// misaligned or has a partial 16-byte chunk is not_supported in the fp32 / fp64 entries but runs warp_fwd_half in the 16-bit
// one; MVDETR_WARP_FWD_NCHW=gather also keeps the patch kernel's size conditions from mattering; the plan entries answer
// not_supported for non-positive sizes where the others answer invalid_value or empty, and look at their pointers first; the
// planned entry does not look at the plan's alignment.
inline WarpRoute warp_route(const WarpQuery &q)
{
    using K = WarpKind;
    using S = WarpStatus;
    const int N = q.N, C = q.C, h = q.h, w = q.w, H = q.H, W = q.W, elem = q.elem_size;
    WarpRoute r{S::ok, K::none, nullptr, (q.layout_nhwc & 2) != 0, (q.layout_nhwc & 1) != 0, (q.layout_nhwc >> 2) & 1, false, 0, 0, 0, 0, 0};
    auto refuse = [&r](S s) { r.status = s; return r; };
    auto launch = [&r](K kind, const char *name, int64_t grid) {
        if (grid > WARP_INT_MAX) { r.status = S::invalid_value; return r; }
        r.kind = kind; r.name = name; r.grid = grid;
        return r;
    };
    auto gather = [&](const char *name) {
        r.kind = K::bwd_gather; r.name = name; r.grid = r.wgs + q.knobs.heavy_wgs;
        r.plan_bytes = (int64_t)warp_plan_layout(N, h, w, H, W).total();
        return r;
    };
    // what the two-step gradient takes: positive sizes, shapes the gather takes, the gather not switched off
    auto plannable = [&] {
        return N > 0 && C > 0 && h > 0 && w > 0 && H > 0 && W > 0 && (elem == 4 || elem == 8) &&
               warp_gather_shapes(elem, N, C, h, w, H, W, r.lgG, r.cgroups, r.wgs) && warp_prod(h, w, C) <= WARP_INT_MAX && !q.knobs.scatter;
    };

    switch (q.entry) {
    case WarpEntry::plan_bytes:
        if (!plannable()) return refuse(S::not_supported);
        r.kind = K::plan; r.plan_bytes = (int64_t)warp_plan_layout(N, h, w, H, W).total();
        return r;
    case WarpEntry::plan:
        if (!q.has_M || !q.has_plan || !q.plan16) return refuse(S::invalid_value);
        if (!plannable()) return refuse(S::not_supported);
        r.kind = K::plan; r.plan_bytes = (int64_t)warp_plan_layout(N, h, w, H, W).total();
        return r;
    case WarpEntry::planned:
        // channel-last on both sides (bits 0 and 1), bilinear or nearest (bit 2): the layouts the gather exists for
        if ((q.layout_nhwc & ~7) || (q.layout_nhwc & 3) != 3 || !q.has_in || !q.has_M || !q.has_plan || !q.has_out) return refuse(S::invalid_value);
        if (!plannable() || !q.in16 || !q.out16) return refuse(S::not_supported);
        return gather("warp_bwd_gather[planned]");
    default:
        break;
    }

    if (N < 0 || C < 0 || h <= 0 || w <= 0 || H < 0 || W < 0) return refuse(S::invalid_value);
    if (q.layout_nhwc & ~7) return refuse(S::invalid_value);
    const int64_t npix = warp_prod(N, H, W);
    if (q.entry == WarpEntry::backward) {
        // grad_src is OVERWRITTEN: the gather stores every element, the scatter kernels start from zeros
        if (warp_prod(N, C, h, w) == 0) return r;
        if (!q.has_out) return refuse(S::invalid_value);
        if (npix == 0) { r.kind = K::zero_fill; return r; }
    }
    if (npix == 0 || C == 0) return refuse(S::empty);
    if (!q.has_in || !q.has_M || !q.has_out) return refuse(S::invalid_value);
    const bool aligned16 = q.in16 && q.out16;
    const int64_t grid_cl = warp_grid(N, H, W, 1), grid_nchw = warp_grid(N, H, W, (C + WARP_CH - 1) / WARP_CH);

    if (q.entry == WarpEntry::forward_half) {
        if (warp_prod(h, w) > WARP_INT_MAX) return refuse(S::invalid_value);             // (a texel offset is an int)
        if (r.src_nhwc && r.dst_nhwc && C % 8 == 0 && aligned16 && warp_prod(h, w, C) <= WARP_INT_MAX)
            return launch(K::fwd_cl_half, "warp_fwd_cl_half", grid_cl);
        return launch(K::fwd_half, "warp_fwd_half", grid_nchw);
    }

    const bool backward = q.entry == WarpEntry::backward;
    if (r.src_nhwc) {
        // channel-last source: implemented for whole 16-byte chunks per pixel and a view that fits 32-bit element offsets
        if (C % (16 / elem) || !aligned16 || warp_prod(h, w, C) > WARP_INT_MAX) return refuse(S::not_supported);
        if (!r.dst_nhwc) {
            // channel-last source, NCHW destination: forward, fp32 only
            if (elem != 4 || backward) return refuse(S::not_supported);
            return launch(K::fwd_cl_nchw, "warp_fwd_cl_nchw", warp_prod(N, warp_tiles(H, WARP_NC_TH), warp_tiles(W, WARP_NC_TW)));
        }
        if (grid_cl > WARP_INT_MAX) return refuse(S::invalid_value);
        if (!backward) return launch(K::fwd_cl, "warp_fwd_cl", grid_cl);
        // the gather, unless it is switched off or does not take the shapes: then the atomic kernel
        if (!q.knobs.scatter && warp_gather_shapes(elem, N, C, h, w, H, W, r.lgG, r.cgroups, r.wgs)) return gather("warp_bwd_gather");
        r.lgG = r.cgroups = 0, r.wgs = 0;
        r.zero_first = true;
        return launch(K::bwd_cl, "warp_bwd_cl", grid_cl);
    }
    if (grid_nchw > WARP_INT_MAX) return refuse(S::invalid_value);
    if (backward) {
        r.zero_first = true;
        return launch(K::bwd, r.dst_nhwc ? "warp_bwd<NHWC>" : "warp_bwd<NCHW>", grid_nchw);
    }
    // NCHW source: 8x8-tile gather kernel for both destination layouts (91 us / 28 % at Wildtrack size for NCHW -> NCHW, the
    // literal layouts of the kornia call).  fp32 NCHW -> NCHW: LDS source patches where whole 16-byte row pieces can be copied
    // (rows of a multiple of 4 texels, aligned base, a view below 2 GiB)
    if (elem == 4 && !r.dst_nhwc && !q.knobs.fwd_nchw_gather && w % 4 == 0 && q.in16 && warp_prod(C, h, w, 4) < WARP_INT_MAX) {
        const int64_t pb = warp_prod(N, warp_tiles(H, WARP_PP_TH), warp_tiles(W, WARP_PP_TW), warp_tiles(C, WARP_PP_CH));
        if (pb <= WARP_INT_MAX) return launch(K::fwd_nchw_patch, "warp_fwd_nchw_patch", pb);
    }
    return launch(K::fwd, r.dst_nhwc ? "warp_fwd<NHWC>" : "warp_fwd<NCHW>", grid_nchw);
}

}  // namespace mvdetr

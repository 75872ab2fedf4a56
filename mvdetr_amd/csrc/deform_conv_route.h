// Which kernel a deformable-convolution call runs: the one decision every C ABI entry of deform_conv.hip and
// deform_conv_half.hip switches on, with the call's shape and the tile constants that both the decision and the kernels need.
// Plain C++ (no HIP include), so a host compiler alone can print the table (tests/test_deform_conv_route.py).  A call is refused
// here, before anything is enqueued.
#pragma once
#include <stdint.h>

namespace mvdetr {

// ---- what the kernels take -------------------------------------------------------------------------------------------------

struct DcShape {
    int B, C, H, W, Co, Ho, Wo, kh, kw, sh, sw, ph, pw, dh, dw, G;
};

constexpr int DC_TP = 64;       // output pixels per forward / g_col workgroup
constexpr int DC_TO = 128;      // output (forward) or input (g_col) channels per workgroup: 4 waves x 32 rows
constexpr int DC_WP = 32;       // pixels per K chunk of dc_bwd_weight_mfma

// a product of sizes (none negative), saturating: every caller compares it with a limit far below
inline int64_t dc_prod(int64_t a, int64_t b, int64_t c = 1, int64_t d = 1)
{
    int64_t p;
    if (__builtin_mul_overflow(a, b, &p) || __builtin_mul_overflow(p, c, &p) || __builtin_mul_overflow(p, d, &p)) return INT64_MAX;
    return p;
}

inline bool dc_shape(int B, int C, int H, int W, int Co, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int G,
                     DcShape &s)
{
    if (B < 0 || C < 0 || H < 1 || W < 1 || Co < 0 || kh < 1 || kw < 1 || sh < 1 || sw < 1 || ph < 0 || pw < 0 || dh < 1 ||
        dw < 1 || G < 1 || C % G != 0)
        return false;
    // (in 64 bits, so that a huge padding or kernel extent is refused and not wrapped)
    const int64_t eh = (int64_t)H + 2 * (int64_t)ph - (int64_t)dh * (kh - 1) - 1, ew = (int64_t)W + 2 * (int64_t)pw - (int64_t)dw * (kw - 1) - 1;
    if (eh < 0 || ew < 0) return false;
    const int64_t Ho = eh / sh + 1, Wo = ew / sw + 1, lim = 1ll << 31;
    if (Ho >= lim || Wo >= lim) return false;              // (an empty batch reaches here with any map size)
    if (dc_prod(B, C, H, W) >= lim || dc_prod(B, Co, Ho, Wo) >= lim || dc_prod(dc_prod(2 * (int64_t)B, G, kh, kw), Ho, Wo) >= lim)
        return false;
    s = DcShape{B, C, H, W, Co, (int)Ho, (int)Wo, kh, kw, sh, sw, ph, pw, dh, dw, G};
    return true;
}

// ---- the route -------------------------------------------------------------------------------------------------------------

// the C ABI entries: fp32 / fp64 forward and backward, the 16-bit forward
enum class DcEntry { forward, backward, forward_half };

// One call as the route sees it.  Pointers the entry does not have (grad_* in the forwards, out in the backward) are ignored.
struct DcQuery {
    DcEntry entry;
    int elem_size;                                  // 2 (float16 / bfloat16), 4, 8
    int B, C, H, W, Co, kh, kw, sh, sw, ph, pw, dh, dw, G;
    int nhwc;
    int64_t out_batch_stride;                       // the 16-bit entry's, in elements
    bool has_in, has_off, has_wt, has_out;          // non-null (bias may be null everywhere)
    bool has_gout, has_gin, has_goff, has_gw;       // the backward's grad_out, grad_input, grad_offset, grad_weight
    bool in16, wt16;                                // 16-byte aligned (wt: the 16-bit entry alone looks)
    bool rest2;                                     // the 16-bit entry: offset, out and a non-null bias are 2-byte aligned
};

enum class DcStatus { ok, empty /* success, nothing to launch */, invalid_value, not_supported };

// bwd_zero_fill: a backward through which nothing flows (no pixels or no channels): the written outputs are zeroed.  The others
// are the kernels of the same names (bwd_mfma: dc_bwd_col_mfma + dc_bwd_weight_mfma; bwd_generic: dc_bwd_input_generic +
// dc_bwd_weight_generic).
enum class DcKind { fwd_generic, fwd_mfma, fwd_mfma_half, bwd_generic, bwd_mfma, bwd_zero_fill };

struct DcGrid {
    unsigned x, y, z;
};

struct DcRoute {
    DcStatus status;
    DcKind kind;
    const char *name;           // what mvdetr_deform_conv2d_last_kernel reports from this call on; null: left as it is
    DcShape s;
    int KC;                     // input channels per K chunk of the MFMA forwards: 32, or 16 when C is no multiple of 32
    DcGrid grid[2];             // the launches in order (one for the forwards)
    bool zero_goff, zero_gw;    // grad_offset / grad_weight are zeroed first (bwd_mfma: the kernels add; bwd_zero_fill: the result)
    int64_t pps;                // bwd_mfma: pixels per range of dc_bwd_weight_mfma (grid[1].z ranges)
};

// Oddities of the table, kept as they are: the 16-bit entry looks at its pointers before it says not_supported and at
// out_batch_stride after; the fp32 / fp64 forward is empty before it looks at a pointer and takes a null `in` / `wt` when
// C == 0; an MFMA forward whose grid does not fit is refused last, where its launch would fail; the other kernels' grids are
// not checked (one that does not fit fails at launch).
inline DcRoute dc_route(const DcQuery &q)
{
    using K = DcKind;
    using S = DcStatus;
    DcRoute r{S::ok, K::fwd_generic, nullptr, {}, 0, {{1, 1, 1}, {1, 1, 1}}, false, false, 0};
    auto refuse = [&r](S s) { r.status = s; return r; };
    auto launch = [&r](K kind, const char *name) { r.kind = kind; r.name = name; return r; };
    auto ceil_div = [](int64_t a, int64_t b) { return (a + b - 1) / b; };
    auto lanes = [](int64_t n) { const int64_t g = (n + 255) / 256; return (unsigned)(g < (1 << 20) ? g : 1 << 20); };

    if (!dc_shape(q.B, q.C, q.H, q.W, q.Co, q.kh, q.kw, q.sh, q.sw, q.ph, q.pw, q.dh, q.dw, q.G, r.s)) return refuse(S::invalid_value);
    const int C = q.C, Co = q.Co;
    const int64_t T = (int64_t)q.kh * q.kw, HWo = (int64_t)r.s.Ho * r.s.Wo, P = q.B * HWo;
    r.KC = C % 32 == 0 ? 32 : 16;
    // the MFMA forwards' grid: 64 pixels x 128 output channels per workgroup
    const DcGrid fwd_grid{(unsigned)ceil_div(P, DC_TP), (unsigned)ceil_div(Co, DC_TO), 1};
    const bool fwd_fits = ceil_div(Co, DC_TO) <= 65535;

    if (q.entry == DcEntry::forward_half) {
        if (!q.has_in || !q.has_off || !q.has_wt || !q.has_out) return refuse(S::invalid_value);
        if (q.G != 1 || !q.nhwc || C < 16 || C % 16 != 0 || Co < 32 || Co % 32 != 0) return refuse(S::not_supported);
        if (!q.in16 || !q.wt16 || !q.rest2) return refuse(S::not_supported);
        if (q.out_batch_stride < dc_prod(Co, HWo) || dc_prod(T, Co, C) >= (1ll << 31)) return refuse(S::invalid_value);
        if (P == 0) return refuse(S::empty);
        if (!fwd_fits) return refuse(S::not_supported);
        r.grid[0] = fwd_grid;
        return launch(K::fwd_mfma_half, "dc_fwd_mfma_half");
    }

    // fp32, one offset group, channel-last input read in 16-byte pieces, whole K chunks and whole 32-row wave tiles
    const bool fast = q.elem_size == 4 && q.nhwc && q.G == 1 && C % 16 == 0 && C > 0 && Co % 32 == 0 && Co > 0 && q.in16;

    if (q.entry == DcEntry::forward) {
        if (P * Co == 0) return refuse(S::empty);
        if (!q.has_out || !q.has_off || (C > 0 && (!q.has_in || !q.has_wt))) return refuse(S::invalid_value);
        if (!fast) {
            r.grid[0] = {lanes(P * Co), 1, 1};
            return launch(K::fwd_generic, "dc_fwd_generic");
        }
        if (!fwd_fits) return refuse(S::not_supported);
        r.grid[0] = fwd_grid;
        return launch(K::fwd_mfma, "dc_fwd_mfma");
    }

    // backward
    const int64_t nw = dc_prod(Co, C, T);
    if ((P * Co * C != 0 && (!q.has_gout || !q.has_in || !q.has_off || !q.has_wt || !q.has_gin)) || (P && !q.has_goff) || (nw && !q.has_gw))
        return refuse(S::invalid_value);
    if (P == 0 || Co == 0 || C == 0) {
        r.zero_goff = P != 0, r.zero_gw = nw != 0;
        return launch(K::bwd_zero_fill, nullptr);
    }
    if (!fast) {
        r.grid[0] = {lanes(P * q.G * T), 1, 1};
        r.grid[1] = {(unsigned)(C * T), (unsigned)ceil_div(Co, 256), 1};
        return launch(K::bwd_generic, "dc_bwd_generic");
    }
    // dc_bwd_col_mfma: (64 pixels, 128 input channels, tap); more than one channel block adds into grad_offset
    const int64_t cblocks = ceil_div(C, DC_TO);
    r.zero_goff = cblocks > 1;
    r.grid[0] = {(unsigned)ceil_div(P, DC_TP), (unsigned)cblocks, (unsigned)T};
    // dc_bwd_weight_mfma: (tap, 32 input channels) x 128 output channels x pixel ranges -- enough workgroups to fill the chip
    // (~2048), each range a multiple of the 32-pixel chunk; more than one range adds into grad_weight
    const int64_t kblocks = T * ceil_div(C, 32) * ceil_div(Co, DC_TO), chunks = ceil_div(P, DC_WP);
    int64_t splits = ceil_div(2048, kblocks);
    splits = splits < chunks ? splits : chunks;
    splits = splits > 1 ? splits : 1;
    r.pps = ceil_div(chunks, splits) * DC_WP;
    const int64_t nz = ceil_div(P, r.pps);
    r.zero_gw = nz > 1;
    r.grid[1] = {(unsigned)(T * ceil_div(C, 32)), (unsigned)ceil_div(Co, DC_TO), (unsigned)nz};
    return launch(K::bwd_mfma, "dc_bwd_mfma");
}

}  // namespace mvdetr

// Feature -> ground-plane homography warp -- gfx950 (MI355X): the C ABI and its one entry path.
//
// Replaces the reference's third-party call
//     kornia.warp_perspective(imgs_feat, proj_mats, Rworld_shape, align_corners=False)
// (multiview_detector/models/mvdetr.py:194-195), which kornia (0.5.x) evaluates as three torch
// ops: normalize_homography + inverse on the 3x3s, transform_points over a normalised meshgrid
// (materialising a [N,H,W,2] grid), and F.grid_sample(bilinear, zeros).  Here it is ONE kernel:
// the 3x3 algebra and the per-pixel source coordinate are evaluated in fp64 registers from the
// caller's matrix (exact w.r.t. kornia's formula on the same inputs -- the fp32 op chain itself
// is only accurate to ~2e-4 near the horizon), the bilinear blend runs in the
// tensor dtype, and pixels whose footprint misses the source image are stored as zeros without
// touching `src`.
//
// Work mapping (wave64): a block is an 8x8 tile of destination pixels (lanes = pixels; its pre-image is a
// compact source patch, so a load instruction touches a handful of cache lines) times a group of up to 64
// channels split over the block's 4 waves.  For the channel-last output the 64x64 (pixel, channel) tile is
// transposed through LDS (65-float rows, conflict-free both ways) so the stores are 256-byte rows.
//
// Where things live: warp_route.h decides which kernel a call runs (and what it refuses), warp_forward.hip and
// warp_backward.hip hold the kernels and their launchers (warp_launch.h), warp_device.h what the kernels share.  Every entry
// below fills one WarpCall, asks for the route, and switches on its kind.
#include "warp_launch.h"
#include "../../include/mvdetr_ops.h"
#include <atomic>
#include <cstdlib>

namespace mvdetr {

// Which kernel the last warp call of this process launched (tests assert the layout routes; bench.py reports it).  Not
// thread-local: autograd runs the backward on its own thread.
static std::atomic<const char *> g_warp_last_kernel{"none"};

// The backward knobs are read on every call (tests set them between calls), MVDETR_WARP_FWD_NCHW once per process, by the
// first forward of the fp32 / fp64 entries.
static WarpKnobs warp_env_knobs(WarpEntry entry)
{
    const char *fwd_nchw = nullptr;
    if (entry == WarpEntry::forward) {
        static const char *const once = getenv("MVDETR_WARP_FWD_NCHW");
        fwd_nchw = once;
    }
    return warp_parse_knobs(getenv("MVDETR_WARP_BWD_IMPL"), getenv("MVDETR_WARP_BWD_GEOMETRY"), getenv("MVDETR_WARP_BWD_HEAVY"),
                            getenv("MVDETR_WARP_BWD_HEAVY_WGS"), fwd_nchw);
}

static WarpRoute warp_call_route(WarpEntry entry, int elem_size, int layout_nhwc, const WarpCall &c)
{
    return warp_route(WarpQuery{entry, elem_size, c.N, c.C, c.h, c.w, c.H, c.W, layout_nhwc, c.in != nullptr, c.M != nullptr,
                                c.out != nullptr, c.plan != nullptr, aligned(c.in, 16), aligned(c.out, 16), aligned(c.plan, 16), c.knobs});
}

static int warp_entry(WarpEntry entry, WarpType type, void *stream, const void *in, const void *M, const void *plan, int N, int C, int h,
                      int w, int H, int W, int layout_nhwc, void *out, uint64_t tag = 0)
{
    // (the gather only reads the caller's plan: the planned entry's const is cast away for the descriptor alone)
    const WarpCall c{reinterpret_cast<hipStream_t>(stream), type, in, M, out, const_cast<void *>(plan), N, C, h, w, H, W, tag, warp_env_knobs(entry)};
    const int elem_size = type == WarpType::f64 ? 8 : type == WarpType::f32 ? 4 : 2;
    const WarpRoute r = warp_call_route(entry, elem_size, layout_nhwc, c);
    if (r.status == WarpStatus::empty) return 0;
    if (r.status != WarpStatus::ok) return (int)(r.status == WarpStatus::invalid_value ? hipErrorInvalidValue : hipErrorNotSupported);
    if (r.zero_first || r.kind == WarpKind::zero_fill) {
        const hipError_t rc = hipMemsetAsync(out, 0, (size_t)N * C * h * w * elem_size, c.st);
        if (rc != hipSuccess || r.kind == WarpKind::zero_fill) return (int)rc;
    }
    if (r.name) g_warp_last_kernel = r.name;
    switch (r.kind) {
    case WarpKind::none:
    case WarpKind::zero_fill: return 0;
    case WarpKind::bwd:
    case WarpKind::bwd_cl: return warp_launch_scatter(c, r);
    case WarpKind::bwd_gather: return entry == WarpEntry::planned ? warp_launch_gather(c, r, static_cast<char *>(c.plan)) : warp_launch_gather_scratch(c, r);
    case WarpKind::plan: return warp_launch_plan(c, static_cast<char *>(c.plan));
    default: return warp_launch_forward(c, r);
    }
}

// [n, rows, cols] -> [n, cols, rows]: turns an NCHW feature map into the channel-last layout the fast warp kernels read
// (rows = C, cols = h*w) and back (rows = h*w, cols = C)
static int transpose_entry(void *stream, int elem_size, const void *src, int n, int rows, int cols, void *dst)
{
    if (n < 0 || rows < 0 || cols < 0) return (int)hipErrorInvalidValue;
    if ((int64_t)n * rows * cols == 0) return 0;
    if (!src || !dst || n > 65535 || (rows + 63) / 64 > 65535) return (int)hipErrorInvalidValue;
    return warp_launch_transpose(reinterpret_cast<hipStream_t>(stream), elem_size, src, n, rows, cols, dst);
}

}  // namespace mvdetr

using mvdetr::WarpEntry;
using mvdetr::WarpType;

extern "C" {

const char *mvdetr_warp_last_kernel(void) { return mvdetr::g_warp_last_kernel.load(); }

int mvdetr_transpose_f32(void *stream, const float *src, int n, int rows, int cols, float *dst)
{
    return mvdetr::transpose_entry(stream, 4, src, n, rows, cols, dst);
}
int mvdetr_transpose_f64(void *stream, const double *src, int n, int rows, int cols, double *dst)
{
    return mvdetr::transpose_entry(stream, 8, src, n, rows, cols, dst);
}

int mvdetr_warp_perspective_forward_f32(void *stream, const float *src, const float *M, int n, int channels, int src_h, int src_w,
                                        int dst_h, int dst_w, int layout_nhwc, float *dst)
{
    return mvdetr::warp_entry(WarpEntry::forward, WarpType::f32, stream, src, M, nullptr, n, channels, src_h, src_w, dst_h, dst_w, layout_nhwc, dst);
}
int mvdetr_warp_perspective_forward_f64(void *stream, const double *src, const double *M, int n, int channels, int src_h, int src_w,
                                        int dst_h, int dst_w, int layout_nhwc, double *dst)
{
    return mvdetr::warp_entry(WarpEntry::forward, WarpType::f64, stream, src, M, nullptr, n, channels, src_h, src_w, dst_h, dst_w, layout_nhwc, dst);
}
int mvdetr_warp_perspective_forward_f16(void *stream, const uint16_t *src, const float *M, int n, int channels, int src_h,
                                        int src_w, int dst_h, int dst_w, int layout_nhwc, uint16_t *dst)
{
    return mvdetr::warp_entry(WarpEntry::forward_half, WarpType::f16, stream, src, M, nullptr, n, channels, src_h, src_w, dst_h, dst_w, layout_nhwc,
                              dst);
}
int mvdetr_warp_perspective_forward_bf16(void *stream, const uint16_t *src, const float *M, int n, int channels, int src_h,
                                         int src_w, int dst_h, int dst_w, int layout_nhwc, uint16_t *dst)
{
    return mvdetr::warp_entry(WarpEntry::forward_half, WarpType::bf16, stream, src, M, nullptr, n, channels, src_h, src_w, dst_h, dst_w, layout_nhwc,
                              dst);
}

int mvdetr_warp_perspective_backward_f32(void *stream, const float *grad_dst, const float *M, int n, int channels, int src_h,
                                         int src_w, int dst_h, int dst_w, int layout_nhwc, float *grad_src)
{
    return mvdetr::warp_entry(WarpEntry::backward, WarpType::f32, stream, grad_dst, M, nullptr, n, channels, src_h, src_w, dst_h, dst_w, layout_nhwc,
                              grad_src);
}
int mvdetr_warp_perspective_backward_f64(void *stream, const double *grad_dst, const double *M, int n, int channels, int src_h,
                                         int src_w, int dst_h, int dst_w, int layout_nhwc, double *grad_src)
{
    return mvdetr::warp_entry(WarpEntry::backward, WarpType::f64, stream, grad_dst, M, nullptr, n, channels, src_h, src_w, dst_h, dst_w, layout_nhwc,
                              grad_src);
}
int mvdetr_warp_perspective_backward_tagged_f32(void *stream, const float *grad_dst, const float *M, int n, int channels,
                                                int src_h, int src_w, int dst_h, int dst_w, int layout_nhwc,
                                                uint64_t matrices_tag, float *grad_src)
{
    return mvdetr::warp_entry(WarpEntry::backward, WarpType::f32, stream, grad_dst, M, nullptr, n, channels, src_h, src_w, dst_h, dst_w, layout_nhwc,
                              grad_src, matrices_tag);
}
int mvdetr_warp_perspective_backward_tagged_f64(void *stream, const double *grad_dst, const double *M, int n, int channels,
                                                int src_h, int src_w, int dst_h, int dst_w, int layout_nhwc,
                                                uint64_t matrices_tag, double *grad_src)
{
    return mvdetr::warp_entry(WarpEntry::backward, WarpType::f64, stream, grad_dst, M, nullptr, n, channels, src_h, src_w, dst_h, dst_w, layout_nhwc,
                              grad_src, matrices_tag);
}

int64_t mvdetr_warp_backward_plan_bytes(int n, int channels, int src_h, int src_w, int dst_h, int dst_w, int elem_size)
{
    mvdetr::WarpCall c{};
    c.N = n, c.C = channels, c.h = src_h, c.w = src_w, c.H = dst_h, c.W = dst_w;
    c.knobs = mvdetr::warp_env_knobs(WarpEntry::plan_bytes);
    const mvdetr::WarpRoute r = mvdetr::warp_call_route(WarpEntry::plan_bytes, elem_size, 0, c);
    return r.status == mvdetr::WarpStatus::ok ? r.plan_bytes : 0;
}

int mvdetr_warp_backward_plan_f32(void *stream, const float *M, int n, int channels, int src_h, int src_w, int dst_h, int dst_w,
                                  void *plan)
{
    return mvdetr::warp_entry(WarpEntry::plan, WarpType::f32, stream, nullptr, M, plan, n, channels, src_h, src_w, dst_h, dst_w, 0, nullptr);
}
int mvdetr_warp_backward_plan_f64(void *stream, const double *M, int n, int channels, int src_h, int src_w, int dst_h, int dst_w,
                                  void *plan)
{
    return mvdetr::warp_entry(WarpEntry::plan, WarpType::f64, stream, nullptr, M, plan, n, channels, src_h, src_w, dst_h, dst_w, 0, nullptr);
}
int mvdetr_warp_perspective_backward_planned_f32(void *stream, const float *grad_dst, const float *M, const void *plan, int n,
                                                 int channels, int src_h, int src_w, int dst_h, int dst_w, int layout_nhwc,
                                                 float *grad_src)
{
    return mvdetr::warp_entry(WarpEntry::planned, WarpType::f32, stream, grad_dst, M, plan, n, channels, src_h, src_w, dst_h, dst_w, layout_nhwc,
                              grad_src);
}
int mvdetr_warp_perspective_backward_planned_f64(void *stream, const double *grad_dst, const double *M, const void *plan, int n,
                                                 int channels, int src_h, int src_w, int dst_h, int dst_w, int layout_nhwc,
                                                 double *grad_src)
{
    return mvdetr::warp_entry(WarpEntry::planned, WarpType::f64, stream, grad_dst, M, plan, n, channels, src_h, src_w, dst_h, dst_w, layout_nhwc,
                              grad_src);
}

}  // extern "C"

// Multi-scale deformable attention, forward -- gfx950 (MI355X) kernels + C ABI.
//
// Replaces ms_deformable_im2col_cuda / ms_deformable_im2col_gpu_kernel of the reference
// (multiview_detector/models/ops/src/cuda/ms_deform_im2col_cuda.cuh:923-954, 237-299, 33-84).
// Written for wave64 / CDNA4 from the operation's definition; not derived from the CUDA source.
//
// Kernels
//   msda_fwd_gather<T, VEC>   any shape/dtype.  One lane owns VEC consecutive channels of one
//                             (b, q, head); the D/VEC lanes of a head read one contiguous
//                             D*sizeof(T) segment per bilinear corner straight from L2/HBM.
//   (the LDS-tiled encoder kernel lives in msda_forward_tile.hip)
#include "common.h"
#include "../../include/mvdetr_ops.h"
#include "msda_dispatch.h"
#include "msda_tile.h"
#include "msda_gather_body.h"
#include <atomic>
#include <stdlib.h>
#include <string.h>

namespace mvdetr {

static std::atomic<int> g_impl_knob{-1};

// MVDETR_MSDA_FWD_IMPL = auto (default) | gather | tile; overridable at run time through mvdetr_msda_set_forward_impl()
static MsdaFwdKnob msda_fwd_impl_knob()
{
    int v = g_impl_knob.load(std::memory_order_relaxed);
    if (v < 0) {
        v = (int)msda_forward_parse_knob(getenv("MVDETR_MSDA_FWD_IMPL"));
        int expect = -1;
        g_impl_knob.compare_exchange_strong(expect, v);
        v = g_impl_knob.load(std::memory_order_relaxed);
    }
    return (MsdaFwdKnob)v;
}

// The environment's part of a route and of a camera-grouped launch's options, read once per process.  MVDETR_MSDA_GROUP=0
// keeps every call off the camera-grouped kernels.
static bool group_enabled()
{
    static const bool enabled = [] { const char *e = getenv("MVDETR_MSDA_GROUP"); return !(e && e[0] == '0'); }();
    return enabled;
}
// MVDETR_MSDA_WINDOW_SHIFT=0 keeps the fused kernels' windows centred on the tile (A/B knob); the jobs are dealt to the XCDs as
// 2-D blocks of the tile grid (GROUP_OPT_BLOCKS: 566 -> 314 MB of memory-side traffic per launch against bands of the job
// list, round 4)
static int group_opts(const MsdaFwdRoute &r)
{
    static const bool no_shift = [] { const char *e = getenv("MVDETR_MSDA_WINDOW_SHIFT"); return e && e[0] == '0'; }();
    return ((r.ref_mode && no_shift) ? GROUP_OPT_NO_SHIFT : 0) | GROUP_OPT_BLOCKS | (r.standdown ? GROUP_OPT_STANDDOWN : 0);
}

template <typename T, int VEC>
__global__ __launch_bounds__(256) void msda_fwd_gather(
    const T *__restrict__ value, const int64_t *__restrict__ shapes,
    const int64_t *__restrict__ lsi, const T *__restrict__ loc, const T *__restrict__ aw,
    int B, int S, int M, int D, int L, int Lq, int P, T *__restrict__ out)
{
    msda_fwd_gather_body<T, VEC>((int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x, value,
                                 shapes, lsi, loc, aw, B, S, M, D, L, Lq, P, out);
}

template <typename T, int VEC>
static int launch_gather(hipStream_t st, const T *value, const int64_t *shapes, const int64_t *lsi,
                         const T *loc, const T *aw, int B, int S, int M, int D, int L, int Lq, int P,
                         T *out)
{
    const int64_t total = (int64_t)B * Lq * M * (D / VEC);
    const int block = 256;
    int64_t blocks = (total + block - 1) / block;
    // Two workgroups per CU walking the items in order: the lanes in flight at any moment then belong to one compact
    // band of queries, whose taps share L2 lines.  Measured at Wildtrack size (realistic / uniform locations):
    // one item per lane 1,112 / 1,542 us; 1024 workgroups 837 / 1,437; 512 -> 537 / 950; 256 -> 819 / 1,017.
    // (not PersistentGrid: no dynamic LDS, no rounding to 8 -- a cap on the grid of a launch that may be smaller)
    static PerDevice<int64_t> resident_of;
    const int64_t resident = resident_of.get([] {
        int dev = 0, cus = 256;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
            cus = 256;
        return (int64_t)2 * cus;
    });
    if (blocks > resident) blocks = resident;
    hipLaunchKernelGGL((msda_fwd_gather<T, VEC>), dim3((unsigned)blocks), dim3(block), 0, st, value,
                       shapes, lsi, loc, aw, B, S, M, D, L, Lq, P, out);
    return (int)hipGetLastError();
}

static thread_local const char *g_last_impl = "none";
static thread_local const char *g_last_kernel = "none";
static thread_local KernelResources g_last_resources = {-1, -1, -1};
void msda_note_forward_kernel(const char *name, const KernelResources *res)
{
    g_last_kernel = name;
    g_last_resources = res ? *res : KernelResources{-1, -1, -1};
}

// what mvdetr_msda_last_forward_impl() says of a route
static const char *impl_name(MsdaFwdKind k)
{
    if (k == MsdaFwdKind::gather) return "gather";
    return k == MsdaFwdKind::tile || k == MsdaFwdKind::group2 || k == MsdaFwdKind::group_many ? "tile" : "tile_fused";
}

// the kernel of an fp32 route other than `gather`, and the statistics pass where the route has one
static int launch_route(const MsdaFwdRoute &r, const MsdaFwdCall &c)
{
    int rc;
    switch (r.kind) {
    case MsdaFwdKind::tile: case MsdaFwdKind::fused_tile: rc = msda_forward_tile(c); break;
    case MsdaFwdKind::group2: case MsdaFwdKind::fused_group2: rc = msda_forward_group2(c); break;
    case MsdaFwdKind::group_many: case MsdaFwdKind::fused_group_many: rc = msda_forward_group_many(c); break;
    default: return (int)hipErrorInvalidValue;
    }
    if (!rc && r.stats_pass) rc = msda_softmax_stats(c.st, c.aw, c.lay, (int64_t)c.B * c.qr.Lq, c.M, c.L, c.stats);
    return rc;
}

template <typename T>
static int forward_entry(void *stream, const T *value, const int64_t *shapes, const int64_t *lsi,
                         const T *loc, const T *aw, int B, int S, int M, int D, int L, int Lq, int P,
                         T *out)
{
    const bool a16 = aligned(value, 16) && aligned(out, 16);
    const MsdaFwdRoute r = msda_forward_route(MsdaFwdQuery{sizeof(T) == 4 ? MsdaFwdEntry::public_f32 : MsdaFwdEntry::public_f64, B, S, M, D, L, Lq, P,
                                                           /*layout, strides*/ 0, 0, 0, /*query levels*/ 0, L, false,
                                                           a16 && aligned(loc, 16) && aligned(aw, 16), a16, msda_fwd_impl_knob(),
                                                           group_enabled(), false});
    if (r.status == MsdaFwdStatus::invalid_value) return (int)hipErrorInvalidValue;
    if (r.status == MsdaFwdStatus::empty) { g_last_impl = "empty"; return 0; }     // nothing to write
    if (!value || !shapes || !lsi || !loc || !aw || !out) return (int)hipErrorInvalidValue;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    g_last_impl = impl_name(r.kind);
    if (r.kind == MsdaFwdKind::gather) {
        msda_note_forward_kernel("msda_fwd_gather");
        constexpr int WIDE = 16 / (int)sizeof(T);            // 4 floats / 2 doubles per 16-byte access
        return r.gather_vec == 1 ? launch_gather<T, 1>(st, value, shapes, lsi, loc, aw, B, S, M, D, L, Lq, P, out)
                                 : launch_gather<T, WIDE>(st, value, shapes, lsi, loc, aw, B, S, M, D, L, Lq, P, out);
    }
    if constexpr (sizeof(T) == 4) {
        MsdaFwdCall c{st, value, shapes, lsi, loc, aw, /*ref*/ nullptr, 0, plain_layout(r.q_l, L * P * 2, P * 2, r.q_w, L * P, P),     // [.., Lq, M, L, P(, 2)]
                      QueryLevels{0, L, S}, r.ref_mode, B, S, M, D, L, out, /*stats*/ nullptr, /*probe*/ nullptr, group_opts(r)};
        // (if the probe's scratch cannot be had, the forward goes on without a probe)
        int *hits = nullptr;
        if (r.probe && hipMallocAsync(reinterpret_cast<void **>(&hits), MSDA_PROBE_INTS * sizeof(int), st) != hipSuccess) hits = nullptr;
        int rc = hits ? msda_launch_locality_probe(st, loc, shapes, B, S, M, L, hits) : 0;
        c.probe = hits;
        if (!rc) rc = launch_route(r, c);
        if (hits) (void)hipFreeAsync(hits, st);
        return rc;
    }
    return (int)hipErrorInvalidValue;       // (fp64 has no route but `gather`)
}

// both fused entries.  stats: the training entry's softmax statistics, null for inference
static int fused_entry(MsdaFwdEntry entry, void *stream, const float *value, const int64_t *shapes, const int64_t *lsi, const float *ref,
                       int64_t ref_bstride, const float *offsets, const float *logits, int layout, int qstride_l, int qstride_w,
                       int ql0, int ql1, int B, int S, int M, int D, int L, int Lq, int P, float *out, float *stats)
{
    const bool a16 = aligned(value, 16) && aligned(out, 16);
    const bool all16 = a16 && aligned(ref, 16) && aligned(offsets, 16) && aligned(logits, 16) && ref_bstride % ((layout & 2) ? 2 : 4) == 0;
    // slice-interleaved layouts: the two pointers address one tensor, the logits start behind the first slice's offsets
    const bool follow = reinterpret_cast<uintptr_t>(logits) == reinterpret_cast<uintptr_t>(offsets) + (uintptr_t)((int64_t)(D == 16 ? 2 : 1) * P * 2 * 4);
    const MsdaFwdRoute r = msda_forward_route(MsdaFwdQuery{entry, B, S, M, D, L, Lq, P, layout, qstride_l, qstride_w, ql0, ql1, follow, all16, a16,
                                                           msda_fwd_impl_knob(), group_enabled(), stats != nullptr});
    if (r.status == MsdaFwdStatus::invalid_value) return (int)hipErrorInvalidValue;
    if (!value || !shapes || !lsi || !ref || !offsets || !logits || !out) return (int)hipErrorInvalidValue;
    if (r.status != MsdaFwdStatus::ok) return (int)hipErrorNotSupported;
    g_last_impl = impl_name(r.kind);
    return launch_route(r, MsdaFwdCall{reinterpret_cast<hipStream_t>(stream), value, shapes, lsi, offsets, logits, ref, ref_bstride,
                                       fused_layout(layout, r.q_l, r.q_w, M, D, L, Lq), QueryLevels{ql0, ql1, Lq}, r.ref_mode, B, S, M, D, L,
                                       out, stats, /*probe*/ nullptr, group_opts(r)});
}

}  // namespace mvdetr

extern "C" {

int mvdetr_ops_abi_version(void) { return MVDETR_OPS_ABI_VERSION; }

const char *mvdetr_msda_last_forward_impl(void) { return mvdetr::g_last_impl; }
int mvdetr_msda_last_forward_resources(int *num_regs, int *scratch_bytes_per_lane, int *static_lds_bytes)
{
    const mvdetr::KernelResources r = mvdetr::g_last_resources;
    if (num_regs) *num_regs = r.num_regs;
    if (scratch_bytes_per_lane) *scratch_bytes_per_lane = r.scratch_bytes;
    if (static_lds_bytes) *static_lds_bytes = r.static_lds_bytes;
    return r.num_regs >= 0;
}
const char *mvdetr_msda_last_forward_kernel(void) { return mvdetr::g_last_kernel; }

int mvdetr_msda_set_forward_impl(int impl)
{
    if (impl < 0 || impl > 2) impl = 0;
    const int prev = (int)mvdetr::msda_fwd_impl_knob();
    mvdetr::g_impl_knob.store(impl);
    return prev;
}

int mvdetr_msda_fused_supported(int batch, int spatial_size, int num_heads, int channels, int num_levels,
                                int num_query, int num_point)
{
    return mvdetr_msda_fused_levels_supported(batch, spatial_size, num_heads, channels, num_levels, num_query,
                                              num_point, 0, num_levels);
}

int mvdetr_msda_fused_levels_supported(int batch, int spatial_size, int num_heads, int channels, int num_levels,
                                       int num_query, int num_point, int query_level_begin, int query_level_end)
{
    return mvdetr::msda_tile_supported(batch, spatial_size, num_heads, channels, num_levels, num_query, num_point, true,
                                       query_level_begin, query_level_end) ? 1 : 0;
}

int mvdetr_msda_forward_fused_f32(void *stream, const float *value, const int64_t *spatial_shapes,
                                  const int64_t *level_start_index, const float *reference_points,
                                  int64_t ref_batch_stride, const float *sampling_offsets,
                                  const float *attn_logits, int level_major, int offsets_query_stride,
                                  int logits_query_stride, int batch, int spatial_size, int num_heads,
                                  int channels, int num_levels, int num_query, int num_point, float *out)
{
    return mvdetr_msda_forward_fused_levels_f32(stream, value, spatial_shapes, level_start_index, reference_points,
                                                ref_batch_stride, sampling_offsets, attn_logits, level_major,
                                                offsets_query_stride, logits_query_stride, 0, num_levels, batch,
                                                spatial_size, num_heads, channels, num_levels, num_query, num_point,
                                                out);
}

int mvdetr_msda_forward_fused_levels_f32(void *stream, const float *value, const int64_t *spatial_shapes,
                                         const int64_t *level_start_index, const float *reference_points,
                                         int64_t ref_batch_stride, const float *sampling_offsets,
                                         const float *attn_logits, int level_major, int offsets_query_stride,
                                         int logits_query_stride, int query_level_begin, int query_level_end,
                                         int batch, int spatial_size, int num_heads, int channels, int num_levels,
                                         int num_query, int num_point, float *out)
{
    return mvdetr::fused_entry(mvdetr::MsdaFwdEntry::fused, stream, value, spatial_shapes, level_start_index, reference_points, ref_batch_stride,
                               sampling_offsets, attn_logits, level_major, offsets_query_stride, logits_query_stride, query_level_begin,
                               query_level_end, batch, spatial_size, num_heads, channels, num_levels, num_query, num_point, out, nullptr);
}

int mvdetr_msda_fused_train_supported(int batch, int spatial_size, int num_heads, int channels, int num_levels, int num_query,
                                      int num_point)
{
    // 6 / 7 levels of 16-channel heads (MVDeTr's own) run msda_fwd_group2 + msda_bwd_onepass<grad_value only> +
    // msda_bwd_fused_sampling; other level counts the one-pass backward (16 channels) or msda_bwd_value_tok + the level-groups
    // sampling kernel (32 channels) behind the inference forward + a statistics pass (msda_backward_route.h).
    return mvdetr::msda_fused_train_supported(batch, spatial_size, num_heads, channels, num_levels, num_query, num_point) ? 1 : 0;
}

int mvdetr_msda_forward_fused_train_f32(void *stream, const float *value, const int64_t *spatial_shapes,
                                        const int64_t *level_start_index, const float *reference_points,
                                        int64_t ref_batch_stride, const float *raw, int raw_query_stride, int batch,
                                        int spatial_size, int num_heads, int channels, int num_levels, int num_point,
                                        float *out, float *stats)
{
    if (!stats || !raw) return (int)hipErrorInvalidValue;
    // (refused here as well as by the route: this refusal precedes the entry's look at the other pointers)
    if (!mvdetr_msda_fused_train_supported(batch, spatial_size, num_heads, channels, num_levels, spatial_size, num_point))
        return (int)hipErrorNotSupported;
    const int hps = channels == 16 ? 2 : 1;
    // layout: the slice-interleaved raw tensor with the level outermost (bits 2 and 4), one reference point per
    // (query, level), level-major (bits 1 and 3)
    return mvdetr::fused_entry(mvdetr::MsdaFwdEntry::fused_train, stream, value, spatial_shapes, level_start_index, reference_points,
                               ref_batch_stride, raw, raw + hps * num_point * 2, 2 | 4 | 8 | 16, raw_query_stride, raw_query_stride, 0,
                               num_levels, batch, spatial_size, num_heads, channels, num_levels, spatial_size, num_point, out, stats);
}

int mvdetr_msda_forward_f32(void *stream, const float *value, const int64_t *spatial_shapes,
                            const int64_t *level_start_index, const float *sampling_loc,
                            const float *attn_weight, int batch, int spatial_size, int num_heads,
                            int channels, int num_levels, int num_query, int num_point, float *out)
{
    return mvdetr::forward_entry<float>(stream, value, spatial_shapes, level_start_index, sampling_loc,
                                        attn_weight, batch, spatial_size, num_heads, channels,
                                        num_levels, num_query, num_point, out);
}

int mvdetr_msda_forward_f64(void *stream, const double *value, const int64_t *spatial_shapes,
                            const int64_t *level_start_index, const double *sampling_loc,
                            const double *attn_weight, int batch, int spatial_size, int num_heads,
                            int channels, int num_levels, int num_query, int num_point, double *out)
{
    return mvdetr::forward_entry<double>(stream, value, spatial_shapes, level_start_index, sampling_loc,
                                         attn_weight, batch, spatial_size, num_heads, channels,
                                         num_levels, num_query, num_point, out);
}

}  // extern "C"

// Multi-scale deformable attention, backward -- gfx950 (MI355X) kernels + C ABI.
//
// Replaces ms_deformable_col2im_cuda and its six kernel variants
// (multiview_detector/models/ops/src/cuda/ms_deform_im2col_cuda.cuh:956-1327, 301-920) and the
// device helpers ms_deform_attn_col2im_bilinear{,_gm} (cuh:87-234).
//
// The reference picks among shared-memory reductions by block size because its block IS the D
// channels of one (b,q,head) (16 threads at MVDeTr's D=16: a quarter of a wave64).  Here:
//   msda_bwd_lanes<T, VEC, G>  G = D/VEC lanes (power of two <= 64; VEC = 1 by default) own one (b,q,head); the
//                              per-tap partial sums for grad_sampling_loc / grad_attn_weight are
//                              reduced across those G lanes with DPP/xor shuffles inside the wave
//                              -- no LDS, no barrier -- and lane 0 of the group stores them.
//   msda_bwd_serial<T>         any D: one lane per (b,q,head) walks the channels itself.
// grad_value is accumulated with hardware fp atomics (global_atomic_add_f32/f64,
// -munsafe-fp-atomics), i.e. the summation order -- like the reference's atomicAdd
// (cuh:125-152) -- is not deterministic.
// Encoder-shaped fp32 calls do not end up here: msda_backward_route.h sends them to the LDS-window kernels
// (msda_backward_value_tok.hip / msda_backward_onepass.hip / msda_backward_sampling.hip / msda_backward_fused.hip).
#include "common.h"
#include "msda_dispatch.h"
#include "msda_backward_lanes.h"
#include "../../include/mvdetr_ops.h"
#include <stdlib.h>
#include <string.h>

#include <atomic>

namespace mvdetr {

// deterministic backward requested (mvdetr_msda_set_backward_deterministic; MVDETR_MSDA_BWD_DETERMINISTIC=1 sets the initial state)
static std::atomic<int> &backward_deterministic()
{
    static std::atomic<int> on{[] { const char *e = getenv("MVDETR_MSDA_BWD_DETERMINISTIC"); return e && *e && strcmp(e, "0") ? 1 : 0; }()};
    return on;
}

template <typename T, int VEC, int G, bool VALUE_GRAD = true>
__global__ __launch_bounds__(256) void msda_bwd_lanes(
    const T *__restrict__ grad_col, const T *__restrict__ value, const int64_t *__restrict__ shapes,
    const int64_t *__restrict__ lsi, const T *__restrict__ loc, const T *__restrict__ aw, int B, int S,
    int M, int D, int L, int Lq, int P, T *__restrict__ grad_value, T *__restrict__ grad_loc,
    T *__restrict__ grad_aw)
{
    msda_bwd_lanes_body<T, VEC, G, VALUE_GRAD>((int64_t)blockIdx.x * blockDim.x + threadIdx.x, grad_col, value, shapes, lsi,
                                               loc, aw, B, S, M, D, L, Lq, P, grad_value, grad_loc, grad_aw);
}

template <typename T>
__global__ __launch_bounds__(256) void msda_bwd_serial(
    const T *__restrict__ grad_col, const T *__restrict__ value, const int64_t *__restrict__ shapes,
    const int64_t *__restrict__ lsi, const T *__restrict__ loc, const T *__restrict__ aw, int B, int S,
    int M, int D, int L, int Lq, int P, T *__restrict__ grad_value, T *__restrict__ grad_loc,
    T *__restrict__ grad_aw)
{
    const int64_t total = (int64_t)B * Lq * M;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t row = (int64_t)M * D;
    for (int64_t bqm = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; bqm < total; bqm += stride) {
        const int m = (int)(bqm % M);
        const int64_t bq = bqm / M;
        const int b = (int)(bq / Lq);
        const T *go = grad_col + bqm * D;
        const int64_t voff = (int64_t)b * S * row + (int64_t)m * D;
        for (int l = 0; l < L; ++l) {
            const int H = (int)shapes[2 * l], W = (int)shapes[2 * l + 1];
            const int64_t poff = voff + lsi[l] * row;
            for (int p = 0; p < P; ++p) {
                const int64_t t = bqm * L * P + l * P + p;
                const T x = loc[t * 2 + 0] * T(W) - T(0.5);
                const T y = loc[t * 2 + 1] * T(H) - T(0.5);
                const T a = aw[t];
                T g_a = 0, g_x = 0, g_y = 0;
                if (y > T(-1) && x > T(-1) && y < T(H) && x < T(W)) {
                    const Footprint<T> f = footprint(y, x, H, W);
                    const int64_t o00 = poff + ((int64_t)f.y0 * W + f.x0) * row;
                    const int64_t o01 = o00 + row, o10 = o00 + (int64_t)W * row, o11 = o10 + row;
                    const bool v00 = f.vy0 && f.vx0, v01 = f.vy0 && f.vx1;
                    const bool v10 = f.vy1 && f.vx0, v11 = f.vy1 && f.vx1;
                    const T w00 = f.wy0 * f.wx0, w01 = f.wy0 * f.wx1, w10 = f.wy1 * f.wx0, w11 = f.wy1 * f.wx1;
                    for (int c = 0; c < D; ++c) {
                        const T g = go[c], ga = g * a;
                        const T c00 = v00 ? value[o00 + c] : T(0), c01 = v01 ? value[o01 + c] : T(0);
                        const T c10 = v10 ? value[o10 + c] : T(0), c11 = v11 ? value[o11 + c] : T(0);
                        g_a += g * (w00 * c00 + w01 * c01 + w10 * c10 + w11 * c11);
                        g_x += g * ((c01 - c00) * f.wy0 + (c11 - c10) * f.wy1);
                        g_y += g * ((c10 - c00) * f.wx0 + (c11 - c01) * f.wx1);
                        if (v00) atomic_add(grad_value + o00 + c, w00 * ga);
                        if (v01) atomic_add(grad_value + o01 + c, w01 * ga);
                        if (v10) atomic_add(grad_value + o10 + c, w10 * ga);
                        if (v11) atomic_add(grad_value + o11 + c, w11 * ga);
                    }
                }
                grad_aw[t] = g_a;
                grad_loc[t * 2 + 0] = T(W) * a * g_x;
                grad_loc[t * 2 + 1] = T(H) * a * g_y;
            }
        }
    }
}

#define MSDA_BWD_ARGS grad_col, value, shapes, lsi, loc, aw, B, S, M, D, L, Lq, P, grad_value, grad_loc, grad_aw

template <typename T, int VEC, int G, bool VALUE_GRAD = true>
static int launch_lanes(hipStream_t st, const T *grad_col, const T *value, const int64_t *shapes,
                        const int64_t *lsi, const T *loc, const T *aw, int B, int S, int M, int D, int L,
                        int Lq, int P, T *grad_value, T *grad_loc, T *grad_aw)
{
    const int64_t total = (int64_t)B * Lq * M * G;
    const int64_t blocks = (total + 255) / 256;
    if (blocks > 0x7fffffffLL) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL((msda_bwd_lanes<T, VEC, G, VALUE_GRAD>), dim3((unsigned)blocks), dim3(256), 0, st, MSDA_BWD_ARGS);
    return (int)hipGetLastError();
}

// msda_bwd_lanes<T, VEC, g> for g = 1, 2, .. 64
template <typename T, int VEC>
static int launch_lanes_g(int g, hipStream_t st, const T *grad_col, const T *value, const int64_t *shapes,
                          const int64_t *lsi, const T *loc, const T *aw, int B, int S, int M, int D, int L,
                          int Lq, int P, T *grad_value, T *grad_loc, T *grad_aw)
{
    switch (g) {
    case 1: return launch_lanes<T, VEC, 1>(st, MSDA_BWD_ARGS);
    case 2: return launch_lanes<T, VEC, 2>(st, MSDA_BWD_ARGS);
    case 4: return launch_lanes<T, VEC, 4>(st, MSDA_BWD_ARGS);
    case 8: return launch_lanes<T, VEC, 8>(st, MSDA_BWD_ARGS);
    case 16: return launch_lanes<T, VEC, 16>(st, MSDA_BWD_ARGS);
    case 32: return launch_lanes<T, VEC, 32>(st, MSDA_BWD_ARGS);
    case 64: return launch_lanes<T, VEC, 64>(st, MSDA_BWD_ARGS);
    default: return (int)hipErrorInvalidValue;
    }
}

// MVDETR_MSDA_BWD_IMPL, read once (msda_backward_route.h says what each setting runs through either entry)
static MsdaBwdKnob backward_knob()
{
    static const MsdaBwdKnob knob = msda_backward_parse_knob(getenv("MVDETR_MSDA_BWD_IMPL"));
    return knob;
}

static thread_local MsdaBwdKind g_last_bwd_route = MsdaBwdKind::none;

// true: the call ends here with `rc` (success for an empty call, else the refusal); false: run the route, now on record
static bool route_refused(const MsdaBwdRoute &r, bool null_pointer, int &rc)
{
    rc = 0;
    if (r.status == MsdaBwdStatus::empty) return true;
    if (r.status == MsdaBwdStatus::invalid_value || null_pointer) rc = (int)hipErrorInvalidValue;
    else if (r.status == MsdaBwdStatus::not_supported) rc = (int)hipErrorNotSupported;
    if (!rc) g_last_bwd_route = r.kind;
    return rc != 0;
}

// the LDS-window routes of both entries
static int run_route(const MsdaBwdRoute &r, const MsdaBwdCall &c)
{
    int rc;
    switch (r.kind) {
    case MsdaBwdKind::twopass: {
        // a stream-ordered scratch carries the locality probe's verdict to both kernels: calls whose taps are far from their
        // queries (e.g. uniformly random locations) run the lane-group backward inside the first launch instead -- no host
        // synchronisation.  (No probe means something else to the sampling kernels -- "take your own sample and skip the tiles
        // the grad_value kernel has taken along" -- and this route's grad_value kernel never takes a tile along: an allocation
        // failure is returned, not papered over.)
        int *hits = nullptr;
        const hipError_t arc = hipMallocAsync(reinterpret_cast<void **>(&hits), MSDA_PROBE_INTS * sizeof(int), c.st);
        if (arc != hipSuccess || !hits) return (int)(arc != hipSuccess ? arc : hipErrorOutOfMemory);
        rc = msda_launch_locality_probe(c.st, c.loc, c.shapes, c.B, c.S, c.M, c.L, hits);
        if (!rc) rc = msda_backward_value_tok(c, hits);
        if (!rc) rc = msda_backward_sampling(c, r.sampling, hits);
        (void)hipFreeAsync(hits, c.st);
        return rc;
    }
    case MsdaBwdKind::split:
        // no probe, no scratch: both kernels take the window shift and the stand-down decision from their jobs' own samples
        rc = msda_backward_scatter(c, 1);
        return rc ? rc : msda_backward_sampling(c, r.sampling, nullptr);
    case MsdaBwdKind::onepass: return msda_backward_onepass(c, 1);
    case MsdaBwdKind::fused_onepass: return msda_backward_onepass(c, 0);
    case MsdaBwdKind::deterministic:
    case MsdaBwdKind::fused_deterministic: return msda_backward_deterministic(c);
    case MsdaBwdKind::fused_split:
        rc = msda_backward_scatter(c, 0);
        return rc ? rc : msda_backward_fused_sampling(c);
    case MsdaBwdKind::fused_twopass:
        rc = msda_backward_value_tok(c, nullptr);
        return rc ? rc : msda_backward_fused_sampling(c);
    case MsdaBwdKind::fused_groups:
        rc = msda_backward_value_tok(c, nullptr);
        return rc ? rc : msda_backward_sampling(c, r.sampling, nullptr);
    default: return (int)hipErrorInvalidValue;
    }
}

template <typename T>
static int backward_entry(void *stream, const T *grad_col, const T *value, const int64_t *shapes,
                          const int64_t *lsi, const T *loc, const T *aw, int B, int S, int M, int D, int L,
                          int Lq, int P, T *grad_value, T *grad_loc, T *grad_aw)
{
    const bool a16 = aligned(value, 16) && aligned(grad_col, 16);
    const bool all16 = a16 && aligned(loc, 16) && aligned(aw, 16) && aligned(grad_value, 16) && aligned(grad_loc, 16) &&
                       aligned(grad_aw, 16);
    const MsdaBwdRoute r = msda_backward_route(sizeof(T) == 4 ? MsdaBwdEntry::public_f32 : MsdaBwdEntry::public_f64, B, S, M, D, L, Lq, P, 0,
                                               all16, a16, backward_knob(), backward_deterministic().load(std::memory_order_relaxed) != 0);
    int rc;
    if (route_refused(r, !grad_col || !value || !shapes || !lsi || !loc || !aw || !grad_value || !grad_loc || !grad_aw, rc)) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if constexpr (sizeof(T) == 4) {
        if (r.kind != MsdaBwdKind::atomic)
            return run_route(r, MsdaBwdCall{st, grad_col, value, shapes, lsi, loc, aw, nullptr, 0, 0, nullptr, false, B, S, M, D, L,
                                            grad_value, grad_loc, grad_aw});
    }
    constexpr int WIDE = 16 / (int)sizeof(T);
    if (r.lanes_vec == 1) return launch_lanes_g<T, 1>(r.lanes_g, st, MSDA_BWD_ARGS);
    if (r.lanes_vec == WIDE) return launch_lanes_g<T, WIDE>(r.lanes_g, st, MSDA_BWD_ARGS);
    const int64_t total = (int64_t)B * Lq * M;
    int64_t blocks = (total + 255) / 256;
    if (blocks > (1 << 20)) blocks = 1 << 20;
    hipLaunchKernelGGL((msda_bwd_serial<T>), dim3((unsigned)blocks), dim3(256), 0, st, MSDA_BWD_ARGS);
    return (int)hipGetLastError();
}

}  // namespace mvdetr

extern "C" {

int mvdetr_msda_backward_f32(void *stream, const float *grad_col, const float *value,
                             const int64_t *spatial_shapes, const int64_t *level_start_index,
                             const float *sampling_loc, const float *attn_weight, int batch,
                             int spatial_size, int num_heads, int channels, int num_levels,
                             int num_query, int num_point, float *grad_value,
                             float *grad_sampling_loc, float *grad_attn_weight)
{
    return mvdetr::backward_entry<float>(stream, grad_col, value, spatial_shapes, level_start_index,
                                         sampling_loc, attn_weight, batch, spatial_size, num_heads,
                                         channels, num_levels, num_query, num_point, grad_value,
                                         grad_sampling_loc, grad_attn_weight);
}

int mvdetr_msda_set_backward_deterministic(int on)
{
    return mvdetr::backward_deterministic().exchange(on ? 1 : 0);
}

int mvdetr_msda_get_backward_deterministic(void) { return mvdetr::backward_deterministic().load(std::memory_order_relaxed); }

int mvdetr_msda_release_scratch(void) { return mvdetr::msda_release_det_scratch(); }

const char *mvdetr_msda_last_backward_route(void) { return mvdetr::msda_backward_route_name(mvdetr::g_last_bwd_route); }

int mvdetr_msda_backward_fused_f32(void *stream, const float *grad_output, const float *value,
                                   const int64_t *spatial_shapes, const int64_t *level_start_index,
                                   const float *reference_points, int64_t ref_batch_stride, const float *raw,
                                   int raw_query_stride, const float *stats, const float *out, int batch, int spatial_size,
                                   int num_heads, int channels, int num_levels, int num_point, float *grad_value,
                                   float *grad_raw)
{
    using namespace mvdetr;
    const bool all16 = aligned(grad_output, 16) && aligned(value, 16) && aligned(raw, 16) && aligned(out, 16) && aligned(grad_value, 16) &&
                       aligned(grad_raw, 16) && aligned(reference_points, 8) && aligned(stats, 8) && !(ref_batch_stride & 1);
    const MsdaBwdRoute r = msda_backward_route(MsdaBwdEntry::fused, batch, spatial_size, num_heads, channels, num_levels, spatial_size,
                                               num_point, raw_query_stride, all16, all16, backward_knob(),
                                               backward_deterministic().load(std::memory_order_relaxed) != 0);
    int rc;
    if (route_refused(r, !grad_output || !value || !spatial_shapes || !level_start_index || !reference_points || !raw || !stats || !out ||
                             !grad_value || !grad_raw, rc))
        return rc;
    return run_route(r, MsdaBwdCall{reinterpret_cast<hipStream_t>(stream), grad_output, value, spatial_shapes, level_start_index, raw, stats,
                                    reference_points, ref_batch_stride, raw_query_stride, out, true, batch, spatial_size, num_heads, channels,
                                    num_levels, grad_value, grad_raw, nullptr});
}

int mvdetr_msda_backward_f64(void *stream, const double *grad_col, const double *value,
                             const int64_t *spatial_shapes, const int64_t *level_start_index,
                             const double *sampling_loc, const double *attn_weight, int batch,
                             int spatial_size, int num_heads, int channels, int num_levels,
                             int num_query, int num_point, double *grad_value,
                             double *grad_sampling_loc, double *grad_attn_weight)
{
    return mvdetr::backward_entry<double>(stream, grad_col, value, spatial_shapes, level_start_index,
                                          sampling_loc, attn_weight, batch, spatial_size, num_heads,
                                          channels, num_levels, num_query, num_point, grad_value,
                                          grad_sampling_loc, grad_attn_weight);
}

}  // extern "C"

// Multi-scale deformable attention forward, LDS-tiled encoder kernel -- gfx950 (MI355X).
//
// Shape of the problem (MVDeTr's shadow transformer, and any deformable *encoder* self-attention):
// the queries ARE the value tokens (Lq == S), a query's reference point is its own cell, and the
// learned offsets are a few pixels.  So the 8x16 block of neighbouring queries of one level samples,
// in every source level, a small window around the same normalised position.  The gather kernel
// pulls every one of the 4 corners x L*P taps x 64-byte head segments through the texture-address
// path (4.3 GB of L2->L1 traffic at Wildtrack size, 67 M cache-line requests); here a workgroup
//
//   1. owns a TH x TW tile of query cells of one level and a 128-byte slice of the token row
//      (two 16-channel heads, or one 32-channel head),
//   2. for each source level copies the (TH+2R) x (TW+2R) window of that slice into LDS with
//      full-line coalesced loads (zero-filled outside the level, so zero padding costs nothing),
//   3. lets each lane -- one (query, head) pair, all D channels in registers -- take its P taps of
//      that level from LDS with ds_read_b128,
//   4. remembers (bit mask) the rare taps whose footprint falls outside the window and finishes
//      them afterwards straight from global memory.
//
// Correct for ANY sampling locations (step 4); fast when they are local.  Shapes and level
// offsets are read on the device, so the host never needs them: the grid is persistent and each
// workgroup strides over the tile list it derives from spatial_shapes.
//
// Replaces (together with msda_forward.hip) ms_deformable_im2col_gpu_kernel of the reference
// (multiview_detector/models/ops/src/cuda/ms_deform_im2col_cuda.cuh:237-299).
#include "common.h"
#include "msda_dispatch.h"
#include "msda_tile.h"
#include "msda_tile_body.h"
#include "msda_gather_body.h"
#include <stdlib.h>
#include <string.h>

namespace mvdetr {

template <typename Cfg, int FUSED>
__global__ __launch_bounds__(Cfg::THREADS, Cfg::WAVES_PER_SIMD) void msda_fwd_tile(
    const float *__restrict__ value, const int64_t *__restrict__ shapes,
    const int64_t *__restrict__ lsi, const float *__restrict__ loc, const float *__restrict__ aw,
    const float *__restrict__ ref, int64_t ref_bstride, SamplingLayout lay, QueryLevels qr, int B, int S, int M,
    int L, float *__restrict__ out, const int *__restrict__ local_hits)
{
    extern __shared__ __attribute__((aligned(16))) float win[];
    if constexpr (FUSED == 0) {
        // the locality probe found the taps far from their queries: windows would be wasted, gather instead
        if (local_hits && *local_hits * MSDA_PROBE_NEAR_DIV < MSDA_PROBE_SAMPLES) {
            msda_fwd_gather_body<float, 4>((int64_t)blockIdx.x * Cfg::THREADS + threadIdx.x, (int64_t)gridDim.x * Cfg::THREADS,
                                           value, shapes, lsi, loc, aw, B, S, M, Cfg::D, L, S, TILE_P, out);
            return;
        }
    }
    msda_fwd_tile_body<Cfg, FUSED>(win, value, shapes, lsi, loc, aw, ref, ref_bstride, lay, qr, B, S, M, L, out);
}

// (maximum, 1 / sum exp) per (query, head): what msda_fwd_group2 leaves in `stats` from its online softmax, for the fused
// training calls that kernel does not take.  The backward recomputes a = __expf(logit - max) * (1 / sum) with the same intrinsic.
__global__ __launch_bounds__(256) void msda_softmax_stats_kernel(const float *__restrict__ logits, SamplingLayout lay,
                                                                 int64_t queries, int M, int L, float *__restrict__ stats)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < queries * M; i += (int64_t)gridDim.x * 256) {
        const int head = (int)(i % M);
        const float *wp = logits + (i / M) * lay.q_w + lay.head_w(head);
        float m = -INFINITY;
        for (int l = 0; l < L; ++l) {
            const float4 v = *reinterpret_cast<const float4 *>(wp + l * lay.l_w);
            m = fmaxf(fmaxf(m, fmaxf(v.x, v.y)), fmaxf(v.z, v.w));
        }
        float s = 0.f;
        for (int l = 0; l < L; ++l) {
            const float4 v = *reinterpret_cast<const float4 *>(wp + l * lay.l_w);
            s += (__expf(v.x - m) + __expf(v.y - m)) + (__expf(v.z - m) + __expf(v.w - m));
        }
        *reinterpret_cast<float2 *>(stats + i * 2) = make_float2(m, 1.f / s);
    }
}

int msda_softmax_stats(hipStream_t st, const float *logits, SamplingLayout lay, int64_t queries, int M, int L, float *stats)
{
    const int64_t n = queries * M;
    if (n == 0) return 0;
    const unsigned blocks = (unsigned)((n + 255) / 256 < 8192 ? (n + 255) / 256 : 8192);
    hipLaunchKernelGGL(msda_softmax_stats_kernel, dim3(blocks), dim3(256), 0, st, logits, lay, queries, M, L, stats);
    return (int)hipGetLastError();
}

template <typename Cfg, int FUSED>
static int launch_tile(const MsdaFwdCall &c)
{
    static PersistentGrid grid;
    const int blocks = grid.occupancy(&msda_fwd_tile<Cfg, FUSED>, Cfg::THREADS, Cfg::LDS_BYTES, 2);
    static const KernelResources res = kernel_resources(reinterpret_cast<const void *>(&msda_fwd_tile<Cfg, FUSED>));
    msda_note_forward_kernel("msda_fwd_tile", &res);
    hipLaunchKernelGGL((msda_fwd_tile<Cfg, FUSED>), dim3((unsigned)blocks), dim3(Cfg::THREADS), Cfg::LDS_BYTES, c.st, c.value, c.shapes, c.lsi,
                       c.loc, c.aw, c.ref, c.ref_bstride, c.lay, c.qr, c.B, c.S, c.M, c.L, c.out, c.probe);
    return (int)hipGetLastError();
}

template <typename Cfg>
static int tile_of_ref_mode(const MsdaFwdCall &c)
{
    return c.ref_mode == 2 ? launch_tile<Cfg, 2>(c) : c.ref_mode ? launch_tile<Cfg, 1>(c) : launch_tile<Cfg, 0>(c);
}

int msda_forward_tile(const MsdaFwdCall &c)
{
    // (128-byte slices; 64-byte ones -- twice the workgroups per CU -- were measured slower: DESIGN 5.2)
    if (c.D == 16) return tile_of_ref_mode<CfgWide16>(c);
    if (c.D == 32) return tile_of_ref_mode<CfgWide32>(c);
    return (int)hipErrorInvalidValue;
}

}  // namespace mvdetr

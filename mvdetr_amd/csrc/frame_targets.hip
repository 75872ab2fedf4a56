// Training targets on the device: the CenterNet-style ground truth of `maps` equally shaped [H, W] maps (the reference's get_gt,
// datasets/frameDataset.py:19-46, with the box half of its random_affine, utils/image_utils.py:46-83) from padded, device-resident
// annotations, in ONE launch and without reading any count back.  The target-side counterpart of ingest.hip.
//
// Arithmetic: frame_targets_core.h, shared with the host path operation for operation; fp64 until the stated roundings and
// compiled without FMA contraction: the Makefile's -ffp-contract=fast would fuse M00 x + M01 y, so it builds this file with
// -ffp-contract=off on top of the pragma below (the pragma alone leaves the backend free to fuse under =fast).  The kernel
// has no sin / cos / sqrt / exp: the per-map shrink factor and the gaussian patch are made on the host and passed in.
//
// Kernel.  A workgroup of 256 threads belongs to one map and owns 1024 consecutive cells of its heat map.  Each workgroup
//   1. rebuilds the map's slot list in LDS: an object per thread and round of 256, the box through M and the keep rules, then the
//      rank among the kept ones by a wave ballot + the per-wave counts (kept boxes are compacted IN ORDER; without M every object
//      is kept and its slot is its index);
//   2. copies the patch table to LDS;
//   3. renders its cells as a gather: per cell the maximum of the patch entries of the slots whose centre is within the radius,
//      one store.  No zero-fill pass, no atomics: every cell is written exactly once and the result is bit-reproducible.
// The first workgroup of a map also writes the slot outputs, every slot of [0, top_k) exactly once.
#pragma clang fp contract(off)
#include "common.h"
#include "frame_targets_core.h"
#include "../../include/mvdetr_ops.h"

#include <atomic>

namespace mvdetr {

constexpr int FT_THREADS = 256;
constexpr int FT_WAVES = FT_THREADS / MVDETR_WAVE;
constexpr int FT_CELLS = 4;                                 // cells per thread
constexpr int FT_PATCH = (2 * MVDETR_FT_MAX_RADIUS + 1) * (2 * MVDETR_FT_MAX_RADIUS + 1);

static std::atomic<int64_t> g_ft_launches{0};

struct FtArgs {
    const double *coords;        // [maps, cap, 4] boxes or [maps, cap, 2] points
    const int32_t *count;        // [maps]
    const int64_t *pids;         // [maps, cap] or null
    const double *mats;          // [maps, 9] or null
    const double *shrink;        // [maps] or null (= 1)
    const uint8_t *keep;         // [maps] or null (= all kept)
    const float *patch;          // [2 radius + 1, 2 radius + 1]
    int is_boxes, maps, cap, H, W, img_h, img_w, radius, top_k;
    double reduce;
    float *heatmap;
    uint8_t *reg_mask;
    int64_t *idx, *pid;
    float *offset, *wh;          // wh: null for points
};

__global__ __launch_bounds__(FT_THREADS) void frame_targets_kernel(FtArgs g)
{
    __shared__ int s_cx[MVDETR_FT_MAX_CAP], s_cy[MVDETR_FT_MAX_CAP];        // slot -> truncated centre; cx = -1: empty slot
    __shared__ float s_patch[FT_PATCH];
    __shared__ int s_wave[FT_WAVES];
    const int m = blockIdx.y, t = threadIdx.x, lane = t % MVDETR_WAVE, wave = t / MVDETR_WAVE;
    const bool first = blockIdx.x == 0;
    const int r = g.radius, side = 2 * r + 1;
    for (int i = t; i < side * side; i += FT_THREADS) s_patch[i] = g.patch[i];

    int n = min(max(g.count[m], 0), g.cap);
    if (g.keep && !g.keep[m]) n = 0;
    const int64_t slot0 = (int64_t)m * g.top_k;
    int used = 0;                                                            // slots handed out so far (uniform)
    for (int base = 0; base < n; base += FT_THREADS) {
        const int i = base + t;
        bool live = i < n;
        double x = 0, y = 0, w = 0, h = 0;
        if (live) {
            const int64_t at = (int64_t)m * g.cap + i;
            if (g.is_boxes) {
                double b[4] = {g.coords[at * 4], g.coords[at * 4 + 1], g.coords[at * 4 + 2], g.coords[at * 4 + 3]};
                if (g.mats)
                    live = ft_move_box(b, g.mats + (int64_t)m * 9, g.shrink ? g.shrink[m] : 1.0, (double)(g.img_w - 1),
                                       (double)(g.img_h - 1), b);
                x = (b[0] + b[2]) / 2, y = b[3], w = b[2] - b[0], h = b[3] - b[1];      // the foot point and the size
            } else {
                x = g.coords[at * 2], y = g.coords[at * 2 + 1];
            }
        }
        const unsigned long long ballot = __ballot(live);
        const int rank = __popcll(ballot & ((1ull << lane) - 1ull));
        if (lane == 0) s_wave[wave] = __popcll(ballot);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int v = 0; v < FT_WAVES; ++v) {
            const int c = s_wave[v];
            total += c;
            if (v < wave) before += c;
        }
        if (live) {
            const int slot = used + before + rank;                           // < n <= cap <= top_k
            const FtSlot s = ft_slot(x, y, w, h, g.reduce, g.H, g.W);
            s_cx[slot] = s.inside ? s.cx : -1;
            s_cy[slot] = s.cy;
            if (first) {
                const int64_t o = slot0 + slot;
                g.reg_mask[o] = s.inside ? 1 : 0;
                g.idx[o] = s.inside ? (int64_t)s.cy * g.W + s.cx : 0;
                g.pid[o] = s.inside && g.pids ? g.pids[(int64_t)m * g.cap + i] : 0;
                g.offset[o * 2] = s.off_x;
                g.offset[o * 2 + 1] = s.off_y;
                if (g.wh) {
                    g.wh[o * 2] = s.wh_x;
                    g.wh[o * 2 + 1] = s.wh_y;
                }
            }
        }
        used += total;
        __syncthreads();                                                     // s_wave is rewritten by the next round
    }
    __syncthreads();                                                         // (n = 0: the patch copy above)
    if (first) {
        for (int slot = used + t; slot < g.top_k; slot += FT_THREADS) {
            const int64_t o = slot0 + slot;
            g.reg_mask[o] = 0;
            g.idx[o] = 0;
            g.pid[o] = 0;
            g.offset[o * 2] = g.offset[o * 2 + 1] = 0.f;
            if (g.wh) g.wh[o * 2] = g.wh[o * 2 + 1] = 0.f;
        }
    }

    const int64_t cells = (int64_t)g.H * g.W;
    float *hm = g.heatmap + (int64_t)m * cells;
#pragma unroll
    for (int j = 0; j < FT_CELLS; ++j) {
        const int64_t cell = ((int64_t)blockIdx.x * FT_CELLS + j) * FT_THREADS + t;
        if (cell >= cells) break;
        const int cy = (int)(cell / g.W), cx = (int)(cell - (int64_t)cy * g.W);
        float v = 0.f;
        for (int s = 0; s < used; ++s) {
            const int ox = s_cx[s];
            if (ox < 0) continue;
            const int dx = cx - ox, dy = cy - s_cy[s];
            if (dx >= -r && dx <= r && dy >= -r && dy <= r) v = fmaxf(v, s_patch[(dy + r) * side + dx + r]);
        }
        hm[cell] = v;
    }
}

}  // namespace mvdetr

extern "C" {

int mvdetr_frame_targets_f64(void *stream, const double *coords, int is_boxes, const int32_t *count, const int64_t *pids,
                             const double *mats, const double *shrink, const uint8_t *keep, const float *patch, int maps, int cap,
                             int height, int width, int img_h, int img_w, int radius, int top_k, double reduce, float *heatmap,
                             uint8_t *reg_mask, int64_t *idx, int64_t *pid, float *offset, float *wh)
{
    using namespace mvdetr;
    if (maps < 0 || maps > 65535 || cap < 1 || cap > MVDETR_FT_MAX_CAP || top_k < cap || height < 1 || width < 1 ||
        height > MVDETR_FT_MAX_DIM || width > MVDETR_FT_MAX_DIM || radius < 0 || radius > MVDETR_FT_MAX_RADIUS || !(reduce > 0.0))
        return 1;
    if ((!is_boxes && (mats || wh)) || (is_boxes && !wh) || (!mats && shrink) || (mats && (img_h < 1 || img_w < 1))) return 1;
    if (maps == 0) return 0;
    if (!coords || !count || !patch || !heatmap || !reg_mask || !idx || !pid || !offset) return 1;
    FtArgs g;
    g.coords = coords, g.count = count, g.pids = pids, g.mats = mats, g.shrink = shrink, g.keep = keep, g.patch = patch;
    g.is_boxes = is_boxes ? 1 : 0, g.maps = maps, g.cap = cap, g.H = height, g.W = width, g.img_h = img_h, g.img_w = img_w;
    g.radius = radius, g.top_k = top_k, g.reduce = reduce;
    g.heatmap = heatmap, g.reg_mask = reg_mask, g.idx = idx, g.pid = pid, g.offset = offset, g.wh = wh;
    const dim3 grid((unsigned)ceil_div((int64_t)height * width, FT_THREADS * FT_CELLS), (unsigned)maps), block(FT_THREADS);
    hipLaunchKernelGGL(frame_targets_kernel, grid, block, 0, static_cast<hipStream_t>(stream), g);
    ++g_ft_launches;
    return (int)hipGetLastError();
}

int mvdetr_frame_targets_max_radius(void) { return MVDETR_FT_MAX_RADIUS; }

int64_t mvdetr_frame_targets_launch_count(void) { return mvdetr::g_ft_launches.load(); }

}  // extern "C"

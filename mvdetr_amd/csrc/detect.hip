// Detection extraction on the device: world heat-map logits (+ offsets) -> ground-plane detections, the last stage of the
// reference's test loop (multiview_detector/trainer.py:121-135 = utils/decode.py:80-93 mvdet_decode, the cls_thres test and
// utils/nms.py:7-44) without a host round-trip.
//
// Two launches per call, neither sized by anything read back from the device:
//   detect_compact  (ceil(H W / 1024), B) workgroups of 256 threads.  Each owns 1024 cells of one frame: sigmoid, threshold,
//                   position, and the survivors (key, x, y, cell) appended to the workgroup's OWN 1024-entry segment of the
//                   workspace through an LDS counter; the segment's count goes to counts[b][k].  No device-scope atomic and
//                   nothing that must be zero on entry: the workspace may hold anything.  The order inside a segment is
//                   whatever the LDS atomic made it; nothing downstream depends on it (the key carries the cell index).
//   detect_nms      one 1024-thread workgroup per frame.  Sums the segment counts (n), gathers the segments into one list --
//                   in LDS when n <= nms_capacity<T>() (3072 fp32 / 1728 fp64 candidates, 48 KiB), else in the workspace --
//                   and runs the greedy NMS on it.  The kernel boundary orders the two kernels' memory traffic.
// The NMS needs no sort: every sweep over the list suppresses what lies within dist_thres of the point kept last and finds
// the maximum of the survivors by (score, cell index) -- one pass per kept point and one workgroup reduction.  Slot j of the
// list is only ever written by thread j % 1024, so the sweeps need no atomics and the result does not depend on timing.
// Finite top_k: the same sweep counts the candidates (dead ones too) that come before the kept point; a kept point with
// top_k or more before it is outside the reference's idx[-top_k:] and ends the loop unwritten.
//
// Arithmetic is written so that it is the same on any IEEE machine: one rounded add and one rounded multiply per coordinate,
// products and sum of the squared distance rounded separately (this file is compiled with -ffp-contract=fast: the __f*_rn /
// __d*_rn forms are never contracted), correctly rounded sqrt and divide.  Only exp may differ from a host's in the last place.
// Tie rule (this library's; the reference's is whatever an unstable torch.sort does): equal scores -> higher index first.
//
// distance_nms runs the NMS stage alone on caller-supplied points (the contract of utils/nms.py), same device function.
// MVDETR_DETECT_ROUTE=global (read once per process) keeps the list in the workspace at every size.
#include "common.h"
#include "../../include/mvdetr_ops.h"

#include <atomic>
#include <cstdlib>
#include <cstring>

namespace mvdetr {

constexpr int DET_NMS_THREADS = 1024;
constexpr int DET_NMS_WAVES = DET_NMS_THREADS / MVDETR_WAVE;
constexpr int DET_TILE = 1024;                 // cells (and segment entries) per detect_compact workgroup
constexpr int DET_COMPACT_THREADS = 256;
constexpr int DET_LDS_BYTES = 48 * 1024;
constexpr int DET_DEAD = (int)0x80000000u;     // bit 31 of a list entry's index: suppressed or already kept
constexpr int64_t DET_MAX_CELLS = (int64_t)1 << 30;

static std::atomic<const char *> g_detect_last_kernel{"none"};
static std::atomic<int64_t> g_detect_launches{0};

template <typename T> struct DetNum;
template <> struct DetNum<float> {
    using K = uint32_t;
    // order-preserving map of a float onto unsigned integers; -0 and +0 get the same key (they are a tie)
    __device__ static K key(float s)
    {
        const uint32_t b = __float_as_uint(s + 0.f);
        return (b >> 31) ? ~b : (b | 0x80000000u);
    }
    __device__ static float score(K k) { return __uint_as_float((k >> 31) ? (k & 0x7fffffffu) : ~k); }
    __device__ static float add(float a, float b) { return __fadd_rn(a, b); }
    __device__ static float mul(float a, float b) { return __fmul_rn(a, b); }
    __device__ static float root(float a) { return __fsqrt_rn(a); }
    __device__ static float sigmoid(float x) { return 1.f / (1.f + expf(-x)); }
    __device__ static K shfl_down(K v, int d) { return (K)__shfl_down((int)v, d); }
};
template <> struct DetNum<double> {
    using K = uint64_t;
    __device__ static K key(double s)
    {
        const uint64_t b = (uint64_t)__double_as_longlong(s + 0.0);
        return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
    }
    __device__ static double score(K k)
    {
        return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
    }
    __device__ static double add(double a, double b) { return __dadd_rn(a, b); }
    __device__ static double mul(double a, double b) { return __dmul_rn(a, b); }
    __device__ static double root(double a) { return __dsqrt_rn(a); }
    __device__ static double sigmoid(double x) { return 1.0 / (1.0 + exp(-x)); }
    __device__ static K shfl_down(K v, int d)
    {
        const uint32_t lo = (uint32_t)__shfl_down((int)(uint32_t)v, d), hi = (uint32_t)__shfl_down((int)(uint32_t)(v >> 32), d);
        return ((uint64_t)hi << 32) | lo;
    }
};

template <typename T> constexpr int nms_capacity()
{
    return DET_LDS_BYTES / (int)(sizeof(typename DetNum<T>::K) + 2 * sizeof(T) + sizeof(int)) / 64 * 64;
}

// one candidate list: key (score), position, index (bit 31 = dead); in LDS or in global memory
template <typename T> struct DetList {
    typename DetNum<T>::K *key;
    T *x, *y;
    int *idx;
};

// where the kept points go: the detect outputs of one frame (det [cap, 3], cell [cap]) or distance_nms's keep [cap]
template <typename T> struct DetOut {
    T *det;
    int32_t *cell;
    int64_t *keep;
    int cap;
};

// byte layout of the workspace for `batch` frames of `cells` cells: counts [batch, nblk] int32, then the segment arrays and the
// list arrays (key, x, y, idx), every one [batch, nblk * DET_TILE]
struct DetWorkspace {
    int nblk;
    int64_t stride;          // entries per frame = nblk * DET_TILE
    int64_t counts, key[2], x[2], y[2], idx[2], bytes;
};

static DetWorkspace workspace_layout(int64_t batch, int64_t cells, int elem)
{
    DetWorkspace w;
    w.nblk = ceil_div(cells, DET_TILE);
    w.stride = (int64_t)w.nblk * DET_TILE;
    const int64_t per = batch * w.stride;
    int64_t at = (batch * w.nblk * (int64_t)sizeof(int32_t) + 15) / 16 * 16;
    w.counts = 0;
    for (int s = 0; s < 2; ++s) {
        w.key[s] = at; at += per * elem;
        w.x[s] = at;   at += per * elem;
        w.y[s] = at;   at += per * elem;
        w.idx[s] = at; at += (per * (int64_t)sizeof(int32_t) + 15) / 16 * 16;
    }
    w.bytes = at;
    return w;
}

template <typename T> static DetList<T> list_at(void *workspace, const DetWorkspace &w, int which)
{
    char *p = static_cast<char *>(workspace);
    return DetList<T>{reinterpret_cast<typename DetNum<T>::K *>(p + w.key[which]), reinterpret_cast<T *>(p + w.x[which]),
                      reinterpret_cast<T *>(p + w.y[which]), reinterpret_cast<int *>(p + w.idx[which])};
}

struct DetStrides {
    int64_t hm[4], off[4];
};

template <typename T>
__global__ __launch_bounds__(DET_COMPACT_THREADS) void detect_compact(const T *__restrict__ hm, const T *__restrict__ off, DetStrides st,
                                                                       int H, int W, T reduce, T cls_thres, int swap_xy,
                                                                       DetList<T> seg, int *__restrict__ counts, int nblk, int64_t stride)
{
    using N = DetNum<T>;
    __shared__ int s_count;
    const int b = blockIdx.y, k = blockIdx.x, cells = H * W;
    if (threadIdx.x == 0) s_count = 0;
    __syncthreads();
    const int64_t base = (int64_t)b * stride + (int64_t)k * DET_TILE;
    for (int e = 0; e < DET_TILE / DET_COMPACT_THREADS; ++e) {
        const int cell = k * DET_TILE + e * DET_COMPACT_THREADS + (int)threadIdx.x;
        if (cell >= cells) break;
        const int row = cell / W, col = cell - row * W;
        const T s = N::sigmoid(hm[b * st.hm[0] + row * st.hm[2] + col * st.hm[3]]);
        if (!(s > cls_thres)) continue;                                    // NaN never passes
        T dx = T(0.5), dy = T(0.5);
        if (off) {
            const T *o = off + b * st.off[0] + row * st.off[2] + col * st.off[3];
            dx = o[0];
            dy = o[st.off[1]];
        }
        const T x = N::mul(N::add(T(col), dx), reduce), y = N::mul(N::add(T(row), dy), reduce);
        const int slot = atomicAdd(&s_count, 1);                           // < DET_TILE: one per cell of this workgroup
        seg.key[base + slot] = N::key(s);
        seg.x[base + slot] = swap_xy ? y : x;
        seg.y[base + slot] = swap_xy ? x : y;
        seg.idx[base + slot] = cell;
    }
    __syncthreads();
    if (threadIdx.x == 0) counts[b * nblk + k] = s_count;
}

template <typename T> struct DetBest {
    typename DetNum<T>::K key;
    int idx, j;                                                            // j < 0: none
};

template <typename T> __device__ __forceinline__ bool det_before(typename DetNum<T>::K ka, int ia, typename DetNum<T>::K kb, int ib)
{
    return ka > kb || (ka == kb && ia > ib);
}

template <typename T> struct DetScratch {
    typename DetNum<T>::K key[DET_NMS_WAVES];
    int idx[DET_NMS_WAVES], j[DET_NMS_WAVES], rank[DET_NMS_WAVES];
};

// maximum of `best` by (key, idx) and sum of `rank` over the workgroup, returned to every thread
template <typename T> __device__ void det_reduce(DetBest<T> &best, int &rank, DetScratch<T> &s)
{
    using N = DetNum<T>;
    for (int d = MVDETR_WAVE / 2; d > 0; d >>= 1) {
        DetBest<T> o;
        o.key = N::shfl_down(best.key, d);
        o.idx = __shfl_down(best.idx, d);
        o.j = __shfl_down(best.j, d);
        rank += __shfl_down(rank, d);
        if (o.j >= 0 && (best.j < 0 || det_before<T>(o.key, o.idx, best.key, best.idx))) best = o;
    }
    const int wave = threadIdx.x / MVDETR_WAVE;
    __syncthreads();                                                       // the previous round's readers are done
    if (threadIdx.x % MVDETR_WAVE == 0) {
        s.key[wave] = best.key; s.idx[wave] = best.idx; s.j[wave] = best.j; s.rank[wave] = rank;
    }
    __syncthreads();
    best.j = -1;
    rank = 0;
    for (int w = 0; w < DET_NMS_WAVES; ++w) {
        rank += s.rank[w];
        if (s.j[w] >= 0 && (best.j < 0 || det_before<T>(s.key[w], s.idx[w], best.key, best.idx)))
            best = DetBest<T>{s.key[w], s.idx[w], s.j[w]};
    }
}

// greedy distance NMS over list[0 .. n): returns the number kept (every thread gets it); thread 0 writes the kept rows
template <typename T>
__device__ int nms_run(const DetList<T> &list, int n, T dist_thres, int top_k, const DetOut<T> &out, DetScratch<T> &scratch)
{
    using N = DetNum<T>;
    using K = typename N::K;
    const bool finite = top_k > 0 && top_k < n;
    int kept = 0, jl = -1, il = 0;
    K kl = 0;
    T xl = T(0), yl = T(0);
    for (;;) {
        DetBest<T> best{0, 0, -1};
        int rank = 0;
        for (int j = threadIdx.x; j < n; j += DET_NMS_THREADS) {
            const int ij = list.idx[j];
            const K kj = list.key[j];
            if (finite && jl >= 0 && det_before<T>(kj, ij & ~DET_DEAD, kl, il)) ++rank;
            if (ij < 0) continue;
            if (jl >= 0) {
                bool dead = j == jl;
                if (!dead) {
                    const T dx = xl - list.x[j], dy = yl - list.y[j];
                    dead = !(N::root(N::add(N::mul(dx, dx), N::mul(dy, dy))) > dist_thres);
                }
                if (dead) {
                    list.idx[j] = ij | DET_DEAD;
                    continue;
                }
            }
            if (best.j < 0 || det_before<T>(kj, ij, best.key, best.idx)) best = DetBest<T>{kj, ij, j};
        }
        det_reduce<T>(best, rank, scratch);
        if (jl >= 0) {
            if (finite && rank >= top_k) break;                            // outside the top_k: so is everything after it
            if (threadIdx.x == 0 && kept < out.cap) {
                if (out.keep) {
                    out.keep[kept] = il;
                } else {
                    out.det[3 * kept + 0] = xl;
                    out.det[3 * kept + 1] = yl;
                    out.det[3 * kept + 2] = N::score(kl);
                    out.cell[kept] = il;
                }
            }
            ++kept;
        }
        if (best.j < 0) break;
        jl = best.j; il = best.idx; kl = best.key;
        xl = list.x[jl];
        yl = list.y[jl];
    }
    return kept;
}

template <typename T> __device__ DetList<T> lds_list(unsigned char *lds)
{
    using K = typename DetNum<T>::K;
    constexpr int CAP = nms_capacity<T>();
    K *key = reinterpret_cast<K *>(lds);
    T *x = reinterpret_cast<T *>(key + CAP);
    return DetList<T>{key, x, x + CAP, reinterpret_cast<int *>(x + 2 * CAP)};
}

template <typename T>
__global__ __launch_bounds__(DET_NMS_THREADS) void detect_nms(DetList<T> seg, DetList<T> glist, const int *__restrict__ counts, int nblk,
                                                               int64_t stride, T dist_thres, int top_k, int max_det, int force_global,
                                                               T *__restrict__ det, int32_t *__restrict__ cell, int32_t *__restrict__ count)
{
    __shared__ __align__(16) unsigned char lds[DET_LDS_BYTES];
    __shared__ DetScratch<T> scratch;
    __shared__ int s_total, s_alloc;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int *cnt = counts + (int64_t)b * nblk;
    if (tid == 0) s_total = s_alloc = 0;
    __syncthreads();
    int part = 0;
    for (int k = tid; k < nblk; k += DET_NMS_THREADS) part += min(max(cnt[k], 0), DET_TILE);
    if (part) atomicAdd(&s_total, part);
    __syncthreads();
    const int n = s_total;                                                 // <= nblk * DET_TILE = stride
    DetList<T> list;
    if (n <= nms_capacity<T>() && !force_global) {
        list = lds_list<T>(lds);
    } else {
        const int64_t o = (int64_t)b * stride;
        list = DetList<T>{glist.key + o, glist.x + o, glist.y + o, glist.idx + o};
    }
    // gather: a wave per segment; where a segment lands in the list does not matter
    const int lane = tid % MVDETR_WAVE;
    for (int k = tid / MVDETR_WAVE; k < nblk; k += DET_NMS_WAVES) {
        const int c = min(max(cnt[k], 0), DET_TILE);
        int at = 0;
        if (lane == 0 && c) at = atomicAdd(&s_alloc, c);
        at = __shfl(at, 0);
        const int64_t from = (int64_t)b * stride + (int64_t)k * DET_TILE;
        for (int e = lane; e < c; e += MVDETR_WAVE) {
            list.key[at + e] = seg.key[from + e];
            list.x[at + e] = seg.x[from + e];
            list.y[at + e] = seg.y[from + e];
            list.idx[at + e] = seg.idx[from + e] & ~DET_DEAD;
        }
    }
    __syncthreads();
    const DetOut<T> out{det + (int64_t)b * max_det * 3, cell + (int64_t)b * max_det, nullptr, max_det};
    const int kept = nms_run<T>(list, n, dist_thres, top_k, out, scratch);
    if (tid == 0) count[b] = kept;                                         // the true number, also beyond max_det
    for (int r = min(kept, max_det) + tid; r < max_det; r += DET_NMS_THREADS) {
        out.det[3 * r] = out.det[3 * r + 1] = out.det[3 * r + 2] = T(0);
        out.cell[r] = 0;
    }
}

template <typename T>
__global__ __launch_bounds__(DET_NMS_THREADS) void distance_nms(const T *__restrict__ points, const T *__restrict__ scores, int n, T dist_thres,
                                                                 int top_k, int force_global, DetList<T> glist, int64_t *__restrict__ keep,
                                                                 int32_t *__restrict__ count)
{
    __shared__ __align__(16) unsigned char lds[DET_LDS_BYTES];
    __shared__ DetScratch<T> scratch;
    const DetList<T> list = (n <= nms_capacity<T>() && !force_global) ? lds_list<T>(lds) : glist;
    for (int j = threadIdx.x; j < n; j += DET_NMS_THREADS) {
        list.key[j] = DetNum<T>::key(scores[j]);
        list.x[j] = points[2 * (int64_t)j];
        list.y[j] = points[2 * (int64_t)j + 1];
        list.idx[j] = j;
    }
    __syncthreads();
    const DetOut<T> out{nullptr, nullptr, keep, n};
    const int kept = nms_run<T>(list, n, dist_thres, top_k, out, scratch);
    if (threadIdx.x == 0) count[0] = kept;
    for (int r = kept + threadIdx.x; r < n; r += DET_NMS_THREADS) keep[r] = 0;
}

static int detect_force_global()
{
    static const int v = [] {
        const char *e = getenv("MVDETR_DETECT_ROUTE");
        return (e && !strcmp(e, "global")) ? 1 : 0;
    }();
    return v;
}

template <typename T>
static int detect_forward(void *stream, const T *hm, const int64_t *hm_stride, const T *off, const int64_t *off_stride, int B, int H, int W,
                          double reduce, double cls_thres, double dist_thres, int top_k, int swap_xy, int max_det, void *workspace, T *det,
                          int32_t *cell, int32_t *count)
{
    if (!hm || !hm_stride || (off && !off_stride) || !workspace || !det || !cell || !count || B < 1 || B > 65535 || H < 1 || W < 1 ||
        max_det < 1 || (int64_t)H * W > DET_MAX_CELLS || !aligned(workspace, 16))
        return 1;
    const DetWorkspace w = workspace_layout(B, (int64_t)H * W, sizeof(T));
    DetStrides st{};
    for (int d = 0; d < 4; ++d) {
        st.hm[d] = hm_stride[d];
        st.off[d] = off ? off_stride[d] : 0;
    }
    const DetList<T> seg = list_at<T>(workspace, w, 0), glist = list_at<T>(workspace, w, 1);
    int *counts = reinterpret_cast<int *>(static_cast<char *>(workspace) + w.counts);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int force = detect_force_global();
    detect_compact<T><<<dim3(w.nblk, B), DET_COMPACT_THREADS, 0, s>>>(hm, off, st, H, W, T(reduce), T(cls_thres), swap_xy, seg, counts, w.nblk,
                                                                      w.stride);
    detect_nms<T><<<B, DET_NMS_THREADS, 0, s>>>(seg, glist, counts, w.nblk, w.stride, T(dist_thres), top_k, max_det, force, det, cell, count);
    g_detect_last_kernel = force ? "detect_compact+detect_nms_global" : "detect_compact+detect_nms";
    g_detect_launches.fetch_add(2);
    return (int)hipGetLastError();
}

template <typename T>
static int nms_forward(void *stream, const T *points, const T *scores, int n, double dist_thres, int top_k, void *workspace, int64_t *keep,
                       int32_t *count)
{
    if (!points || !scores || !workspace || !keep || !count || n < 1 || n > DET_MAX_CELLS || !aligned(workspace, 16)) return 1;
    const DetWorkspace w = workspace_layout(1, n, sizeof(T));
    const int force = detect_force_global();
    distance_nms<T><<<1, DET_NMS_THREADS, 0, reinterpret_cast<hipStream_t>(stream)>>>(points, scores, n, T(dist_thres), top_k, force,
                                                                                     list_at<T>(workspace, w, 1), keep, count);
    g_detect_last_kernel = force ? "distance_nms_global" : "distance_nms";
    g_detect_launches.fetch_add(1);
    return (int)hipGetLastError();
}

}  // namespace mvdetr

extern "C" int64_t mvdetr_detect_workspace_bytes(int batch, int height, int width, int elem_size)
{
    if (batch < 1 || height < 1 || width < 1 || (elem_size != 4 && elem_size != 8) || (int64_t)height * width > mvdetr::DET_MAX_CELLS)
        return -1;
    return mvdetr::workspace_layout(batch, (int64_t)height * width, elem_size).bytes;
}

#define MVDETR_DETECT_ENTRIES(T, SFX)                                                                                                     \
    extern "C" int mvdetr_detect_forward_##SFX(void *stream, const T *heatmap, const int64_t *heatmap_stride, const T *offset,              \
                                               const int64_t *offset_stride, int batch, int height, int width, double reduce,             \
                                               double cls_thres, double dist_thres, int top_k, int swap_xy, int max_det, void *workspace,  \
                                               T *det, int32_t *cell, int32_t *count)                                                      \
    {                                                                                                                                     \
        return mvdetr::detect_forward<T>(stream, heatmap, heatmap_stride, offset, offset_stride, batch, height, width, reduce, cls_thres,  \
                                         dist_thres, top_k, swap_xy, max_det, workspace, det, cell, count);                                \
    }                                                                                                                                     \
    extern "C" int mvdetr_distance_nms_##SFX(void *stream, const T *points, const T *scores, int n, double dist_thres, int top_k,          \
                                             void *workspace, int64_t *keep, int32_t *count)                                               \
    {                                                                                                                                     \
        return mvdetr::nms_forward<T>(stream, points, scores, n, dist_thres, top_k, workspace, keep, count);                               \
    }
MVDETR_DETECT_ENTRIES(float, f32)
MVDETR_DETECT_ENTRIES(double, f64)

extern "C" const char *mvdetr_detect_last_kernel(void) { return mvdetr::g_detect_last_kernel.load(); }

extern "C" int64_t mvdetr_detect_launch_count(void) { return mvdetr::g_detect_launches.load(); }

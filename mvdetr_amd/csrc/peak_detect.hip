// Peak extraction on the device: heat-map logits (+ offset, + wh maps) -> the top_k local maxima of every map, the reference's
// ctdet_decode (multiview_detector/utils/decode.py:7-77: sigmoid, 3x3 max-pool equality, two topk, gathers, cat) for
// single-channel maps, as a fixed-capacity result without a host round-trip.
//
// Two launches per call, neither sized by anything read back from the device:
//   peak_compact  (ceil(H W / 1024), B) workgroups of 256 threads.  Each owns a row-major run of 1024 cells of one map.  The
//                 scores of the run, of the run one row up and of the run one row down (each with one cell more on either
//                 side: 3 x 1026 entries) go to LDS once, from ONE expression, so a cell and its neighbour are compared on the
//                 bits everybody else sees.  A cell is a candidate when no cell of its 3x3 neighbourhood inside the map has a
//                 greater score (= its score equals the neighbourhood's maximum: max_pool2d pads with -inf) and, with a
//                 threshold, score > cls_thres.  Survivors (key, cell) are appended to the workgroup's OWN 1024-entry segment
//                 of the workspace through an LDS counter (one atomic per wave: ballot + prefix count); the segment's count
//                 goes to counts[b][k].  No device-scope atomic, nothing that must be zero on entry.  The order inside a
//                 segment is whatever the LDS atomic made it; nothing downstream depends on it.
//   peak_select   one 1024-thread workgroup per map.  Sums the segment counts (n = the map's count), gathers the segments into
//                 one list -- in LDS when n <= peak_capacity<T>() (5120 fp32 / 3392 fp64 candidates, 40 KiB), else in the
//                 workspace -- and finds the m = min(n, top_k) first entries by (score, cell) descending:
//                   1. a digit-by-digit select (8 bits a pass, most significant first, over the score key and then the cell
//                      index: an LDS histogram of integer counts, one wave picks the digit) gives the m-th entry itself;
//                   2. the entries at or before it -- exactly m, the (key, cell) pairs are all different -- are copied to an
//                      LDS array of 1024 slots and ordered by a bitonic network over the next power of two >= m.
//                 Thread r then owns row r: it gathers offset and wh at its cell through their strides and writes the row;
//                 threads m .. top_k - 1 write zeros.  Histogram counts and a sort of distinct keys do not depend on the order
//                 the LDS atomics ran in: the result never depends on timing.
// Non-finite logits: a NaN score is never a candidate and is ignored in its neighbours' test (max_pool2d would propagate it and
// erase the neighbours; this is the library's deviation).  -inf / +inf give scores 0 / 1 and take part as such.
//
// Arithmetic: one rounded add per coordinate; the box is (x - 0.5 w) scale, (y - h) scale, (x + 0.5 w) scale, y scale with
// every product, sum and difference rounded on its own (the pragma below and the __f*_rn / __d*_rn forms: nothing contracts
// into a fused multiply-add although the file is compiled with -ffp-contract=fast).  Only exp may differ from a host's.
// Tie rule (the library's, detect.hip): equal scores -> higher row-major cell index first.
#include "common.h"
#include "../../include/mvdetr_ops.h"

#include <atomic>

#pragma clang fp contract(off)

namespace mvdetr {

constexpr int PK_TILE = 1024;                  // cells (and segment entries) per peak_compact workgroup
constexpr int PK_HALO = PK_TILE + 2;           // a run with one cell more on either side
constexpr int PK_COMPACT_THREADS = 256;
constexpr int PK_SELECT_THREADS = 1024;
constexpr int PK_MAX_TOP_K = PK_SELECT_THREADS;
constexpr int PK_LIST_BYTES = 40 * 1024;
constexpr int64_t PK_MAX_CELLS = (int64_t)1 << 30;

static std::atomic<int> g_peak_last_device{-1};
static std::atomic<int64_t> g_peak_launches{0};

// 1 when a map of the device's last call kept its list in the workspace: reset by peak_compact, set by peak_select, read
// back by mvdetr_peak_detect_last_kernel only
__device__ int g_peak_used_global;

template <typename T> struct PeakNum;
template <> struct PeakNum<float> {
    using K = uint32_t;
    // order-preserving map of a float onto unsigned integers (scores are >= +0: every real key is >= 0x80000000)
    __device__ static K key(float s)
    {
        const uint32_t b = __float_as_uint(s + 0.f);
        return (b >> 31) ? ~b : (b | 0x80000000u);
    }
    __device__ static float score(K k) { return __uint_as_float((k >> 31) ? (k & 0x7fffffffu) : ~k); }
    __device__ static float add(float a, float b) { return __fadd_rn(a, b); }
    __device__ static float sub(float a, float b) { return __fsub_rn(a, b); }
    __device__ static float mul(float a, float b) { return __fmul_rn(a, b); }
    __device__ static float sigmoid(float x) { return 1.f / (1.f + expf(-x)); }
};
template <> struct PeakNum<double> {
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
    __device__ static double sub(double a, double b) { return __dsub_rn(a, b); }
    __device__ static double mul(double a, double b) { return __dmul_rn(a, b); }
    __device__ static double sigmoid(double x) { return 1.0 / (1.0 + exp(-x)); }
};

template <typename T> constexpr int peak_capacity()
{
    return PK_LIST_BYTES / (int)(sizeof(typename PeakNum<T>::K) + sizeof(int)) / 64 * 64;
}

// one candidate list: key (score) and cell; in LDS or in global memory
template <typename T> struct PeakList {
    typename PeakNum<T>::K *key;
    int *cell;
};

// byte layout of the workspace for `batch` maps of `cells` cells: counts [batch, nblk] int32, then the segment arrays and the
// list arrays (key, cell), every one [batch, nblk * PK_TILE]
struct PeakWorkspace {
    int nblk;
    int64_t stride;          // entries per map = nblk * PK_TILE
    int64_t counts, key[2], cell[2], bytes;
};

static PeakWorkspace peak_workspace_layout(int64_t batch, int64_t cells, int elem)
{
    PeakWorkspace w;
    w.nblk = ceil_div(cells, PK_TILE);
    w.stride = (int64_t)w.nblk * PK_TILE;
    const int64_t per = batch * w.stride;
    int64_t at = (batch * w.nblk * (int64_t)sizeof(int32_t) + 15) / 16 * 16;
    w.counts = 0;
    for (int s = 0; s < 2; ++s) {
        w.key[s] = at;  at += per * elem;
        w.cell[s] = at; at += (per * (int64_t)sizeof(int32_t) + 15) / 16 * 16;
    }
    w.bytes = at;
    return w;
}

template <typename T> static PeakList<T> peak_list_at(void *workspace, const PeakWorkspace &w, int which)
{
    char *p = static_cast<char *>(workspace);
    return PeakList<T>{reinterpret_cast<typename PeakNum<T>::K *>(p + w.key[which]), reinterpret_cast<int *>(p + w.cell[which])};
}

struct PeakStrides {
    int64_t hm[4], off[4], wh[4];
};

template <typename T>
__global__ __launch_bounds__(PK_COMPACT_THREADS) void peak_compact(const T *__restrict__ hm, PeakStrides st, int H, int W, T cls_thres,
                                                                    int use_thres, PeakList<T> seg, int *__restrict__ counts, int nblk,
                                                                    int64_t stride)
{
    using N = PeakNum<T>;
    __shared__ T s_score[3 * PK_HALO];
    __shared__ int s_count;
    const int b = blockIdx.y, k = blockIdx.x, cells = H * W, tid = threadIdx.x;
    const int start = k * PK_TILE;
    if (tid == 0) {
        s_count = 0;
        if (b == 0 && k == 0) g_peak_used_global = 0;
    }
    // entry r * PK_HALO + j + 1 holds the score of cell start + (r - 1) W + j, j = -1 .. PK_TILE
    for (int i = tid; i < 3 * PK_HALO; i += PK_COMPACT_THREADS) {
        const int r = i / PK_HALO, j = i - r * PK_HALO - 1;
        const int64_t cell = (int64_t)start + (int64_t)(r - 1) * W + j;
        T s = T(0);
        if (cell >= 0 && cell < cells) {
            const int row = (int)cell / W, col = (int)cell - row * W;
            s = N::sigmoid(hm[b * st.hm[0] + row * st.hm[2] + col * st.hm[3]]);
        }
        s_score[i] = s;
    }
    __syncthreads();
    const int64_t base = (int64_t)b * stride + start;
    const int lane = tid % MVDETR_WAVE;
    for (int e = 0; e < PK_TILE / PK_COMPACT_THREADS; ++e) {
        const int j = e * PK_COMPACT_THREADS + tid, cell = start + j;
        bool cand = false;
        T s = T(0);
        if (cell < cells) {
            const int row = cell / W, col = cell - row * W;
            s = s_score[PK_HALO + j + 1];
            cand = s == s;                                                 // a NaN never is
            if (use_thres) cand = cand && s > cls_thres;
            for (int dr = -1; dr <= 1; ++dr) {
                if ((unsigned)(row + dr) >= (unsigned)H) continue;
                for (int dc = -1; dc <= 1; ++dc) {
                    if ((unsigned)(col + dc) >= (unsigned)W) continue;
                    cand = cand && !(s_score[(dr + 1) * PK_HALO + j + dc + 1] > s);   // a NaN neighbour is ignored
                }
            }
        }
        // one LDS atomic per wave: the first candidate lane reserves the wave's slots (< PK_TILE in all: one per cell)
        const unsigned long long mask = __ballot(cand);
        if (!mask) continue;                                               // wave-uniform
        const int leader = __ffsll((long long)mask) - 1;
        int first = 0;
        if (lane == leader) first = atomicAdd(&s_count, __popcll(mask));
        first = __shfl(first, leader);
        if (cand) {
            const int slot = first + __popcll(mask & ((1ull << lane) - 1));
            seg.key[base + slot] = N::key(s);
            seg.cell[base + slot] = cell;
        }
    }
    __syncthreads();
    if (tid == 0) counts[b * nblk + k] = s_count;
}

template <typename K> __device__ __forceinline__ bool peak_before(K ka, int ia, K kb, int ib)
{
    return ka > kb || (ka == kb && ia > ib);
}

template <typename T> struct PeakOut {
    T *xy, *wh, *box, *score;
    int32_t *cell, *count;
};

template <typename T>
__global__ __launch_bounds__(PK_SELECT_THREADS) void peak_select(PeakList<T> seg, PeakList<T> glist, const int *__restrict__ counts, int nblk,
                                                                  int64_t stride, const T *__restrict__ off, const T *__restrict__ wh,
                                                                  PeakStrides st, int H, int W, int top_k, T scale, PeakOut<T> out)
{
    using N = PeakNum<T>;
    using K = typename N::K;
    constexpr int KD = (int)sizeof(K);                                     // 8-bit digits of a key
    __shared__ __align__(16) unsigned char lds[PK_LIST_BYTES];
    __shared__ K s_key[PK_MAX_TOP_K];
    __shared__ int s_cell[PK_MAX_TOP_K];
    __shared__ int s_hist[256];
    __shared__ int s_total, s_alloc, s_taken, s_digit, s_rank;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid % MVDETR_WAVE;
    const int *cnt = counts + (int64_t)b * nblk;
    if (tid == 0) s_total = s_alloc = s_taken = 0;
    __syncthreads();
    int part = 0;
    for (int k = tid; k < nblk; k += PK_SELECT_THREADS) part += min(max(cnt[k], 0), PK_TILE);
    if (part) atomicAdd(&s_total, part);
    __syncthreads();
    const int n = s_total;                                                 // <= nblk * PK_TILE = stride
    PeakList<T> list;
    if (n <= peak_capacity<T>()) {
        K *key = reinterpret_cast<K *>(lds);
        list = PeakList<T>{key, reinterpret_cast<int *>(key + peak_capacity<T>())};
    } else {
        const int64_t o = (int64_t)b * stride;
        list = PeakList<T>{glist.key + o, glist.cell + o};
        if (tid == 0) g_peak_used_global = 1;
    }
    // gather: a wave per segment; where a segment lands in the list does not matter
    for (int k = tid / MVDETR_WAVE; k < nblk; k += PK_SELECT_THREADS / MVDETR_WAVE) {
        const int c = min(max(cnt[k], 0), PK_TILE);
        int at = 0;
        if (lane == 0 && c) at = atomicAdd(&s_alloc, c);
        at = __shfl(at, 0);
        const int64_t from = (int64_t)b * stride + (int64_t)k * PK_TILE;
        for (int e = lane; e < c; e += MVDETR_WAVE) {
            list.key[at + e] = seg.key[from + e];
            list.cell[at + e] = seg.cell[from + e];
        }
    }
    __syncthreads();

    const int m = min(n, top_k);
    // 1. the m-th entry by (key, cell) descending, digit by digit; n <= top_k: everything is taken
    K tkey = 0, kmask = 0;
    uint32_t tcell = 0, cmask = 0;
    if (n > top_k) {
        int CD = 1;                                                        // 8-bit digits of a cell index
        while (CD < 4 && ((int64_t)H * W - 1) >> (8 * CD)) ++CD;
        int rank = top_k;                                                  // 1-based, among the entries that match the prefix
        for (int d = 0; d < KD + CD; ++d) {
            const bool in_key = d < KD;
            const int shift = 8 * (in_key ? KD - 1 - d : CD - 1 - (d - KD));
            if (tid < 256) s_hist[tid] = 0;
            __syncthreads();
            // a thread counts runs of one digit privately, and a wave whose lanes all ended on one digit adds once: a plateau
            // (every key equal) would otherwise serialise n atomics on one address
            int dig = -1, cnt = 0;
            for (int j = tid; j < n; j += PK_SELECT_THREADS) {
                const K kj = list.key[j];
                const uint32_t cj = (uint32_t)list.cell[j];
                if ((kj & kmask) != tkey || (cj & cmask) != tcell) continue;
                const int dj = in_key ? (int)((kj >> shift) & 255) : (int)((cj >> shift) & 255);
                if (dj != dig && cnt) {
                    atomicAdd(&s_hist[dig], cnt);
                    cnt = 0;
                }
                dig = dj;
                ++cnt;
            }
            int dmax = cnt ? dig : -1, sum = cnt;
            for (int s = MVDETR_WAVE / 2; s > 0; s >>= 1) {
                dmax = max(dmax, __shfl_xor(dmax, s));
                sum += __shfl_xor(sum, s);
            }
            if (__all(cnt == 0 || dig == dmax)) {
                if (lane == 0 && sum) atomicAdd(&s_hist[dmax], sum);
            } else if (cnt) {
                atomicAdd(&s_hist[dig], cnt);
            }
            __syncthreads();
            if (tid < MVDETR_WAVE) {
                // lane l owns the digits 255 - 4 l .. 252 - 4 l; `above` = the matching entries with a greater digit
                int c[4], sum = 0;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    c[q] = s_hist[255 - 4 * lane - q];
                    sum += c[q];
                }
                int incl = sum;
                for (int s = 1; s < MVDETR_WAVE; s <<= 1) {
                    const int o = __shfl_up(incl, s);
                    if (lane >= s) incl += o;
                }
                int above = incl - sum;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (above < rank && rank <= above + c[q]) {
                        s_digit = 255 - 4 * lane - q;
                        s_rank = rank - above;
                    }
                    above += c[q];
                }
            }
            __syncthreads();
            rank = s_rank;
            if (in_key) {
                tkey |= (K)s_digit << shift;
                kmask |= (K)255 << shift;
            } else {
                tcell |= (uint32_t)s_digit << shift;
                cmask |= 255u << shift;
            }
        }
    }
    // 2. the m entries at or before it, ordered
    int P = 1;
    while (P < m) P <<= 1;
    for (int j = tid; j < n; j += PK_SELECT_THREADS) {
        const K kj = list.key[j];
        const int cj = list.cell[j];
        if (kj > tkey || (kj == tkey && cj >= (int)tcell)) {
            const int slot = atomicAdd(&s_taken, 1);
            if (slot < PK_MAX_TOP_K) {
                s_key[slot] = kj;
                s_cell[slot] = cj;
            }
        }
    }
    for (int i = m + tid; i < P; i += PK_SELECT_THREADS) {                 // padding: after every real entry
        s_key[i] = 0;
        s_cell[i] = -1;
    }
    __syncthreads();
    for (int k2 = 2; k2 <= P; k2 <<= 1)
        for (int j2 = k2 >> 1; j2 > 0; j2 >>= 1) {
            if (tid < P / 2) {
                const int i = ((tid & ~(j2 - 1)) << 1) | (tid & (j2 - 1)), l = i + j2;
                const K ka = s_key[i], kb = s_key[l];
                const int ia = s_cell[i], ib = s_cell[l];
                const bool ordered = (i & k2) ? !peak_before<K>(ka, ia, kb, ib) : !peak_before<K>(kb, ib, ka, ia);
                if (!ordered) {
                    s_key[i] = kb; s_cell[i] = ib;
                    s_key[l] = ka; s_cell[l] = ia;
                }
            }
            __syncthreads();
        }

    if (tid == 0) out.count[b] = n;                                        // the true number, also beyond top_k
    if (tid >= top_k) return;
    const int64_t r = (int64_t)b * top_k + tid;
    T x = T(0), y = T(0), w = T(0), h = T(0), s = T(0), x1 = T(0), y1 = T(0), x2 = T(0), y2 = T(0);
    int cell = 0;
    if (tid < m) {
        cell = s_cell[tid];
        s = N::score(s_key[tid]);
        const int row = cell / W, col = cell - row * W;
        T dx = T(0.5), dy = T(0.5);
        if (off) {
            const T *o = off + b * st.off[0] + row * st.off[2] + col * st.off[3];
            dx = o[0];
            dy = o[st.off[1]];
        }
        x = N::add(T(col), dx);
        y = N::add(T(row), dy);
        if (wh) {
            const T *p = wh + b * st.wh[0] + row * st.wh[2] + col * st.wh[3];
            w = p[0];
            h = p[st.wh[1]];
            const T half = N::mul(T(0.5), w);
            x1 = N::mul(N::sub(x, half), scale);
            y1 = N::mul(N::sub(y, h), scale);
            x2 = N::mul(N::add(x, half), scale);
            y2 = N::mul(y, scale);
        }
    }
    out.xy[2 * r] = x;
    out.xy[2 * r + 1] = y;
    out.score[r] = s;
    out.cell[r] = cell;
    if (wh) {
        out.wh[2 * r] = w;
        out.wh[2 * r + 1] = h;
        out.box[4 * r] = x1;
        out.box[4 * r + 1] = y1;
        out.box[4 * r + 2] = x2;
        out.box[4 * r + 3] = y2;
    }
}

template <typename T>
static int peak_detect_forward(void *stream, const T *hm, const int64_t *hm_stride, const T *off, const int64_t *off_stride, const T *wh,
                               const int64_t *wh_stride, int B, int H, int W, int top_k, double cls_thres, int use_thres, double scale,
                               void *workspace, T *xy, T *wh_out, T *box, T *score, int32_t *cell, int32_t *count)
{
    if (!hm || !hm_stride || (off && !off_stride) || (wh && (!wh_stride || !wh_out || !box)) || !workspace || !xy || !score || !cell ||
        !count || B < 1 || B > 65535 || H < 1 || W < 1 || top_k < 1 || top_k > PK_MAX_TOP_K || (int64_t)H * W > PK_MAX_CELLS ||
        !aligned(workspace, 16))
        return 1;
    const PeakWorkspace w = peak_workspace_layout(B, (int64_t)H * W, sizeof(T));
    PeakStrides st{};
    for (int d = 0; d < 4; ++d) {
        st.hm[d] = hm_stride[d];
        st.off[d] = off ? off_stride[d] : 0;
        st.wh[d] = wh ? wh_stride[d] : 0;
    }
    const PeakList<T> seg = peak_list_at<T>(workspace, w, 0), glist = peak_list_at<T>(workspace, w, 1);
    int *counts = reinterpret_cast<int *>(static_cast<char *>(workspace) + w.counts);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    peak_compact<T><<<dim3(w.nblk, B), PK_COMPACT_THREADS, 0, s>>>(hm, st, H, W, T(cls_thres), use_thres, seg, counts, w.nblk, w.stride);
    peak_select<T><<<B, PK_SELECT_THREADS, 0, s>>>(seg, glist, counts, w.nblk, w.stride, off, wh, st, H, W, top_k, T(scale),
                                                   PeakOut<T>{xy, wh_out, box, score, cell, count});
    g_peak_last_device = dev;
    g_peak_launches.fetch_add(2);
    return (int)hipGetLastError();
}

}  // namespace mvdetr

extern "C" int64_t mvdetr_peak_detect_workspace_bytes(int batch, int height, int width, int elem_size)
{
    if (batch < 1 || height < 1 || width < 1 || (elem_size != 4 && elem_size != 8) || (int64_t)height * width > mvdetr::PK_MAX_CELLS)
        return -1;
    return mvdetr::peak_workspace_layout(batch, (int64_t)height * width, elem_size).bytes;
}

extern "C" int mvdetr_peak_detect_lds_capacity(int elem_size)
{
    return elem_size == 4 ? mvdetr::peak_capacity<float>() : elem_size == 8 ? mvdetr::peak_capacity<double>() : -1;
}

#define MVDETR_PEAK_ENTRY(T, SFX)                                                                                                         \
    extern "C" int mvdetr_peak_detect_forward_##SFX(void *stream, const T *heatmap, const int64_t *heatmap_stride, const T *offset,         \
                                                    const int64_t *offset_stride, const T *wh, const int64_t *wh_stride, int batch,        \
                                                    int height, int width, int top_k, double cls_thres, int use_thres, double scale,       \
                                                    void *workspace, T *xy, T *wh_out, T *box, T *score, int32_t *cell, int32_t *count)    \
    {                                                                                                                                     \
        return mvdetr::peak_detect_forward<T>(stream, heatmap, heatmap_stride, offset, offset_stride, wh, wh_stride, batch, height, width, \
                                              top_k, cls_thres, use_thres, scale, workspace, xy, wh_out, box, score, cell, count);         \
    }
MVDETR_PEAK_ENTRY(float, f32)
MVDETR_PEAK_ENTRY(double, f64)

// The route is decided on the device by the candidate counts, so this waits for the device of the last call and reads one flag
// back: a diagnostic for tests and tools, not for a hot path.
extern "C" const char *mvdetr_peak_detect_last_kernel(void)
{
    const int dev = mvdetr::g_peak_last_device.load();
    if (dev < 0) return "none";
    int cur = 0, used = 0;
    const bool have_cur = hipGetDevice(&cur) == hipSuccess;
    if (have_cur && cur != dev) (void)hipSetDevice(dev);
    const bool ok = hipDeviceSynchronize() == hipSuccess &&
                    hipMemcpyFromSymbol(&used, HIP_SYMBOL(mvdetr::g_peak_used_global), sizeof(int), 0, hipMemcpyDeviceToHost) == hipSuccess;
    if (have_cur && cur != dev) (void)hipSetDevice(cur);
    if (!ok) return "unknown";
    return used ? "peak_compact+peak_select_global" : "peak_compact+peak_select";
}

extern "C" int64_t mvdetr_peak_detect_launch_count(void) { return mvdetr::g_peak_launches.load(); }

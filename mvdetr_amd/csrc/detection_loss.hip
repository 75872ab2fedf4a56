// The detection objective's two losses, forward and backward -- gfx950 (MI355X).
//
//   focal   CornerNet focal loss over a heat map: p = clamp(sigmoid(x), 1e-4, 1 - 1e-4);
//           pos = sum_{t == 1} log(p) (1-p)^2;  neg = sum_{t < 1} log(1-p) p^2 (1-t)^4 [mask];
//           loss = -(pos + neg) / num_pos, or -neg when there is no positive.
//   reg_l1  masked L1 at K gathered positions: pred[b,k,c] = out[b,c,ind[b,k]];
//           loss = sum m |pred - target| / (C sum m + 1e-4).
//
// As torch ops each is ~25 launches forward and as many backward over maps of 43k-100k elements, with a host
// synchronise (`if num_pos == 0`) in the middle.  Here a call is ONE launch that takes up to MVDETR_LOSS_MAX_SEGMENTS
// segments (maps of different shape, target, normaliser and weight: the world and the image heads of one training step),
// described by value in the kernel arguments; every branch of the formula is resolved on the device and the results stay
// there: per-segment losses in out[0 .. nseg-1], their weighted sum in out[nseg].
//
// Layouts: the head outputs (and their gradients) are addressed through their four strides, so NCHW and channel-last
// tensors are read and written in place.  When the strides are those of a dense NCHW tensor (true of every C == 1 map
// in either layout) and the pointers are 16-byte aligned, a lane moves 16 bytes per access.
//
// Determinism: no floating-point atomics anywhere.  Focal forward: a lane adds its elements in index order in fp64, a wave
// reduces by xor-shuffles, the block adds its four waves in order and stores three partial sums; the block of a segment
// that draws the last integer ticket adds that segment's partials in block order (fp64) and finishes the loss.  The block
// partition depends on the segment's shape alone, so a segment gives the same bits alone or beside others.  reg_l1
// forward is one workgroup (a few thousand gathers).  reg_l1 backward: a block owns a tile of one map, zero-fills it, and
// after a barrier the FIRST slot k holding a position adds every later slot with the same position in k order and stores
// the sum once.  The backward passes recompute from the inputs; the forward saves one fp64 scalar per segment.
#include <atomic>
#include <cmath>

#include "common.h"
#include "../../include/mvdetr_ops.h"

namespace mvdetr {

static std::atomic<const char *> g_loss_last_kernel{"none"};
static std::atomic<int64_t> g_loss_launches{0};

constexpr int LOSS_THREADS = 256;
constexpr int LOSS_WAVES = LOSS_THREADS / MVDETR_WAVE;
constexpr int MAX_SEG = MVDETR_LOSS_MAX_SEGMENTS;
constexpr int L1_MAX_K = 1024;                  // slots per map the backward keeps in LDS
constexpr int L1_TILE = 2048;                   // positions of one map a backward block owns

__device__ __forceinline__ float exp_(float x) { return expf(x); }
__device__ __forceinline__ double exp_(double x) { return exp(x); }
__device__ __forceinline__ float log1p_(float x) { return log1pf(x); }
__device__ __forceinline__ double log1p_(double x) { return log1p(x); }

// offset of logical NCHW index i in a tensor with strides s (elements)
__device__ __forceinline__ int64_t strided_offset(int64_t i, int C, int H, int W, const int64_t *s)
{
    const int w = (int)(i % W);
    int64_t r = i / W;
    const int h = (int)(r % H);
    r /= H;
    const int c = (int)(r % C);
    const int64_t b = r / C;
    return b * s[0] + c * s[1] + h * s[2] + w * s[3];
}

// ---- focal ------------------------------------------------------------------------------------------------------------

struct FocalSeg {
    const void *x, *t, *m;      // logits (strided), target and optional mask (dense NCHW)
    void *g;                    // gradient of the logits (strided), backward only; null: this segment gets none
    int64_t sx[4], sg[4];
    int64_t numel;
    int C, H, W;
    int vec;                    // logits (and gradient) dense NCHW, everything 16-byte aligned, numel % lanes-per-16-bytes == 0
    int block0, nblocks;        // this segment's blocks in the grid
    double weight;
};
struct FocalArgs {
    FocalSeg seg[MAX_SEG];
    int nseg;
};

template <typename T> struct FocalConst;
template <> struct FocalConst<float> {
    static constexpr float LO = 1e-4f, HI = 0.9999f, LOG_LO = -9.210340371976182f, LOG_HI = -1.0000500033334732e-4f;
};
template <> struct FocalConst<double> {
    static constexpr double LO = 1e-4, HI = 1.0 - 1e-4, LOG_LO = -9.210340371976182, LOG_HI = -1.0000500033334732e-4;
};

// p = clamp(sigmoid(x)), q = 1 - p, their logarithms, and whether the clamp cut (then the gradient is zero).  q and both
// logarithms are formed from exp(-|x|), not from 1 - p, so fp32 keeps full relative precision at either end.
template <typename T>
__device__ __forceinline__ void focal_point(T x, T &p, T &q, T &lp, T &lq, bool &cut)
{
    using K = FocalConst<T>;
    const T e = exp_(-fabs(x));
    const T inv = T(1) / (T(1) + e);
    const T small = e * inv;
    const T l1p = log1p_(e);
    p = x >= T(0) ? inv : small;
    q = x >= T(0) ? small : inv;
    lp = (x < T(0) ? x : T(0)) - l1p;
    lq = (x > T(0) ? -x : T(0)) - l1p;
    const bool lo = p < K::LO, hi = q < K::LO;
    if (lo) { p = K::LO; q = K::HI; lp = K::LOG_LO; lq = K::LOG_HI; }
    if (hi) { p = K::HI; q = K::LO; lp = K::LOG_HI; lq = K::LOG_LO; }
    cut = lo || hi;
}

template <typename T> __device__ __forceinline__ T pow4(T a) { const T b = a * a; return b * b; }

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = MVDETR_WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, MVDETR_WAVE);
    return v;
}

// sum of three values over the block, in lane 0 of wave 0 (fixed order: xor tree in the wave, waves 0..3)
__device__ __forceinline__ void block_sum3(double &a, double &b, double &c, double (*lds)[3])
{
    a = wave_sum(a);
    b = wave_sum(b);
    c = wave_sum(c);
    const int wave = threadIdx.x / MVDETR_WAVE;
    if (threadIdx.x % MVDETR_WAVE == 0) { lds[wave][0] = a; lds[wave][1] = b; lds[wave][2] = c; }
    __syncthreads();
    if (threadIdx.x == 0) {
        a = lds[0][0]; b = lds[0][1]; c = lds[0][2];
#pragma unroll
        for (int w = 1; w < LOSS_WAVES; ++w) { a += lds[w][0]; b += lds[w][1]; c += lds[w][2]; }
    }
    __syncthreads();
}

__device__ __forceinline__ int segment_of_block(const int *block0, int nseg)
{
    int s = 0;
#pragma unroll
    for (int i = 1; i < MAX_SEG; ++i) s += (i < nseg && (int)blockIdx.x >= block0[i]) ? 1 : 0;
    return s;
}

__device__ __forceinline__ void agent_store(double *p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ double agent_load(const double *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// workspace: [total blocks][3] partial sums, then [MAX_SEG] finished losses (fp64).  counters: [MAX_SEG + 1] tickets, zero on
// entry and zero again on exit (the block that draws the last ticket resets it).
template <typename T>
__global__ __launch_bounds__(LOSS_THREADS) void focal_loss_fwd(FocalArgs a, double *workspace, unsigned *counters, int total_blocks,
                                                               T *out, double *stats)
{
    constexpr int V = 16 / sizeof(T);
    __shared__ double lds[LOSS_WAVES][3];
    __shared__ int s_last;
    int block0[MAX_SEG];
#pragma unroll
    for (int i = 0; i < MAX_SEG; ++i) block0[i] = a.seg[i].block0;
    const int s = segment_of_block(block0, a.nseg);
    const FocalSeg &g = a.seg[s];
    const int blk = (int)blockIdx.x - g.block0;
    const T *x = static_cast<const T *>(g.x), *t = static_cast<const T *>(g.t), *m = static_cast<const T *>(g.m);

    double pos = 0.0, neg = 0.0, npos = 0.0;
    const int64_t i0 = ((int64_t)blk * LOSS_THREADS + threadIdx.x) * V;
    if (i0 < g.numel) {
        T xv[V], tv[V], mv[V];
        if (g.vec) {
            const Pack<T, V> px = Pack<T, V>::load(x + i0), pt = Pack<T, V>::load(t + i0);
#pragma unroll
            for (int j = 0; j < V; ++j) { xv[j] = px.v[j]; tv[j] = pt.v[j]; mv[j] = T(1); }
            if (m) {
                const Pack<T, V> pm = Pack<T, V>::load(m + i0);
#pragma unroll
                for (int j = 0; j < V; ++j) mv[j] = pm.v[j];
            }
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const bool in = i0 + j < g.numel;
                const int64_t i = in ? i0 + j : i0;
                xv[j] = x[strided_offset(i, g.C, g.H, g.W, g.sx)];
                tv[j] = in ? t[i] : T(2);                                  // a target above 1 is in neither sum
                mv[j] = m ? m[i] : T(1);
            }
        }
#pragma unroll
        for (int j = 0; j < V; ++j) {
            T p, q, lp, lq;
            bool cut;
            focal_point(xv[j], p, q, lp, lq, cut);
            if (tv[j] == T(1)) {
                pos += (double)(lp * q * q);
                npos += 1.0;
            } else if (tv[j] < T(1)) {
                neg += (double)(lq * p * p * pow4(T(1) - tv[j]) * mv[j]);
            }
        }
    }
    block_sum3(pos, neg, npos, lds);

    double *partial = workspace + (int64_t)blockIdx.x * 3;
    double *seg_loss = workspace + (int64_t)total_blocks * 3;
    if (threadIdx.x == 0) {
        agent_store(partial + 0, pos);
        agent_store(partial + 1, neg);
        agent_store(partial + 2, npos);
        __threadfence();
        s_last = atomicAdd(counters + s, 1u) == (unsigned)g.nblocks - 1u;
    }
    __syncthreads();
    if (!s_last) return;

    // the last block of this segment: every partial of the segment is visible behind the ticket
    __threadfence();
    pos = neg = npos = 0.0;
    const double *first = workspace + (int64_t)g.block0 * 3;
    for (int b = threadIdx.x; b < g.nblocks; b += LOSS_THREADS) {
        pos += agent_load(first + (int64_t)b * 3 + 0);
        neg += agent_load(first + (int64_t)b * 3 + 1);
        npos += agent_load(first + (int64_t)b * 3 + 2);
    }
    block_sum3(pos, neg, npos, lds);
    if (threadIdx.x != 0) return;
    const double loss = -(pos + neg) / (npos == 0.0 ? 1.0 : npos);
    out[s] = (T)loss;
    stats[s] = npos;
    agent_store(seg_loss + s, loss);
    __hip_atomic_store(counters + s, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __threadfence();
    if (atomicAdd(counters + MAX_SEG, 1u) != (unsigned)a.nseg - 1u) return;
    __threadfence();
    double total = 0.0;
    for (int i = 0; i < a.nseg; ++i) total += a.seg[i].weight * agent_load(seg_loss + i);
    out[a.nseg] = (T)total;
    __hip_atomic_store(counters + MAX_SEG, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// grad_out: [nseg + 1] (the per-segment losses and the weighted sum); stats[s] = num_pos of the forward
template <typename T>
__global__ __launch_bounds__(LOSS_THREADS) void focal_loss_bwd(FocalArgs a, const T *grad_out, const double *stats)
{
    constexpr int V = 16 / sizeof(T);
    int block0[MAX_SEG];
#pragma unroll
    for (int i = 0; i < MAX_SEG; ++i) block0[i] = a.seg[i].block0;
    const int s = segment_of_block(block0, a.nseg);
    const FocalSeg &g = a.seg[s];
    T *gx = static_cast<T *>(g.g);
    if (!gx) return;
    const int blk = (int)blockIdx.x - g.block0;
    const T *x = static_cast<const T *>(g.x), *t = static_cast<const T *>(g.t), *m = static_cast<const T *>(g.m);
    const int64_t i0 = ((int64_t)blk * LOSS_THREADS + threadIdx.x) * V;
    if (i0 >= g.numel) return;
    const double npos = stats[s];
    const T coef = (T)(-((double)grad_out[s] + (double)grad_out[a.nseg] * g.weight) / (npos == 0.0 ? 1.0 : npos));

    T xv[V], tv[V], mv[V], gv[V];
    if (g.vec) {
        const Pack<T, V> px = Pack<T, V>::load(x + i0), pt = Pack<T, V>::load(t + i0);
#pragma unroll
        for (int j = 0; j < V; ++j) { xv[j] = px.v[j]; tv[j] = pt.v[j]; mv[j] = T(1); }
        if (m) {
            const Pack<T, V> pm = Pack<T, V>::load(m + i0);
#pragma unroll
            for (int j = 0; j < V; ++j) mv[j] = pm.v[j];
        }
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const bool in = i0 + j < g.numel;
            const int64_t i = in ? i0 + j : i0;
            xv[j] = x[strided_offset(i, g.C, g.H, g.W, g.sx)];
            tv[j] = t[i];
            mv[j] = m ? m[i] : T(1);
        }
    }
#pragma unroll
    for (int j = 0; j < V; ++j) {
        T p, q, lp, lq;
        bool cut;
        focal_point(xv[j], p, q, lp, lq, cut);
        T d = T(0);
        if (tv[j] == T(1)) d = q * q * (q - T(2) * p * lp);
        else if (tv[j] < T(1)) d = p * p * (T(2) * q * lq - p) * pow4(T(1) - tv[j]) * mv[j];
        gv[j] = cut ? T(0) : d * coef;
    }
    if (g.vec) {
        Pack<T, V> pg;
#pragma unroll
        for (int j = 0; j < V; ++j) pg.v[j] = gv[j];
        pg.store(gx + i0);
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j)
            if (i0 + j < g.numel) gx[strided_offset(i0 + j, g.C, g.H, g.W, g.sg)] = gv[j];
    }
}

// ---- masked L1 at gathered positions ------------------------------------------------------------------------------------

struct L1Seg {
    const void *x;              // [B, C, H, W] through strides
    const uint8_t *mask;        // [B, K]
    const int64_t *ind;         // [B, K]
    const void *t;              // [B, K, C] dense
    void *g;                    // gradient of x (strided), backward only; null: none
    int64_t sx[4], sg[4];
    int B, C, H, W, K;
    int block0, nblocks;        // backward grid
    double weight;
};
struct L1Args {
    L1Seg seg[MAX_SEG];
    int nseg;
};

// one workgroup; stats[s] = the denominator C sum m + 1e-4 (formed in fp32, as the mask sum of the formula is)
template <typename T>
__global__ __launch_bounds__(LOSS_THREADS) void reg_l1_loss_fwd(L1Args a, T *out, double *stats)
{
    __shared__ double lds[LOSS_WAVES][3];
    double total = 0.0;
    for (int s = 0; s < a.nseg; ++s) {
        const L1Seg &g = a.seg[s];
        const T *x = static_cast<const T *>(g.x), *t = static_cast<const T *>(g.t);
        const int HW = g.H * g.W, KC = g.K * g.C;
        const int n = g.B * KC;
        double sum = 0.0, cnt = 0.0, unused = 0.0;
        for (int i = threadIdx.x; i < n; i += LOSS_THREADS) {
            const int b = i / KC, k = (i - b * KC) / g.C, c = i % g.C;
            const int slot = b * g.K + k;
            if (!g.mask[slot]) continue;
            cnt += 1.0;                                                      // over the mask expanded to C channels
            const int64_t pos = g.ind[slot];
            if (pos < 0 || pos >= HW) continue;                              // never dereferenced, contributes nothing
            const int h = (int)pos / g.W, w = (int)pos % g.W;
            const T pred = x[(int64_t)b * g.sx[0] + c * g.sx[1] + h * g.sx[2] + w * g.sx[3]];
            sum += (double)fabs(pred - t[i]);
        }
        block_sum3(sum, cnt, unused, lds);
        if (threadIdx.x == 0) {
            const double den = (double)((float)cnt + 1e-4f);
            const double loss = sum / den;
            out[s] = (T)loss;
            stats[s] = den;
            total += g.weight * loss;
        }
    }
    if (threadIdx.x == 0) out[a.nseg] = (T)total;
}

// zero n elements from p (element-aligned): scalar head up to a 16-byte boundary, 16-byte body, scalar tail
template <typename T> __device__ __forceinline__ void zero_run(T *p, int64_t n)
{
    constexpr int V = 16 / sizeof(T);
    int64_t head = (int64_t)(((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15) / sizeof(T));
    if (head > n) head = n;
    if ((int64_t)threadIdx.x < head) p[threadIdx.x] = T(0);
    T *body = p + head;
    const int64_t nv = (n - head) / V;
    for (int64_t i = threadIdx.x; i < nv; i += LOSS_THREADS) Pack<T, V>::zero().store(body + i * V);
    const int64_t done = head + nv * V;
    if ((int64_t)threadIdx.x < n - done) p[done + threadIdx.x] = T(0);
}

// a block owns positions [lo, hi) of map b of one segment, all channels: zero fill, barrier, then the owners' entries
template <typename T>
__global__ __launch_bounds__(LOSS_THREADS) void reg_l1_loss_bwd(L1Args a, const T *grad_out, const double *stats)
{
    __shared__ int s_pos[L1_MAX_K];
    int block0[MAX_SEG];
#pragma unroll
    for (int i = 0; i < MAX_SEG; ++i) block0[i] = a.seg[i].block0;
    const int s = segment_of_block(block0, a.nseg);
    const L1Seg &g = a.seg[s];
    T *gx = static_cast<T *>(g.g);
    if (!gx) return;
    const int HW = g.H * g.W;
    const int tiles = (HW + L1_TILE - 1) / L1_TILE;
    const int local = (int)blockIdx.x - g.block0;
    const int b = local / tiles, tile = local - b * tiles;
    const int lo = tile * L1_TILE, hi = min(lo + L1_TILE, HW);

    for (int k = threadIdx.x; k < g.K; k += LOSS_THREADS) {
        const int64_t pos = g.ind[b * g.K + k];
        s_pos[k] = (g.mask[b * g.K + k] && pos >= lo && pos < hi) ? (int)pos : -1;
    }

    T *gb = gx + (int64_t)b * g.sg[0];
    const bool rows = g.sg[3] == 1 && g.sg[2] == g.W;                                        // a channel's positions are contiguous
    const bool pixels = g.sg[1] == 1 && g.sg[3] == g.C && g.sg[2] == (int64_t)g.W * g.C;     // channel-last, dense
    if (rows) {
        for (int c = 0; c < g.C; ++c) zero_run(gb + c * g.sg[1] + lo, hi - lo);
    } else if (pixels) {
        zero_run(gb + (int64_t)lo * g.C, (int64_t)(hi - lo) * g.C);
    } else {
        for (int i = threadIdx.x; i < (hi - lo) * g.C; i += LOSS_THREADS) {
            const int pos = lo + i / g.C, c = i % g.C;
            gb[c * g.sg[1] + (pos / g.W) * g.sg[2] + (pos % g.W) * g.sg[3]] = T(0);
        }
    }
    __syncthreads();                                                                         // the fill has landed (vmcnt(0)), s_pos is complete

    const double coef = ((double)grad_out[s] + (double)grad_out[a.nseg] * g.weight) / stats[s];
    const T *x = static_cast<const T *>(g.x), *t = static_cast<const T *>(g.t);
    for (int k = threadIdx.x; k < g.K; k += LOSS_THREADS) {
        const int pos = s_pos[k];
        if (pos < 0) continue;
        bool owner = true;
        for (int j = 0; j < k; ++j) owner = owner && s_pos[j] != pos;
        if (!owner) continue;
        const int h = pos / g.W, w = pos % g.W;
        for (int c = 0; c < g.C; ++c) {
            const T pred = x[(int64_t)b * g.sx[0] + c * g.sx[1] + h * g.sx[2] + w * g.sx[3]];
            double acc = 0.0;
            for (int j = k; j < g.K; ++j) {
                if (s_pos[j] != pos) continue;
                const T d = pred - t[((int64_t)b * g.K + j) * g.C + c];
                acc += d > T(0) ? coef : d < T(0) ? -coef : 0.0;
            }
            gb[c * g.sg[1] + h * g.sg[2] + w * g.sg[3]] = (T)acc;
        }
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------

static bool dense_nchw(const int64_t *s, int B, int C, int H, int W)
{
    // strides of size-1 dimensions are never used
    int64_t want = 1;
    const int size[4] = {B, C, H, W};
    for (int d = 3; d >= 0; --d) {
        if (size[d] != 1 && s[d] != want) return false;
        want *= size[d];
    }
    return true;
}

template <typename T> static int focal_pack(const mvdetr_focal_segment *segs, int nseg, bool backward, FocalArgs &a, int &total_blocks)
{
    constexpr int V = 16 / sizeof(T);
    if (!segs || nseg < 1 || nseg > MAX_SEG) return 1;
    int64_t blocks = 0;
    a.nseg = nseg;
    for (int s = 0; s < MAX_SEG; ++s) {
        FocalSeg &g = a.seg[s];
        g = FocalSeg{};
        g.block0 = INT32_MAX;
        if (s >= nseg) continue;
        const mvdetr_focal_segment &in = segs[s];
        if (!in.logits || !in.target || in.batch < 1 || in.channels < 1 || in.height < 1 || in.width < 1) return 1;
        g.x = in.logits; g.t = in.target; g.m = in.mask; g.g = backward ? in.grad : nullptr;
        g.C = in.channels; g.H = in.height; g.W = in.width;
        g.numel = (int64_t)in.batch * in.channels * in.height * in.width;
        g.weight = in.weight;
        bool vec = g.numel % V == 0 && dense_nchw(in.stride, in.batch, g.C, g.H, g.W) && aligned(g.x, 16) && aligned(g.t, 16) &&
                   (!g.m || aligned(g.m, 16));
        for (int d = 0; d < 4; ++d) { g.sx[d] = in.stride[d]; g.sg[d] = in.grad_stride[d]; }
        if (g.g) vec = vec && dense_nchw(in.grad_stride, in.batch, g.C, g.H, g.W) && aligned(g.g, 16);
        g.vec = vec ? 1 : 0;
        g.block0 = (int)blocks;
        g.nblocks = ceil_div(g.numel, (int64_t)LOSS_THREADS * V);
        blocks += g.nblocks;
        if (blocks > (1 << 24)) return 1;
    }
    total_blocks = (int)blocks;
    return 0;
}

template <typename T>
static int focal_forward(void *stream, const mvdetr_focal_segment *segs, int nseg, void *workspace, int32_t *counters, T *out, double *stats)
{
    FocalArgs a;
    int total = 0;
    if (focal_pack<T>(segs, nseg, false, a, total) || !workspace || !counters || !out || !stats || !aligned(workspace, 8)) return 1;
    focal_loss_fwd<T><<<total, LOSS_THREADS, 0, reinterpret_cast<hipStream_t>(stream)>>>(
        a, static_cast<double *>(workspace), reinterpret_cast<unsigned *>(counters), total, out, stats);
    g_loss_last_kernel = "focal_loss_fwd";
    g_loss_launches.fetch_add(1);
    return (int)hipGetLastError();
}

template <typename T>
static int focal_backward(void *stream, const mvdetr_focal_segment *segs, int nseg, const T *grad_out, const double *stats)
{
    FocalArgs a;
    int total = 0;
    if (focal_pack<T>(segs, nseg, true, a, total) || !grad_out || !stats) return 1;
    focal_loss_bwd<T><<<total, LOSS_THREADS, 0, reinterpret_cast<hipStream_t>(stream)>>>(a, grad_out, stats);
    g_loss_last_kernel = "focal_loss_bwd";
    g_loss_launches.fetch_add(1);
    return (int)hipGetLastError();
}

static int l1_pack(const mvdetr_l1_segment *segs, int nseg, bool backward, L1Args &a, int &total_blocks)
{
    if (!segs || nseg < 1 || nseg > MAX_SEG) return 1;
    int64_t blocks = 0;
    a.nseg = nseg;
    for (int s = 0; s < MAX_SEG; ++s) {
        L1Seg &g = a.seg[s];
        g = L1Seg{};
        g.block0 = INT32_MAX;
        if (s >= nseg) continue;
        const mvdetr_l1_segment &in = segs[s];
        if (!in.output || !in.mask || !in.ind || !in.target || in.batch < 1 || in.channels < 1 || in.height < 1 || in.width < 1 ||
            in.k < 1 || in.k > L1_MAX_K)
            return 1;
        if ((int64_t)in.height * in.width > INT32_MAX || (int64_t)in.batch * in.k * in.channels > INT32_MAX) return 1;
        g.x = in.output; g.mask = in.mask; g.ind = in.ind; g.t = in.target; g.g = backward ? in.grad : nullptr;
        for (int d = 0; d < 4; ++d) { g.sx[d] = in.stride[d]; g.sg[d] = in.grad_stride[d]; }
        g.B = in.batch; g.C = in.channels; g.H = in.height; g.W = in.width; g.K = in.k;
        g.weight = in.weight;
        g.block0 = (int)blocks;
        g.nblocks = in.batch * ceil_div((int64_t)in.height * in.width, L1_TILE);
        blocks += g.nblocks;
        if (blocks > (1 << 24)) return 1;
    }
    total_blocks = (int)blocks;
    return 0;
}

template <typename T> static int l1_forward(void *stream, const mvdetr_l1_segment *segs, int nseg, T *out, double *stats)
{
    L1Args a;
    int total = 0;
    if (l1_pack(segs, nseg, false, a, total) || !out || !stats) return 1;
    reg_l1_loss_fwd<T><<<1, LOSS_THREADS, 0, reinterpret_cast<hipStream_t>(stream)>>>(a, out, stats);
    g_loss_last_kernel = "reg_l1_loss_fwd";
    g_loss_launches.fetch_add(1);
    return (int)hipGetLastError();
}

template <typename T> static int l1_backward(void *stream, const mvdetr_l1_segment *segs, int nseg, const T *grad_out, const double *stats)
{
    L1Args a;
    int total = 0;
    if (l1_pack(segs, nseg, true, a, total) || !grad_out || !stats) return 1;
    reg_l1_loss_bwd<T><<<total, LOSS_THREADS, 0, reinterpret_cast<hipStream_t>(stream)>>>(a, grad_out, stats);
    g_loss_last_kernel = "reg_l1_loss_bwd";
    g_loss_launches.fetch_add(1);
    return (int)hipGetLastError();
}

}  // namespace mvdetr

extern "C" int64_t mvdetr_focal_loss_workspace_bytes(const mvdetr_focal_segment *segs, int nseg, int elem_size)
{
    mvdetr::FocalArgs a;
    int total = 0;
    const int rc = elem_size == 8 ? mvdetr::focal_pack<double>(segs, nseg, false, a, total)
                                  : mvdetr::focal_pack<float>(segs, nseg, false, a, total);
    if (rc || (elem_size != 4 && elem_size != 8)) return -1;
    return ((int64_t)total * 3 + mvdetr::MAX_SEG) * (int64_t)sizeof(double);
}

extern "C" int mvdetr_focal_loss_forward_f32(void *stream, const mvdetr_focal_segment *segs, int nseg, void *workspace, int32_t *counters,
                                             float *out, double *stats)
{
    return mvdetr::focal_forward<float>(stream, segs, nseg, workspace, counters, out, stats);
}

extern "C" int mvdetr_focal_loss_forward_f64(void *stream, const mvdetr_focal_segment *segs, int nseg, void *workspace, int32_t *counters,
                                             double *out, double *stats)
{
    return mvdetr::focal_forward<double>(stream, segs, nseg, workspace, counters, out, stats);
}

extern "C" int mvdetr_focal_loss_backward_f32(void *stream, const mvdetr_focal_segment *segs, int nseg, const float *grad_out,
                                              const double *stats)
{
    return mvdetr::focal_backward<float>(stream, segs, nseg, grad_out, stats);
}

extern "C" int mvdetr_focal_loss_backward_f64(void *stream, const mvdetr_focal_segment *segs, int nseg, const double *grad_out,
                                              const double *stats)
{
    return mvdetr::focal_backward<double>(stream, segs, nseg, grad_out, stats);
}

extern "C" int mvdetr_reg_l1_loss_forward_f32(void *stream, const mvdetr_l1_segment *segs, int nseg, float *out, double *stats)
{
    return mvdetr::l1_forward<float>(stream, segs, nseg, out, stats);
}

extern "C" int mvdetr_reg_l1_loss_forward_f64(void *stream, const mvdetr_l1_segment *segs, int nseg, double *out, double *stats)
{
    return mvdetr::l1_forward<double>(stream, segs, nseg, out, stats);
}

extern "C" int mvdetr_reg_l1_loss_backward_f32(void *stream, const mvdetr_l1_segment *segs, int nseg, const float *grad_out,
                                               const double *stats)
{
    return mvdetr::l1_backward<float>(stream, segs, nseg, grad_out, stats);
}

extern "C" int mvdetr_reg_l1_loss_backward_f64(void *stream, const mvdetr_l1_segment *segs, int nseg, const double *grad_out,
                                               const double *stats)
{
    return mvdetr::l1_backward<double>(stream, segs, nseg, grad_out, stats);
}

extern "C" const char *mvdetr_loss_last_kernel(void) { return mvdetr::g_loss_last_kernel.load(); }

extern "C" int64_t mvdetr_loss_launch_count(void) { return mvdetr::g_loss_launches.load(); }

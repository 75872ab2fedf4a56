// Fused multi-head attention for gfx950: out[b,h,i,:] = sum_j softmax_j(scale * q[b,h,i,:] . k[b,h,j,:]) * v[b,h,j,:],
// scale = 1 / sqrt(D), Sq queries and Sk keys, no masks; forward and backward; no score or probability ever reaches HBM.
// q, k, v, out and the gradients are addressed by element strides (batch, head, token) with the channel contiguous, so the
// seq-first [S, B, 3E] result of an in-projection GEMM and batch-first layouts are read in place.
//
// Routes (mvdetr_attention_last_kernel names them):
//   attn_fwd_mfma   fp32, D = 16 or 32, 16-byte aligned rows.  A workgroup = 8 waves = 128 queries of one (batch, head); wave
//                   w owns 32 queries (w & 3) and one 32-key half (w >> 2) of every 64-key tile pair (K row-major and V
//                   transposed in LDS, double-buffered, the next pair's global loads in flight during the MFMAs):
//                   S^T = K Q^T on v_mfma_f32_32x32x2_f32 -- the swapped product, so lane (query = lane & 31, half = lane >> 5)
//                   holds 16 of its query's 32 scores and the row maximum / sum are 15 register ops + one cross-half shuffle;
//                   online softmax in registers (exp2 of scores already reduced by the running maximum); O^T += V^T P^T with
//                   the probabilities as the B operand straight from the registers they were computed in (the key order of
//                   the contraction is the accumulator layout's, and V^T is stored in LDS in that order), so O's column is the
//                   lane's own query and the rescale needs no cross-lane traffic either.  The two key halves' (max, sum, O)
//                   are merged through LDS.  Writes out and lse = ln sum_j exp(scale * s_ij).
//   attn_bwd_mfma   (same conditions) attn_delta (delta_i = grad_out_i . out_i), then two kernels that recompute P from lse:
//                   attn_bwd_dq_mfma    a wave owns 32 queries (lane = query) and loops over key tiles:  S^T, dP^T = V dO^T,
//                                       dS = P (dP - delta), dQ^T += K^T dS^T;
//                   attn_bwd_dkv_mfma   a wave owns 32 keys (lane = key) and loops over query tiles:  S = Q K^T, dP = dO V^T,
//                                       dV^T += dO^T P, dK^T += Q^T dS.
//                   Every output element is owned by one lane: NO atomics, bit-reproducible run to run.
//   attn_fwd_mfma_half   fp16 / bf16 storage, forward only: attention_half.hip.
//   attn_fwd_generic / attn_bwd_generic   any D <= 256, fp32 and fp64, any alignment: one wave per query row (forward, dQ) or
//                   per key row (dK, dV), 64 scores at a time through LDS; same determinism.
// Dropout (template parameter, absent from the p = 0 instantiations): element (b, h, i, j) is kept iff
// mvdetr_attn_hash(seed, ((b H + h) Sq + i) Sk + j) >= p 2^32 (attention_hash.h); kept probabilities are scaled by
// 1 / (1 - p) in the P V product only, lse uses the undropped probabilities, the backward applies the same mask to dO V^T.
#include "../../include/mvdetr_ops.h"
#include "attention.h"
#include "half_mfma.h"

#include <cmath>
#include <type_traits>

namespace mvdetr {

template <typename T> __device__ __forceinline__ T attn_exp(T x);
template <> __device__ __forceinline__ float attn_exp<float>(float x) { return expf(x); }
template <> __device__ __forceinline__ double attn_exp<double>(double x) { return exp(x); }
template <typename T> __device__ __forceinline__ T attn_log(T x);
template <> __device__ __forceinline__ float attn_log<float>(float x) { return logf(x); }
template <> __device__ __forceinline__ double attn_log<double>(double x) { return log(x); }

__device__ __forceinline__ bool attn_keep(const AttnP &p, int b, int hd, int i, int j)
{
    const uint64_t idx = (((uint64_t)b * p.H + hd) * p.Sq + i) * (uint64_t)p.Sk + j;
    return mvdetr_attn_hash(p.seed, idx) >= p.thresh;
}

// ---- delta[b, h, i] = grad_out[b, h, i, :] . out[b, h, i, :] --------------------------------------------------------------

template <typename T>
__global__ __launch_bounds__(256) void attn_delta(const T *__restrict__ go, const T *__restrict__ out, T *__restrict__ delta,
                                                  AttnP p)
{
    const int64_t rows = (int64_t)p.B * p.H * p.Sq;
    for (int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x; row < rows; row += (int64_t)gridDim.x * 256) {
        const int i = (int)(row % p.Sq), hd = (int)((row / p.Sq) % p.H), b = (int)(row / ((int64_t)p.Sq * p.H));
        const T *g = go + b * p.go[0] + hd * p.go[1] + i * p.go[2];
        const T *o = out + b * p.o[0] + hd * p.o[1] + i * p.o[2];
        T acc = T(0);
        for (int d = 0; d < p.D; ++d) acc += g[d] * o[d];
        delta[row] = acc;
    }
}

// ---- generic kernels ------------------------------------------------------------------------------------------------------

template <typename T> __device__ __forceinline__ T attn_dot(const T *__restrict__ a, const T *__restrict__ b, int D)
{
    T s = T(0);
    for (int d = 0; d < D; ++d) s += a[d] * b[d];
    return s;
}

// one wave per query row; pass 1: lse over the keys (each lane an online (max, sum) of its keys, merged by a fixed
// butterfly); pass 2: 64 probabilities at a time through LDS, lanes own channels d = lane + 64 c.  A probability is
// exp(s - max) / sum, NOT exp(s - lse): lse is a rounded number of the logits' magnitude, and probabilities off by
// eps |lse| each no longer sum to 1 -- at logits ~ 80 a saturated row's out, and through delta = grad_out . out the
// backward's dS (a small difference there), would carry 1e-5 of their operands' size
template <typename T, bool DROP>
__global__ __launch_bounds__(256) void attn_fwd_generic(const T *__restrict__ q, const T *__restrict__ k,
                                                        const T *__restrict__ v, T *__restrict__ out, T *__restrict__ lse,
                                                        AttnP p)
{
    __shared__ T sq[4][ATTN_GD];
    __shared__ T sp[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t rows = (int64_t)p.B * p.H * p.Sq;
    const T scale = T(1) / sqrt(T(p.D));
    for (int64_t r0 = (int64_t)blockIdx.x * 4; r0 < rows; r0 += (int64_t)gridDim.x * 4) {
        const bool rv = r0 + wave < rows;
        const int64_t row = rv ? r0 + wave : rows - 1;
        const int i = (int)(row % p.Sq), hd = (int)((row / p.Sq) % p.H), b = (int)(row / ((int64_t)p.Sq * p.H));
        const T *qp = q + b * p.q[0] + hd * p.q[1] + i * p.q[2];
        const T *kb = k + b * p.k[0] + hd * p.k[1];
        const T *vb = v + b * p.v[0] + hd * p.v[1];
        __syncthreads();
        for (int d = lane; d < p.D; d += 64) sq[wave][d] = qp[d];
        __syncthreads();
        T m = -INFINITY, l = T(0);
        for (int j = lane; j < p.Sk; j += 64) {
            const T s = scale * attn_dot(sq[wave], kb + j * p.k[2], p.D);
            if (s > m) {
                l = l * attn_exp(m - s) + T(1);
                m = s;
            } else {
                l += attn_exp(s - m);
            }
        }
#pragma unroll
        for (int w = 32; w >= 1; w >>= 1) {
            const T m2 = __shfl_xor(m, w), l2 = __shfl_xor(l, w);
            const T mm = m > m2 ? m : m2;
            l = (m == -INFINITY ? T(0) : l * attn_exp(m - mm)) + (m2 == -INFINITY ? T(0) : l2 * attn_exp(m2 - mm));
            m = mm;
        }
        const T L = m + attn_log(l), inv_l = T(1) / l;
        T acc[ATTN_GD / 64];
#pragma unroll
        for (int c = 0; c < ATTN_GD / 64; ++c) acc[c] = T(0);
        for (int j0 = 0; j0 < p.Sk; j0 += 64) {
            const int j = j0 + lane;
            T pv = T(0);
            if (j < p.Sk) {
                pv = attn_exp(scale * attn_dot(sq[wave], kb + j * p.k[2], p.D) - m) * inv_l;
                if (DROP) pv = attn_keep(p, b, hd, i, j) ? pv * T(p.inv_keep) : T(0);
            }
            __syncthreads();
            sp[wave][lane] = pv;
            __syncthreads();
            const int n = p.Sk - j0 < 64 ? p.Sk - j0 : 64;
#pragma unroll
            for (int c = 0; c < ATTN_GD / 64; ++c) {
                const int d = lane + 64 * c;
                if (d < p.D)
                    for (int kk = 0; kk < n; ++kk) acc[c] += sp[wave][kk] * vb[(j0 + kk) * p.v[2] + d];
            }
        }
        if (rv) {
            T *op = out + b * p.o[0] + hd * p.o[1] + i * p.o[2];
#pragma unroll
            for (int c = 0; c < ATTN_GD / 64; ++c)
                if (lane + 64 * c < p.D) op[lane + 64 * c] = acc[c];
            if (lane == 0) lse[row] = L;
        }
    }
}

// dQ: one wave per query row, 64 dS at a time through LDS
template <typename T, bool DROP>
__global__ __launch_bounds__(256) void attn_bwd_dq_generic(const T *__restrict__ go, const T *__restrict__ q,
                                                           const T *__restrict__ k, const T *__restrict__ v,
                                                           const T *__restrict__ lse, const T *__restrict__ delta,
                                                           T *__restrict__ gq, AttnP p)
{
    __shared__ T sq[4][ATTN_GD];
    __shared__ T sg[4][ATTN_GD];
    __shared__ T sds[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t rows = (int64_t)p.B * p.H * p.Sq;
    const T scale = T(1) / sqrt(T(p.D));
    for (int64_t r0 = (int64_t)blockIdx.x * 4; r0 < rows; r0 += (int64_t)gridDim.x * 4) {
        const bool rv = r0 + wave < rows;
        const int64_t row = rv ? r0 + wave : rows - 1;
        const int i = (int)(row % p.Sq), hd = (int)((row / p.Sq) % p.H), b = (int)(row / ((int64_t)p.Sq * p.H));
        const T *qp = q + b * p.q[0] + hd * p.q[1] + i * p.q[2];
        const T *gp = go + b * p.go[0] + hd * p.go[1] + i * p.go[2];
        const T *kb = k + b * p.k[0] + hd * p.k[1];
        const T *vb = v + b * p.v[0] + hd * p.v[1];
        const T L = lse[row], dl = delta[row];
        __syncthreads();
        for (int d = lane; d < p.D; d += 64) {
            sq[wave][d] = qp[d];
            sg[wave][d] = gp[d];
        }
        __syncthreads();
        T acc[ATTN_GD / 64];
#pragma unroll
        for (int c = 0; c < ATTN_GD / 64; ++c) acc[c] = T(0);
        for (int j0 = 0; j0 < p.Sk; j0 += 64) {
            const int j = j0 + lane;
            T ds = T(0);
            if (j < p.Sk) {
                const T pv = attn_exp(scale * attn_dot(sq[wave], kb + j * p.k[2], p.D) - L);
                T dp = attn_dot(sg[wave], vb + j * p.v[2], p.D);
                if (DROP) dp = attn_keep(p, b, hd, i, j) ? dp * T(p.inv_keep) : T(0);
                ds = pv * (dp - dl);
            }
            __syncthreads();
            sds[wave][lane] = ds;
            __syncthreads();
            const int n = p.Sk - j0 < 64 ? p.Sk - j0 : 64;
#pragma unroll
            for (int c = 0; c < ATTN_GD / 64; ++c) {
                const int d = lane + 64 * c;
                if (d < p.D)
                    for (int kk = 0; kk < n; ++kk) acc[c] += sds[wave][kk] * kb[(j0 + kk) * p.k[2] + d];
            }
        }
        if (rv) {
            T *op = gq + b * p.dq[0] + hd * p.dq[1] + i * p.dq[2];
#pragma unroll
            for (int c = 0; c < ATTN_GD / 64; ++c)
                if (lane + 64 * c < p.D) op[lane + 64 * c] = scale * acc[c];
        }
    }
}

// dK and dV: one wave per key row, 64 queries at a time
template <typename T, bool DROP>
__global__ __launch_bounds__(256) void attn_bwd_dkv_generic(const T *__restrict__ go, const T *__restrict__ q,
                                                            const T *__restrict__ k, const T *__restrict__ v,
                                                            const T *__restrict__ lse, const T *__restrict__ delta,
                                                            T *__restrict__ gk, T *__restrict__ gv, AttnP p)
{
    __shared__ T sk[4][ATTN_GD];
    __shared__ T sv[4][ATTN_GD];
    __shared__ T sp[4][64];
    __shared__ T sds[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t rows = (int64_t)p.B * p.H * p.Sk;
    const T scale = T(1) / sqrt(T(p.D));
    for (int64_t r0 = (int64_t)blockIdx.x * 4; r0 < rows; r0 += (int64_t)gridDim.x * 4) {
        const bool rv = r0 + wave < rows;
        const int64_t row = rv ? r0 + wave : rows - 1;
        const int j = (int)(row % p.Sk), hd = (int)((row / p.Sk) % p.H), b = (int)(row / ((int64_t)p.Sk * p.H));
        const T *kp = k + b * p.k[0] + hd * p.k[1] + j * p.k[2];
        const T *vp = v + b * p.v[0] + hd * p.v[1] + j * p.v[2];
        const T *qb = q + b * p.q[0] + hd * p.q[1];
        const T *gb = go + b * p.go[0] + hd * p.go[1];
        const T *lb = lse + ((int64_t)b * p.H + hd) * p.Sq, *db = delta + ((int64_t)b * p.H + hd) * p.Sq;
        __syncthreads();
        for (int d = lane; d < p.D; d += 64) {
            sk[wave][d] = kp[d];
            sv[wave][d] = vp[d];
        }
        __syncthreads();
        T ak[ATTN_GD / 64], av[ATTN_GD / 64];
#pragma unroll
        for (int c = 0; c < ATTN_GD / 64; ++c) ak[c] = av[c] = T(0);
        for (int i0 = 0; i0 < p.Sq; i0 += 64) {
            const int i = i0 + lane;
            T pd = T(0), ds = T(0);
            if (i < p.Sq) {
                const T pv = attn_exp(scale * attn_dot(sk[wave], qb + i * p.q[2], p.D) - lb[i]);
                T dp = attn_dot(sv[wave], gb + i * p.go[2], p.D);
                pd = pv;
                if (DROP) {
                    const bool keep = attn_keep(p, b, hd, i, j);
                    dp = keep ? dp * T(p.inv_keep) : T(0);
                    pd = keep ? pv * T(p.inv_keep) : T(0);
                }
                ds = pv * (dp - db[i]);
            }
            __syncthreads();
            sp[wave][lane] = pd;
            sds[wave][lane] = ds;
            __syncthreads();
            const int n = p.Sq - i0 < 64 ? p.Sq - i0 : 64;
#pragma unroll
            for (int c = 0; c < ATTN_GD / 64; ++c) {
                const int d = lane + 64 * c;
                if (d < p.D)
                    for (int kk = 0; kk < n; ++kk) {
                        av[c] += sp[wave][kk] * gb[(i0 + kk) * p.go[2] + d];
                        ak[c] += sds[wave][kk] * qb[(i0 + kk) * p.q[2] + d];
                    }
            }
        }
        if (rv) {
            T *okp = gk + b * p.dk[0] + hd * p.dk[1] + j * p.dk[2];
            T *ovp = gv + b * p.dv[0] + hd * p.dv[1] + j * p.dv[2];
#pragma unroll
            for (int c = 0; c < ATTN_GD / 64; ++c)
                if (lane + 64 * c < p.D) {
                    okp[lane + 64 * c] = scale * ak[c];
                    ovp[lane + 64 * c] = av[c];
                }
        }
    }
}

// ---- MFMA kernels (fp32, D = 16 or 32) ------------------------------------------------------------------------------------
//
// v_mfma_f32_32x32x2_f32: D[i][j] += A[i][k] B[k][j], k = 0, 1.  Lane (r = lane & 31, h = lane >> 5) supplies A[r][h] and
// B[h][r] and holds D[crow(e, h)][r] in accumulator register e, crow = mfma_crow (half_mfma.h).  The contraction
// index of a step is free as long as A and B agree on it:
//   "row" products (contraction over the channel):   half h takes channels h D/2 + step (D/2 contiguous floats of its row);
//   "col" products (contraction over the 32 rows of a tile):  step s of half h takes row crow(s, h) -- the row whose value the
//   lane holds in register s of a previous product -- and the transposed LDS image stores row x at column tpos(x) = 16 h + s.

__device__ __forceinline__ int attn_tpos(int x) { return 16 * ((x >> 2) & 1) + (x & 3) + 4 * (x >> 3); }

// acc += rows_lds (this lane's row: D/2 contiguous floats) x breg
template <int KS> __device__ __forceinline__ void attn_mfma_row(const float *a_row, const float (&b)[KS], floatx16 &acc)
{
#pragma unroll
    for (int s = 0; s < KS; s += 4) {
        const float4 a = *reinterpret_cast<const float4 *>(a_row + s);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b[s], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b[s + 1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b[s + 2], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b[s + 3], acc, 0, 0, 0);
    }
}

// acc += transposed image row (16 contiguous floats: this half's 16 tile rows) x the 16 values of b
__device__ __forceinline__ void attn_mfma_col(const float *a_row, const floatx16 &b, floatx16 &acc)
{
#pragma unroll
    for (int s = 0; s < 16; s += 4) {
        const float4 a = *reinterpret_cast<const float4 *>(a_row + s);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b[s], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b[s + 1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b[s + 2], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b[s + 3], acc, 0, 0, 0);
    }
}

// this lane's D/2 channels of row `row` (clamped to a valid row by the caller) into registers
template <int KS> __device__ __forceinline__ void attn_load_row(const float *base, int64_t stride, int row, int h, float (&r)[KS])
{
    const float *src = base + row * stride + h * KS;
#pragma unroll
    for (int s = 0; s < KS; s += 4) {
        const float4 a = *reinterpret_cast<const float4 *>(src + s);
        r[s] = a.x; r[s + 1] = a.y; r[s + 2] = a.z; r[s + 3] = a.w;
    }
}

// a 32-row tile of a [rows, D] tensor -> registers (one float4 per thread and 32 x D / 4 / 256 rounds; rows >= n read 0)
template <int D> struct AttnTile {
    static constexpr int C4 = D / 4, N = (32 * C4 + 255) / 256, LD = D + 4;
    float4 v[N];
    __device__ __forceinline__ void fetch(const float *base, int64_t stride, int row0, int n, int t)
    {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const int f = t + 256 * i, row = f / C4, c4 = f - row * C4;
            const bool ok = row < 32 && row0 + row < n;
            v[i] = load4_or_zero(base + (int64_t)(row0 + row) * stride + 4 * c4, ok, base);
        }
    }
    // row-major image [32][D + 4]
    __device__ __forceinline__ void put_rows(float (*dst)[LD], int t) const
    {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const int f = t + 256 * i, row = f / C4, c4 = f - row * C4;
            if (row < 32) *reinterpret_cast<float4 *>(&dst[row][4 * c4]) = v[i];
        }
    }
    // transposed image [D][36], tile row x at column tpos(x)
    __device__ __forceinline__ void put_cols(float (*dst)[36], int t) const
    {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const int f = t + 256 * i, row = f / C4, c4 = f - row * C4;
            if (row < 32) {
                const int pos = attn_tpos(row);
                dst[4 * c4][pos] = v[i].x;
                dst[4 * c4 + 1][pos] = v[i].y;
                dst[4 * c4 + 2][pos] = v[i].z;
                dst[4 * c4 + 3][pos] = v[i].w;
            }
        }
    }
};

// the lane's 16 accumulator values are rows crow(e, h) = 4 consecutive channels per group of 4 registers: float4 stores
template <int D> __device__ __forceinline__ void attn_store_acc(float *row_ptr, const floatx16 &acc, int h, float mul)
{
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int d0 = 8 * g + 4 * h;
        if (d0 < D)
            *reinterpret_cast<float4 *>(row_ptr + d0) =
                make_float4(acc[4 * g] * mul, acc[4 * g + 1] * mul, acc[4 * g + 2] * mul, acc[4 * g + 3] * mul);
    }
}

constexpr float ATTN_LOG2E = 1.4426950408889634f;

// 8 waves: wave w owns queries 32 (w & 3) .. + 31 of the workgroup's 128 and the keys of sub-tile w >> 2 of every 64-key
// tile pair, so a SIMD holds two waves (one's softmax VALU work overlaps the other's MFMAs) and a wave walks half the keys;
// the two partial (max, sum, O) of a query are merged through LDS at the end.
template <int D, bool DROP>
__global__ __launch_bounds__(512) void attn_fwd_mfma(const float *__restrict__ q, const float *__restrict__ k,
                                                     const float *__restrict__ v, float *__restrict__ out,
                                                     float *__restrict__ lse, AttnP p)
{
    constexpr int KS = D / 2, LD = D + 4;
    __shared__ __attribute__((aligned(16))) float sK[2][2][32][LD];      // [buffer][sub-tile] K tile [key][d]
    __shared__ __attribute__((aligned(16))) float sVt[2][2][D][36];      // V tile transposed [d][tpos(key)]
    __shared__ float sMerge[4][18][64];                                  // the second key half's O, max, sum per lane
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
    const int qw = wave & 3, ks = wave >> 2, tt = t & 255, sub = t >> 8;   // sub: the sub-tile this thread stages
    const int b = blockIdx.z, hd = blockIdx.y;
    const int q0 = blockIdx.x * ATTN_TQ + qw * 32, qi = q0 + r;
    const bool active = q0 < p.Sq, qv = qi < p.Sq;
    const float *qb = q + b * p.q[0] + hd * p.q[1];
    const float *kb = k + b * p.k[0] + hd * p.k[1];
    const float *vb = v + b * p.v[0] + hd * p.v[1];
    const float scale = 1.f / sqrtf((float)D), c2 = scale * ATTN_LOG2E;
    const float inv_keep = (float)p.inv_keep;

    float qr[KS];
    attn_load_row<KS>(qb, p.q[2], qv ? qi : 0, h, qr);
    floatx16 o;
#pragma unroll
    for (int e = 0; e < 16; ++e) o[e] = 0.f;
    float m = -3.0e38f, l = 0.f;

    const int nt = (p.Sk + 63) / 64;
    AttnTile<D> tk, tv;
    tk.fetch(kb, p.k[2], sub * 32, p.Sk, tt);
    tv.fetch(vb, p.v[2], sub * 32, p.Sk, tt);
    tk.put_rows(sK[0][sub], tt);
    tv.put_cols(sVt[0][sub], tt);
    __syncthreads();
    for (int kt = 0; kt < nt; ++kt) {
        const int buf = kt & 1, key0 = kt * 64 + ks * 32;
        if (kt + 1 < nt) {
            tk.fetch(kb, p.k[2], (kt + 1) * 64 + sub * 32, p.Sk, tt);
            tv.fetch(vb, p.v[2], (kt + 1) * 64 + sub * 32, p.Sk, tt);
        }
        if (active && key0 < p.Sk) {
            floatx16 s;
#pragma unroll
            for (int e = 0; e < 16; ++e) s[e] = 0.f;
            attn_mfma_row<KS>(&sK[buf][ks][r][h * KS], qr, s);
            if (key0 + 32 > p.Sk) {
#pragma unroll
                for (int e = 0; e < 16; ++e)
                    if (key0 + mfma_crow(e, h) >= p.Sk) s[e] = -INFINITY;
            }
            float mx = s[0];
#pragma unroll
            for (int e = 1; e < 16; ++e) mx = fmaxf(mx, s[e]);
            mx = fmaxf(mx, __shfl_xor(mx, 32));
            const float mn = fmaxf(m, mx);
            const float alpha = __builtin_amdgcn_exp2f((m - mn) * c2);
            float ls = 0.f;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                s[e] = __builtin_amdgcn_exp2f((s[e] - mn) * c2);
                ls += s[e];
            }
            l = l * alpha + ls;
            m = mn;
#pragma unroll
            for (int e = 0; e < 16; ++e) o[e] *= alpha;
            if (DROP) {
#pragma unroll
                for (int e = 0; e < 16; ++e)
                    s[e] = attn_keep(p, b, hd, qv ? qi : 0, key0 + mfma_crow(e, h)) ? s[e] * inv_keep : 0.f;
            }
            attn_mfma_col(&sVt[buf][ks][r & (D - 1)][16 * h], s, o);
        }
        if (kt + 1 < nt) {
            tk.put_rows(sK[buf ^ 1][sub], tt);
            tv.put_cols(sVt[buf ^ 1][sub], tt);
        }
        __syncthreads();
    }
    if (ks == 1) {
#pragma unroll
        for (int e = 0; e < 16; ++e) sMerge[qw][e][lane] = o[e];
        sMerge[qw][16][lane] = m;
        sMerge[qw][17][lane] = l;
    }
    __syncthreads();
    if (ks == 1 || !qv) return;
    {
        // (a half that saw no key has m = -3e38 and l = 0: its weight underflows to 0)
        const float m1 = sMerge[qw][16][lane], l1 = sMerge[qw][17][lane];
        const float mt = fmaxf(m, m1);
        const float a0 = __builtin_amdgcn_exp2f((m - mt) * c2), a1 = __builtin_amdgcn_exp2f((m1 - mt) * c2);
#pragma unroll
        for (int e = 0; e < 16; ++e) o[e] = o[e] * a0 + sMerge[qw][e][lane] * a1;
        l = l * a0 + l1 * a1;
        m = mt;
    }
    l += __shfl_xor(l, 32);
    attn_store_acc<D>(out + b * p.o[0] + hd * p.o[1] + qi * p.o[2], o, h, 1.f / l);
    if (h == 0) lse[((int64_t)b * p.H + hd) * p.Sq + qi] = m * scale + logf(l);
}

// dQ: lane = query.  Per key tile: S^T = K Q^T, dP^T = V dO^T, dS = P (dP - delta), dQ^T += K^T dS^T.
template <int D, bool DROP>
__global__ __launch_bounds__(256) void attn_bwd_dq_mfma(const float *__restrict__ go, const float *__restrict__ q,
                                                        const float *__restrict__ k, const float *__restrict__ v,
                                                        const float *__restrict__ lse, const float *__restrict__ delta,
                                                        float *__restrict__ gq, AttnP p)
{
    constexpr int KS = D / 2, LD = D + 4;
    __shared__ __attribute__((aligned(16))) float sK[32][LD];
    __shared__ __attribute__((aligned(16))) float sV[32][LD];
    __shared__ __attribute__((aligned(16))) float sKt[D][36];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
    const int b = blockIdx.z, hd = blockIdx.y;
    const int q0 = blockIdx.x * ATTN_TQ + wave * 32, qi = q0 + r;
    const bool active = q0 < p.Sq, qv = qi < p.Sq;
    const int qc = qv ? qi : 0;
    const float *kb = k + b * p.k[0] + hd * p.k[1];
    const float *vb = v + b * p.v[0] + hd * p.v[1];
    const float scale = 1.f / sqrtf((float)D), c2 = scale * ATTN_LOG2E;
    const float inv_keep = (float)p.inv_keep;

    float qr[KS], gr[KS];
    attn_load_row<KS>(q + b * p.q[0] + hd * p.q[1], p.q[2], qc, h, qr);
    attn_load_row<KS>(go + b * p.go[0] + hd * p.go[1], p.go[2], qc, h, gr);
    const int64_t srow = ((int64_t)b * p.H + hd) * p.Sq + qc;
    const float l2 = lse[srow] * ATTN_LOG2E, dl = delta[srow];
    floatx16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;

    const int nt = (p.Sk + 31) / 32;
    AttnTile<D> tk, tv;
    tk.fetch(kb, p.k[2], 0, p.Sk, t);
    tv.fetch(vb, p.v[2], 0, p.Sk, t);
    for (int kt = 0; kt < nt; ++kt) {
        __syncthreads();
        tk.put_rows(sK, t);
        tk.put_cols(sKt, t);
        tv.put_rows(sV, t);
        __syncthreads();
        if (kt + 1 < nt) {                                   // the next tile's loads fly during this tile's MFMAs
            tk.fetch(kb, p.k[2], (kt + 1) * 32, p.Sk, t);
            tv.fetch(vb, p.v[2], (kt + 1) * 32, p.Sk, t);
        }
        if (active) {
            floatx16 s, dp;
#pragma unroll
            for (int e = 0; e < 16; ++e) s[e] = dp[e] = 0.f;
            attn_mfma_row<KS>(&sK[r][h * KS], qr, s);
            attn_mfma_row<KS>(&sV[r][h * KS], gr, dp);
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int key = kt * 32 + mfma_crow(e, h);
                const float pv = key < p.Sk ? __builtin_amdgcn_exp2f(s[e] * c2 - l2) : 0.f;
                float d = dp[e];
                if (DROP) d = attn_keep(p, b, hd, qc, key) ? d * inv_keep : 0.f;
                s[e] = pv * (d - dl);
            }
            attn_mfma_col(&sKt[r & (D - 1)][16 * h], s, acc);
        }
    }
    if (!qv) return;
    attn_store_acc<D>(gq + b * p.dq[0] + hd * p.dq[1] + qi * p.dq[2], acc, h, scale);
}

// dK, dV: lane = key.  Per query tile: S = Q K^T, dP = dO V^T, dV^T += dO^T P, dK^T += Q^T dS.
template <int D, bool DROP>
__global__ __launch_bounds__(256) void attn_bwd_dkv_mfma(const float *__restrict__ go, const float *__restrict__ q,
                                                         const float *__restrict__ k, const float *__restrict__ v,
                                                         const float *__restrict__ lse, const float *__restrict__ delta,
                                                         float *__restrict__ gk, float *__restrict__ gv, AttnP p)
{
    constexpr int KS = D / 2, LD = D + 4;
    __shared__ __attribute__((aligned(16))) float sQ[32][LD];
    __shared__ __attribute__((aligned(16))) float sG[32][LD];
    __shared__ __attribute__((aligned(16))) float sQt[D][36];
    __shared__ __attribute__((aligned(16))) float sGt[D][36];
    __shared__ __attribute__((aligned(16))) float sL[32], sDl[32];     // lse * log2(e) and delta of the tile, at tpos(query)
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
    const int b = blockIdx.z, hd = blockIdx.y;
    const int k0 = blockIdx.x * ATTN_TQ + wave * 32, kj = k0 + r;
    const bool active = k0 < p.Sk, kv = kj < p.Sk;
    const int kc = kv ? kj : 0;
    const float *qb = q + b * p.q[0] + hd * p.q[1];
    const float *gb = go + b * p.go[0] + hd * p.go[1];
    const float *lb = lse + ((int64_t)b * p.H + hd) * p.Sq, *db = delta + ((int64_t)b * p.H + hd) * p.Sq;
    const float scale = 1.f / sqrtf((float)D), c2 = scale * ATTN_LOG2E;
    const float inv_keep = (float)p.inv_keep;

    float kr[KS], vr[KS];
    attn_load_row<KS>(k + b * p.k[0] + hd * p.k[1], p.k[2], kc, h, kr);
    attn_load_row<KS>(v + b * p.v[0] + hd * p.v[1], p.v[2], kc, h, vr);
    floatx16 ak, av;
#pragma unroll
    for (int e = 0; e < 16; ++e) ak[e] = av[e] = 0.f;

    const int nt = (p.Sq + 31) / 32;
    AttnTile<D> tq, tg;
    float lv = 0.f, dv_ = 0.f;
    auto fetch = [&](int qt) {
        tq.fetch(qb, p.q[2], qt * 32, p.Sq, t);
        tg.fetch(gb, p.go[2], qt * 32, p.Sq, t);
        const bool ok = t < 32 && qt * 32 + t < p.Sq;
        lv = ok ? lb[qt * 32 + t] * ATTN_LOG2E : 0.f;
        dv_ = ok ? db[qt * 32 + t] : 0.f;
    };
    fetch(0);
    for (int qt = 0; qt < nt; ++qt) {
        __syncthreads();
        tq.put_rows(sQ, t);
        tq.put_cols(sQt, t);
        tg.put_rows(sG, t);
        tg.put_cols(sGt, t);
        if (t < 32) {
            sL[attn_tpos(t)] = lv;
            sDl[attn_tpos(t)] = dv_;
        }
        __syncthreads();
        if (qt + 1 < nt) fetch(qt + 1);                      // the next tile's loads fly during this tile's MFMAs
        if (active) {
            floatx16 s, dp;
#pragma unroll
            for (int e = 0; e < 16; ++e) s[e] = dp[e] = 0.f;
            attn_mfma_row<KS>(&sQ[r][h * KS], kr, s);
            attn_mfma_row<KS>(&sG[r][h * KS], vr, dp);
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int qi = qt * 32 + mfma_crow(e, h);
                const float pv = qi < p.Sq ? __builtin_amdgcn_exp2f(s[e] * c2 - sL[16 * h + e]) : 0.f;
                float d = dp[e], pd = pv;
                if (DROP) {
                    const bool keep = attn_keep(p, b, hd, qi < p.Sq ? qi : 0, kc);
                    d = keep ? d * inv_keep : 0.f;
                    pd = keep ? pv * inv_keep : 0.f;
                }
                s[e] = pv * (d - sDl[16 * h + e]);
                dp[e] = pd;
            }
            attn_mfma_col(&sGt[r & (D - 1)][16 * h], dp, av);
            attn_mfma_col(&sQt[r & (D - 1)][16 * h], s, ak);
        }
    }
    if (!kv) return;
    attn_store_acc<D>(gk + b * p.dk[0] + hd * p.dk[1] + kj * p.dk[2], ak, h, scale);
    attn_store_acc<D>(gv + b * p.dv[0] + hd * p.dv[1] + kj * p.dv[2], av, h, 1.f);
}

// ---- launchers and the entry path: one AttnCall, attn_route(), a switch on the route's kind ---------------------------------

static std::atomic<const char *> g_attn_last_kernel{"none"};

static dim3 attn_dim3(const AttnGrid &g) { return dim3(g.x, g.y, g.z); }

// f(bool_constant<DROP>) for the route's dropout flag; f(integral_constant<int, D>, bool_constant<DROP>) for an MFMA route
template <typename F> static void attn_for_drop(const AttnRoute &r, F f)
{
    if (r.drop) f(std::true_type());
    else f(std::false_type());
}
template <typename F> static void attn_for_mfma(const AttnRoute &r, F f)
{
    attn_for_drop(r, [&](auto drop) {
        if (r.D == 16) f(std::integral_constant<int, 16>(), drop);
        else f(std::integral_constant<int, 32>(), drop);
    });
}

// every kind of the fp32 / fp64 entries; the backward's after attn_delta
template <typename T> static int attn_launch(const AttnCall &c)
{
    const AttnRoute &r = c.r;
    const AttnP &p = c.p;
    const T *go = (const T *)c.go, *q = (const T *)c.q, *k = (const T *)c.k, *v = (const T *)c.v;
    T *out = (T *)c.out, *lse = (T *)c.lse, *delta = (T *)c.work, *gq = (T *)c.gq, *gk = (T *)c.gk, *gv = (T *)c.gv;
    const dim3 grid = attn_dim3(r.grid), grid_kv = attn_dim3(r.grid_kv);
    if (r.with_dq) hipLaunchKernelGGL((attn_delta<T>), dim3(r.grid_delta), dim3(256), 0, c.st, go, out, delta, p);
    if constexpr (std::is_same<T, float>::value) {
        if (r.kind == AttnKind::fwd_mfma || r.kind == AttnKind::bwd_mfma) {
            attn_for_mfma(r, [&](auto d, auto drop) {
                constexpr int D = decltype(d)::value;
                constexpr bool DROP = decltype(drop)::value;
                if (r.kind == AttnKind::fwd_mfma) {
                    hipLaunchKernelGGL((attn_fwd_mfma<D, DROP>), grid, dim3(512), 0, c.st, q, k, v, out, lse, p);
                } else {
                    hipLaunchKernelGGL((attn_bwd_dq_mfma<D, DROP>), grid, dim3(256), 0, c.st, go, q, k, v, lse, delta, gq, p);
                    hipLaunchKernelGGL((attn_bwd_dkv_mfma<D, DROP>), grid_kv, dim3(256), 0, c.st, go, q, k, v, lse, delta, gk, gv, p);
                }
            });
            return (int)hipGetLastError();
        }
    }
    attn_for_drop(r, [&](auto drop) {
        constexpr bool DROP = decltype(drop)::value;
        if (r.kind == AttnKind::fwd_generic) {
            hipLaunchKernelGGL((attn_fwd_generic<T, DROP>), grid, dim3(256), 0, c.st, q, k, v, out, lse, p);
        } else {
            if (r.with_dq) hipLaunchKernelGGL((attn_bwd_dq_generic<T, DROP>), grid, dim3(256), 0, c.st, go, q, k, v, lse, delta, gq, p);
            hipLaunchKernelGGL((attn_bwd_dkv_generic<T, DROP>), grid_kv, dim3(256), 0, c.st, go, q, k, v, lse, delta, gk, gv, p);
        }
    });
    return (int)hipGetLastError();
}

int attn_entry(AttnEntry entry, AttnCall c, const int64_t *strides, int B, int H, int Sq, int Sk, int D, double dropout_p, uint64_t seed)
{
    const bool half = entry == AttnEntry::forward_half, bwd = entry == AttnEntry::backward;
    // the strides of q, k, v, out (and the backward's grad_out, grad_q, grad_k, grad_v): float4 / 16-byte access to every row
    const int nstr = bwd ? 24 : 12;
    const bool ptrs16 = aligned(c.q, 16) && aligned(c.k, 16) && aligned(c.v, 16) &&
                        (bwd ? aligned(c.go, 16) && aligned(c.gq, 16) && aligned(c.gk, 16) && aligned(c.gv, 16) : aligned(c.out, 16));
    bool strides_ok = strides != nullptr;
    for (int i = 0; strides && i < nstr; ++i) strides_ok = strides_ok && strides[i] % (half ? 8 : 4) == 0;
    c.r = attn_route(AttnQuery{entry, half ? 2 : c.type == AttnType::f32 ? 4 : 8, B, H, Sq, Sk, D, dropout_p, half ? g_ah_query_tile.load() : 0,
                               strides != nullptr, strides_ok, c.q != nullptr, c.k != nullptr, c.v != nullptr, c.out != nullptr,
                               c.lse != nullptr, c.go != nullptr, c.work != nullptr, c.gq != nullptr, c.gk != nullptr, c.gv != nullptr, ptrs16});
    const AttnRoute &r = c.r;
    if (r.status == AttnStatus::empty) return 0;
    if (r.status != AttnStatus::ok) return (int)(r.status == AttnStatus::invalid_value ? hipErrorInvalidValue : hipErrorNotSupported);
    c.p.B = B; c.p.H = H; c.p.Sq = Sq; c.p.Sk = Sk; c.p.D = D;
    int64_t *dst[8] = {c.p.q, c.p.k, c.p.v, c.p.o, c.p.go, c.p.dq, c.p.dk, c.p.dv};
    for (int i = 0; i < 24; ++i) dst[i / 3][i % 3] = i < nstr ? strides[i] : 0;
    c.p.thresh = mvdetr_attn_threshold(dropout_p);
    c.p.seed = seed;
    c.p.inv_keep = 1.0 / (1.0 - dropout_p);
    g_attn_last_kernel = r.name;
    if (half) return attn_launch_forward_half(c);
    return c.type == AttnType::f32 ? attn_launch<float>(c) : attn_launch<double>(c);
}

}  // namespace mvdetr

using namespace mvdetr;

extern "C" {

const char *mvdetr_attention_last_kernel(void) { return g_attn_last_kernel.load(); }

int64_t mvdetr_attention_workspace_bytes(int batch, int heads, int sq, int sk, int head_dim, int elem_size)
{
    if (batch < 0 || heads < 0 || sq < 0 || sk < 0 || head_dim < 0 || elem_size < 0) return -1;
    return (int64_t)batch * heads * sq * elem_size;         // delta
}

int mvdetr_attention_route_kind(int entry, int elem_size, int batch, int heads, int sq, int sk, int head_dim, double dropout_p,
                                int strides_ok, int aligned)
{
    if (entry < 0 || entry > (int)AttnEntry::forward_half) return -(int)AttnStatus::invalid_value;
    const AttnRoute r = attn_route(AttnQuery{(AttnEntry)entry, elem_size, batch, heads, sq, sk, head_dim, dropout_p, g_ah_query_tile.load(), true,
                                             strides_ok != 0, true, true, true, true, true, true, true, true, true, true, aligned != 0});
    return r.status == AttnStatus::ok ? (int)r.kind : -(int)r.status;
}

#define MVDETR_ATTN_ENTRIES(T, SFX, TYPE)                                                                                    \
    int mvdetr_attention_forward_##SFX(void *stream, const T *q, const T *k, const T *v, const int64_t *strides, int batch,  \
                                       int heads, int sq, int sk, int head_dim, double dropout_p, uint64_t seed, T *out,     \
                                       T *lse)                                                                               \
    {                                                                                                                        \
        return attn_entry(AttnEntry::forward, AttnCall{(hipStream_t)stream, TYPE, nullptr, q, k, v, out, lse, nullptr, nullptr, nullptr, \
                                                       nullptr, {}, {}}, strides, batch, heads, sq, sk, head_dim, dropout_p, seed);  \
    }                                                                                                                        \
    int mvdetr_attention_backward_##SFX(void *stream, const T *grad_out, const T *q, const T *k, const T *v, const T *out,   \
                                        const T *lse, const int64_t *strides, int batch, int heads, int sq, int sk,          \
                                        int head_dim, double dropout_p, uint64_t seed, void *workspace, T *grad_q,           \
                                        T *grad_k, T *grad_v)                                                                \
    {                                                                                                                        \
        /* (the backward only reads out and lse: their const is cast away for the descriptor alone) */                      \
        return attn_entry(AttnEntry::backward, AttnCall{(hipStream_t)stream, TYPE, grad_out, q, k, v, const_cast<T *>(out),  \
                                                        const_cast<T *>(lse), workspace, grad_q, grad_k, grad_v, {}, {}},    \
                          strides, batch, heads, sq, sk, head_dim, dropout_p, seed);                                         \
    }

MVDETR_ATTN_ENTRIES(float, f32, AttnType::f32)
MVDETR_ATTN_ENTRIES(double, f64, AttnType::f64)

}  // extern "C"

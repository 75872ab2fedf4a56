// Deformable convolution (torchvision.ops.deform_conv2d, v1: no modulation mask, weight groups 1) for gfx950.
//
// out[b, o, h, w] = bias[o] + sum_{c, i, j} weight[o, c, i, j] * sample(input[b, c], y, x)
//   y = h * stride_h - pad_h + i * dil_h + offset[b, 2 * (g * kh * kw + i * kw + j), h, w]       (x likewise, channel + 1)
// sampled bilinearly in pixel units with NO -0.5 shift; 0 when y <= -1, y >= H, x <= -1 or x >= W; a corner outside the
// image contributes 0.  g is the offset group of channel c (C / offset_groups channels each).
//
// Routes (mvdetr_deform_conv2d_last_kernel names them):
//   dc_fwd_mfma      implicit GEMM D[o, p] = W[o, k] . col[k, p] on v_mfma_f32_32x32x2_f32.  A workgroup owns 64 output
//                    pixels x 128 output channels; its K loop runs over (tap, 32 or 16 input channels): the 64 pixels' taps
//                    are sampled from the channel-last input (a bilinear corner = C contiguous floats, one 16-byte load per
//                    4 channels) into an LDS column tile and multiplied against the weight tile.  No column buffer in HBM,
//                    no scratch.  fp32, offset_groups 1, channel-last input, C % 16 == 0, C_out % 32 == 0.
//   dc_bwd_mfma      (same preconditions) two kernels:
//                    dc_bwd_col_mfma     g_col[c, p] = W[:, c, tap]^T . grad_out[:, p] per (64-pixel tile, 128 channels,
//                                        tap) by MFMA; its epilogue reduces the offset gradient over the lane's channels
//                                        in registers (then across lanes and waves through LDS) and adds g_col x corner
//                                        weight into grad_input with fp32 atomics.
//                    dc_bwd_weight_mfma  grad_W[o, (c, tap)] = grad_out[o, :] . col[(c, tap), :] over a pixel range, the
//                                        column tile re-sampled in LDS as the forward does; the pixel ranges' partial
//                                        sums are added with atomics.
//   dc_fwd_generic / dc_bwd_generic   any shape, fp32 and fp64, NCHW or channel-last input: one lane per output element
//                    (forward), one lane per (batch, group, tap, pixel) (grad_input / grad_offset), one workgroup per
//                    (input channel, tap) row of grad_W.
// Results of the backward are not bit-reproducible run to run (fp32 / fp64 atomics), like torchvision's CUDA kernel.
#include "../../include/mvdetr_ops.h"
#include "common.h"
#include "deform_conv.h"
#include "half_mfma.h"

#include <atomic>

namespace mvdetr {

// sampling position of output pixel (ho, wo), tap (i, j), from the offset tensor [B, 2 * G * T, Ho, Wo]
template <typename T>
__device__ __forceinline__ void dc_pos(const T *__restrict__ off, const DcShape &s, int b, int g, int tap, int ho, int wo,
                                       T &y, T &x)
{
    const int T_ = s.kh * s.kw, HWo = s.Ho * s.Wo;
    const int i = tap / s.kw, j = tap - i * s.kw;
    const T *o = off + ((int64_t)b * 2 * s.G * T_ + 2 * (g * T_ + tap)) * HWo + ho * s.Wo + wo;
    y = T(ho * s.sh - s.ph + i * s.dh) + o[0];
    x = T(wo * s.sw - s.pw + j * s.dw) + o[HWo];
}

// ---- generic kernels (any shape, fp32 / fp64, NCHW or channel-last input) -----------------------------------------------

template <typename T>
__global__ __launch_bounds__(256) void dc_fwd_generic(const T *__restrict__ in, const T *__restrict__ off,
                                                      const T *__restrict__ wt, const T *__restrict__ bias, T *__restrict__ out,
                                                      DcShape s, int cl)
{
    const int T_ = s.kh * s.kw, Cg = s.C / s.G;
    const int64_t HW = (int64_t)s.H * s.W, pst = cl ? s.C : 1, cst = cl ? 1 : HW;
    const int64_t n = (int64_t)s.B * s.Co * s.Ho * s.Wo;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * 256) {
        const int wo = (int)(idx % s.Wo);
        int64_t r = idx / s.Wo;
        const int ho = (int)(r % s.Ho);
        r /= s.Ho;
        const int o = (int)(r % s.Co), b = (int)(r / s.Co);
        const T *inb = in + (int64_t)b * s.C * HW;
        T acc = bias ? bias[o] : T(0);
        for (int g = 0; g < s.G; ++g)
            for (int tap = 0; tap < T_; ++tap) {
                T y, x;
                dc_pos(off, s, b, g, tap, ho, wo, y, x);
                const DcFoot<T> f = dc_foot(y, x, s.H, s.W);
                if (!f.in) continue;
                for (int c = g * Cg; c < (g + 1) * Cg; ++c) {
                    const T *pc = inb + c * cst;
                    T v = T(0);
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (f.ok[q]) v += f.w[q] * pc[f.pix[q] * pst];
                    acc += wt[((int64_t)o * s.C + c) * T_ + tap] * v;
                }
            }
        out[idx] = acc;
    }
}

// grad_input (accumulated with atomics) and grad_offset (written) : one lane per (b, g, tap, pixel)
template <typename T>
__global__ __launch_bounds__(256) void dc_bwd_input_generic(const T *__restrict__ gout, const T *__restrict__ in,
                                                            const T *__restrict__ off, const T *__restrict__ wt,
                                                            T *__restrict__ gin, T *__restrict__ goff, DcShape s, int cl)
{
    const int T_ = s.kh * s.kw, Cg = s.C / s.G, HWo = s.Ho * s.Wo;
    const int64_t HW = (int64_t)s.H * s.W, pst = cl ? s.C : 1, cst = cl ? 1 : HW;
    const int64_t n = (int64_t)s.B * s.G * T_ * HWo;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * 256) {
        const int p = (int)(idx % HWo);
        int64_t r = idx / HWo;
        const int tap = (int)(r % T_);
        r /= T_;
        const int g = (int)(r % s.G), b = (int)(r / s.G);
        const int ho = p / s.Wo, wo = p - ho * s.Wo;
        T y, x;
        dc_pos(off, s, b, g, tap, ho, wo, y, x);
        const DcFoot<T> f = dc_foot(y, x, s.H, s.W);
        T gy = T(0), gx = T(0);
        if (f.in) {
            const T *inb = in + (int64_t)b * s.C * HW;
            T *ginb = gin + (int64_t)b * s.C * HW;
            const T *gob = gout + (int64_t)b * s.Co * HWo + p;
            for (int c0 = g * Cg; c0 < (g + 1) * Cg; c0 += 4) {
                const int nc = min(4, (g + 1) * Cg - c0);
                T gc[4] = {T(0), T(0), T(0), T(0)};
                for (int o = 0; o < s.Co; ++o) {
                    const T go = gob[(int64_t)o * HWo];
                    const T *wp = wt + ((int64_t)o * s.C + c0) * T_ + tap;
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (q < nc) gc[q] += wp[q * T_] * go;
                }
                for (int q = 0; q < nc; ++q) {
                    const T *pc = inb + (c0 + q) * cst;
                    T *gc_ = ginb + (c0 + q) * cst;
                    T v[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) v[k] = f.ok[k] ? pc[f.pix[k] * pst] : T(0);
                    gy += gc[q] * ((T(1) - f.lx) * (v[2] - v[0]) + f.lx * (v[3] - v[1]));
                    gx += gc[q] * ((T(1) - f.ly) * (v[1] - v[0]) + f.ly * (v[3] - v[2]));
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (f.ok[k]) atomicAdd(gc_ + f.pix[k] * pst, f.w[k] * gc[q]);
                }
            }
        }
        T *go_ = goff + ((int64_t)b * 2 * s.G * T_ + 2 * (g * T_ + tap)) * HWo + p;
        go_[0] = gy;
        go_[HWo] = gx;
    }
}

// grad_weight (written): one workgroup per (input channel, tap) and 256 output channels; the row's samples are staged in LDS
// 256 pixels at a time and every lane (one output channel) runs over them.
template <typename T>
__global__ __launch_bounds__(256) void dc_bwd_weight_generic(const T *__restrict__ gout, const T *__restrict__ in,
                                                             const T *__restrict__ off, T *__restrict__ gw, DcShape s, int cl)
{
    __shared__ T samp[256];
    const int T_ = s.kh * s.kw, Cg = s.C / s.G, HWo = s.Ho * s.Wo;
    const int64_t HW = (int64_t)s.H * s.W, pst = cl ? s.C : 1, cst = cl ? 1 : HW;
    const int c = blockIdx.x / T_, tap = blockIdx.x - c * T_, g = c / Cg;
    const int o = blockIdx.y * 256 + threadIdx.x;
    const int64_t P = (int64_t)s.B * HWo;
    T acc = T(0);
    for (int64_t p0 = 0; p0 < P; p0 += 256) {
        const int64_t gp = p0 + threadIdx.x;
        T v = T(0);
        if (gp < P) {
            const int b = (int)(gp / HWo), p = (int)(gp - (int64_t)b * HWo);
            const int ho = p / s.Wo, wo = p - ho * s.Wo;
            T y, x;
            dc_pos(off, s, b, g, tap, ho, wo, y, x);
            const DcFoot<T> f = dc_foot(y, x, s.H, s.W);
            const T *pc = in + (int64_t)b * s.C * HW + c * cst;
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (f.ok[q]) v += f.w[q] * pc[f.pix[q] * pst];
        }
        samp[threadIdx.x] = v;
        __syncthreads();
        if (o < s.Co) {
            const int n = (int)(P - p0 < 256 ? P - p0 : 256);
            int b = (int)(p0 / HWo), p = (int)(p0 - (int64_t)b * HWo);
            const T *go = gout + ((int64_t)b * s.Co + o) * HWo;
            for (int k = 0; k < n; ++k) {
                acc += go[p] * samp[k];
                if (++p == HWo) {
                    p = 0;
                    go += (int64_t)s.Co * HWo;
                }
            }
        }
        __syncthreads();
    }
    if (o < s.Co) gw[((int64_t)o * s.C + c) * T_ + tap] = acc;
}

// ---- MFMA kernels (fp32, offset_groups 1, channel-last input, C % 16 == 0, C_out % 32 == 0) -----------------------------

// KS MFMA steps over an LDS A tile (rows = 32 lanes' i, k contiguous) and B tile (rows = j, k contiguous): lane half h takes
// local k = h * KS + step, so each lane reads KS contiguous floats of its row (16-byte LDS reads; rows padded by 4 floats).
template <int KS, int NB>
__device__ __forceinline__ void dc_mfma_tile(const float *a_row, const float *const (&b_rows)[NB], floatx16 (&acc)[NB])
{
    float a[KS], bb[NB][KS];
#pragma unroll
    for (int q = 0; q < KS; q += 4) {
        const float4 v = *reinterpret_cast<const float4 *>(a_row + q);
        a[q] = v.x; a[q + 1] = v.y; a[q + 2] = v.z; a[q + 3] = v.w;
#pragma unroll
        for (int n = 0; n < NB; ++n) {
            const float4 u = *reinterpret_cast<const float4 *>(b_rows[n] + q);
            bb[n][q] = u.x; bb[n][q + 1] = u.y; bb[n][q + 2] = u.z; bb[n][q + 3] = u.w;
        }
    }
#pragma unroll
    for (int q = 0; q < KS; ++q)
#pragma unroll
        for (int n = 0; n < NB; ++n) acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q], bb[n][q], acc[n], 0, 0, 0);
}

template <int KC>
__global__ __launch_bounds__(256) void dc_fwd_mfma(const float *__restrict__ in, const float *__restrict__ off,
                                                   const float *__restrict__ wt, const float *__restrict__ bias,
                                                   float *__restrict__ out, DcShape s)
{
    constexpr int KS = KC / 2, CPT = KC / 4;     // MFMA steps per chunk; channels each sampler lane stages
    __shared__ __attribute__((aligned(16))) float sW[DC_TO][KC + 4];    // weight tile [o][k]
    __shared__ __attribute__((aligned(16))) float sX[DC_TP][KC + 4];    // column tile [p][k]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
    const int T_ = s.kh * s.kw, HWo = s.Ho * s.Wo;
    const int64_t P = (int64_t)s.B * HWo, p0 = (int64_t)blockIdx.x * DC_TP;
    const int o0 = blockIdx.y * DC_TO;
    const bool active = o0 + wave * 32 < s.Co;

    // sampler role: pixel sp, channels [sq * CPT, sq * CPT + CPT) of each chunk
    const int sp = t >> 2, sq = t & 3;
    const int64_t gp = p0 + sp;
    const bool pv = gp < P;
    int b = 0, p = 0, ho = 0, wo = 0;
    if (pv) dc_pixel(s, gp, b, p, ho, wo);
    const float *inb = in + (int64_t)b * s.H * s.W * s.C;

    floatx16 acc[2];
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[n][e] = 0.f;

    for (int tap = 0; tap < T_; ++tap) {
        float y = -2.f, x = -2.f;
        if (pv) dc_pos(off, s, b, 0, tap, ho, wo, y, x);
        const DcFoot<float> f = dc_foot(y, x, s.H, s.W);
        const float *cp[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) cp[k] = inb + (int64_t)f.pix[k] * s.C + sq * CPT;
        for (int c0 = 0; c0 < s.C; c0 += KC) {
#pragma unroll
            for (int v = 0; v < CPT; v += 4) {
                float4 acc4 = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float4 u = load4_or_zero(cp[k] + c0 + v, f.ok[k], inb);
                    acc4.x += f.w[k] * u.x; acc4.y += f.w[k] * u.y; acc4.z += f.w[k] * u.z; acc4.w += f.w[k] * u.w;
                }
                *reinterpret_cast<float4 *>(&sX[sp][sq * CPT + v]) = acc4;
            }
            for (int e = t; e < DC_TO * KC; e += 256) {
                const int o = e / KC, k = e - o * KC;
                sW[o][k] = o0 + o < s.Co ? wt[((int64_t)(o0 + o) * s.C + c0 + k) * T_ + tap] : 0.f;
            }
            __syncthreads();
            if (active) {
                const float *brow[2] = {&sX[r][h * KS], &sX[32 + r][h * KS]};
                dc_mfma_tile<KS, 2>(&sW[wave * 32 + r][h * KS], brow, acc);
            }
            __syncthreads();
        }
    }
    if (!active) return;
    // D[i][j]: column j = lane & 31 (pixel), row i = mfma_crow(reg, lane >> 5) (output channel)
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        const int64_t q = p0 + n * 32 + r;
        if (q >= P) continue;
        int qb, qp, qh, qw;
        dc_pixel(s, q, qb, qp, qh, qw);
        float *ob = out + (int64_t)qb * s.Co * HWo + qp;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int o = o0 + wave * 32 + mfma_crow(e, h);
            ob[(int64_t)o * HWo] = acc[n][e] + (bias ? bias[o] : 0.f);
        }
    }
}

// g_col = W[:, c, tap]^T . grad_out per (64-pixel tile, 128 input channels, tap); epilogue: grad_input += g_col x corner
// weight (atomics), grad_offset = sum_c g_col x d sample / d (y, x)
__global__ __launch_bounds__(256) void dc_bwd_col_mfma(const float *__restrict__ gout, const float *__restrict__ in,
                                                       const float *__restrict__ off, const float *__restrict__ wt,
                                                       float *__restrict__ gin, float *__restrict__ goff, DcShape s)
{
    constexpr int KC = 32, KS = 16;
    __shared__ __attribute__((aligned(16))) float sA[DC_TO][KC + 4];    // W^T tile [c][o]
    __shared__ __attribute__((aligned(16))) float sB[DC_TP][KC + 4];    // grad_out tile [p][o]
    __shared__ float sRed[4][2][DC_TP];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
    const int T_ = s.kh * s.kw, HWo = s.Ho * s.Wo;
    const int64_t P = (int64_t)s.B * HWo, p0 = (int64_t)blockIdx.x * DC_TP;
    const int cb = blockIdx.y * DC_TO, tap = blockIdx.z;
    const bool active = cb + wave * 32 < s.C;

    // staging role for grad_out: pixel t % 64 (the same for every element this lane stages)
    const int64_t sgp = p0 + (t & 63);
    int sb = 0, sp = 0, sh_ = 0, sw_ = 0;
    if (sgp < P) dc_pixel(s, sgp, sb, sp, sh_, sw_);
    const float *gst = gout + (int64_t)sb * s.Co * HWo + sp;

    floatx16 acc[2];
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[n][e] = 0.f;

    for (int o0 = 0; o0 < s.Co; o0 += KC) {
        for (int e = t; e < DC_TO * KC; e += 256) {
            const int c = e % DC_TO, k = e / DC_TO;
            sA[c][k] = cb + c < s.C ? wt[((int64_t)(o0 + k) * s.C + cb + c) * T_ + tap] : 0.f;
        }
        for (int e = t; e < DC_TP * KC; e += 256) {
            const int k = e / DC_TP;
            sB[t & 63][k] = sgp < P ? gst[(int64_t)(o0 + k) * HWo] : 0.f;
        }
        __syncthreads();
        if (active) {
            const float *brow[2] = {&sB[r][h * KS], &sB[32 + r][h * KS]};
            dc_mfma_tile<KS, 2>(&sA[wave * 32 + r][h * KS], brow, acc);
        }
        __syncthreads();
    }

    float gy[2] = {0.f, 0.f}, gx[2] = {0.f, 0.f};
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        const int64_t q = p0 + n * 32 + r;
        if (!active || q >= P) continue;
        int qb, qp, qh, qw;
        dc_pixel(s, q, qb, qp, qh, qw);
        float y, x;
        dc_pos(off, s, qb, 0, tap, qh, qw, y, x);
        const DcFoot<float> f = dc_foot(y, x, s.H, s.W);
        if (!f.in) continue;
        const float *inb = in + (int64_t)qb * s.H * s.W * s.C;
        float *ginb = gin + (int64_t)qb * s.H * s.W * s.C;
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const int c = cb + wave * 32 + 8 * g4 + 4 * h;       // rows 4 g4' .. of this lane: 4 consecutive channels
            if (c >= s.C) continue;
            float4 v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = load4_or_zero(inb + (int64_t)f.pix[k] * s.C + c, f.ok[k], inb);
            const float gc[4] = {acc[n][4 * g4], acc[n][4 * g4 + 1], acc[n][4 * g4 + 2], acc[n][4 * g4 + 3]};
            const float *v0 = &v[0].x, *v1 = &v[1].x, *v2 = &v[2].x, *v3 = &v[3].x;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                gy[n] += gc[e] * ((1.f - f.lx) * (v2[e] - v0[e]) + f.lx * (v3[e] - v1[e]));
                gx[n] += gc[e] * ((1.f - f.ly) * (v1[e] - v0[e]) + f.ly * (v3[e] - v2[e]));
            }
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (f.ok[k]) {
                    float *dst = ginb + (int64_t)f.pix[k] * s.C + c;
#pragma unroll
                    for (int e = 0; e < 4; ++e) atomicAdd(dst + e, f.w[k] * gc[e]);
                }
        }
    }
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        gy[n] += __shfl_xor(gy[n], 32);
        gx[n] += __shfl_xor(gx[n], 32);
        if (h == 0) {
            sRed[wave][0][n * 32 + r] = gy[n];
            sRed[wave][1][n * 32 + r] = gx[n];
        }
    }
    __syncthreads();
    if (t < 2 * DC_TP) {
        const int pl = t & 63, dir = t >> 6;
        const int64_t q = p0 + pl;
        if (q < P) {
            const float sum = sRed[0][dir][pl] + sRed[1][dir][pl] + sRed[2][dir][pl] + sRed[3][dir][pl];
            int qb, qp, qh, qw;
            dc_pixel(s, q, qb, qp, qh, qw);
            float *dst = goff + ((int64_t)qb * 2 * T_ + 2 * tap + dir) * HWo + qp;
            if (gridDim.y == 1) *dst = sum;
            else atomicAdd(dst, sum);                               // (zeroed by the entry)
        }
    }
}

// grad_W[o, c, tap] (+)= sum over a pixel range of grad_out[o, p] x col[(c, tap), p]: workgroup = (tap, 32 input channels)
// x 128 output channels x one pixel range; K loop over 32-pixel chunks, both tiles staged in LDS
__global__ __launch_bounds__(256) void dc_bwd_weight_mfma(const float *__restrict__ gout, const float *__restrict__ in,
                                                          const float *__restrict__ off, float *__restrict__ gw, DcShape s,
                                                          int64_t pix_per_split)
{
    constexpr int KS = DC_WP / 2;
    __shared__ __attribute__((aligned(16))) float sA[DC_TO][DC_WP + 4];    // grad_out tile [o][p]
    __shared__ __attribute__((aligned(16))) float sB[32][DC_WP + 4];       // column tile [c][p]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
    const int T_ = s.kh * s.kw, HWo = s.Ho * s.Wo;
    const int64_t P = (int64_t)s.B * HWo;
    const int tap = blockIdx.x % T_, cbk = (blockIdx.x / T_) * 32, o0 = blockIdx.y * DC_TO;
    const int64_t ps = (int64_t)blockIdx.z * pix_per_split, pe = ps + pix_per_split < P ? ps + pix_per_split : P;
    const bool active = o0 + wave * 32 < s.Co;
    const int sp = t >> 3, sg = t & 7, sc = cbk + 4 * sg;     // sampler: pixel, 4 channels
    const int ap = t & 31;                                    // grad_out staging: pixel (the same for all its elements)

    floatx16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;

    for (int64_t pc = ps; pc < pe; pc += DC_WP) {
        {
            const int64_t q = pc + sp;
            float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
            if (q < pe && sc < s.C) {
                int qb, qp, qh, qw;
                dc_pixel(s, q, qb, qp, qh, qw);
                float y, x;
                dc_pos(off, s, qb, 0, tap, qh, qw, y, x);
                const DcFoot<float> f = dc_foot(y, x, s.H, s.W);
                const float *inb = in + (int64_t)qb * s.H * s.W * s.C;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float4 u = load4_or_zero(inb + (int64_t)f.pix[k] * s.C + sc, f.ok[k], inb);
                    val.x += f.w[k] * u.x; val.y += f.w[k] * u.y; val.z += f.w[k] * u.z; val.w += f.w[k] * u.w;
                }
            }
            sB[4 * sg][sp] = val.x;
            sB[4 * sg + 1][sp] = val.y;
            sB[4 * sg + 2][sp] = val.z;
            sB[4 * sg + 3][sp] = val.w;
        }
        {
            const int64_t q = pc + ap;
            const bool qv = q < pe;
            int qb = 0, qp = 0, qh, qw;
            if (qv) dc_pixel(s, q, qb, qp, qh, qw);
            const float *go = gout + ((int64_t)qb * s.Co + o0) * HWo + qp;
            for (int e = t; e < DC_TO * DC_WP; e += 256) {
                const int o = e / DC_WP;
                sA[o][ap] = qv && o0 + o < s.Co ? go[(int64_t)o * HWo] : 0.f;
            }
        }
        __syncthreads();
        if (active) {
            const float *brow[1] = {&sB[r][h * KS]};
            floatx16 a1[1] = {acc};
            dc_mfma_tile<KS, 1>(&sA[wave * 32 + r][h * KS], brow, a1);
            acc = a1[0];
        }
        __syncthreads();
    }
    if (!active) return;
    const int c = cbk + r;
    if (c >= s.C) return;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int o = o0 + wave * 32 + mfma_crow(e, h);
        float *dst = gw + ((int64_t)o * s.C + c) * T_ + tap;
        if (gridDim.z == 1) *dst = acc[e];
        else atomicAdd(dst, acc[e]);                                   // (zeroed by the entry)
    }
}

// ---- launchers and the entry path: one DcCall, dc_route(), a switch on the route's kind --------------------------------------

static std::atomic<const char *> g_dc_last_kernel{"none"};

static dim3 dc_dim3(const DcGrid &g) { return dim3(g.x, g.y, g.z); }
static size_t dc_elem_size(DcType type) { return type == DcType::f64 ? 8 : type == DcType::f32 ? 4 : 2; }

// zeroes grad_weight or grad_offset
static hipError_t dc_zero(const DcCall &c, bool weight)
{
    const DcShape &s = c.r.s;
    const size_t n = weight ? (size_t)s.Co * s.C : (size_t)s.B * s.Ho * s.Wo * 2 * s.G;
    return hipMemsetAsync(weight ? c.gw : c.goff, 0, dc_elem_size(c.type) * n * s.kh * s.kw, c.st);
}

template <typename T> static int dc_launch_generic(const DcCall &c)
{
    const DcRoute &r = c.r;
    const T *in = (const T *)c.in, *off = (const T *)c.off, *wt = (const T *)c.wt, *gout = (const T *)c.gout;
    const int cl = c.nhwc ? 1 : 0;
    if (r.kind == DcKind::fwd_generic) {
        hipLaunchKernelGGL((dc_fwd_generic<T>), dc_dim3(r.grid[0]), dim3(256), 0, c.st, in, off, wt, (const T *)c.bias, (T *)c.out, r.s, cl);
    } else {
        hipLaunchKernelGGL((dc_bwd_input_generic<T>), dc_dim3(r.grid[0]), dim3(256), 0, c.st, gout, in, off, wt, (T *)c.gin, (T *)c.goff, r.s, cl);
        hipLaunchKernelGGL((dc_bwd_weight_generic<T>), dc_dim3(r.grid[1]), dim3(256), 0, c.st, gout, in, off, (T *)c.gw, r.s, cl);
    }
    return (int)hipGetLastError();
}

static int dc_launch_mfma(const DcCall &c)
{
    const DcRoute &r = c.r;
    const float *in = (const float *)c.in, *off = (const float *)c.off, *wt = (const float *)c.wt, *gout = (const float *)c.gout;
    if (r.kind == DcKind::fwd_mfma) {
        hipLaunchKernelGGL(r.KC == 32 ? dc_fwd_mfma<32> : dc_fwd_mfma<16>, dc_dim3(r.grid[0]), dim3(256), 0, c.st, in, off, wt,
                           (const float *)c.bias, (float *)c.out, r.s);
        return (int)hipGetLastError();
    }
    hipError_t e;
    if (r.zero_goff && (e = dc_zero(c, false)) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(dc_bwd_col_mfma, dc_dim3(r.grid[0]), dim3(256), 0, c.st, gout, in, off, wt, (float *)c.gin, (float *)c.goff, r.s);
    if (r.zero_gw && (e = dc_zero(c, true)) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(dc_bwd_weight_mfma, dc_dim3(r.grid[1]), dim3(256), 0, c.st, gout, in, off, (float *)c.gw, r.s, r.pps);
    return (int)hipGetLastError();
}

int dc_entry(DcEntry entry, DcCall c, const int (&sh)[14])
{
    // (the last flag is the 16-bit entry's alone; a null bias counts as aligned, and the other entries' null `out` too)
    c.r = dc_route(DcQuery{entry, (int)dc_elem_size(c.type), sh[0], sh[1], sh[2], sh[3], sh[4], sh[5], sh[6], sh[7], sh[8], sh[9], sh[10],
                           sh[11], sh[12], sh[13], c.nhwc, c.obs, c.in != nullptr, c.off != nullptr, c.wt != nullptr, c.out != nullptr,
                           c.gout != nullptr, c.gin != nullptr, c.goff != nullptr, c.gw != nullptr, aligned(c.in, 16), aligned(c.wt, 16),
                           aligned(c.off, 2) && aligned(c.out, 2) && aligned(c.bias, 2)});
    const DcRoute &r = c.r;
    if (r.status == DcStatus::empty) return 0;
    if (r.status != DcStatus::ok) return (int)(r.status == DcStatus::invalid_value ? hipErrorInvalidValue : hipErrorNotSupported);
    if (r.name) g_dc_last_kernel = r.name;
    switch (r.kind) {
    case DcKind::bwd_zero_fill: {                       // nothing flows: the written outputs are zero
        hipError_t e = r.zero_goff ? dc_zero(c, false) : hipSuccess;
        if (e == hipSuccess && r.zero_gw) e = dc_zero(c, true);
        return (int)e;
    }
    case DcKind::fwd_mfma_half: return dc_launch_forward_half(c);
    case DcKind::fwd_mfma:
    case DcKind::bwd_mfma: return dc_launch_mfma(c);
    default: return c.type == DcType::f32 ? dc_launch_generic<float>(c) : dc_launch_generic<double>(c);
    }
}

}  // namespace mvdetr

using namespace mvdetr;

extern "C" {

const char *mvdetr_deform_conv2d_last_kernel(void) { return g_dc_last_kernel.load(); }

int mvdetr_deform_conv2d_route_kind(int entry, int elem_size, MVDETR_DC_SHAPE_PARAMS, int input_nhwc, int aligned)
{
    if (entry < 0 || entry > (int)DcEntry::forward_half) return -(int)DcStatus::invalid_value;
    const int sh[14] = MVDETR_DC_SHAPE;
    const DcRoute r = dc_route(DcQuery{(DcEntry)entry, elem_size, sh[0], sh[1], sh[2], sh[3], sh[4], sh[5], sh[6], sh[7], sh[8], sh[9],
                                       sh[10], sh[11], sh[12], sh[13], input_nhwc, INT64_MAX, true, true, true, true, true, true, true, true,
                                       aligned != 0, aligned != 0, true});
    return r.status == DcStatus::ok ? (int)r.kind : -(int)r.status;
}

#define MVDETR_DC_ENTRIES(T, SFX, TYPE)                                                                                      \
    int mvdetr_deform_conv2d_forward_##SFX(void *stream, const T *input, const T *offset, const T *weight, const T *bias,   \
                                           MVDETR_DC_SHAPE_PARAMS, int input_nhwc, T *out)                                   \
    {                                                                                                                        \
        return dc_entry(DcEntry::forward, DcCall{(hipStream_t)stream, TYPE, nullptr, input, offset, weight, bias, out, nullptr, nullptr, \
                                                 nullptr, input_nhwc, 0, 0, {}}, MVDETR_DC_SHAPE);                           \
    }                                                                                                                        \
    int mvdetr_deform_conv2d_backward_##SFX(void *stream, const T *grad_out, const T *input, const T *offset, const T *weight,   \
                                            MVDETR_DC_SHAPE_PARAMS, int input_nhwc, T *grad_input, T *grad_offset, T *grad_weight) \
    {                                                                                                                        \
        return dc_entry(DcEntry::backward, DcCall{(hipStream_t)stream, TYPE, grad_out, input, offset, weight, nullptr, nullptr,  \
                                                  grad_input, grad_offset, grad_weight, input_nhwc, 0, 0, {}}, MVDETR_DC_SHAPE); \
    }

MVDETR_DC_ENTRIES(float, f32, DcType::f32)
MVDETR_DC_ENTRIES(double, f64, DcType::f64)

}  // extern "C"

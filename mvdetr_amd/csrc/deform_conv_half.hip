// Deformable convolution (deform_conv.hip's contract) in 16-bit storage (float16 / bfloat16), forward only -- gfx950 (MI355X).
// The house contract of half_types.h: tensors are raw 16-bit words, every arithmetic step is fp32, ONE rounding on the way out.
//
// dc_fwd_mfma_half<Conv, KC> is dc_fwd_mfma on v_mfma_f32_32x32x16_{f16,bf16} with its launch geometry: a workgroup of 256
// lanes owns 64 output pixels x 128 output channels, wave w the channels 32 w .. 32 w + 31 of all 64 pixels as two 32x32 fp32
// accumulators; the K loop runs over (tap, KC = 32 or 16 input channels).  Lane (r = lane & 31, h = lane >> 5):
//   sampling   lane t samples pixel t / 4, channels 8 (t % 4) .. + 7 of the chunk (KC = 16: the lanes with t % 4 < 2) from the
//              channel-last input: one 16-byte load8_or_zero per bilinear corner, blended in fp32.  Positions are formed in fp32
//              from the 16-bit offset; validity is dc_foot's (NaN, +-inf and far-outside offsets sample 0).
//   column     the sampled value is an fp32 number and is NOT rounded to 16 bits once (2^-9 / 2^-12 of every term): it is
//              split as attention_half.hip splits P, hi = rn16(col), lo = rn16(col - hi) (the difference is exact), both images
//              are staged in LDS and take one MFMA each against the same weight operand.  Products of two 16-bit numbers are
//              exact in fp32 and the accumulator is fp32: the result is what fp32 arithmetic gives on the upcast inputs, less
//              2^-18 (bf16) / 2^-22 (fp16) of a column value.
//   fp16 range nothing depends on what the MFMA does with subnormal column operands: a |col| below 2^-14 has hi = 0 (lo then
//              carries the value whole) and lo is scaled by 2^11 into accumulators of its own, folded in as
//              acc + 2^-11 acc_lo before the store (powers of two: exact).  bf16 has fp32's exponent range and needs none of it.
//   weights    the entry takes the weight PERMUTED to [kh * kw][C_out][C_in]: a weight-tile row of a chunk is a contiguous,
//              16-byte aligned run (the fp32 kernel's gather of wt[(o C + c) T + tap] would be 2-byte strided loads).
//   LDS        rows of KC + 8 halves (80 or 48 bytes): every fragment read is one aligned 16-byte read of k = 16 s + 8 h + j,
//              j = 0 .. 7, of the lane's row.  Two buffers: chunk i + 1 is written while other waves may still read chunk i, so
//              the loop has ONE barrier per chunk, and the next chunk's global loads are in flight during the MFMAs.
//   epilogue   + bias (fp32, upcast from 16 bits), optional ReLU, one rounding to nearest even, NCHW 16-bit store with a
//              caller-given batch stride (a channel slice of a larger [B, N C, H, W] tensor is written in place).
// No scratch, no atomics; every output element is owned by one lane: bit-reproducible run to run.
#include "../../include/mvdetr_ops.h"
#include "common.h"
#include "deform_conv.h"
#include "half_mfma.h"

namespace mvdetr {

// eight fp32 column values -> the hi and lo images (fp16: lo carries HALF_LO_SCALE)
template <typename Conv> __device__ __forceinline__ void dch_split(const float (&x)[8], uint4 &hi, uint4 &lo)
{
    uint32_t wh[4], wl[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) split2<Conv, true>(x[2 * j], x[2 * j + 1], wh[j], wl[j]);
    hi = make_uint4(wh[0], wh[1], wh[2], wh[3]);
    lo = make_uint4(wl[0], wl[1], wl[2], wl[3]);
}

// sampling position of output pixel (ho, wo), tap (i, j), one offset group: fp32 from the 16-bit offset
template <typename Conv>
__device__ __forceinline__ void dch_pos(const uint16_t *__restrict__ off, const DcShape &s, int b, int tap, int ho, int wo,
                                        float &y, float &x)
{
    const int T_ = s.kh * s.kw, HWo = s.Ho * s.Wo;
    const int i = tap / s.kw, j = tap - i * s.kw;
    const uint16_t *o = off + ((int64_t)b * 2 * T_ + 2 * tap) * HWo + ho * s.Wo + wo;
    y = (float)(ho * s.sh - s.ph + i * s.dh) + Conv::up(o[0]);
    x = (float)(wo * s.sw - s.pw + j * s.dw) + Conv::up(o[HWo]);
}

template <typename Conv, int KC>
__global__ __launch_bounds__(256) void dc_fwd_mfma_half(const uint16_t *__restrict__ in, const uint16_t *__restrict__ off,
                                                        const uint16_t *__restrict__ wt, const uint16_t *__restrict__ bias,
                                                        uint16_t *__restrict__ out, DcShape s, int relu, int64_t obs)
{
    constexpr bool FP16 = std::is_same<Conv, F16>::value;
    constexpr int LD = KC + 8, KST = KC / 16, C8 = KC / 8, NW = DC_TO * C8 / 256;    // NW weight items (16 bytes) per lane
    __shared__ __attribute__((aligned(16))) uint16_t sW[2][DC_TO][LD];               // weight tile [o][k]
    __shared__ __attribute__((aligned(16))) uint16_t sXh[2][DC_TP][LD];              // column tile, hi image [p][k]
    __shared__ __attribute__((aligned(16))) uint16_t sXl[2][DC_TP][LD];              // lo image
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
    const int T_ = s.kh * s.kw, HWo = s.Ho * s.Wo, nc = s.C / KC, nit = T_ * nc;
    const int64_t P = (int64_t)s.B * HWo, p0 = (int64_t)blockIdx.x * DC_TP;
    const int o0 = blockIdx.y * DC_TO;
    const bool active = o0 + wave * 32 < s.Co;

    // sampler role: pixel sp, channels [8 sq, 8 sq + 8) of each chunk
    const int sp = t >> 2, sq = t & 3;
    const bool samples = sq < C8;
    const int64_t gp = p0 + sp;
    const bool pv = gp < P;
    int b = 0, p = 0, ho = 0, wo = 0;
    if (pv) dc_pixel(s, gp, b, p, ho, wo);
    const uint16_t *inb = in + (int64_t)b * s.H * s.W * s.C;

    floatx16 acc[2], acc2[2];                                // acc2: the fp16 lo term's accumulators (unused for bf16)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[n][e] = acc2[n][e] = 0.f;

    // one (tap, chunk) in registers: four corners of 8 channels, their weights, NW weight-tile items
    uint4 cv[4], wv[NW];
    float cw[4];
    DcFoot<float> f;
    auto fetch = [&](int it) {
        const int tap = it / nc, c0 = (it - tap * nc) * KC;
        if (c0 == 0) {                                       // a new tap: its footprint
            float y = -2.f, x = -2.f;
            if (pv) dch_pos<Conv>(off, s, b, tap, ho, wo, y, x);
            f = dc_foot(y, x, s.H, s.W);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            cv[k] = load8_or_zero(inb + (int64_t)f.pix[k] * s.C + c0 + 8 * sq, f.ok[k] && samples, inb);
            cw[k] = f.w[k];
        }
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            const int e = t + 256 * i, o = e / C8, c8 = e - o * C8;
            wv[i] = load8_or_zero(wt + ((int64_t)tap * s.Co + o0 + o) * s.C + c0 + 8 * c8, o0 + o < s.Co, wt);
        }
    };
    auto put = [&](int buf) {
        if (samples) {
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float u[8];
                up8<Conv>(cv[k], u);
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] += cw[k] * u[e];
            }
            uint4 hi, lo;
            dch_split<Conv>(v, hi, lo);
            *reinterpret_cast<uint4 *>(&sXh[buf][sp][8 * sq]) = hi;
            *reinterpret_cast<uint4 *>(&sXl[buf][sp][8 * sq]) = lo;
        }
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            const int e = t + 256 * i, o = e / C8, c8 = e - o * C8;
            *reinterpret_cast<uint4 *>(&sW[buf][o][8 * c8]) = wv[i];
        }
    };

    fetch(0);
    for (int it = 0; it < nit; ++it) {
        const int buf = it & 1;
        put(buf);
        // (the buffer written here was last read two chunks ago: every wave has passed the barrier of the chunk in between)
        __syncthreads();
        if (it + 1 < nit) fetch(it + 1);
        if (active) {
#pragma unroll
            for (int ks = 0; ks < KST; ++ks) {
                const uint4 a = *reinterpret_cast<const uint4 *>(&sW[buf][wave * 32 + r][16 * ks + 8 * h]);
#pragma unroll
                for (int n = 0; n < 2; ++n) {
                    const uint4 bh = *reinterpret_cast<const uint4 *>(&sXh[buf][n * 32 + r][16 * ks + 8 * h]);
                    const uint4 bl = *reinterpret_cast<const uint4 *>(&sXl[buf][n * 32 + r][16 * ks + 8 * h]);
                    acc[n] = mfma16<Conv>(a, bh, acc[n]);
                    if (FP16)
                        acc2[n] = mfma16<Conv>(a, bl, acc2[n]);
                    else
                        acc[n] = mfma16<Conv>(a, bl, acc[n]);
                }
            }
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
        uint16_t *ob = out + (int64_t)qb * obs + qp;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int o = o0 + wave * 32 + mfma_crow(e, h);
            float v = acc[n][e];
            if (FP16) v += acc2[n][e] * (1.f / HALF_LO_SCALE);
            if (bias) v += Conv::up(bias[o]);
            if (relu) v = fmaxf(v, 0.f);
            ob[(int64_t)o * HWo] = Conv::down(v);
        }
    }
}

template <typename Conv> static void dc_launch_half(const DcCall &c)
{
    const DcRoute &r = c.r;
    hipLaunchKernelGGL((r.KC == 32 ? dc_fwd_mfma_half<Conv, 32> : dc_fwd_mfma_half<Conv, 16>), dim3(r.grid[0].x, r.grid[0].y), dim3(256), 0, c.st,
                       (const uint16_t *)c.in, (const uint16_t *)c.off, (const uint16_t *)c.wt, (const uint16_t *)c.bias, (uint16_t *)c.out,
                       r.s, c.relu, c.obs);
}

int dc_launch_forward_half(const DcCall &c)
{
    if (c.type == DcType::f16) dc_launch_half<F16>(c);
    else dc_launch_half<BF16>(c);
    return (int)hipGetLastError();
}

}  // namespace mvdetr

using namespace mvdetr;

extern "C" {

#define MVDETR_DC_HALF_ENTRY(SFX, TYPE)                                                                                      \
    int mvdetr_deform_conv2d_forward_##SFX(void *stream, const uint16_t *input, const uint16_t *offset, const uint16_t *weight,  \
                                           const uint16_t *bias, MVDETR_DC_SHAPE_PARAMS, int input_nhwc, int relu,           \
                                           int64_t out_batch_stride, uint16_t *out)                                          \
    {                                                                                                                        \
        return dc_entry(DcEntry::forward_half, DcCall{(hipStream_t)stream, TYPE, nullptr, input, offset, weight, bias, out, nullptr, \
                                                      nullptr, nullptr, input_nhwc, relu, out_batch_stride, {}}, MVDETR_DC_SHAPE);   \
    }

MVDETR_DC_HALF_ENTRY(f16, DcType::f16)
MVDETR_DC_HALF_ENTRY(bf16, DcType::bf16)

}  // extern "C"

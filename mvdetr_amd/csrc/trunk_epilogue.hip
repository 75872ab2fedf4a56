// The ResNet trunk's inference epilogues, one pass each -- gfx950 (MI355X).
//
// In eval mode every BatchNorm2d, ReLU, residual add and the stem's max-pool of the trunk is a pass of its own over the
// activation tensor in torch (BN 2T, ReLU 2T, add 3T, pool 1.25T bytes per tensor of T bytes), each already at copy
// speed, so the only way to make them cheaper is to run fewer of them.  Two kernel families, channel-last fp32:
//
//   bn_act           y = act( x*s[c] + t[c]  [+ r]  [+ r*s2[c] + t2[c]] ),  s = gamma / sqrt(var + eps), t = beta - mean*s
//                    (the block's bn1+relu: 2T; bn2 + identity + relu or bn2 + downsample-BN + relu: 3T).  y may be x.
//   bn_relu_maxpool  the stem: MaxPool2d(3, 2, 1) over relu(bn(x)); reads the convolution output once, writes a quarter.
//
// s and t are formed in the kernel from the BatchNorm's four vectors on every call (nothing cached, nothing to go stale).
// A lane keeps ONE group of four channels for the whole grid-stride loop (the block is laid out [rows, C/4] over the
// tensor), so the constants are computed once per lane; 16 bytes per lane and access.  NaN propagates as in torch:
// relu(NaN) = NaN, and a NaN in a pooling window gives NaN (neither is written with fmaxf, which drops NaN).
// Both families also exist over float16 / bfloat16 storage (eight channels per lane, fp32 arithmetic, one rounding): below.
#include <atomic>

#include "bn_epilogue.h"
#include "common.h"
#include "half_types.h"
#include "../../include/mvdetr_ops.h"

namespace mvdetr {

static std::atomic<const char *> g_trunk_last_kernel{"none"};
static std::atomic<int64_t> g_trunk_launches{0};

// BnVectors, bn_fold4 (s and t of four consecutive channels), relu_nan and the finishing step: bn_epilogue.h, shared with
// the Winograd convolution's fused store
__device__ __forceinline__ float max_nan(float a, float b) { return (b > a || b != b) ? b : a; }   // torch's pooling update

__device__ __forceinline__ float4 fma4(float4 x, float4 s, float4 t)
{
    return make_float4(bn_apply(x.x, s.x, t.x), bn_apply(x.y, s.y, t.y), bn_apply(x.z, s.z, t.z), bn_apply(x.w, s.w, t.w));
}

// MODE 0: no residual; 1: + r; 2: + (r*s2 + t2).  x, r, y: [rows, C] (channel-last).  The block is TX lanes wide over the
// channel groups (TX = min(C/4, 256); blockIdx.y picks the 256-group chunk when C > 1024) and 256/TX rows deep; two rows
// per lane and iteration are in flight.  y may alias x (a lane reads its elements before it writes them); r must not.
template <int MODE, bool RELU>
__global__ __launch_bounds__(256) void bn_act_cl(const float *x, BnVectors bn, const float *__restrict__ r, BnVectors bn2,
                                                 int64_t rows, int C, int tx, float *y)
{
    const int col = blockIdx.y * 256 + (int)threadIdx.x % tx;
    const int rpb = 256 / tx;                                                   // rows per block and step
    const int64_t step = (int64_t)gridDim.x * rpb;
    int64_t row = (int64_t)blockIdx.x * rpb + (int)threadIdx.x / tx;
    float4 s, t, s2, t2;
    bn_fold4(bn, col * 4, s, t);
    if (MODE == 2) {
        bn_fold4(bn2, col * 4, s2, t2);
        t = make_float4(t.x + t2.x, t.y + t2.y, t.z + t2.z, t.w + t2.w);
    }
    auto finish = [&](float4 z, float4 q) {
        return make_float4(bn_finish<MODE, RELU>(z.x, q.x, s2.x), bn_finish<MODE, RELU>(z.y, q.y, s2.y),
                           bn_finish<MODE, RELU>(z.z, q.z, s2.z), bn_finish<MODE, RELU>(z.w, q.w, s2.w));
    };
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    for (; row + step < rows; row += 2 * step) {
        const int64_t o0 = row * C + col * 4, o1 = (row + step) * C + col * 4;
        const float4 a0 = *reinterpret_cast<const float4 *>(x + o0);
        const float4 a1 = *reinterpret_cast<const float4 *>(x + o1);
        const float4 q0 = MODE ? *reinterpret_cast<const float4 *>(r + o0) : zero;
        const float4 q1 = MODE ? *reinterpret_cast<const float4 *>(r + o1) : zero;
        *reinterpret_cast<float4 *>(y + o0) = finish(fma4(a0, s, t), q0);
        *reinterpret_cast<float4 *>(y + o1) = finish(fma4(a1, s, t), q1);
    }
    if (row < rows) {
        const int64_t o0 = row * C + col * 4;
        const float4 a0 = *reinterpret_cast<const float4 *>(x + o0);
        const float4 q0 = MODE ? *reinterpret_cast<const float4 *>(r + o0) : zero;
        *reinterpret_cast<float4 *>(y + o0) = finish(fma4(a0, s, t), q0);
    }
}

// Any C % 4 == 0 that the layout above does not tile (C/4 neither divides 256 nor is a multiple of it): flat over the
// float4 groups, constants formed per element (they sit in L1/L2).
template <int MODE, bool RELU>
__global__ __launch_bounds__(256) void bn_act_cl_any(const float *x, BnVectors bn, const float *__restrict__ r, BnVectors bn2,
                                                     int64_t groups, int C, float *y)
{
    const int cg = C >> 2;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < groups; i += (int64_t)gridDim.x * 256) {
        const int col = (int)(i % cg);
        float4 s, t, s2;
        bn_fold4(bn, col * 4, s, t);
        if (MODE == 2) {                                                        // t + t2 first, as in bn_act_cl: one arithmetic
            float4 t2;
            bn_fold4(bn2, col * 4, s2, t2);
            t = make_float4(t.x + t2.x, t.y + t2.y, t.z + t2.z, t.w + t2.w);
        }
        float4 z = fma4(*reinterpret_cast<const float4 *>(x + i * 4), s, t);
        if (MODE) {
            const float4 q = *reinterpret_cast<const float4 *>(r + i * 4);
            if (MODE == 1) z = make_float4(z.x + q.x, z.y + q.y, z.z + q.z, z.w + q.w);
            if (MODE == 2) z = fma4(q, s2, z);
        }
        if (RELU) z = make_float4(relu_nan(z.x), relu_nan(z.y), relu_nan(z.z), relu_nan(z.w));
        *reinterpret_cast<float4 *>(y + i * 4) = z;
    }
}

// y[n, oh, ow, c] = max over the 3x3 window at stride 2, padding 1 of relu(x*s + t); x [N, H, W, C], y [N, OH, OW, C].
// A lane owns four channels and walks output pixels; taps outside the image are skipped (padding is -inf in torch and every
// window holds at least one pixel).  The nine taps of neighbouring outputs overlap 2.25x: L2 serves the repeats.
// I: the type the output-pixel index is split in (int below 2^31 pixels: 64-bit divisions are long software sequences).
template <typename I>
__global__ __launch_bounds__(256) void bn_relu_maxpool_cl(const float *__restrict__ x, BnVectors bn, int N, int H, int W, int C,
                                                          int OH, int OW, int tx, float *__restrict__ y)
{
    const int col = blockIdx.y * 256 + (int)threadIdx.x % tx;
    const int ppb = 256 / tx;                                                   // output pixels per block and step
    const I pixels = (I)N * OH * OW;
    float4 s, t;
    bn_fold4(bn, col * 4, s, t);
    for (I p = (I)blockIdx.x * ppb + (int)threadIdx.x / tx; p < pixels; p += (I)gridDim.x * ppb) {
        const int ow = (int)(p % OW);
        const I q = p / OW;
        const int oh = (int)(q % OH);
        const int64_t n = q / OH;
        const float ninf = -__builtin_huge_valf();
        float4 m = make_float4(ninf, ninf, ninf, ninf);
#pragma unroll
        for (int kh = 0; kh < 3; ++kh) {
            const int ih = 2 * oh - 1 + kh;
            if (ih < 0 || ih >= H) continue;
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const int iw = 2 * ow - 1 + kw;
                if (iw < 0 || iw >= W) continue;
                const float4 z = fma4(*reinterpret_cast<const float4 *>(x + ((n * H + ih) * W + iw) * C + col * 4), s, t);
                m = make_float4(max_nan(m.x, relu_nan(z.x)), max_nan(m.y, relu_nan(z.y)), max_nan(m.z, relu_nan(z.z)),
                                max_nan(m.w, relu_nan(z.w)));
            }
        }
        *reinterpret_cast<float4 *>(y + (int64_t)p * C + col * 4) = m;
    }
}

// ---- the same two families over 16-bit storage (half_types.h: raw words in, fp32 arithmetic, one rounding out) ----------
// A lane owns EIGHT channels -- still one 16-byte access -- so the block is [rows, C/8] and a lane's constants are 16 fp32
// registers (24 with the downsample BatchNorm).  The BatchNorm vectors stay fp32.  The sum bn(x) + identity is formed in
// fp32 and rounded once at the store (torch's 16-bit chain rounds after every op), and the pool takes its max on the fp32
// values: rounding to nearest is monotone, so that equals the pool of the rounded bn_act output bit for bit.

// The folded constants are needed HERE: without this the compiler sinks a fold's divisions and square roots down to the
// loop that uses them while its loads stay put, so that all 32 (64 with the downsample BatchNorm) loaded values are live
// at once and the kernel spills.  (An empty statement the values pass through; loads do not move across it.)
__device__ __forceinline__ void pin4(float4 &a, float4 &b)
{
    asm volatile("" : "+v"(a.x), "+v"(a.y), "+v"(a.z), "+v"(a.w), "+v"(b.x), "+v"(b.y), "+v"(b.z), "+v"(b.w) : : "memory");
}

// scale and shift of eight consecutive channels
__device__ __forceinline__ void bn_fold8(const BnVectors &bn, int c, float (&s)[8], float (&t)[8])
{
    float4 s0, t0, s1, t1;
    bn_fold4(bn, c, s0, t0);
    pin4(s0, t0);
    bn_fold4(bn, c + 4, s1, t1);
    pin4(s1, t1);
    s[0] = s0.x, s[1] = s0.y, s[2] = s0.z, s[3] = s0.w, s[4] = s1.x, s[5] = s1.y, s[6] = s1.z, s[7] = s1.w;
    t[0] = t0.x, t[1] = t0.y, t[2] = t0.z, t[3] = t0.w, t[4] = t1.x, t[5] = t1.y, t[6] = t1.z, t[7] = t1.w;
}

// act( x*s + t [+ q | + q*s2] ) of two raw values in one word (t already holds t + t2 in MODE 2), rounded once
template <typename CV, int MODE, bool RELU>
__device__ __forceinline__ uint32_t bn_finish2(uint32_t a, uint32_t q, const float *s, const float *t, const float *s2)
{
    float z0, z1, f0 = 0.f, f1 = 0.f;
    up2<CV>(a, z0, z1);
    if (MODE) up2<CV>(q, f0, f1);
    z0 = z0 * s[0] + t[0];
    z1 = z1 * s[1] + t[1];
    if (MODE == 1) z0 += f0, z1 += f1;
    if (MODE == 2) z0 = f0 * s2[0] + z0, z1 = f1 * s2[1] + z1;
    if (RELU) z0 = relu_nan(z0), z1 = relu_nan(z1);
    return down2<CV>(z0, z1);
}

// ... of eight: word by word, so that only the raw words and one pair of fp32 values are live beside the constants
template <typename CV, int MODE, bool RELU>
__device__ __forceinline__ uint4 bn_finish8(const uint4 &a, const uint4 &q, const float (&s)[8], const float (&t)[8],
                                            const float (&s2)[8])
{
    return make_uint4(bn_finish2<CV, MODE, RELU>(a.x, q.x, s, t, s2), bn_finish2<CV, MODE, RELU>(a.y, q.y, s + 2, t + 2, s2 + 2),
                      bn_finish2<CV, MODE, RELU>(a.z, q.z, s + 4, t + 4, s2 + 4), bn_finish2<CV, MODE, RELU>(a.w, q.w, s + 6, t + 6, s2 + 6));
}

// bn_act_cl over 16-bit x, r, y: TX = min(C/8, 256) lanes across, blockIdx.y picks the 256-group chunk when C > 2048.
template <typename CV, int MODE, bool RELU>
__global__ __launch_bounds__(256, 8) void bn_act_cl_half(const uint16_t *x, BnVectors bn, const uint16_t *__restrict__ r,
                                                      BnVectors bn2, int64_t rows, int C, int tx, uint16_t *y)
{
    const int col = blockIdx.y * 256 + (int)threadIdx.x % tx;
    const int rpb = 256 / tx;
    const int64_t step = (int64_t)gridDim.x * rpb;
    int64_t row = (int64_t)blockIdx.x * rpb + (int)threadIdx.x / tx;
    float s[8], t[8], s2[8];
    bn_fold8(bn, col * 8, s, t);
    if (MODE == 2) {
        float t2[8];
        bn_fold8(bn2, col * 8, s2, t2);
#pragma unroll
        for (int i = 0; i < 8; ++i) t[i] += t2[i];
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) s2[i] = 0.f;                              // (never read)
    }
    // two rows in flight; the odd last row travels as a second copy of itself that is not stored (one loop body, no tail
    // copy of it: a tail keeps the constants alive in a second arrangement and pushes the kernel past 64 registers)
    const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
    for (; row < rows; row += 2 * step) {
        const bool two = row + step < rows;
        const int64_t o0 = row * C + col * 8, o1 = (two ? row + step : row) * C + col * 8;
        const uint4 a0 = *reinterpret_cast<const uint4 *>(x + o0);
        const uint4 a1 = *reinterpret_cast<const uint4 *>(x + o1);
        const uint4 q0 = MODE ? *reinterpret_cast<const uint4 *>(r + o0) : zero;
        const uint4 q1 = MODE ? *reinterpret_cast<const uint4 *>(r + o1) : zero;
        *reinterpret_cast<uint4 *>(y + o0) = bn_finish8<CV, MODE, RELU>(a0, q0, s, t, s2);
        if (two) *reinterpret_cast<uint4 *>(y + o1) = bn_finish8<CV, MODE, RELU>(a1, q1, s, t, s2);
    }
}

// Any C % 8 == 0 that the layout above does not tile: flat over the groups of eight, constants formed per element.
template <typename CV, int MODE, bool RELU>
__global__ __launch_bounds__(256, 8) void bn_act_cl_any_half(const uint16_t *x, BnVectors bn, const uint16_t *__restrict__ r,
                                                          BnVectors bn2, int64_t groups, int C, uint16_t *y)
{
    const int cg = C >> 3;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < groups; i += (int64_t)gridDim.x * 256) {
        const int col = (int)(i % cg);
        const uint4 a = *reinterpret_cast<const uint4 *>(x + i * 8);
        const uint4 q = MODE ? *reinterpret_cast<const uint4 *>(r + i * 8) : make_uint4(0u, 0u, 0u, 0u);
        uint32_t out[4];
#pragma unroll
        for (int h = 0; h < 2; ++h) {                                          // four channels at a time: their constants only
            float4 s, t, s2 = make_float4(0.f, 0.f, 0.f, 0.f), t2;
            bn_fold4(bn, col * 8 + h * 4, s, t);
            pin4(s, t);
            if (MODE == 2) {
                bn_fold4(bn2, col * 8 + h * 4, s2, t2);
                pin4(s2, t2);
                t = make_float4(t.x + t2.x, t.y + t2.y, t.z + t2.z, t.w + t2.w);
            }
            const float sv[4] = {s.x, s.y, s.z, s.w}, tv[4] = {t.x, t.y, t.z, t.w}, s2v[4] = {s2.x, s2.y, s2.z, s2.w};
            out[2 * h] = bn_finish2<CV, MODE, RELU>(h ? a.z : a.x, h ? q.z : q.x, sv, tv, s2v);
            out[2 * h + 1] = bn_finish2<CV, MODE, RELU>(h ? a.w : a.y, h ? q.w : q.y, sv + 2, tv + 2, s2v + 2);
        }
        *reinterpret_cast<uint4 *>(y + i * 8) = make_uint4(out[0], out[1], out[2], out[3]);
    }
}

// bn_relu_maxpool_cl over 16-bit x, y, eight channels per lane; the max runs on the fp32 values and is rounded at the end.
template <typename CV, typename I>
__global__ __launch_bounds__(256, 8) void bn_relu_maxpool_cl_half(const uint16_t *__restrict__ x, BnVectors bn, int N, int H, int W,
                                                               int C, int OH, int OW, int tx, uint16_t *__restrict__ y)
{
    const int col = blockIdx.y * 256 + (int)threadIdx.x % tx;
    const int ppb = 256 / tx;
    const I pixels = (I)N * OH * OW;
    float s[8], t[8];
    bn_fold8(bn, col * 8, s, t);
    for (I p = (I)blockIdx.x * ppb + (int)threadIdx.x / tx; p < pixels; p += (I)gridDim.x * ppb) {
        const int ow = (int)(p % OW);
        const I q = p / OW;
        const int oh = (int)(q % OH);
        const int64_t n = q / OH;
        float m[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) m[i] = -__builtin_huge_valf();
#pragma unroll
        for (int kh = 0; kh < 3; ++kh) {
            const int ih = 2 * oh - 1 + kh;
            if (ih < 0 || ih >= H) continue;
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const int iw = 2 * ow - 1 + kw;
                if (iw < 0 || iw >= W) continue;
                float z[8];
                up8<CV>(*reinterpret_cast<const uint4 *>(x + ((n * H + ih) * W + iw) * C + col * 8), z);
#pragma unroll
                for (int i = 0; i < 8; ++i) m[i] = max_nan(m[i], relu_nan(z[i] * s[i] + t[i]));
            }
        }
        *reinterpret_cast<uint4 *>(y + (int64_t)p * C + col * 8) = down8<CV>(m);
    }
}

static bool bn_ok(const BnVectors &b)
{
    return b.mean && b.var && aligned(b.mean, 16) && aligned(b.var, 16) && (!b.gamma || aligned(b.gamma, 16)) &&
           (!b.beta || aligned(b.beta, 16));
}

// lanes across the channel groups of `vec` channels, or 0 when the tiled layout does not fit C
static int lanes_across(int C, int vec)
{
    const int cg = C / vec;
    if (cg <= 256) return 256 % cg == 0 ? cg : 0;
    return cg % 256 == 0 ? 256 : 0;
}

static unsigned grid_for(int64_t items, int per_block)
{
    const int64_t want = (items + per_block - 1) / per_block;
    return (unsigned)(want < 2048 ? (want > 0 ? want : 1) : 2048);             // 8 blocks per CU, grid-stride above
}

// A storage family: its element type, the channels a lane owns, and its kernels.  The entry points below are written once.
struct Fp32Family {
    using T = float;
    static constexpr int VEC = 4;
    static constexpr bool HALF = false;
    template <int MODE, bool RELU> static auto tiled() { return bn_act_cl<MODE, RELU>; }
    template <int MODE, bool RELU> static auto any() { return bn_act_cl_any<MODE, RELU>; }
    template <typename I> static auto pool() { return bn_relu_maxpool_cl<I>; }
};

template <typename CV>
struct HalfFamily {
    using T = uint16_t;
    static constexpr int VEC = 8;
    static constexpr bool HALF = true;
    template <int MODE, bool RELU> static auto tiled() { return bn_act_cl_half<CV, MODE, RELU>; }
    template <int MODE, bool RELU> static auto any() { return bn_act_cl_any_half<CV, MODE, RELU>; }
    template <typename I> static auto pool() { return bn_relu_maxpool_cl_half<CV, I>; }
};

template <typename F, int MODE, bool RELU>
static void launch_bn_act(hipStream_t st, const typename F::T *x, const BnVectors &bn, const typename F::T *r, const BnVectors &bn2,
                          int64_t rows, int C, typename F::T *y)
{
    const int tx = lanes_across(C, F::VEC);
    if (tx) {
        const int rpb = 256 / tx;
        const dim3 grid(grid_for((rows + 1) / 2, rpb), (unsigned)((C / F::VEC + 255) / 256));
        hipLaunchKernelGGL((F::template tiled<MODE, RELU>()), grid, dim3(256), 0, st, x, bn, r, bn2, rows, C, tx, y);
    } else {
        const int64_t groups = rows * (C / F::VEC);
        hipLaunchKernelGGL((F::template any<MODE, RELU>()), dim3(grid_for(groups, 256)), dim3(256), 0, st, x, bn, r, bn2, groups, C, y);
    }
}

// [half][mode][relu]
static const char *const kBnActNames[2][3][2] = {
    {{"bn", "bn_relu"}, {"bn_add", "bn_add_relu"}, {"bn_bn_add", "bn_bn_add_relu"}},
    {{"bn_half", "bn_relu_half"}, {"bn_add_half", "bn_add_relu_half"}, {"bn_bn_add_half", "bn_bn_add_relu_half"}}};

template <typename F>
static int bn_act_entry(void *stream, const typename F::T *x, const BnVectors &bn, const typename F::T *res, const BnVectors &bn2,
                        int64_t rows, int channels, int relu, typename F::T *y)
{
    if (rows < 0 || channels <= 0 || channels % F::VEC != 0) return (int)hipErrorInvalidValue;
    if (rows == 0) return 0;
    const bool res_bn = bn2.mean || bn2.var || bn2.gamma || bn2.beta;
    if (!x || !y || !aligned(x, 16) || !aligned(y, 16) || !bn_ok(bn)) return (int)hipErrorInvalidValue;
    if (res && (!aligned(res, 16) || res == y)) return (int)hipErrorInvalidValue;            // the residual is never overwritten
    if (res_bn && (!res || !bn_ok(bn2))) return (int)hipErrorInvalidValue;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int mode = !res ? 0 : res_bn ? 2 : 1;
    if (mode == 0) {
        if (relu) launch_bn_act<F, 0, true>(st, x, bn, res, bn2, rows, channels, y);
        else launch_bn_act<F, 0, false>(st, x, bn, res, bn2, rows, channels, y);
    } else if (mode == 1) {
        if (relu) launch_bn_act<F, 1, true>(st, x, bn, res, bn2, rows, channels, y);
        else launch_bn_act<F, 1, false>(st, x, bn, res, bn2, rows, channels, y);
    } else {
        if (relu) launch_bn_act<F, 2, true>(st, x, bn, res, bn2, rows, channels, y);
        else launch_bn_act<F, 2, false>(st, x, bn, res, bn2, rows, channels, y);
    }
    g_trunk_last_kernel = kBnActNames[F::HALF][mode][relu ? 1 : 0];
    g_trunk_launches.fetch_add(1);
    return (int)hipGetLastError();
}

template <typename F>
static int bn_relu_maxpool_entry(void *stream, const typename F::T *x, const BnVectors &bn, int n, int h, int w, int channels,
                                 typename F::T *y)
{
    if (n < 0 || h <= 0 || w <= 0 || channels <= 0 || channels % F::VEC != 0) return (int)hipErrorInvalidValue;
    if (n == 0) return 0;
    if (!x || !y || x == y || !aligned(x, 16) || !aligned(y, 16) || !bn_ok(bn)) return (int)hipErrorInvalidValue;
    const int tx = lanes_across(channels, F::VEC);
    if (!tx) return (int)hipErrorNotSupported;
    const int OH = (h - 1) / 2 + 1, OW = (w - 1) / 2 + 1;
    const dim3 grid(grid_for((int64_t)n * OH * OW, 256 / tx), (unsigned)((channels / F::VEC + 255) / 256));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if ((int64_t)n * OH * OW < (int64_t)1 << 30)                               // (p + a grid stride stays below 2^31)
        hipLaunchKernelGGL((F::template pool<int>()), grid, dim3(256), 0, st, x, bn, n, h, w, channels, OH, OW, tx, y);
    else
        hipLaunchKernelGGL((F::template pool<int64_t>()), grid, dim3(256), 0, st, x, bn, n, h, w, channels, OH, OW, tx, y);
    g_trunk_last_kernel = F::HALF ? "bn_relu_maxpool_half" : "bn_relu_maxpool";
    g_trunk_launches.fetch_add(1);
    return (int)hipGetLastError();
}

}  // namespace mvdetr

#define MVDETR_BN_ACT_ENTRY(NAME, T, FAMILY)                                                                                   \
    extern "C" int NAME(void *stream, const T *x, const float *mean, const float *var, const float *gamma, const float *beta, \
                        float eps, const T *res, const float *res_mean, const float *res_var, const float *res_gamma,         \
                        const float *res_beta, float res_eps, int64_t rows, int channels, int relu, T *y)                     \
    {                                                                                                                          \
        return mvdetr::bn_act_entry<FAMILY>(stream, x, mvdetr::BnVectors{mean, var, gamma, beta, eps}, res,                    \
                                            mvdetr::BnVectors{res_mean, res_var, res_gamma, res_beta, res_eps}, rows, channels, \
                                            relu, y);                                                                          \
    }
#define MVDETR_BN_RELU_MAXPOOL_ENTRY(NAME, T, FAMILY)                                                                          \
    extern "C" int NAME(void *stream, const T *x, const float *mean, const float *var, const float *gamma, const float *beta, \
                        float eps, int n, int h, int w, int channels, T *y)                                                    \
    {                                                                                                                          \
        return mvdetr::bn_relu_maxpool_entry<FAMILY>(stream, x, mvdetr::BnVectors{mean, var, gamma, beta, eps}, n, h, w,      \
                                                     channels, y);                                                             \
    }

MVDETR_BN_ACT_ENTRY(mvdetr_bn_act_f32, float, mvdetr::Fp32Family)
MVDETR_BN_ACT_ENTRY(mvdetr_bn_act_f16, uint16_t, mvdetr::HalfFamily<mvdetr::F16>)
MVDETR_BN_ACT_ENTRY(mvdetr_bn_act_bf16, uint16_t, mvdetr::HalfFamily<mvdetr::BF16>)
MVDETR_BN_RELU_MAXPOOL_ENTRY(mvdetr_bn_relu_maxpool_f32, float, mvdetr::Fp32Family)
MVDETR_BN_RELU_MAXPOOL_ENTRY(mvdetr_bn_relu_maxpool_f16, uint16_t, mvdetr::HalfFamily<mvdetr::F16>)
MVDETR_BN_RELU_MAXPOOL_ENTRY(mvdetr_bn_relu_maxpool_bf16, uint16_t, mvdetr::HalfFamily<mvdetr::BF16>)

extern "C" const char *mvdetr_trunk_last_kernel(void) { return mvdetr::g_trunk_last_kernel.load(); }

extern "C" int64_t mvdetr_trunk_launch_count(void) { return mvdetr::g_trunk_launches.load(); }

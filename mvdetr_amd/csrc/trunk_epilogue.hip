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
#include <atomic>

#include "common.h"
#include "../../include/mvdetr_ops.h"

namespace mvdetr {

static std::atomic<const char *> g_trunk_last_kernel{"none"};
static std::atomic<int64_t> g_trunk_launches{0};

struct BnVectors {
    const float *mean, *var, *gamma, *beta;                   // [C]; gamma / beta may be null (1 / 0)
    float eps;
};

// scale and shift of four consecutive channels
__device__ __forceinline__ void bn_fold4(const BnVectors &bn, int c, float4 &s, float4 &t)
{
    const float4 m = *reinterpret_cast<const float4 *>(bn.mean + c);
    const float4 v = *reinterpret_cast<const float4 *>(bn.var + c);
    const float4 g = bn.gamma ? *reinterpret_cast<const float4 *>(bn.gamma + c) : make_float4(1.f, 1.f, 1.f, 1.f);
    const float4 b = bn.beta ? *reinterpret_cast<const float4 *>(bn.beta + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    s = make_float4(g.x / sqrtf(v.x + bn.eps), g.y / sqrtf(v.y + bn.eps), g.z / sqrtf(v.z + bn.eps), g.w / sqrtf(v.w + bn.eps));
    t = make_float4(b.x - m.x * s.x, b.y - m.y * s.y, b.z - m.z * s.z, b.w - m.w * s.w);
}

__device__ __forceinline__ float relu_nan(float z) { return z < 0.f ? 0.f : z; }              // NaN stays NaN
__device__ __forceinline__ float max_nan(float a, float b) { return (b > a || b != b) ? b : a; }   // torch's pooling update

__device__ __forceinline__ float4 fma4(float4 x, float4 s, float4 t)
{
    return make_float4(x.x * s.x + t.x, x.y * s.y + t.y, x.z * s.z + t.z, x.w * s.w + t.w);
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
        if (MODE == 1) z = make_float4(z.x + q.x, z.y + q.y, z.z + q.z, z.w + q.w);
        if (MODE == 2) z = fma4(q, s2, z);
        if (RELU) z = make_float4(relu_nan(z.x), relu_nan(z.y), relu_nan(z.z), relu_nan(z.w));
        return z;
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
        float4 s, t;
        bn_fold4(bn, col * 4, s, t);
        float4 z = fma4(*reinterpret_cast<const float4 *>(x + i * 4), s, t);
        if (MODE) {
            const float4 q = *reinterpret_cast<const float4 *>(r + i * 4);
            if (MODE == 1) z = make_float4(z.x + q.x, z.y + q.y, z.z + q.z, z.w + q.w);
            if (MODE == 2) {
                float4 s2, t2;
                bn_fold4(bn2, col * 4, s2, t2);
                z = fma4(q, s2, make_float4(z.x + t2.x, z.y + t2.y, z.z + t2.z, z.w + t2.w));
            }
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

static bool bn_ok(const BnVectors &b)
{
    return b.mean && b.var && aligned(b.mean, 16) && aligned(b.var, 16) && (!b.gamma || aligned(b.gamma, 16)) &&
           (!b.beta || aligned(b.beta, 16));
}

// lanes across the channel groups, or 0 when the tiled layout does not fit C
static int lanes_across(int C)
{
    const int cg = C / 4;
    if (cg <= 256) return 256 % cg == 0 ? cg : 0;
    return cg % 256 == 0 ? 256 : 0;
}

static unsigned grid_for(int64_t items, int per_block)
{
    const int64_t want = (items + per_block - 1) / per_block;
    return (unsigned)(want < 2048 ? (want > 0 ? want : 1) : 2048);             // 8 blocks per CU, grid-stride above
}

template <int MODE, bool RELU>
static void launch_bn_act(hipStream_t st, const float *x, const BnVectors &bn, const float *r, const BnVectors &bn2, int64_t rows,
                          int C, float *y)
{
    const int tx = lanes_across(C);
    if (tx) {
        const int rpb = 256 / tx;
        const dim3 grid(grid_for((rows + 1) / 2, rpb), (unsigned)((C / 4 + 255) / 256));
        hipLaunchKernelGGL((bn_act_cl<MODE, RELU>), grid, dim3(256), 0, st, x, bn, r, bn2, rows, C, tx, y);
    } else {
        const int64_t groups = rows * (C / 4);
        hipLaunchKernelGGL((bn_act_cl_any<MODE, RELU>), dim3(grid_for(groups, 256)), dim3(256), 0, st, x, bn, r, bn2, groups, C, y);
    }
}

}  // namespace mvdetr

extern "C" int mvdetr_bn_act_f32(void *stream, const float *x, const float *mean, const float *var, const float *gamma,
                                 const float *beta, float eps, const float *res, const float *res_mean, const float *res_var,
                                 const float *res_gamma, const float *res_beta, float res_eps, int64_t rows, int channels,
                                 int relu, float *y)
{
    using namespace mvdetr;
    if (rows < 0 || channels <= 0 || channels % 4 != 0) return (int)hipErrorInvalidValue;
    if (rows == 0) return 0;
    const BnVectors bn{mean, var, gamma, beta, eps};
    const BnVectors bn2{res_mean, res_var, res_gamma, res_beta, res_eps};
    const bool res_bn = res_mean || res_var || res_gamma || res_beta;
    if (!x || !y || !aligned(x, 16) || !aligned(y, 16) || !bn_ok(bn)) return (int)hipErrorInvalidValue;
    if (res && (!aligned(res, 16) || res == y)) return (int)hipErrorInvalidValue;            // the residual is never overwritten
    if (res_bn && (!res || !bn_ok(bn2))) return (int)hipErrorInvalidValue;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int mode = !res ? 0 : res_bn ? 2 : 1;
    const char *name;
    if (mode == 0) {
        if (relu) launch_bn_act<0, true>(st, x, bn, res, bn2, rows, channels, y);
        else launch_bn_act<0, false>(st, x, bn, res, bn2, rows, channels, y);
        name = relu ? "bn_relu" : "bn";
    } else if (mode == 1) {
        if (relu) launch_bn_act<1, true>(st, x, bn, res, bn2, rows, channels, y);
        else launch_bn_act<1, false>(st, x, bn, res, bn2, rows, channels, y);
        name = relu ? "bn_add_relu" : "bn_add";
    } else {
        if (relu) launch_bn_act<2, true>(st, x, bn, res, bn2, rows, channels, y);
        else launch_bn_act<2, false>(st, x, bn, res, bn2, rows, channels, y);
        name = relu ? "bn_bn_add_relu" : "bn_bn_add";
    }
    g_trunk_last_kernel = name;
    g_trunk_launches.fetch_add(1);
    return (int)hipGetLastError();
}

extern "C" int mvdetr_bn_relu_maxpool_f32(void *stream, const float *x, const float *mean, const float *var, const float *gamma,
                                          const float *beta, float eps, int n, int h, int w, int channels, float *y)
{
    using namespace mvdetr;
    if (n < 0 || h <= 0 || w <= 0 || channels <= 0 || channels % 4 != 0) return (int)hipErrorInvalidValue;
    if (n == 0) return 0;
    const BnVectors bn{mean, var, gamma, beta, eps};
    if (!x || !y || x == y || !aligned(x, 16) || !aligned(y, 16) || !bn_ok(bn)) return (int)hipErrorInvalidValue;
    const int tx = lanes_across(channels);
    if (!tx) return (int)hipErrorNotSupported;
    const int OH = (h - 1) / 2 + 1, OW = (w - 1) / 2 + 1;
    const dim3 grid(grid_for((int64_t)n * OH * OW, 256 / tx), (unsigned)((channels / 4 + 255) / 256));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if ((int64_t)n * OH * OW < (int64_t)1 << 30)                               // (p + a grid stride stays below 2^31)
        hipLaunchKernelGGL(bn_relu_maxpool_cl<int>, grid, dim3(256), 0, st, x, bn, n, h, w, channels, OH, OW, tx, y);
    else
        hipLaunchKernelGGL(bn_relu_maxpool_cl<int64_t>, grid, dim3(256), 0, st, x, bn, n, h, w, channels, OH, OW, tx, y);
    g_trunk_last_kernel = "bn_relu_maxpool";
    g_trunk_launches.fetch_add(1);
    return (int)hipGetLastError();
}

extern "C" const char *mvdetr_trunk_last_kernel(void) { return mvdetr::g_trunk_last_kernel.load(); }

extern "C" int64_t mvdetr_trunk_launch_count(void) { return mvdetr::g_trunk_launches.load(); }

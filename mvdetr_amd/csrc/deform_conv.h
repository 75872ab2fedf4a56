// What the deformable-convolution kernels of deform_conv.hip (fp32 / fp64) and deform_conv_half.hip (float16 / bfloat16)
// share: the bilinear footprint of one tap, the pixel decomposition, and one call as the C ABI entries of deform_conv.hip fill
// it.  What a call may ask for is checked by dc_route() (deform_conv_route.h: the shape and the tile constants too), once,
// before a launcher runs; a launcher picks the instantiation and launches.
#pragma once
#include "common.h"
#include "deform_conv_route.h"

namespace mvdetr {

enum class DcType { f16, bf16, f32, f64 };

struct DcCall {
    hipStream_t st;
    DcType type;
    const void *gout, *in, *off, *wt, *bias;        // gout: the backward's grad_out
    void *out, *gin, *goff, *gw;
    int nhwc, relu;
    int64_t obs;                                    // the 16-bit entry's out_batch_stride
    DcRoute r;                                      // r.s: the shape
};

// the one entry path (deform_conv.hip) and the C ABI's shape arguments as it takes them
#define MVDETR_DC_SHAPE_PARAMS                                                                                                   \
    int batch, int in_channels, int in_h, int in_w, int out_channels, int kernel_h, int kernel_w, int stride_h, int stride_w, int pad_h, \
        int pad_w, int dil_h, int dil_w, int offset_groups
#define MVDETR_DC_SHAPE {batch, in_channels, in_h, in_w, out_channels, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w, offset_groups}
int dc_entry(DcEntry entry, DcCall c, const int (&sh)[14]);
// dc_fwd_mfma_half (deform_conv_half.hip)
int dc_launch_forward_half(const DcCall &c);

// bilinear footprint of one tap: corner pixel indices (y * W + x), weights, validity; `in` = the sample is not 0
template <typename T> struct DcFoot {
    int pix[4];          // (y0,x0) (y0,x1) (y1,x0) (y1,x1)
    T w[4];
    bool ok[4];
    bool in;
    T ly, lx;
};

template <typename T> __device__ __forceinline__ DcFoot<T> dc_foot(T y, T x, int H, int W)
{
    DcFoot<T> f;
    f.in = y > T(-1) && y < T(H) && x > T(-1) && x < T(W);          // (NaN offsets sample 0)
    const T fy = f.in ? ffloor(y) : T(0), fx = f.in ? ffloor(x) : T(0);
    const int y0 = (int)fy, x0 = (int)fx;
    f.ly = f.in ? y - fy : T(0);
    f.lx = f.in ? x - fx : T(0);
    const T hy = T(1) - f.ly, hx = T(1) - f.lx;
    f.ok[0] = f.in && y0 >= 0 && x0 >= 0;
    f.ok[1] = f.in && y0 >= 0 && x0 + 1 < W;
    f.ok[2] = f.in && y0 + 1 < H && x0 >= 0;
    f.ok[3] = f.in && y0 + 1 < H && x0 + 1 < W;
    f.pix[0] = f.ok[0] ? y0 * W + x0 : 0;
    f.pix[1] = f.ok[1] ? y0 * W + x0 + 1 : 0;
    f.pix[2] = f.ok[2] ? (y0 + 1) * W + x0 : 0;
    f.pix[3] = f.ok[3] ? (y0 + 1) * W + x0 + 1 : 0;
    f.w[0] = hy * hx;
    f.w[1] = hy * f.lx;
    f.w[2] = f.ly * hx;
    f.w[3] = f.ly * f.lx;
    return f;
}

__device__ __forceinline__ void dc_pixel(const DcShape &s, int64_t gp, int &b, int &p, int &ho, int &wo)
{
    const int HWo = s.Ho * s.Wo;
    b = (int)(gp / HWo);
    p = (int)(gp - (int64_t)b * HWo);
    ho = p / s.Wo;
    wo = p - ho * s.Wo;
}

}  // namespace mvdetr

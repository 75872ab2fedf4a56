// What the deformable-convolution kernels of deform_conv.hip (fp32 / fp64) and deform_conv_half.hip (float16 / bfloat16)
// share: the call's shape, the bilinear footprint of one tap, the pixel decomposition and the MFMA tile geometry.
#pragma once
#include "common.h"

#include <atomic>

namespace mvdetr {

extern std::atomic<const char *> g_dc_last_kernel;         // deform_conv.hip

struct DcShape {
    int B, C, H, W, Co, Ho, Wo, kh, kw, sh, sw, ph, pw, dh, dw, G;
};

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

constexpr int DC_TP = 64;       // output pixels per forward / g_col workgroup
constexpr int DC_TO = 128;      // output (forward) or input (g_col) channels per workgroup: 4 waves x 32 rows

__device__ __forceinline__ void dc_pixel(const DcShape &s, int64_t gp, int &b, int &p, int &ho, int &wo)
{
    const int HWo = s.Ho * s.Wo;
    b = (int)(gp / HWo);
    p = (int)(gp - (int64_t)b * HWo);
    ho = p / s.Wo;
    wo = p - ho * s.Wo;
}

inline bool dc_shape(int B, int C, int H, int W, int Co, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int G,
                     DcShape &s)
{
    if (B < 0 || C < 0 || H < 1 || W < 1 || Co < 0 || kh < 1 || kw < 1 || sh < 1 || sw < 1 || ph < 0 || pw < 0 || dh < 1 ||
        dw < 1 || G < 1 || C % G != 0)
        return false;
    const int Ho = (H + 2 * ph - dh * (kh - 1) - 1) / sh + 1, Wo = (W + 2 * pw - dw * (kw - 1) - 1) / sw + 1;
    if (H + 2 * ph - dh * (kh - 1) - 1 < 0 || W + 2 * pw - dw * (kw - 1) - 1 < 0) return false;
    if ((int64_t)B * C * H * W >= (1ll << 31) || (int64_t)B * Co * Ho * Wo >= (1ll << 31) ||
        (int64_t)B * 2 * G * kh * kw * Ho * Wo >= (1ll << 31))
        return false;
    s = DcShape{B, C, H, W, Co, Ho, Wo, kh, kw, sh, sw, ph, pw, dh, dw, G};
    return true;
}

}  // namespace mvdetr

// What the perspective-warp kernels of warp_forward.hip and warp_backward.hip share on the device: the source position of a
// destination pixel under kornia's convention, its bilinear footprint, and the block id -> tile mapping.
#pragma once
#include "common.h"
#include "warp_route.h"

namespace mvdetr {

struct SrcCoord {
    int y0, x0;
    double wy0, wy1, wx0, wx1;   // blend weights (rounded to the tensor dtype by the caller)
    bool v00, v01, v10, v11;
    bool any;
};

// Source sampling position of destination pixel (i, j) under kornia's convention.
template <typename T>
__device__ __forceinline__ void source_position(const T *__restrict__ Mn, int i, int j, int h, int w,
                                                double &x, double &y)
{
    // true inverse of the dst<-src homography, in fp64
    const double m0 = Mn[0], m1 = Mn[1], m2 = Mn[2], m3 = Mn[3], m4 = Mn[4], m5 = Mn[5], m6 = Mn[6],
                 m7 = Mn[7], m8 = Mn[8];
    const double c0 = m4 * m8 - m5 * m7, c1 = m5 * m6 - m3 * m8, c2 = m3 * m7 - m4 * m6;
    const double r = 1.0 / (m0 * c0 + m1 * c1 + m2 * c2);
    const double dj = (double)j, di = (double)i;
    // p = M^-1 (j, i, 1): source pixel, homogeneous
    const double px = (c0 * dj + (m2 * m7 - m1 * m8) * di + (m1 * m5 - m2 * m4)) * r;
    const double py = (c1 * dj + (m0 * m8 - m2 * m6) * di + (m2 * m3 - m0 * m5)) * r;
    const double pz = (c2 * dj + (m1 * m6 - m0 * m7) * di + (m0 * m4 - m1 * m3)) * r;
    // kornia normalises source pixels with the corner-aligned map 2p/(size-1) - 1 ...
    const double wd = w == 1 ? 1e-14 : (double)(w - 1), hd = h == 1 ? 1e-14 : (double)(h - 1);
    const double qx = 2.0 * px / wd - pz, qy = 2.0 * py / hd - pz;
    // ... divides only where |z| > 1e-8 (convert_points_from_homogeneous) ...
    const double s = fabs(pz) > 1e-8 ? 1.0 / pz : 1.0;
    // ... and hands the result to an align_corners=False sampler: ((g + 1) * size - 1) / 2
    x = ((qx * s + 1.0) * (double)w - 1.0) * 0.5;
    y = ((qy * s + 1.0) * (double)h - 1.0) * 0.5;
}

// nearest: grid_sample(mode='nearest') rounds the position half-to-even and takes that texel; here it becomes a
// bilinear footprint whose first corner carries all the weight (the call kornia.warp_perspective(..., 'nearest') of
// frameDataset.py:80)
__device__ __forceinline__ SrcCoord make_coord(double x, double y, int h, int w, int nearest)
{
    SrcCoord c;
    if (nearest) {
        x = rint(x);
        y = rint(y);
    }
    // reject far-out / non-finite positions before the int conversion
    const bool in = x > -1.0 && y > -1.0 && x < (double)w && y < (double)h;
    const double fx = floor(x), fy = floor(y);
    c.x0 = in ? (int)fx : 0;
    c.y0 = in ? (int)fy : 0;
    c.wx1 = x - fx;
    c.wy1 = y - fy;
    c.wx0 = 1.0 - c.wx1;
    c.wy0 = 1.0 - c.wy1;
    const bool vx0 = c.x0 >= 0, vx1 = c.x0 + 1 < w, vy0 = c.y0 >= 0, vy1 = c.y0 + 1 < h;
    c.v00 = in && vy0 && vx0;
    c.v01 = in && vy0 && vx1 && !nearest;
    c.v10 = in && vy1 && vx0 && !nearest;
    c.v11 = in && vy1 && vx1 && !nearest;
    c.any = c.v00 || c.v01 || c.v10 || c.v11;
    return c;
}

// Two x-adjacent source texels with one 8-byte load when both are inside the row (global loads only
// need dword alignment on gfx950), else two guarded scalar loads.
template <typename T>
__device__ __forceinline__ void load_pair(const T *p, bool v0, bool v1, T &a, T &b)
{
    if constexpr (sizeof(T) == 4) {
        if (v0 && v1) {
            float2 t;
            __builtin_memcpy(&t, p, 8);
            a = t.x;
            b = t.y;
            return;
        }
    }
    a = v0 ? p[0] : T(0);
    b = v1 ? p[1] : T(0);
}

// a destination pixel's bilinear footprint in the source view: what the channel-last kernels and (round 5) warp_fwd share
// per tile through LDS
// (T is the type the blend is COMPUTED in and the matrices come in: the tensor's own type for fp32 / fp64 tensors, float for
// the 16-bit kernels, whose storage type is a converter of half_types.h and never appears here)
template <typename T> struct WarpTexel {
    int o00;                     // element offset of corner (y0, x0) inside the view, in texels (not scaled by C)
    T w00, w01, w10, w11;
    int valid;                   // bit 0..3: corners 00, 01, 10, 11 inside the source
};

template <typename T>
__device__ __forceinline__ WarpTexel<T> warp_texel(const T *__restrict__ Mn, int i, int j, int h, int w, bool live, int nearest)
{
    WarpTexel<T> t;
    t.o00 = 0;
    t.valid = 0;
    t.w00 = t.w01 = t.w10 = t.w11 = T(0);
    if (live) {
        double x, y;
        source_position(Mn, i, j, h, w, x, y);
        const SrcCoord sc = make_coord(x, y, h, w, nearest);
        t.o00 = sc.y0 * w + sc.x0;
        t.w00 = T(sc.wy0 * sc.wx0);
        t.w01 = T(sc.wy0 * sc.wx1);
        t.w10 = T(sc.wy1 * sc.wx0);
        t.w11 = T(sc.wy1 * sc.wx1);
        t.valid = (sc.v00 ? 1 : 0) | (sc.v01 ? 2 : 0) | (sc.v10 ? 4 : 0) | (sc.v11 ? 8 : 0);
    }
    return t;
}

struct WarpBlock {
    int n, i0, j0, group;
};

__device__ __forceinline__ bool warp_block(int N, int H, int W, int groups, WarpBlock &wb)
{
    const int tx = (W + WARP_TW - 1) / WARP_TW, ty = (H + WARP_TH - 1) / WARP_TH;
    int r = blockIdx.x;
    wb.group = r % groups;
    r /= groups;
    wb.j0 = (r % tx) * WARP_TW;
    r /= tx;
    wb.i0 = (r % ty) * WARP_TH;
    wb.n = r / ty;
    return wb.n < N;
}

// The blend of both 16-bit kernels in ONE order of fused multiply-adds (under -ffp-contract=fast the compiler picks an order
// per kernel): the result of a call does not depend on which of the two its layout and alignment select.
__device__ __forceinline__ float warp_blend_half(float w00, float a, float w01, float b, float w10, float c, float w11, float d)
{
    return fmaf(w11, d, fmaf(w10, c, fmaf(w01, b, w00 * a)));
}

}  // namespace mvdetr

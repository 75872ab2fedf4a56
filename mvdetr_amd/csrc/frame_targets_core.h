// The per-object arithmetic of the training targets (mvdetr_frame_targets_*), shared by the device kernel (frame_targets.hip)
// and the host path (host_path.cpp) so that both run the SAME operations in the SAME order: include/mvdetr_ops.h has the
// contract, DESIGN 4.14 the reasons.  Everything is fp64 until the stated roundings and must be compiled WITHOUT FMA contraction
// (frame_targets.hip switches it off for itself, the Makefile builds host_path.cpp with -ffp-contract=off).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MVDETR_FT_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define MVDETR_FT_HD inline
#endif

#define MVDETR_FT_MAX_CAP 1024        /* objects per map */
#define MVDETR_FT_MAX_RADIUS 15       /* the gaussian patch is at most 31 x 31 */
#define MVDETR_FT_MAX_DIM 16384       /* rows / columns of a map */

// (np.minimum / np.maximum on finite numbers; NaN is outside the contract)
MVDETR_FT_HD double ft_min(double a, double b) { return b < a ? b : a; }
MVDETR_FT_HD double ft_max(double a, double b) { return b > a ? b : a; }

// One box (x1, y1, x2, y2) through the first two rows of M (row-major 3x3), as augment.affine_boxes moves it: the hull of the
// four mapped corners, shrunk about its centre by `shrink`, clipped to [0, lim_x] x [0, lim_y].  Returns whether the box is kept.
MVDETR_FT_HD bool ft_move_box(const double *box, const double *M, double shrink, double lim_x, double lim_y, double *moved)
{
    const double x1 = box[0], y1 = box[1], x2 = box[2], y2 = box[3];
    const double px[4] = {x1, x2, x1, x2}, py[4] = {y1, y2, y2, y1};
    double lo_x = 0, hi_x = 0, lo_y = 0, hi_y = 0;
    for (int k = 0; k < 4; ++k) {
        const double X = (M[0] * px[k] + M[1] * py[k]) + M[2];
        const double Y = (M[3] * px[k] + M[4] * py[k]) + M[5];
        lo_x = k ? ft_min(lo_x, X) : X;
        hi_x = k ? ft_max(hi_x, X) : X;
        lo_y = k ? ft_min(lo_y, Y) : Y;
        hi_y = k ? ft_max(hi_y, Y) : Y;
    }
    const double cx = (hi_x + lo_x) / 2, sx = (hi_x - lo_x) * shrink;
    const double cy = (hi_y + lo_y) / 2, sy = (hi_y - lo_y) * shrink;
    const double nx1 = ft_min(ft_max(cx - sx / 2, 0.0), lim_x), nx2 = ft_min(ft_max(cx + sx / 2, 0.0), lim_x);
    const double ny1 = ft_min(ft_max(cy - sy / 2, 0.0), lim_y), ny2 = ft_min(ft_max(cy + sy / 2, 0.0), lim_y);
    moved[0] = nx1, moved[1] = ny1, moved[2] = nx2, moved[3] = ny2;
    const double w = nx2 - nx1, h = ny2 - ny1, area = (x2 - x1) * (y2 - y1), tiny = 1e-16;
    const bool big_enough = w > 4 && h > 4;
    const bool mostly_there = w * h / (area + tiny) > 0.1;
    const bool not_a_sliver = ft_max(w / (h + tiny), h / (w + tiny)) < 10;
    return big_enough && mostly_there && not_a_sliver;
}

// What one object at (x, y) with size (w, h), all at `reduce` times the map's resolution, puts into its slot.
struct FtSlot {
    int inside;              // the fp32 centre lies in [0, W) x [0, H); the other fields mean something only then
    int cx, cy;              // the truncated centre
    float off_x, off_y;      // centre - truncated centre, fp32
    float wh_x, wh_y;        // (w, h) / reduce
};

MVDETR_FT_HD FtSlot ft_slot(double x, double y, double w, double h, double reduce, int H, int W)
{
    FtSlot s;
    const float fx = (float)(x / reduce), fy = (float)(y / reduce);          // fp64 division, then ONE rounding
    s.inside = fx >= 0.f && fy >= 0.f && fx < (float)W && fy < (float)H;
    s.cx = s.cy = 0;
    s.off_x = s.off_y = s.wh_x = s.wh_y = 0.f;
    if (s.inside) {
        s.cx = (int)fx;
        s.cy = (int)fy;
        s.off_x = fx - (float)s.cx;
        s.off_y = fy - (float)s.cy;
        s.wh_x = (float)(w / reduce);
        s.wh_y = (float)(h / reduce);
    }
    return s;
}

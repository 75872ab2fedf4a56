// The perspective warp's backward: the two scatter kernels, the gather with its geometry pass (the "plan"), the per-stream
// scratch that holds a call's plan, and the launchers.  Which one a call runs: warp_route.h.
#include "warp_device.h"
#include "warp_launch.h"
#include "../../include/mvdetr_ops.h"
#include <map>
#include <mutex>
#include <utility>
#include <cstring>

namespace mvdetr {

template <typename T, bool NHWC>
__global__ __launch_bounds__(WARP_PIX *WARP_SUB) void warp_bwd(
    const T *__restrict__ grad_dst, const T *__restrict__ Mv, int N, int C, int h, int w, int H, int W,
    int nearest, T *__restrict__ grad_src)
{
    const int lane = threadIdx.x & (WARP_PIX - 1);
    const int sub = threadIdx.x / WARP_PIX;
    WarpBlock wb;
    if (!warp_block(N, H, W, (C + WARP_CH - 1) / WARP_CH, wb)) return;
    const int n = wb.n, i = wb.i0 + lane / WARP_TW, j = wb.j0 + lane % WARP_TW;
    if (i >= H || j >= W) return;
    const int64_t pix = ((int64_t)n * H + i) * W + j;
    const int cbase = wb.group * WARP_CH;
    constexpr int CPT = WARP_CH / WARP_SUB;
    double x, y;
    source_position(Mv + (int64_t)n * 9, i, j, h, w, x, y);
    const SrcCoord sc = make_coord(x, y, h, w, nearest);
    if (!sc.any) return;
    const T w00 = T(sc.wy0 * sc.wx0), w01 = T(sc.wy0 * sc.wx1);
    const T w10 = T(sc.wy1 * sc.wx0), w11 = T(sc.wy1 * sc.wx1);
    const int64_t plane = (int64_t)h * w;
    const int64_t o00 = (int64_t)sc.y0 * w + sc.x0;
    for (int k = 0; k < CPT; ++k) {
        const int c = cbase + sub * CPT + k;
        if (c >= C) break;
        const T g = NHWC ? grad_dst[pix * C + c] : grad_dst[(((int64_t)n * C + c) * H + i) * W + j];
        T *gp = grad_src + ((int64_t)n * C + c) * plane + o00;
        if (sc.v00) atomicAdd(gp, w00 * g);
        if (sc.v01) atomicAdd(gp + 1, w01 * g);
        if (sc.v10) atomicAdd(gp + w, w10 * g);
        if (sc.v11) atomicAdd(gp + w + 1, w11 * g);
    }
}

template <typename T>
__global__ __launch_bounds__(WARP_CL_THREADS) void warp_bwd_cl(
    const T *__restrict__ grad_dst, const T *__restrict__ Mv, int N, int C, int h, int w, int H, int W,
    int nearest, T *__restrict__ grad_src)
{
    __shared__ WarpTexel<T> tex[WARP_PIX];
    WarpBlock wb;
    if (!warp_block(N, H, W, 1, wb)) return;
    const int n = wb.n;
    if (threadIdx.x < WARP_PIX) {
        const int i = wb.i0 + threadIdx.x / WARP_TW, j = wb.j0 + threadIdx.x % WARP_TW;
        tex[threadIdx.x] = warp_texel(Mv + (int64_t)n * 9, i, j, h, w, i < H && j < W, nearest);
    }
    __syncthreads();
    T *view = grad_src + (int64_t)n * h * w * C;
    const int rowC = w * C;
    // One CHANNEL per lane (not a 16-byte chunk as in the forward): the memory-side atomic units take a wave's
    // atomic instruction as one request per contiguous segment, so 64 consecutive channels of a corner are 4
    // requests, where 16-byte chunks per lane made every instruction 4-byte pieces 16 bytes apart -- 4x the
    // requests (measured 1.46 ms -> see DESIGN.md).
    for (int item = threadIdx.x; item < WARP_PIX * C; item += WARP_CL_THREADS) {
        const int p = item / C, c = item - p * C;
        const int i = wb.i0 + p / WARP_TW, j = wb.j0 + p % WARP_TW;
        if (i >= H || j >= W) continue;
        const WarpTexel<T> t = tex[p];
        if (!t.valid) continue;
        const T g = grad_dst[(((int64_t)n * H + i) * W + j) * C + c];
        T *gp = view + (int64_t)t.o00 * C + c;
        if (t.valid & 1) atomicAdd(gp, t.w00 * g);
        if (t.valid & 2) atomicAdd(gp + C, t.w01 * g);
        if (t.valid & 4) atomicAdd(gp + rowC, t.w10 * g);
        if (t.valid & 8) atomicAdd(gp + rowC + C, t.w11 * g);
    }
}

// ---- backward as a GATHER (channel-last on both sides; no atomics, deterministic) ------------------------------------
// grid_sample's backward scatters: every destination pixel adds w_k * grad to the four source texels of its bilinear
// footprint (warp_bwd / warp_bwd_cl above: one memory-side atomic request per contiguous segment, 382 us at Wildtrack
// size, 6.8 % of the roofline).  The homography is invertible, so the sum can be turned around: the destination pixels
// whose footprint touches a 2 x 2 BLOCK of source texels are those whose source position lies in
// [2bx-1, 2bx+2) x [2by-1, 2by+2), and that set is the image of this square under M (dst <- src) -- a convex
// quadrilateral of a few dozen pixels (a few hundred for the far field, where the ground plane is magnified).
//   * warp_bwd_gather: a group of G = C/4 lanes (32 at 128 channels; two groups per wave) owns one block.
//     1. Candidate scan: when the square does not cross the line that maps to infinity (the horizon: same sign of the
//        homogeneous coordinate at all four corners) its image is the hull of the four projected corners.  Far-field
//        images are long diagonal slivers whose bounding box is ~10x their area, so the scan is a SHEARED box: lines
//        (rows or columns, whichever is cheaper) u0..u1, and on line u the `len` pixels from ceil(a + s (u - uc)) on,
//        with the shear s taken from one of the hull's edges (the cheapest of five candidates).  Squares that do cross
//        the horizon get plain boxes from clipping the destination rectangle (Sutherland-Hodgman, one lane, LDS)
//        against the five linear inequalities "source position inside the square", once per sign of the homogeneous
//        coordinate.  Scans are only candidate sets: membership is decided by the exact test below.
//     2. The G lanes test G candidates at a time with the forward's own source_position / make_coord (forward and
//        backward use the same weights bit for bit), compact the hits in scan order into LDS (ballot + popcount: the
//        order of every sum is fixed -> deterministic results), then every lane walks the hits, loads its 16-byte
//        channel chunk of grad_dst (the group reads whole 512-byte pixel rows) and accumulates into the block's four
//        texels in registers.
//     grad_src is written once, with plain stores: it need not be zeroed, and each grad_dst row is read ~2.25 times
//     (once per block its footprint touches), mostly from L2.  One difference from a scatter: a hit adds 0 * g to the
//     block texels its footprint misses, so a NON-FINITE upstream gradient spreads to the other texels of the 2 x 2 block.
//   * Pixels kornia does not divide: convert_points_from_homogeneous divides by z only where |z| > 1e-8, so a destination
//     pixel with |z| <= 1e-8 samples a position unrelated to the projective map and no scan finds it.  warp_bwd_scans
//     lists such pixels (normally none) in pixel order; the gather tests the listed ones as extra candidates of every
//     block and leaves them out of its scans, so they are counted exactly once and in a fixed order as well.
template <typename T> struct WarpRec {
    int pix;                     // destination pixel index (n * H + i) * W + j
    int mask;                    // bit t: the footprint touches block texel t = 2 * (Y - 2by) + (X - 2bx)
    T w[4];                      // its weight there (the forward's T(wy * wx))
};

// homogeneous coordinate of destination pixel (i, j) under M^-1 (the pz of source_position): the forward divides by it
// only where |pz| > 1e-8
template <typename T> __device__ __forceinline__ double source_pz(const T *__restrict__ Mn, int i, int j)
{
    const double m0 = Mn[0], m1 = Mn[1], m2 = Mn[2], m3 = Mn[3], m4 = Mn[4], m5 = Mn[5], m6 = Mn[6],
                 m7 = Mn[7], m8 = Mn[8];
    const double c0 = m4 * m8 - m5 * m7, c1 = m5 * m6 - m3 * m8, c2 = m3 * m7 - m4 * m6;
    const double r = 1.0 / (m0 * c0 + m1 * c1 + m2 * c2);
    return (c2 * (double)j + (m1 * m6 - m0 * m7) * (double)i + (m0 * m4 - m1 * m3)) * r;
}

constexpr int WARP_CLIP_MAXV = 12;      // rectangle (4) + one new vertex per clip (5), rounded up
constexpr int WARP_CLIP_SLOTS = 4 * WARP_CLIP_MAXV + 15;        // polygon double buffer + the 5 x 3 coefficients

// bounding box of {(j, i) in [-1, W] x [-1, H] : e[k] . (j, i, 1) >= 0 for all k}; false when empty.  `lds` is this lane's
// scratch, slot-major over the workgroup's lanes (slot s of lane l at lds[s * WARP_SCAN_THREADS]: conflict-free);
// slots 0..4*MAXV-1 hold the polygon double buffer, the 15 coefficients follow.
__device__ inline bool warp_clip_box(double *lds, int H, int W, int &i0, int &i1, int &j0, int &j1)
{
#define SLOT(k) lds[(k) * WARP_SCAN_THREADS]
    constexpr int PX = 0, PY = WARP_CLIP_MAXV, QX = 2 * WARP_CLIP_MAXV, QY = 3 * WARP_CLIP_MAXV, E = 4 * WARP_CLIP_MAXV;
    int n = 4;
    SLOT(PX + 0) = -1.0; SLOT(PY + 0) = -1.0;
    SLOT(PX + 1) = (double)W; SLOT(PY + 1) = -1.0;
    SLOT(PX + 2) = (double)W; SLOT(PY + 2) = (double)H;
    SLOT(PX + 3) = -1.0; SLOT(PY + 3) = (double)H;
#pragma unroll 1
    for (int k = 0; k < 5; ++k) {
        int m = 0;
        const double e0 = SLOT(E + 3 * k), e1 = SLOT(E + 3 * k + 1), e2 = SLOT(E + 3 * k + 2);
#pragma unroll 1
        for (int v = 0; v < n; ++v) {
            const int u = v + 1 == n ? 0 : v + 1;
            const double ax = SLOT(PX + v), ay = SLOT(PY + v), bx = SLOT(PX + u), by = SLOT(PY + u);
            const double da = e0 * ax + e1 * ay + e2, db = e0 * bx + e1 * by + e2;
            const bool ia = da >= 0.0, ib = db >= 0.0;
            if (ia && m < WARP_CLIP_MAXV) { SLOT(QX + m) = ax; SLOT(QY + m) = ay; ++m; }
            if (ia != ib && m < WARP_CLIP_MAXV) {
                const double t = da / (da - db);
                SLOT(QX + m) = ax + t * (bx - ax);
                SLOT(QY + m) = ay + t * (by - ay);
                ++m;
            }
        }
        n = m;
        if (n == 0) return false;
#pragma unroll 1
        for (int v = 0; v < n; ++v) { SLOT(PX + v) = SLOT(QX + v); SLOT(PY + v) = SLOT(QY + v); }
    }
    double xa = SLOT(PX), xb = xa, ya = SLOT(PY), yb = ya;
#pragma unroll 1
    for (int v = 1; v < n; ++v) {
        xa = fmin(xa, SLOT(PX + v)); xb = fmax(xb, SLOT(PX + v));
        ya = fmin(ya, SLOT(PY + v)); yb = fmax(yb, SLOT(PY + v));
    }
    j0 = max(0, (int)floor(xa) - 1); j1 = min(W - 1, (int)ceil(xb) + 1);
    i0 = max(0, (int)floor(ya) - 1); i1 = min(H - 1, (int)ceil(yb) + 1);
    return j0 <= j1 && i0 <= i1;
}

__device__ __forceinline__ WarpScan warp_scan_none()
{
    WarpScan z;
    z.u0 = 0; z.u1 = -1; z.len = 0; z.swap = 0; z.a = 0.0; z.s = 0.0; z.uc = 0.0;
    return z;
}

__device__ __forceinline__ WarpScan warp_scan_box(int i0, int i1, int j0, int j1)
{
    WarpScan z;
    z.u0 = i0; z.u1 = i1; z.len = j1 - j0 + 1; z.swap = 0; z.a = (double)j0; z.s = 0.0; z.uc = 0.0;
    return z;
}

// warp_bwd_scans: one lane per 2 x 2 block of source texels -> its (up to two) candidate scans of the destination pixels
// whose source position can lie in [2bx-1, 2bx+2) x [2by-1, 2by+2).  force_clip: take the clipping path for every block
// (a test knob: MVDETR_WARP_BWD_GEOMETRY=clip).  Blocks with more than heavy_above candidates are listed apart.
template <typename T>
__global__ __launch_bounds__(WARP_SCAN_THREADS) void warp_bwd_scans(const T *__restrict__ Mv, int N, int h, int w, int H,
                                                                    int W, int force_clip, int heavy_above,
                                                                    WarpScan *__restrict__ scans, int *__restrict__ heavy_list,
                                                                    int *__restrict__ counts, int *__restrict__ odd_list)
{
    __shared__ double clip[WARP_CLIP_SLOTS * WARP_SCAN_THREADS];
    const int bw2 = (w + 1) / 2, bh2 = (h + 1) / 2;
    const int64_t nblk = (int64_t)N * bh2 * bw2;
    const int scan_wgs = (int)((nblk + WARP_SCAN_THREADS - 1) / WARP_SCAN_THREADS);
    if ((int)blockIdx.x >= scan_wgs) {
        // The last WARP_ODD_SEGS workgroups: kornia divides by z only where |z| > 1e-8 (convert_points_from_homogeneous), so
        // a destination pixel with |z| <= 1e-8 samples a position unrelated to the projective map and no scan finds it.
        // Each of these workgroups (one wave) walks a contiguous range of destination pixels IN ORDER and lists the ones
        // it finds (normally none) in its own segment: the gather then tests them as extra candidates, in a fixed order.
        const int seg = (int)blockIdx.x - scan_wgs;
        const int64_t npix = (int64_t)N * H * W, per = (npix + WARP_ODD_SEGS - 1) / WARP_ODD_SEGS;
        const int64_t p0 = seg * per, p1 = min(npix, p0 + per);
        const int lane = threadIdx.x;
        int found = 0;
        for (int64_t base = p0; base < p1; base += WARP_SCAN_THREADS) {
            const int64_t p = base + lane;
            bool odd = false;
            if (p < p1) {
                const int n = (int)(p / ((int64_t)H * W)), rem = (int)(p - (int64_t)n * H * W);
                const int i = rem / W, j = rem - i * W;
                // cheap screen first: z = zu / det with zu linear in (j, i); far from zero (a factor 4 of slack for the
                // rounding of the exact expression) -> not odd, no division
                const T *Mn = Mv + (int64_t)n * 9;
                const double m0 = Mn[0], m1 = Mn[1], m2 = Mn[2], m3 = Mn[3], m4 = Mn[4], m5 = Mn[5], m6 = Mn[6], m7 = Mn[7],
                             m8 = Mn[8];
                const double det = m0 * (m4 * m8 - m5 * m7) + m1 * (m5 * m6 - m3 * m8) + m2 * (m3 * m7 - m4 * m6);
                const double zu = (m3 * m7 - m4 * m6) * (double)j + (m1 * m6 - m0 * m7) * (double)i + (m0 * m4 - m1 * m3);
                if (!(fabs(zu) > 4e-8 * fabs(det)))
                    odd = fabs(source_pz(Mn, i, j)) <= 1e-8;                                // (NaN: neither scanned nor listed)
            }
            const uint64_t m = __ballot(odd);
            if (odd) odd_list[p0 + found + __popcll(m & ((1ull << lane) - 1ull))] = (int)p;
            found += __popcll(m);
        }
        if (lane == 0) {
            counts[2 + seg] = found;
            if (found) atomicAdd(counts + 1, found);
        }
        return;
    }
    const int64_t idx = (int64_t)blockIdx.x * WARP_SCAN_THREADS + threadIdx.x;
    if (idx >= nblk) return;
    const int n = (int)(idx / ((int64_t)bh2 * bw2)), rem = (int)(idx - (int64_t)n * bh2 * bw2);
    const int by = rem / bw2, bx = rem - by * bw2;
    const double xl = 2.0 * bx - 1.0, xh = 2.0 * bx + 2.0, yl = 2.0 * by - 1.0, yh = 2.0 * by + 2.0;
    const T *Mn = Mv + (int64_t)n * 9;
    double *const lds = clip + threadIdx.x;
    WarpScan b0, b1;
    [&] {
    const double m0 = Mn[0], m1 = Mn[1], m2 = Mn[2], m3 = Mn[3], m4 = Mn[4], m5 = Mn[5], m6 = Mn[6],
                 m7 = Mn[7], m8 = Mn[8];
    b0 = warp_scan_none();
    b1 = warp_scan_none();
    // kornia's chain: position = p * size / (size - 1) - 0.5 for the source pixel p = M^-1 (j, i, 1)
    const double wd = w == 1 ? 1e-14 : (double)(w - 1), hd = h == 1 ? 1e-14 : (double)(h - 1);
    const double ax = (double)w / wd, ay = (double)h / hd;
    const double det = m0 * (m4 * m8 - m5 * m7) + m1 * (m5 * m6 - m3 * m8) + m2 * (m3 * m7 - m4 * m6);
    const double rdet = 1.0 / det;
    // singular or non-finite matrix: the forward's positions are all inf / NaN -> zeros everywhere, no gradient
    if (!(fabs(rdet) <= 1.79e308) || !(fabs(det) <= 1.79e308)) return;
    bool fast = !force_clip;
    double X[4], Y[4];
    int pos = 0, neg = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double sx = (k & 1) ? xh : xl, sy = (k & 2) ? yh : yl;
        const double qx = (sx + 0.5) / ax, qy = (sy + 0.5) / ay;                    // source pixel
        const double dx = m0 * qx + m1 * qy + m2, dy = m3 * qx + m4 * qy + m5, dz = m6 * qx + m7 * qy + m8;
        pos += dz > 0.0;
        neg += dz < 0.0;
        X[k] = dx / dz;
        Y[k] = dy / dz;
        if (!(fabs(X[k]) <= 1e300) || !(fabs(Y[k]) <= 1e300)) fast = false;
    }
    if (fast && (pos == 4 || neg == 4)) {
        // the square is on one side of the horizon: its image is the convex hull of the four corner images.  Five
        // ways to scan it: rows or columns sheared along the image of the square's x or y side, or plain rows.
        constexpr double MARGIN = 0.01;                      // pixels; fp64 rounding of the hull is ~1e-12
        double best = 1e300;
#pragma unroll 1
        for (int opt = 0; opt < 5; ++opt) {
            const int swap = opt >> 1 & (opt < 4);           // options 2, 3: lines are columns
            const int edge = opt & 1;                        // sheared along corner 0 -> 1 (x side) or 0 -> 2 (y side)
            const double Xe = edge ? X[2] : X[1], Ye = edge ? Y[2] : Y[1];
            const double du = swap ? Xe - X[0] : Ye - Y[0], dv = swap ? Ye - Y[0] : Xe - X[0];
            double sh = 0.0;
            if (opt < 4) {
                if (!(fabs(du) > 1e-3 * fabs(dv)) || !(fabs(du) > 1e-9)) continue;   // (nearly) along the lines: no shear
                sh = dv / du;
            }
            const double uc = swap ? X[0] : Y[0];
            double ua = 0, ub = 0, va = 0, vb = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double u = swap ? X[k] : Y[k], v = (swap ? Y[k] : X[k]) - sh * (u - uc);
                ua = k ? fmin(ua, u) : u; ub = k ? fmax(ub, u) : u;
                va = k ? fmin(va, v) : v; vb = k ? fmax(vb, v) : v;
            }
            const double U = swap ? (double)W : (double)H;
            const double u0 = fmax(ceil(ua - MARGIN), 0.0), u1 = fmin(floor(ub + MARGIN), U - 1.0);
            WarpScan z = warp_scan_none();
            double cost = 0.0;
            if (u0 <= u1) {
                const double len = floor(vb - va + 2.0 * MARGIN) + 2.0;
                cost = (u1 - u0 + 1.0) * len;
                // (a square just below the horizon has a far-end image 1e5 .. 1e7 pixels long: the lines are clamped to the
                // grid but their length is not, so such a scan walks millions of candidates outside the grid.  The clipping
                // path below never costs more than H * W candidates: anything dearer than that is left to it.)
                if (!(cost <= (double)H * (double)W)) continue;
                z.u0 = (int)u0; z.u1 = (int)u1; z.len = (int)len; z.swap = swap; z.a = va - MARGIN; z.s = sh; z.uc = uc;
            }
            if (cost < best) { best = cost; b0 = z; }
        }
        if (best < 1e300) return;
    }
    {
        // rows of adj(M) acting on (j, i, 1) (a positive or negative multiple of M^-1: both signs are clipped)
        const double A0[3] = {m4 * m8 - m5 * m7, m2 * m7 - m1 * m8, m1 * m5 - m2 * m4};
        const double A1[3] = {m5 * m6 - m3 * m8, m0 * m8 - m2 * m6, m2 * m3 - m0 * m5};
        const double A2[3] = {m3 * m7 - m4 * m6, m1 * m6 - m0 * m7, m0 * m4 - m1 * m3};
        double big = 0.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) big = fmax(big, fmax(fabs(A0[c]), fmax(fabs(A1[c]), fabs(A2[c]))));
        int4 c0 = make_int4(0, -1, 0, -1), c1 = c0;
        if (!(big > 0.0 && big <= 1e300)) {
            c0 = make_int4(0, H - 1, 0, W - 1);                                      // cannot reason: scan everything
        } else {
            const double sc = 1.0 / big;
#pragma unroll 1
            for (int sgn = 0; sgn < 2; ++sgn) {
                const double sg = sgn ? -sc : sc;
                constexpr int E = 4 * WARP_CLIP_MAXV;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const double gx = ax * A0[c] - 0.5 * A2[c], gy = ay * A1[c] - 0.5 * A2[c], gz = A2[c];
                    lds[(E + 0 + c) * WARP_SCAN_THREADS] = sg * gz;
                    lds[(E + 3 + c) * WARP_SCAN_THREADS] = sg * (gx - xl * gz);
                    lds[(E + 6 + c) * WARP_SCAN_THREADS] = sg * (xh * gz - gx);
                    lds[(E + 9 + c) * WARP_SCAN_THREADS] = sg * (gy - yl * gz);
                    lds[(E + 12 + c) * WARP_SCAN_THREADS] = sg * (yh * gz - gy);
                }
                // (most squares that cross the horizon map outside the destination: one inequality fails at all four
                // corners of the rectangle -> nothing to clip)
                bool empty = false;
#pragma unroll
                for (int k = 0; k < 5; ++k) {
                    const double e0 = lds[(E + 3 * k) * WARP_SCAN_THREADS], e1 = lds[(E + 3 * k + 1) * WARP_SCAN_THREADS],
                                 e2 = lds[(E + 3 * k + 2) * WARP_SCAN_THREADS];
                    const double r00 = e2 - e0 - e1, r10 = e0 * W - e1 + e2, r11 = e0 * W + e1 * H + e2, r01 = e1 * H - e0 + e2;
                    empty = empty || (r00 < 0.0 && r10 < 0.0 && r11 < 0.0 && r01 < 0.0);
                }
                int i0, i1, j0, j1;
                if (!empty && warp_clip_box(lds, H, W, i0, i1, j0, j1)) {
                    const int4 b = make_int4(i0, i1, j0, j1);
                    if (sgn) c1 = b; else c0 = b;
                }
            }
            // two overlapping boxes would count their common pixels twice: merge them
            if (c0.x <= c0.y && c1.x <= c1.y && c0.x <= c1.y && c1.x <= c0.y && c0.z <= c1.w && c1.z <= c0.w) {
                c0 = make_int4(min(c0.x, c1.x), max(c0.y, c1.y), min(c0.z, c1.z), max(c0.w, c1.w));
                c1 = make_int4(0, -1, 0, -1);
            }
        }
        if (c0.x <= c0.y) b0 = warp_scan_box(c0.x, c0.y, c0.z, c0.w);
        if (c1.x <= c1.y) b1 = warp_scan_box(c1.x, c1.y, c1.z, c1.w);
    }
    }();
    // heavy blocks (far field: hundreds of candidates) go to a work list and are flagged in their first scan; the others are
    // found by the gather's light waves directly
    const int64_t c0 = b0.u1 >= b0.u0 ? (int64_t)(b0.u1 - b0.u0 + 1) * b0.len : 0;
    const int64_t c1 = b1.u1 >= b1.u0 ? (int64_t)(b1.u1 - b1.u0 + 1) * b1.len : 0;
    const bool is_heavy = c0 + c1 > heavy_above;
    if (is_heavy) b0.swap |= 2;
    scans[2 * idx] = b0;
    scans[2 * idx + 1] = b1;
    // one atomic per wave (25 K atomics on one address take 11 ns each: 285 us); the order inside the list does not matter
    const int lane = threadIdx.x & 63;
    const uint64_t hv = __ballot(is_heavy);
    if (is_heavy) {
        const int leader = __ffsll((unsigned long long)hv) - 1;
        int slot = 0;
        if (lane == leader) slot = atomicAdd(counts, __popcll(hv));
        slot = __shfl(slot, leader, 64) + __popcll(hv & ((1ull << lane) - 1ull));
        heavy_list[slot] = (int)idx;
    }
}
#undef SLOT

constexpr int WARP_GU = 8;          // grad_dst loads in flight per lane

// The candidate rounds first, first + stride, ... (64 candidates each) of one 2 x 2 texel block, run by one wave.
// Lane = (hit stream, channel chunk): with G = 2^lgG >= C/4 lanes per stream the wave runs 64 / G streams that take the
// compacted hits round-robin (two at 128 channels).  Candidates: the block's (up to two) scans, then -- normally none --
// the listed pixels that kornia does not divide (counts[1] of them in all, counts[2 + seg] in segment seg of odd_list).
template <typename T>
__device__ __forceinline__ void warp_gather_rounds(
    const T *__restrict__ gchunk, const T (&Mn)[9], const WarpScan &sc0, const WarpScan &sc1, const int *__restrict__ counts,
    const int *__restrict__ odd_list, int64_t odd_per, int n, int bx, int by, int C, int h, int w, int H, int W, int nearest,
    int lgG, bool has_ch, int first, int stride, WarpRec<T> *mine, T (&acc)[4][16 / (int)sizeof(T)])
{
    constexpr int VEC = 16 / (int)sizeof(T);
    using Rec = WarpRec<T>;
    const int S = 64 >> lgG;
    const int lane = threadIdx.x & 63, st = lane >> lgG;
    const uint64_t below = (1ull << lane) - 1ull;

    // one round: this lane's candidate (i, j) (if `cand`), an ordinary pixel (|z| > 1e-8) or a listed odd one
    auto round = [&](bool cand, int i, int j, bool odd) {
        bool hit = false;
        Rec r;
        r.pix = 0;
        r.mask = 0;
#pragma unroll
        for (int t = 0; t < 4; ++t) r.w[t] = T(0);
        if (cand && (fabs(source_pz(Mn, i, j)) > 1e-8) != odd) {
            double x, y;
            source_position(Mn, i, j, h, w, x, y);
            const SrcCoord c = make_coord(x, y, h, w, nearest);
            const int dx = c.x0 - 2 * bx, dy = c.y0 - 2 * by;                      // corner 00 relative to the block
            if (c.any && dx >= -1 && dx <= 1 && dy >= -1 && dy <= 1) {
                const T w00 = T(c.wy0 * c.wx0), w01 = T(c.wy0 * c.wx1);
                const T w10 = T(c.wy1 * c.wx0), w11 = T(c.wy1 * c.wx1);
                // corner (cy, cx) lies on block texel (dy + cy, dx + cx) when that is in {0, 1}^2
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int ty = t >> 1, tx = t & 1, cy = ty - dy, cx = tx - dx;
                    if (cy >= 0 && cy <= 1 && cx >= 0 && cx <= 1) {
                        const bool ok = cy ? (cx ? c.v11 : c.v10) : (cx ? c.v01 : c.v00);
                        const T ww = cy ? (cx ? w11 : w10) : (cx ? w01 : w00);
                        if (ok) {
                            r.mask |= 1 << t;
                            r.w[t] = ww;
                        }
                    }
                }
                r.pix = ((n * H + i) * W + j) * C;                                  // element offset (< 2^31: checked on the host)
                hit = r.mask != 0;
            }
        }
        const uint64_t hits = __ballot(hit);
        const int nhit = __popcll(hits);
        if (hit) mine[__popcll(hits & below)] = r;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // stream st takes hits st, st + S, ...: WARP_GU of them in flight.  (q0 + u * S < nhit is wave-uniform: whole
        // steps are skipped with a scalar branch; the one stream that runs out a hit early gets zero weights.)
        for (int q0 = 0; q0 < nhit; q0 += WARP_GU * S) {
            Pack<T, VEC> g[WARP_GU];
#pragma unroll
            for (int u = 0; u < WARP_GU; ++u) {               // the loads first (only the offsets are read here) ...
                const int off = mine[min(q0 + u * S + st, nhit - 1)].pix;          // (clamped: branch-free, so they overlap)
                g[u] = has_ch ? Pack<T, VEC>::load(gchunk + off) : Pack<T, VEC>::zero();
            }
#pragma unroll
            for (int u = 0; u < WARP_GU; ++u) {               // ... then the weights, re-read from LDS
                if (q0 + u * S < nhit) {
                    const int qq = q0 + u * S + st;
                    const Rec rr = mine[min(qq, nhit - 1)];
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const T wt = qq < nhit ? rr.w[t] : T(0);           // (texels the footprint misses have weight 0)
#pragma unroll
                        for (int v = 0; v < VEC; ++v) acc[t][v] += wt * g[u].v[v];
                    }
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    };

    for (int bsel = 0; bsel < 2; ++bsel) {
        const WarpScan &sc = bsel ? sc1 : sc0;
        const int swap = sc.swap & 1;
        const int cnt = sc.u1 >= sc.u0 && sc.len > 0 ? (sc.u1 - sc.u0 + 1) * sc.len : 0;
        const int V = swap ? H : W;
        const float rlen = 1.0f / (float)sc.len;
        const bool small = cnt < (1 << 22);                   // k * rlen is then within one of the quotient
        for (int base = first * 64; base < cnt; base += stride * 64) {
            const int k = base + lane;
            int i = 0, j = 0;
            bool cand = false;
            if (k < cnt) {
                int du;
                if (small) {
                    du = (int)((float)k * rlen);
                    du -= du * sc.len > k;
                    du += (du + 1) * sc.len <= k;
                } else {
                    du = k / sc.len;
                }
                const int u = sc.u0 + du;
                const int v = (int)ceil(sc.a + sc.s * ((double)u - sc.uc)) + (k - du * sc.len);
                i = swap ? v : u;
                j = swap ? u : v;
                cand = v >= 0 && v < V;
            }
            round(cand, i, j, false);
        }
    }
    if (counts[1] != 0) {
        // pixels kornia does not divide (listed by warp_bwd_scans, segment by segment in pixel order)
        const int64_t npix = (int64_t)H * W;                  // per view
        for (int seg = 0; seg < WARP_ODD_SEGS; ++seg) {
            const int cnt = counts[2 + seg];
            for (int base = first * 64; base < cnt; base += stride * 64) {
                const int k = base + lane;
                int i = 0, j = 0;
                bool cand = false;
                if (k < cnt) {
                    const int p = odd_list[seg * odd_per + k];
                    const int pn = (int)(p / npix), rem = (int)(p - pn * npix);
                    i = rem / W;
                    j = rem - i * W;
                    cand = pn == n;
                }
                round(cand, i, j, true);
            }
        }
    }
    // the streams' partial sums, in a fixed order
    for (int off = 1 << lgG; off < 64; off <<= 1)
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[t][v] += __shfl_xor(acc[t][v], off, 64);
}

// Workgroups [0, heavy_wgs): the heavy blocks (far field: hundreds of candidates; listed by warp_bwd_scans), one
// workgroup per (block, channel group) at a time, its four waves taking the candidate rounds in turn and adding their
// partial sums in wave order.  The other workgroups: one WAVE per (block, channel group), which returns at once if the
// block is flagged heavy.  counts = [heavy blocks, odd pixels, odd pixels per segment ...].
template <typename T>
__global__ __launch_bounds__(256) void warp_bwd_gather(
    const T *__restrict__ grad_dst, const T *__restrict__ Mv, const WarpScan *__restrict__ scans,
    const int *__restrict__ heavy_list, const int *__restrict__ counts, const int *__restrict__ odd_list, int N, int C, int h,
    int w, int H, int W, int nearest, int lgG, int cgroups, int heavy_wgs, T *__restrict__ grad_src)
{
    constexpr int VEC = 16 / (int)sizeof(T);
    __shared__ WarpRec<T> recs[4][64];
    __shared__ T part[3][64][4 * VEC];                        // heavy path: the partial sums of waves 1..3
    const int G = 1 << lgG;
    const int tid = threadIdx.x, lane = tid & 63, lg = lane & (G - 1), st = lane >> lgG;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);  // (wave-uniform: block, view, matrix and scans live in SGPRs)
    const int bw2 = (w + 1) / 2, bh2 = (h + 1) / 2;
    const int64_t nblk = (int64_t)N * bh2 * bw2;
    const bool heavy = (int)blockIdx.x < heavy_wgs;
    const int64_t nitems = heavy ? (int64_t)counts[0] * cgroups : nblk * cgroups;
    for (int64_t item = heavy ? (int64_t)blockIdx.x : ((int64_t)blockIdx.x - heavy_wgs) * 4 + wv; item < nitems;
         item += heavy ? (int64_t)heavy_wgs : nitems) {
        const int64_t blk = heavy ? (int64_t)heavy_list[item / cgroups] : item / cgroups;
        const int cgi = (int)(item % cgroups);
        const WarpScan sc0 = scans[2 * blk], sc1 = scans[2 * blk + 1];
        if (!heavy && (sc0.swap & 2)) return;                 // a heavy block: the workgroups above take it
        const int n = (int)(blk / ((int64_t)bh2 * bw2));
        const int rem = (int)(blk - (int64_t)n * bh2 * bw2);
        const int by = rem / bw2, bx = rem - by * bw2;
        const int chunk = cgi * G + lg;
        const bool has_ch = chunk < C / VEC;
        T Mn[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) Mn[k] = Mv[(int64_t)n * 9 + k];
        T acc[4][VEC];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[t][v] = T(0);
        const int64_t odd_per = ((int64_t)N * H * W + WARP_ODD_SEGS - 1) / WARP_ODD_SEGS;
        warp_gather_rounds<T>(grad_dst + (int64_t)chunk * VEC, Mn, sc0, sc1, counts, odd_list, odd_per, n, bx, by, C, h, w, H,
                              W, nearest, lgG, has_ch, heavy ? wv : 0, heavy ? 4 : 1, recs[wv], acc);
        if (heavy) {
            if (wv > 0 && st == 0)
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int v = 0; v < VEC; ++v) part[wv - 1][lg][t * VEC + v] = acc[t][v];
            __syncthreads();
            if (wv == 0 && st == 0)
                for (int o = 0; o < 3; ++o)
#pragma unroll
                    for (int t = 0; t < 4; ++t)
#pragma unroll
                        for (int v = 0; v < VEC; ++v) acc[t][v] += part[o][lg][t * VEC + v];
            __syncthreads();
        }
        if (has_ch && st == 0 && (!heavy || wv == 0)) {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int Y = 2 * by + (t >> 1), X = 2 * bx + (t & 1);
                if (Y < h && X < w) {
                    Pack<T, VEC> o;
#pragma unroll
                    for (int v = 0; v < VEC; ++v) o.v[v] = acc[t][v];
                    o.store(grad_src + (((int64_t)n * h + Y) * w + X) * C + (int64_t)chunk * VEC);
                }
            }
        }
    }
}

// Scratch of the gather backward, one buffer per (device, stream), grown on demand and kept for the life of the process: every
// use is enqueued on that stream, so reuse is ordered; calls on different streams get different buffers (thread-safe).
// Not for HIP graph capture (the allocation would be captured once and the pointer reused across replays): capturing callers
// use the two-step form (mvdetr_warp_backward_plan_* into their own buffer).  Streams that have been destroyed leave their
// entry behind; mvdetr_warp_release_scratch() drops every entry (call it when no warp backward is in flight).
// (tag, key): the caller's version tag and the shapes of the plan the scratch currently holds (0: none)
struct WarpScratchEntry { char *ptr; size_t size; uint64_t tag; int64_t key[6]; };
static std::mutex g_warp_scratch_mu;
static std::map<std::pair<int, hipStream_t>, WarpScratchEntry> g_warp_scratch;
// `tag` != 0: the caller's promise that calls with the same tag (on this device and stream, with the same shapes) have the same
// matrices; `reuse` is set when the scratch already holds the plan of such a call -- the geometry pass is then skipped.
static char *warp_stream_scratch(hipStream_t st, size_t bytes, hipError_t &rc, uint64_t tag = 0, const int64_t *key = nullptr,
                                 bool *reuse = nullptr)
{
    using Entry = WarpScratchEntry;
    std::mutex &mu = g_warp_scratch_mu;
    auto &cache = g_warp_scratch;
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lock(mu);
    Entry &e = cache[{dev, st}];
    if (reuse) *reuse = false;
    if (e.size < bytes) {
        if (e.ptr) (void)hipFreeAsync(e.ptr, st);              // (after the work already queued on this stream)
        e.ptr = nullptr;
        e.size = 0;
        e.tag = 0;
        const size_t want = bytes + bytes / 4;
        rc = hipMallocAsync(reinterpret_cast<void **>(&e.ptr), want, st);
        if (rc != hipSuccess) { e.ptr = nullptr; return nullptr; }
        e.size = want;
    }
    if (tag && key && e.tag == tag && !memcmp(e.key, key, sizeof(e.key))) {
        if (reuse) *reuse = true;
    } else {
        e.tag = key ? tag : 0;                               // (an untagged call overwrites the plan: forget the tag)
        if (key) memcpy(e.key, key, sizeof(e.key));
    }
    return e.ptr;
}

// ---- launchers -------------------------------------------------------------------------------------------------------------
int warp_launch_scatter(const WarpCall &c, const WarpRoute &r)
{
    auto launch = [&](auto t) {
        using T = decltype(t);
        if (r.kind == WarpKind::bwd_cl) warp_launch_kernel<T, T>(warp_bwd_cl<T>, WARP_CL_THREADS, 0, c, r);
        else if (r.dst_nhwc) warp_launch_kernel<T, T>(warp_bwd<T, true>, WARP_PIX * WARP_SUB, 0, c, r);
        else warp_launch_kernel<T, T>(warp_bwd<T, false>, WARP_PIX * WARP_SUB, 0, c, r);
    };
    warp_for_type(c.type, launch);
    return (int)hipGetLastError();
}

// the geometry pass: candidate scans of every block, the heavy-block list, the pixels kornia does not divide
int warp_launch_plan(const WarpCall &c, char *plan)
{
    const WarpPlanLayout L = warp_plan_layout(c.N, c.h, c.w, c.H, c.W);
    const WarpPlanParts p = warp_plan_parts(plan, L);
    // the two running counters start from zero: one 8-byte stream write (a command-processor packet, no fill kernel)
    hipError_t rc = hipStreamWriteValue64(c.st, p.counts, 0, 0);
    if (rc != hipSuccess) {
        (void)hipGetLastError();
        rc = hipMemsetAsync(p.counts, 0, 2 * sizeof(int), c.st);
        if (rc != hipSuccess) return (int)rc;
    }
    const dim3 grid((unsigned)((L.nblk + WARP_SCAN_THREADS - 1) / WARP_SCAN_THREADS + WARP_ODD_SEGS));
    auto launch = [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((warp_bwd_scans<T>), grid, dim3(WARP_SCAN_THREADS), 0, c.st, static_cast<const T *>(c.M), c.N, c.h, c.w, c.H, c.W,
                           (int)c.knobs.force_clip, c.knobs.heavy_above, p.scans, p.heavy_list, p.counts, p.odd_list);
    };
    warp_for_type(c.type, launch);
    return (int)hipGetLastError();
}

// the gradient from a plan of the same matrices and shapes (the plan is only read)
int warp_launch_gather(const WarpCall &c, const WarpRoute &r, char *plan)
{
    const WarpPlanParts p = warp_plan_parts(plan, warp_plan_layout(c.N, c.h, c.w, c.H, c.W));
    auto launch = [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((warp_bwd_gather<T>), dim3((unsigned)r.grid), dim3(256), 0, c.st, static_cast<const T *>(c.in), static_cast<const T *>(c.M),
                           p.scans, p.heavy_list, p.counts, p.odd_list, c.N, c.C, c.h, c.w, c.H, c.W, r.nearest, r.lgG, r.cgroups,
                           c.knobs.heavy_wgs, static_cast<T *>(c.out));
    };
    warp_for_type(c.type, launch);
    return (int)hipGetLastError();
}

// The plan of this call in stream-ordered scratch (kept per stream between calls: hipMallocAsync + hipFreeAsync cost the host
// ~10 us per call, more than the launches).  A caller-supplied version tag of the matrices lets consecutive calls reuse the
// plan itself (mvdetr_warp_perspective_backward_tagged_*): the gather is then the only launch.  Callers who own a plan buffer
// use mvdetr_warp_backward_plan_* / mvdetr_warp_perspective_backward_planned_* instead.
int warp_launch_gather_scratch(const WarpCall &c, const WarpRoute &r)
{
    hipError_t rc = hipSuccess;
    const int64_t key[6] = {c.N, c.h, c.w, ((int64_t)c.H << 32) | (unsigned)c.W, c.type == WarpType::f32 ? 4 : 8, c.knobs.plan_key()};
    bool reuse = false;
    char *scratch = warp_stream_scratch(c.st, (size_t)r.plan_bytes, rc, c.tag, key, &reuse);
    if (!scratch) return (int)rc;
    if (!reuse) {
        const int r1 = warp_launch_plan(c, scratch);
        if (r1) {
            (void)warp_stream_scratch(c.st, 0, rc, 0, key, nullptr);      // (no plan was built: forget the tag)
            return r1;
        }
    }
    return warp_launch_gather(c, r, scratch);
}

}  // namespace mvdetr

extern "C" int mvdetr_warp_release_scratch(void)
{
    std::lock_guard<std::mutex> lock(mvdetr::g_warp_scratch_mu);
    int prev = 0, rc = 0;
    (void)hipGetDevice(&prev);
    for (auto &kv : mvdetr::g_warp_scratch) {
        if (!kv.second.ptr) continue;
        (void)hipSetDevice(kv.first.first);
        const hipError_t e = hipFree(kv.second.ptr);           // (synchronises with the device: nothing is still using it)
        if (e != hipSuccess && !rc) rc = (int)e;
    }
    mvdetr::g_warp_scratch.clear();
    (void)hipSetDevice(prev);
    return rc;
}

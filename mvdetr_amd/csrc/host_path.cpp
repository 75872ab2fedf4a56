// CPU path of libmvdetr_ops.so: multi-scale deformable attention forward / backward and the perspective warp on
// host tensors (plain C++17, std::thread; no GPU, no PyTorch).
//
// The reference's extension has none -- ms_deform_attn_cpu.cpp:17-41 are stubs that raise "Not implement on cpu" --
// so its model code cannot run the deform_trans path without CUDA, and BASELINE.json's configs[0] ("PyTorch CPU-only")
// exists only for --world_feat conv.  This file makes CPU tensors work behind the same Python face.
// It is product code, separate from the test suite's checker under oracle/ (nothing here includes or calls it); the
// arithmetic follows the reference kernels' definitions:
//   forward   ms_deformable_im2col_gpu_kernel + ms_deform_attn_im2col_bilinear       (ms_deform_im2col_cuda.cuh:237-299, 33-84)
//   backward  ms_deformable_col2im_* + ms_deform_attn_col2im_bilinear                 (cuh:301-920, 87-158)
//   warp      kornia.warp_perspective(bilinear, zeros, align_corners=False)           (call site mvdetr.py:194)
// Work decomposition (different from the GPU kernels on purpose -- no atomics, deterministic results):
//   forward   threads own contiguous ranges of (batch, query);
//   backward  threads own (batch, head) pairs: grad_value[b, :, m, :] is then written by exactly one thread;
//   warp      forward: threads own destination rows; backward: threads own (view, channel) planes of grad_src.
//   deform_conv  (torchvision.ops.deform_conv2d v1) per batch item and 1024-pixel chunk: the column matrix col[p][c kh kw + tap]
//             and its gradient g_col are formed with threads owning pixels; grad_weight with threads owning output channels,
//             grad_input with threads owning input channels.
//   attention    (softmax(q k^T / sqrt(D)) v, strided operands) forward and dQ: threads own query rows and walk the keys 64 at a
//             time (online softmax; never more than that tile of scores); dK / dV: threads own key rows and walk the queries,
//             the probabilities recomputed from lse.  Dropout by the shared counter-based hash (attention_hash.h).
//   frame targets  threads own maps for the slot lists (the compaction of a map is serial), then rows of the heat maps; the
//             per-object arithmetic is the kernel's own (frame_targets_core.h), uncontracted.
#include "../../include/mvdetr_ops.h"
#include "attention_hash.h"
#include "frame_targets_core.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <thread>
#include <vector>

namespace {

int host_threads()
{
    static const int n = [] {
        if (const char *e = getenv("MVDETR_HOST_THREADS")) return std::max(1, atoi(e));
        if (const char *e = getenv("OMP_NUM_THREADS")) return std::max(1, atoi(e));        // the reference pins this to 1 (main.py:3)
        const unsigned hw = std::thread::hardware_concurrency();
        return (int)std::min<unsigned>(hw ? hw : 1, 64);
    }();
    return n;
}

// fn(first, last) over [0, n) split into contiguous chunks, one thread each
template <typename Fn> void parallel_ranges(int64_t n, Fn fn)
{
    const int t = (int)std::min<int64_t>(host_threads(), std::max<int64_t>(n, 1));
    if (t <= 1) {
        fn((int64_t)0, n);
        return;
    }
    std::vector<std::thread> pool;
    pool.reserve(t);
    for (int i = 0; i < t; ++i) pool.emplace_back([=] { fn(n * i / t, n * (i + 1) / t); });
    for (auto &th : pool) th.join();
}

// bilinear footprint of a sampling point given in pixel units (loc * size - 0.5): integer corner, weights, validity
template <typename T> struct Tap {
    int y0, x0;
    T w[4];             // corner weights (y0,x0) (y0,x1) (y1,x0) (y1,x1)
    bool ok[4];
    T fy, fx;           // fractional parts
};

template <typename T> inline bool make_tap(T y, T x, int H, int W, Tap<T> &t)
{
    if (!(y > T(-1) && x > T(-1) && y < T(H) && x < T(W))) return false;      // cuh:288 (NaN fails too)
    const T yl = std::floor(y), xl = std::floor(x);
    t.y0 = (int)yl;
    t.x0 = (int)xl;
    t.fy = y - yl;
    t.fx = x - xl;
    const T hy = T(1) - t.fy, hx = T(1) - t.fx;
    t.w[0] = hy * hx;
    t.w[1] = hy * t.fx;
    t.w[2] = t.fy * hx;
    t.w[3] = t.fy * t.fx;
    const bool y0 = t.y0 >= 0, y1 = t.y0 + 1 <= H - 1, x0 = t.x0 >= 0, x1 = t.x0 + 1 <= W - 1;
    t.ok[0] = y0 && x0;
    t.ok[1] = y0 && x1;
    t.ok[2] = y1 && x0;
    t.ok[3] = y1 && x1;
    return true;
}

bool bad(int B, int S, int M, int D, int L, int Lq, int P) { return B < 0 || S < 0 || M < 1 || D < 1 || L < 1 || Lq < 0 || P < 1; }

template <typename T>
int msda_forward_host(const T *value, const int64_t *shapes, const int64_t *lsi, const T *loc, const T *aw, int B, int S, int M,
                      int D, int L, int Lq, int P, T *out)
{
    if (bad(B, S, M, D, L, Lq, P) || !shapes || !lsi || (!out && B > 0 && Lq > 0)) return 1;
    const int64_t row = (int64_t)M * D;
    parallel_ranges((int64_t)B * Lq, [=](int64_t first, int64_t last) {
        std::vector<T> acc(D);
        for (int64_t bq = first; bq < last; ++bq) {
            const int64_t b = bq / Lq;
            for (int m = 0; m < M; ++m) {
                std::fill(acc.begin(), acc.end(), T(0));
                const T *lp = loc + (bq * M + m) * (int64_t)L * P * 2;
                const T *wp = aw + (bq * M + m) * (int64_t)L * P;
                for (int l = 0; l < L; ++l) {
                    const int H = (int)shapes[2 * l], W = (int)shapes[2 * l + 1];
                    const T *plane = value + (b * S + lsi[l]) * row + (int64_t)m * D;
                    for (int p = 0; p < P; ++p) {
                        Tap<T> t;
                        if (!make_tap(lp[(l * P + p) * 2 + 1] * T(H) - T(0.5), lp[(l * P + p) * 2] * T(W) - T(0.5), H, W, t)) continue;
                        const T a = wp[l * P + p];
                        for (int k = 0; k < 4; ++k) {
                            if (!t.ok[k]) continue;
                            const T *v = plane + ((int64_t)(t.y0 + (k >> 1)) * W + t.x0 + (k & 1)) * row;
                            const T wk = t.w[k] * a;
                            for (int c = 0; c < D; ++c) acc[c] += wk * v[c];
                        }
                    }
                }
                std::copy(acc.begin(), acc.end(), out + bq * row + (int64_t)m * D);
            }
        }
    });
    return 0;
}

template <typename T>
int msda_backward_host(const T *go, const T *value, const int64_t *shapes, const int64_t *lsi, const T *loc, const T *aw, int B,
                       int S, int M, int D, int L, int Lq, int P, T *gv, T *gl, T *ga)
{
    if (bad(B, S, M, D, L, Lq, P) || !shapes || !lsi) return 1;
    const int64_t row = (int64_t)M * D;
    // grad_value is accumulated: the caller hands it over zeroed (like the reference's zeros_like, cu:121)
    parallel_ranges((int64_t)B * M, [=](int64_t first, int64_t last) {
        for (int64_t bm = first; bm < last; ++bm) {
            const int64_t b = bm / M;
            const int m = (int)(bm % M);
            for (int64_t q = 0; q < Lq; ++q) {
                const int64_t bq = b * Lq + q;
                const T *g = go + bq * row + (int64_t)m * D;
                const T *lp = loc + (bq * M + m) * (int64_t)L * P * 2;
                const T *wp = aw + (bq * M + m) * (int64_t)L * P;
                T *glp = gl + (bq * M + m) * (int64_t)L * P * 2;
                T *gap = ga + (bq * M + m) * (int64_t)L * P;
                for (int l = 0; l < L; ++l) {
                    const int H = (int)shapes[2 * l], W = (int)shapes[2 * l + 1];
                    const T *plane = value + (b * S + lsi[l]) * row + (int64_t)m * D;
                    T *gplane = gv + (b * S + lsi[l]) * row + (int64_t)m * D;
                    for (int p = 0; p < P; ++p) {
                        T d_a = 0, d_x = 0, d_y = 0;
                        Tap<T> t;
                        if (make_tap(lp[(l * P + p) * 2 + 1] * T(H) - T(0.5), lp[(l * P + p) * 2] * T(W) - T(0.5), H, W, t)) {
                            const T a = wp[l * P + p];
                            // d(weight_k)/dy, d(weight_k)/dx of the four corners (cuh:115-152)
                            const T dy[4] = {-(T(1) - t.fx), -t.fx, T(1) - t.fx, t.fx};
                            const T dx[4] = {-(T(1) - t.fy), T(1) - t.fy, -t.fy, t.fy};
                            for (int k = 0; k < 4; ++k) {
                                if (!t.ok[k]) continue;
                                const int64_t tok = ((int64_t)(t.y0 + (k >> 1)) * W + t.x0 + (k & 1)) * row;
                                const T *v = plane + tok;
                                T *gvk = gplane + tok;
                                T dot = 0;
                                const T wk = t.w[k] * a;
                                for (int c = 0; c < D; ++c) {
                                    dot += g[c] * v[c];
                                    gvk[c] += wk * g[c];
                                }
                                d_a += t.w[k] * dot;
                                d_y += dy[k] * dot;
                                d_x += dx[k] * dot;
                            }
                            d_x *= a * T(W);
                            d_y *= a * T(H);
                        }
                        gap[l * P + p] = d_a;
                        glp[(l * P + p) * 2] = d_x;
                        glp[(l * P + p) * 2 + 1] = d_y;
                    }
                }
            }
        }
    });
    return 0;
}

// 3x3 inverse in double; false if singular
bool invert3(const double *m, double *inv)
{
    const double c00 = m[4] * m[8] - m[5] * m[7], c01 = m[5] * m[6] - m[3] * m[8], c02 = m[3] * m[7] - m[4] * m[6];
    const double det = m[0] * c00 + m[1] * c01 + m[2] * c02;
    if (!(std::fabs(det) > 0)) return false;
    const double r = 1.0 / det;
    inv[0] = c00 * r;
    inv[1] = (m[2] * m[7] - m[1] * m[8]) * r;
    inv[2] = (m[1] * m[5] - m[2] * m[4]) * r;
    inv[3] = c01 * r;
    inv[4] = (m[0] * m[8] - m[2] * m[6]) * r;
    inv[5] = (m[2] * m[3] - m[0] * m[5]) * r;
    inv[6] = c02 * r;
    inv[7] = (m[1] * m[6] - m[0] * m[7]) * r;
    inv[8] = (m[0] * m[4] - m[1] * m[3]) * r;
    return true;
}

// where destination pixel (i, j) samples the source, in source pixel units of grid_sample(align_corners=False):
// kornia normalises with (size - 1) and samples with align_corners=False, hence the size / (size - 1) factor
// (the same quirk the HIP kernel reproduces)
inline void source_position(const double *inv, int i, int j, int sh, int sw, double &y, double &x, bool &finite)
{
    // p = M^-1 (j, i, 1), homogeneous; normalised like kornia does (2 p / (size - 1) - 1, scaled by z), divided only
    // where |z| > 1e-8, then mapped by the align_corners=False sampler: ((g + 1) * size - 1) / 2
    const double px = inv[0] * j + inv[1] * i + inv[2], py = inv[3] * j + inv[4] * i + inv[5], pz = inv[6] * j + inv[7] * i + inv[8];
    const double wd = sw == 1 ? 1e-14 : (double)(sw - 1), hd = sh == 1 ? 1e-14 : (double)(sh - 1);
    const double qx = 2.0 * px / wd - pz, qy = 2.0 * py / hd - pz;
    const double s = std::fabs(pz) > 1e-8 ? 1.0 / pz : 1.0;
    x = ((qx * s + 1.0) * sw - 1.0) * 0.5;
    y = ((qy * s + 1.0) * sh - 1.0) * 0.5;
    finite = std::isfinite(x) && std::isfinite(y);
}

// mode: 0 bilinear, 1 nearest.  layout bit 0: dst NHWC, bit 1: src NHWC
template <typename T, bool BACKWARD>
int warp_host(const T *src_or_gdst, const T *mats, int n, int C, int sh, int sw, int dh, int dw, int layout, int mode, T *dst_or_gsrc)
{
    if (n < 0 || C < 1 || sh < 1 || sw < 1 || dh < 1 || dw < 1) return 1;
    const bool dst_nhwc = layout & 1, src_nhwc = layout & 2;
    auto s_idx = [=](int v, int c, int y, int x) { return src_nhwc ? (((int64_t)v * sh + y) * sw + x) * C + c : (((int64_t)v * C + c) * sh + y) * sw + x; };
    auto d_idx = [=](int v, int c, int y, int x) { return dst_nhwc ? (((int64_t)v * dh + y) * dw + x) * C + c : (((int64_t)v * C + c) * dh + y) * dw + x; };
    std::vector<double> inv((size_t)n * 9);
    std::vector<char> good(n);
    for (int v = 0; v < n; ++v) {
        double m[9];
        for (int k = 0; k < 9; ++k) m[k] = (double)mats[v * 9 + k];
        good[v] = invert3(m, &inv[(size_t)v * 9]);
    }
    const double *invp = inv.data();
    const char *goodp = good.data();
    // forward: units are destination rows; backward: units are (view, channel) planes of grad_src (race-free scatter)
    const int64_t units = BACKWARD ? (int64_t)n * C : (int64_t)n * dh;
    parallel_ranges(units, [=](int64_t first, int64_t last) {
        for (int64_t u = first; u < last; ++u) {
            const int v = BACKWARD ? (int)(u / C) : (int)(u / dh);
            const int c_only = BACKWARD ? (int)(u % C) : -1;
            const int i0 = BACKWARD ? 0 : (int)(u % dh), i1 = BACKWARD ? dh : i0 + 1;
            for (int i = i0; i < i1; ++i)
                for (int j = 0; j < dw; ++j) {
                    double y, x;
                    bool fin = goodp[v];
                    if (fin) source_position(invp + (size_t)v * 9, i, j, sh, sw, y, x, fin);
                    int ys[4], xs[4], nk = 0;
                    double ws[4];
                    if (fin) {
                        if (mode == 1) {
                            const double ry = std::nearbyint(y), rx = std::nearbyint(x);          // grid_sample 'nearest' rounds half to even
                            if (ry >= 0 && ry < sh && rx >= 0 && rx < sw) { ys[0] = (int)ry; xs[0] = (int)rx; ws[0] = 1.0; nk = 1; }
                        } else if (y > -1 && x > -1 && y < sh && x < sw) {
                            const double yl = std::floor(y), xl = std::floor(x), fy = y - yl, fx = x - xl;
                            const int yy[2] = {(int)yl, (int)yl + 1}, xx[2] = {(int)xl, (int)xl + 1};
                            const double wy[2] = {1 - fy, fy}, wx[2] = {1 - fx, fx};
                            for (int a = 0; a < 2; ++a)
                                for (int b = 0; b < 2; ++b)
                                    if (yy[a] >= 0 && yy[a] < sh && xx[b] >= 0 && xx[b] < sw) { ys[nk] = yy[a]; xs[nk] = xx[b]; ws[nk] = wy[a] * wx[b]; ++nk; }
                        }
                    }
                    if constexpr (!BACKWARD) {
                        for (int c = 0; c < C; ++c) {
                            double acc = 0;
                            for (int k = 0; k < nk; ++k) acc += ws[k] * (double)src_or_gdst[s_idx(v, c, ys[k], xs[k])];
                            dst_or_gsrc[d_idx(v, c, i, j)] = (T)acc;
                        }
                    } else {
                        const T g = src_or_gdst[d_idx(v, c_only, i, j)];
                        for (int k = 0; k < nk; ++k) dst_or_gsrc[s_idx(v, c_only, ys[k], xs[k])] += (T)(ws[k] * (double)g);
                    }
                }
        }
    });
    return 0;
}

// ---- deformable convolution ----------------------------------------------------------------------------------------------

struct DcDims {
    int B, C, H, W, Co, Ho, Wo, kh, kw, sh, sw, ph, pw, dh, dw, G, nhwc;
};

bool dc_dims(int B, int C, int H, int W, int Co, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int G, int nhwc,
             DcDims &d)
{
    if (B < 0 || C < 0 || H < 1 || W < 1 || Co < 0 || kh < 1 || kw < 1 || sh < 1 || sw < 1 || ph < 0 || pw < 0 || dh < 1 ||
        dw < 1 || G < 1 || C % G != 0)
        return false;
    const int eh = H + 2 * ph - dh * (kh - 1) - 1, ew = W + 2 * pw - dw * (kw - 1) - 1;
    if (eh < 0 || ew < 0) return false;
    d = DcDims{B, C, H, W, Co, eh / sh + 1, ew / sw + 1, kh, kw, sh, sw, ph, pw, dh, dw, G, nhwc ? 1 : 0};
    return true;
}

// footprint of output pixel p, group g, tap: corner element offsets (channel 0 of batch item 0), weights, validity
template <typename T> struct DcTap {
    int64_t at[4];
    T w[4];
    bool ok[4];
    bool in;
    T ly, lx;
};

template <typename T> DcTap<T> dc_tap(const DcDims &d, const T *off, int b, int g, int tap, int p)
{
    const int T_ = d.kh * d.kw, HWo = d.Ho * d.Wo;
    const int ho = p / d.Wo, wo = p % d.Wo, i = tap / d.kw, j = tap % d.kw;
    const T *o = off + ((int64_t)b * 2 * d.G * T_ + 2 * (g * T_ + tap)) * HWo + p;
    const T y = T(ho * d.sh - d.ph + i * d.dh) + o[0], x = T(wo * d.sw - d.pw + j * d.dw) + o[HWo];
    DcTap<T> t;
    t.in = y > T(-1) && y < T(d.H) && x > T(-1) && x < T(d.W);
    const T fy = t.in ? std::floor(y) : T(0), fx = t.in ? std::floor(x) : T(0);
    const int y0 = (int)fy, x0 = (int)fx;
    t.ly = t.in ? y - fy : T(0);
    t.lx = t.in ? x - fx : T(0);
    const int ys[4] = {y0, y0, y0 + 1, y0 + 1}, xs[4] = {x0, x0 + 1, x0, x0 + 1};
    const T wy[4] = {1 - t.ly, 1 - t.ly, t.ly, t.ly}, wx[4] = {1 - t.lx, t.lx, 1 - t.lx, t.lx};
    const int64_t pst = d.nhwc ? d.C : 1;
    for (int k = 0; k < 4; ++k) {
        t.ok[k] = t.in && ys[k] >= 0 && ys[k] < d.H && xs[k] >= 0 && xs[k] < d.W;
        t.at[k] = t.ok[k] ? ((int64_t)ys[k] * d.W + xs[k]) * pst : 0;
        t.w[k] = wy[k] * wx[k];
    }
    return t;
}

constexpr int DC_CHUNK = 1024;

// col[pl][c * T + tap] for the pixels [p0, p0 + np) of batch item b
template <typename T> void dc_columns(const DcDims &d, const T *in, const T *off, int b, int p0, int np, T *col)
{
    const int T_ = d.kh * d.kw, Cg = d.C / d.G, K = d.C * T_;
    const int64_t HW = (int64_t)d.H * d.W, cst = d.nhwc ? 1 : HW;
    const T *inb = in + (int64_t)b * d.C * HW;
    parallel_ranges(np, [&](int64_t a, int64_t e) {
        for (int64_t pl = a; pl < e; ++pl) {
            T *row = col + pl * K;
            for (int g = 0; g < d.G; ++g)
                for (int tap = 0; tap < T_; ++tap) {
                    const DcTap<T> t = dc_tap(d, off, b, g, tap, p0 + (int)pl);
                    for (int c = g * Cg; c < (g + 1) * Cg; ++c) {
                        T v = T(0);
                        for (int k = 0; k < 4; ++k)
                            if (t.ok[k]) v += t.w[k] * inb[c * cst + t.at[k]];
                        row[c * T_ + tap] = v;
                    }
                }
        }
    });
}

template <typename T>
int dc_forward_host(const T *in, const T *off, const T *wt, const T *bias, const DcDims &d, T *out)
{
    const int K = d.C * d.kh * d.kw, HWo = d.Ho * d.Wo;
    std::vector<T> col((size_t)DC_CHUNK * K);
    for (int b = 0; b < d.B; ++b)
        for (int p0 = 0; p0 < HWo; p0 += DC_CHUNK) {
            const int np = std::min(DC_CHUNK, HWo - p0);
            dc_columns(d, in, off, b, p0, np, col.data());
            parallel_ranges(np, [&](int64_t a, int64_t e) {
                for (int64_t pl = a; pl < e; ++pl) {
                    const T *row = col.data() + pl * K;
                    for (int o = 0; o < d.Co; ++o) {
                        const T *w = wt + (int64_t)o * K;
                        T acc = bias ? bias[o] : T(0);
                        for (int k = 0; k < K; ++k) acc += w[k] * row[k];
                        out[((int64_t)b * d.Co + o) * HWo + p0 + pl] = acc;
                    }
                }
            });
        }
    return 0;
}

template <typename T>
int dc_backward_host(const T *gout, const T *in, const T *off, const T *wt, const DcDims &d, T *gin, T *goff, T *gw)
{
    const int T_ = d.kh * d.kw, K = d.C * T_, HWo = d.Ho * d.Wo, Cg = d.C / d.G;
    const int64_t HW = (int64_t)d.H * d.W, cst = d.nhwc ? 1 : HW;
    std::fill(gw, gw + (int64_t)d.Co * K, T(0));
    std::vector<T> col((size_t)DC_CHUNK * K), gcol((size_t)DC_CHUNK * K);
    for (int b = 0; b < d.B; ++b)
        for (int p0 = 0; p0 < HWo; p0 += DC_CHUNK) {
            const int np = std::min(DC_CHUNK, HWo - p0);
            const T *gob = gout + (int64_t)b * d.Co * HWo + p0;
            dc_columns(d, in, off, b, p0, np, col.data());
            parallel_ranges(d.Co, [&](int64_t a, int64_t e) {                  // grad_weight: threads own output channels
                for (int64_t o = a; o < e; ++o) {
                    T *w = gw + o * K;
                    for (int pl = 0; pl < np; ++pl) {
                        const T go = gob[o * HWo + pl];
                        const T *row = col.data() + (int64_t)pl * K;
                        for (int k = 0; k < K; ++k) w[k] += go * row[k];
                    }
                }
            });
            parallel_ranges(np, [&](int64_t a, int64_t e) {                    // g_col and grad_offset: threads own pixels
                for (int64_t pl = a; pl < e; ++pl) {
                    T *row = gcol.data() + pl * K;
                    std::fill(row, row + K, T(0));
                    for (int o = 0; o < d.Co; ++o) {
                        const T go = gob[(int64_t)o * HWo + pl];
                        const T *w = wt + (int64_t)o * K;
                        for (int k = 0; k < K; ++k) row[k] += w[k] * go;
                    }
                    const T *inb = in + (int64_t)b * d.C * HW;
                    for (int g = 0; g < d.G; ++g)
                        for (int tap = 0; tap < T_; ++tap) {
                            const DcTap<T> t = dc_tap(d, off, b, g, tap, p0 + (int)pl);
                            T gy = T(0), gx = T(0);
                            if (t.in)
                                for (int c = g * Cg; c < (g + 1) * Cg; ++c) {
                                    T v[4];
                                    for (int k = 0; k < 4; ++k) v[k] = t.ok[k] ? inb[c * cst + t.at[k]] : T(0);
                                    const T gc = row[c * T_ + tap];
                                    gy += gc * ((1 - t.lx) * (v[2] - v[0]) + t.lx * (v[3] - v[1]));
                                    gx += gc * ((1 - t.ly) * (v[1] - v[0]) + t.ly * (v[3] - v[2]));
                                }
                            T *go_ = goff + ((int64_t)b * 2 * d.G * T_ + 2 * (g * T_ + tap)) * HWo + p0 + pl;
                            go_[0] = gy;
                            go_[HWo] = gx;
                        }
                }
            });
            parallel_ranges(d.C, [&](int64_t a, int64_t e) {                   // grad_input: threads own input channels
                T *ginb = gin + (int64_t)b * d.C * HW;
                for (int64_t c = a; c < e; ++c) {
                    const int g = (int)(c / Cg);
                    for (int pl = 0; pl < np; ++pl)
                        for (int tap = 0; tap < T_; ++tap) {
                            const DcTap<T> t = dc_tap(d, off, b, g, tap, p0 + pl);
                            if (!t.in) continue;
                            const T gc = gcol[(int64_t)pl * K + c * T_ + tap];
                            for (int k = 0; k < 4; ++k)
                                if (t.ok[k]) ginb[c * cst + t.at[k]] += t.w[k] * gc;
                        }
                }
            });
        }
    return 0;
}

}  // namespace

extern "C" {

int mvdetr_msda_forward_host_f32(const float *value, const int64_t *spatial_shapes, const int64_t *level_start_index,
                                 const float *sampling_loc, const float *attn_weight, int batch, int spatial_size, int num_heads,
                                 int channels, int num_levels, int num_query, int num_point, float *out)
{
    return msda_forward_host(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, batch, spatial_size, num_heads,
                             channels, num_levels, num_query, num_point, out);
}
int mvdetr_msda_forward_host_f64(const double *value, const int64_t *spatial_shapes, const int64_t *level_start_index,
                                 const double *sampling_loc, const double *attn_weight, int batch, int spatial_size, int num_heads,
                                 int channels, int num_levels, int num_query, int num_point, double *out)
{
    return msda_forward_host(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, batch, spatial_size, num_heads,
                             channels, num_levels, num_query, num_point, out);
}
int mvdetr_msda_backward_host_f32(const float *grad_output, const float *value, const int64_t *spatial_shapes,
                                  const int64_t *level_start_index, const float *sampling_loc, const float *attn_weight, int batch,
                                  int spatial_size, int num_heads, int channels, int num_levels, int num_query, int num_point,
                                  float *grad_value, float *grad_sampling_loc, float *grad_attn_weight)
{
    return msda_backward_host(grad_output, value, spatial_shapes, level_start_index, sampling_loc, attn_weight, batch, spatial_size,
                              num_heads, channels, num_levels, num_query, num_point, grad_value, grad_sampling_loc, grad_attn_weight);
}
int mvdetr_msda_backward_host_f64(const double *grad_output, const double *value, const int64_t *spatial_shapes,
                                  const int64_t *level_start_index, const double *sampling_loc, const double *attn_weight, int batch,
                                  int spatial_size, int num_heads, int channels, int num_levels, int num_query, int num_point,
                                  double *grad_value, double *grad_sampling_loc, double *grad_attn_weight)
{
    return msda_backward_host(grad_output, value, spatial_shapes, level_start_index, sampling_loc, attn_weight, batch, spatial_size,
                              num_heads, channels, num_levels, num_query, num_point, grad_value, grad_sampling_loc, grad_attn_weight);
}
int mvdetr_warp_perspective_forward_host_f32(const float *src, const float *mats, int n, int channels, int src_h, int src_w, int dst_h,
                                             int dst_w, int layout_nhwc, int mode, float *dst)
{
    return warp_host<float, false>(src, mats, n, channels, src_h, src_w, dst_h, dst_w, layout_nhwc, mode, dst);
}
int mvdetr_warp_perspective_forward_host_f64(const double *src, const double *mats, int n, int channels, int src_h, int src_w,
                                             int dst_h, int dst_w, int layout_nhwc, int mode, double *dst)
{
    return warp_host<double, false>(src, mats, n, channels, src_h, src_w, dst_h, dst_w, layout_nhwc, mode, dst);
}
int mvdetr_warp_perspective_backward_host_f32(const float *grad_dst, const float *mats, int n, int channels, int src_h, int src_w,
                                              int dst_h, int dst_w, int layout_nhwc, int mode, float *grad_src)
{
    return warp_host<float, true>(grad_dst, mats, n, channels, src_h, src_w, dst_h, dst_w, layout_nhwc, mode, grad_src);
}
int mvdetr_warp_perspective_backward_host_f64(const double *grad_dst, const double *mats, int n, int channels, int src_h, int src_w,
                                              int dst_h, int dst_w, int layout_nhwc, int mode, double *grad_src)
{
    return warp_host<double, true>(grad_dst, mats, n, channels, src_h, src_w, dst_h, dst_w, layout_nhwc, mode, grad_src);
}

#define MVDETR_DC_HOST_ENTRIES(T, SFX)                                                                                        \
    int mvdetr_deform_conv2d_forward_host_##SFX(const T *input, const T *offset, const T *weight, const T *bias, int batch,   \
                                                int in_channels, int in_h, int in_w, int out_channels, int kernel_h,         \
                                                int kernel_w, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h,   \
                                                int dil_w, int offset_groups, int input_nhwc, T *out)                        \
    {                                                                                                                         \
        DcDims d;                                                                                                             \
        if (!dc_dims(batch, in_channels, in_h, in_w, out_channels, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w,      \
                     dil_h, dil_w, offset_groups, input_nhwc, d))                                                             \
            return 1;                                                                                                         \
        if ((int64_t)d.B * d.Co * d.Ho * d.Wo == 0) return 0;                                                                 \
        if (!out || !offset || (d.C && (!input || !weight))) return 1;                                                        \
        return dc_forward_host<T>(input, offset, weight, bias, d, out);                                                       \
    }                                                                                                                         \
    int mvdetr_deform_conv2d_backward_host_##SFX(const T *grad_out, const T *input, const T *offset, const T *weight,         \
                                                 int batch, int in_channels, int in_h, int in_w, int out_channels,            \
                                                 int kernel_h, int kernel_w, int stride_h, int stride_w, int pad_h, int pad_w, \
                                                 int dil_h, int dil_w, int offset_groups, int input_nhwc, T *grad_input,      \
                                                 T *grad_offset, T *grad_weight)                                              \
    {                                                                                                                         \
        DcDims d;                                                                                                             \
        if (!dc_dims(batch, in_channels, in_h, in_w, out_channels, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w,      \
                     dil_h, dil_w, offset_groups, input_nhwc, d))                                                             \
            return 1;                                                                                                         \
        const int64_t np = (int64_t)d.B * d.Ho * d.Wo, nw = (int64_t)d.Co * d.C * d.kh * d.kw;                               \
        if ((np && (!grad_offset || !offset)) || (nw && !grad_weight)) return 1;                                              \
        if (np * d.Co * d.C != 0 && (!grad_out || !input || !weight || !grad_input)) return 1;                                     \
        if (np * d.Co * d.C == 0) {                                                                                           \
            if (np) std::fill(grad_offset, grad_offset + np * 2 * d.G * d.kh * d.kw, T(0));                                  \
            if (nw) std::fill(grad_weight, grad_weight + nw, T(0));                                                           \
            return 0;                                                                                                         \
        }                                                                                                                     \
        return dc_backward_host<T>(grad_out, input, offset, weight, d, grad_input, grad_offset, grad_weight);                 \
    }

MVDETR_DC_HOST_ENTRIES(float, f32)
MVDETR_DC_HOST_ENTRIES(double, f64)

}  // extern "C"

// ---- attention ------------------------------------------------------------------------------------------------------------

namespace {

struct AtDims {
    int B, H, Sq, Sk, D;
    int64_t q[3], k[3], v[3], o[3], go[3], dq[3], dk[3], dv[3];
    uint32_t thresh;
    uint64_t seed;
    double inv_keep;
};

bool at_dims(const int64_t *strides, int nstr, int B, int H, int Sq, int Sk, int D, double p, uint64_t seed, AtDims &d)
{
    if (!strides || B < 0 || H < 0 || Sq < 0 || Sk < 1 || D < 1 || !(p >= 0.0) || !(p < 1.0)) return false;
    d.B = B; d.H = H; d.Sq = Sq; d.Sk = Sk; d.D = D;
    int64_t *dst[8] = {d.q, d.k, d.v, d.o, d.go, d.dq, d.dk, d.dv};
    for (int i = 0; i < 8; ++i)
        for (int j = 0; j < 3; ++j) dst[i][j] = i < nstr ? strides[3 * i + j] : 0;
    d.thresh = mvdetr_attn_threshold(p);
    d.seed = seed;
    d.inv_keep = 1.0 / (1.0 - p);
    return true;
}

inline bool at_keep(const AtDims &d, int b, int h, int i, int j)
{
    return mvdetr_attn_hash(d.seed, (((uint64_t)b * d.H + h) * d.Sq + i) * (uint64_t)d.Sk + j) >= d.thresh;
}

template <typename T> inline T at_dot(const T *a, const T *b, int D)
{
    T s = T(0);
    for (int c = 0; c < D; ++c) s += a[c] * b[c];
    return s;
}

constexpr int AT_TILE = 64;         // keys (or queries) whose scores exist at one time

template <typename T> int attention_forward_host(const T *q, const T *k, const T *v, const AtDims &d, T *out, T *lse)
{
    const T scale = T(1) / std::sqrt(T(d.D));
    const bool drop = d.thresh != 0;
    parallel_ranges((int64_t)d.B * d.H * d.Sq, [=, &d](int64_t first, int64_t last) {
        std::vector<T> acc(d.D);
        T s[AT_TILE];
        for (int64_t row = first; row < last; ++row) {
            const int i = (int)(row % d.Sq), h = (int)((row / d.Sq) % d.H), b = (int)(row / ((int64_t)d.Sq * d.H));
            const T *qp = q + b * d.q[0] + h * d.q[1] + i * d.q[2];
            const T *kb = k + b * d.k[0] + h * d.k[1], *vb = v + b * d.v[0] + h * d.v[1];
            std::fill(acc.begin(), acc.end(), T(0));
            T m = -std::numeric_limits<T>::infinity(), l = T(0);
            for (int j0 = 0; j0 < d.Sk; j0 += AT_TILE) {
                const int n = std::min(AT_TILE, d.Sk - j0);
                T mx = m;
                for (int t = 0; t < n; ++t) {
                    s[t] = scale * at_dot(qp, kb + (j0 + t) * d.k[2], d.D);
                    mx = std::max(mx, s[t]);
                }
                const T alpha = std::exp(m - mx);              // (0 on the first tile: m = -inf)
                l *= alpha;
                for (int c = 0; c < d.D; ++c) acc[c] *= alpha;
                m = mx;
                for (int t = 0; t < n; ++t) {
                    T pv = std::exp(s[t] - m);
                    l += pv;
                    if (drop) {
                        if (!at_keep(d, b, h, i, j0 + t)) continue;
                        pv *= T(d.inv_keep);
                    }
                    const T *vp = vb + (j0 + t) * d.v[2];
                    for (int c = 0; c < d.D; ++c) acc[c] += pv * vp[c];
                }
            }
            T *op = out + b * d.o[0] + h * d.o[1] + i * d.o[2];
            for (int c = 0; c < d.D; ++c) op[c] = acc[c] / l;
            lse[row] = m + std::log(l);
        }
    });
    return 0;
}

template <typename T>
int attention_backward_host(const T *go, const T *q, const T *k, const T *v, const T *out, const T *lse, const AtDims &d, T *gq,
                            T *gk, T *gv)
{
    const T scale = T(1) / std::sqrt(T(d.D));
    const bool drop = d.thresh != 0;
    const int64_t rows = (int64_t)d.B * d.H * d.Sq;
    std::vector<T> delta_v(std::max<int64_t>(rows, 1));
    T *delta = delta_v.data();
    // dQ (and delta): threads own query rows
    parallel_ranges(rows, [=, &d](int64_t first, int64_t last) {
        std::vector<T> acc(d.D);
        T ds[AT_TILE];
        for (int64_t row = first; row < last; ++row) {
            const int i = (int)(row % d.Sq), h = (int)((row / d.Sq) % d.H), b = (int)(row / ((int64_t)d.Sq * d.H));
            const T *qp = q + b * d.q[0] + h * d.q[1] + i * d.q[2];
            const T *gp = go + b * d.go[0] + h * d.go[1] + i * d.go[2];
            const T *kb = k + b * d.k[0] + h * d.k[1], *vb = v + b * d.v[0] + h * d.v[1];
            const T dl = at_dot(gp, out + b * d.o[0] + h * d.o[1] + i * d.o[2], d.D);
            delta[row] = dl;
            std::fill(acc.begin(), acc.end(), T(0));
            for (int j0 = 0; j0 < d.Sk; j0 += AT_TILE) {
                const int n = std::min(AT_TILE, d.Sk - j0);
                for (int t = 0; t < n; ++t) {
                    const T pv = std::exp(scale * at_dot(qp, kb + (j0 + t) * d.k[2], d.D) - lse[row]);
                    T dp = at_dot(gp, vb + (j0 + t) * d.v[2], d.D);
                    if (drop) dp = at_keep(d, b, h, i, j0 + t) ? dp * T(d.inv_keep) : T(0);
                    ds[t] = pv * (dp - dl);
                }
                for (int t = 0; t < n; ++t) {
                    const T *kp = kb + (j0 + t) * d.k[2];
                    for (int c = 0; c < d.D; ++c) acc[c] += ds[t] * kp[c];
                }
            }
            T *op = gq + b * d.dq[0] + h * d.dq[1] + i * d.dq[2];
            for (int c = 0; c < d.D; ++c) op[c] = scale * acc[c];
        }
    });
    // dK, dV: threads own key rows
    parallel_ranges((int64_t)d.B * d.H * d.Sk, [=, &d](int64_t first, int64_t last) {
        std::vector<T> ak(d.D), av(d.D);
        T ds[AT_TILE], pd[AT_TILE];
        for (int64_t row = first; row < last; ++row) {
            const int j = (int)(row % d.Sk), h = (int)((row / d.Sk) % d.H), b = (int)(row / ((int64_t)d.Sk * d.H));
            const T *kp = k + b * d.k[0] + h * d.k[1] + j * d.k[2], *vp = v + b * d.v[0] + h * d.v[1] + j * d.v[2];
            const T *qb = q + b * d.q[0] + h * d.q[1], *gb = go + b * d.go[0] + h * d.go[1];
            const int64_t r0 = ((int64_t)b * d.H + h) * d.Sq;
            std::fill(ak.begin(), ak.end(), T(0));
            std::fill(av.begin(), av.end(), T(0));
            for (int i0 = 0; i0 < d.Sq; i0 += AT_TILE) {
                const int n = std::min(AT_TILE, d.Sq - i0);
                for (int t = 0; t < n; ++t) {
                    const int i = i0 + t;
                    const T pv = std::exp(scale * at_dot(qb + i * d.q[2], kp, d.D) - lse[r0 + i]);
                    T dp = at_dot(gb + i * d.go[2], vp, d.D);
                    pd[t] = pv;
                    if (drop) {
                        const bool keep = at_keep(d, b, h, i, j);
                        dp = keep ? dp * T(d.inv_keep) : T(0);
                        pd[t] = keep ? pv * T(d.inv_keep) : T(0);
                    }
                    ds[t] = pv * (dp - delta[r0 + i]);
                }
                for (int t = 0; t < n; ++t) {
                    const T *qp = qb + (i0 + t) * d.q[2], *gp = gb + (i0 + t) * d.go[2];
                    for (int c = 0; c < d.D; ++c) {
                        av[c] += pd[t] * gp[c];
                        ak[c] += ds[t] * qp[c];
                    }
                }
            }
            T *okp = gk + b * d.dk[0] + h * d.dk[1] + j * d.dk[2], *ovp = gv + b * d.dv[0] + h * d.dv[1] + j * d.dv[2];
            for (int c = 0; c < d.D; ++c) {
                okp[c] = scale * ak[c];
                ovp[c] = av[c];
            }
        }
    });
    return 0;
}

}  // namespace

extern "C" {

int mvdetr_attention_dropout_mask_host(uint64_t seed, double dropout_p, int batch, int heads, int sq, int sk, uint8_t *mask)
{
    if (batch < 0 || heads < 0 || sq < 0 || sk < 0 || !(dropout_p >= 0.0) || !(dropout_p < 1.0)) return 1;
    const int64_t n = (int64_t)batch * heads * sq * sk;
    if (n == 0) return 0;
    if (!mask) return 1;
    const uint32_t thresh = mvdetr_attn_threshold(dropout_p);
    parallel_ranges(n, [=](int64_t first, int64_t last) {
        for (int64_t e = first; e < last; ++e) mask[e] = mvdetr_attn_hash(seed, (uint64_t)e) >= thresh ? 1 : 0;
    });
    return 0;
}

#define MVDETR_ATTN_HOST_ENTRIES(T, SFX)                                                                                      \
    int mvdetr_attention_forward_host_##SFX(const T *q, const T *k, const T *v, const int64_t *strides, int batch, int heads, \
                                            int sq, int sk, int head_dim, double dropout_p, uint64_t seed, T *out, T *lse)    \
    {                                                                                                                         \
        AtDims d;                                                                                                             \
        if (!at_dims(strides, 4, batch, heads, sq, sk, head_dim, dropout_p, seed, d)) return 1;                               \
        if ((int64_t)batch * heads * sq == 0) return 0;                                                                       \
        if (!q || !k || !v || !out || !lse) return 1;                                                                         \
        return attention_forward_host<T>(q, k, v, d, out, lse);                                                               \
    }                                                                                                                         \
    int mvdetr_attention_backward_host_##SFX(const T *grad_out, const T *q, const T *k, const T *v, const T *out,             \
                                             const T *lse, const int64_t *strides, int batch, int heads, int sq, int sk,      \
                                             int head_dim, double dropout_p, uint64_t seed, T *grad_q, T *grad_k, T *grad_v)  \
    {                                                                                                                         \
        AtDims d;                                                                                                             \
        if (!at_dims(strides, 8, batch, heads, sq, sk, head_dim, dropout_p, seed, d)) return 1;                               \
        if (batch * heads == 0) return 0;                                                                                     \
        if (!k || !v || !grad_k || !grad_v || (sq && (!grad_out || !q || !out || !lse || !grad_q))) return 1;                 \
        return attention_backward_host<T>(grad_out, q, k, v, out, lse, d, grad_q, grad_k, grad_v);                            \
    }

MVDETR_ATTN_HOST_ENTRIES(float, f32)
MVDETR_ATTN_HOST_ENTRIES(double, f64)

}  // extern "C"

// ---- detection extraction (csrc/detect.hip's contract on host memory) ------------------------------------------------------------------
// The reference's mvdet_decode -> cls_thres -> nms (utils/decode.py:80-93, trainer.py:130-135, utils/nms.py:7-44), one thread per frame:
// the candidates are sorted once by (score, index) descending -- equal scores: higher index first, the library's tie rule -- cut to the
// first top_k and swept greedily against the kept points.  Sum and products of the squared distance are separate roundings (this file is
// compiled for baseline x86-64: no fused multiply-add exists to contract them into).
namespace {

template <typename T> struct DetCand {
    T score, x, y;
    int idx;
};

template <typename T> int nms_host(std::vector<DetCand<T>> &c, T dist_thres, int top_k, std::vector<int> &kept)
{
    std::sort(c.begin(), c.end(), [](const DetCand<T> &a, const DetCand<T> &b) { return a.score > b.score || (a.score == b.score && a.idx > b.idx); });
    if (top_k > 0 && (size_t)top_k < c.size()) c.resize(top_k);
    kept.clear();
    for (size_t j = 0; j < c.size(); ++j) {
        bool keep = true;
        for (int k : kept) {
            const T dx = c[k].x - c[j].x, dy = c[k].y - c[j].y;
            const T xx = dx * dx, yy = dy * dy;
            if (!(std::sqrt(xx + yy) > dist_thres)) {
                keep = false;
                break;
            }
        }
        if (keep) kept.push_back((int)j);
    }
    return (int)kept.size();
}

template <typename T>
int detect_host(const T *hm, const int64_t *hs, const T *off, const int64_t *os, int B, int H, int W, double reduce, double cls_thres,
                double dist_thres, int top_k, int swap_xy, int max_det, T *det, int32_t *cell, int32_t *count)
{
    if (!hm || !hs || (off && !os) || !det || !cell || !count || B < 1 || H < 1 || W < 1 || max_det < 1 || (int64_t)H * W > ((int64_t)1 << 30))
        return 1;
    const T red = T(reduce), thres = T(cls_thres), dist = T(dist_thres);
    parallel_ranges(B, [=](int64_t b0, int64_t b1) {
        std::vector<DetCand<T>> cand;
        std::vector<int> kept;
        for (int64_t b = b0; b < b1; ++b) {
            cand.clear();
            for (int row = 0; row < H; ++row)
                for (int col = 0; col < W; ++col) {
                    const T s = T(1) / (T(1) + std::exp(-hm[b * hs[0] + row * hs[2] + col * hs[3]]));
                    if (!(s > thres)) continue;
                    T dx = T(0.5), dy = T(0.5);
                    if (off) {
                        const T *o = off + b * os[0] + row * os[2] + col * os[3];
                        dx = o[0];
                        dy = o[os[1]];
                    }
                    const T x = (T(col) + dx) * red, y = (T(row) + dy) * red;
                    cand.push_back(DetCand<T>{s + T(0), swap_xy ? y : x, swap_xy ? x : y, row * W + col});
                }
            const int n = nms_host(cand, dist, top_k, kept);
            count[b] = n;
            T *d = det + b * max_det * 3;
            int32_t *c = cell + b * max_det;
            for (int r = 0; r < max_det; ++r) {
                const bool on = r < n;
                const DetCand<T> *p = on ? &cand[kept[r]] : nullptr;
                d[3 * r] = on ? p->x : T(0);
                d[3 * r + 1] = on ? p->y : T(0);
                d[3 * r + 2] = on ? p->score : T(0);
                c[r] = on ? p->idx : 0;
            }
        }
    });
    return 0;
}

template <typename T> int distance_nms_host(const T *points, const T *scores, int n, double dist_thres, int top_k, int64_t *keep, int32_t *count)
{
    if (!points || !scores || !keep || !count || n < 1) return 1;
    std::vector<DetCand<T>> cand(n);
    for (int j = 0; j < n; ++j) cand[j] = DetCand<T>{scores[j] + T(0), points[2 * (int64_t)j], points[2 * (int64_t)j + 1], j};
    std::vector<int> kept;
    const int m = nms_host(cand, T(dist_thres), top_k, kept);
    for (int r = 0; r < n; ++r) keep[r] = r < m ? cand[kept[r]].idx : 0;
    count[0] = m;
    return 0;
}

}  // namespace

extern "C" {

#define MVDETR_DETECT_HOST_ENTRIES(T, SFX)                                                                                       \
    int mvdetr_detect_forward_host_##SFX(const T *heatmap, const int64_t *heatmap_stride, const T *offset, const int64_t *offset_stride, \
                                         int batch, int height, int width, double reduce, double cls_thres, double dist_thres,  \
                                         int top_k, int swap_xy, int max_det, T *det, int32_t *cell, int32_t *count)             \
    {                                                                                                                           \
        return detect_host<T>(heatmap, heatmap_stride, offset, offset_stride, batch, height, width, reduce, cls_thres,           \
                              dist_thres, top_k, swap_xy, max_det, det, cell, count);                                            \
    }                                                                                                                           \
    int mvdetr_distance_nms_host_##SFX(const T *points, const T *scores, int n, double dist_thres, int top_k, int64_t *keep,      \
                                       int32_t *count)                                                                           \
    {                                                                                                                           \
        return distance_nms_host<T>(points, scores, n, dist_thres, top_k, keep, count);                                          \
    }
MVDETR_DETECT_HOST_ENTRIES(float, f32)
MVDETR_DETECT_HOST_ENTRIES(double, f64)

}  // extern "C"

// ---- peak extraction (csrc/peak_detect.hip's contract on host memory) ---------------------------------------------------------
// The reference's ctdet_decode (utils/decode.py:7-77) for single-channel maps, one thread per map: scores once into a plane, a
// cell is a candidate when no neighbour inside the map has a greater score (a NaN is never one and is ignored as a neighbour),
// the candidates are sorted by (score, cell) descending -- the library's tie rule -- and the first top_k written.  Every product,
// sum and difference of the box is a separate rounding (baseline x86-64: nothing to contract into).
namespace {

template <typename T>
int peak_detect_host(const T *hm, const int64_t *hs, const T *off, const int64_t *os, const T *wh, const int64_t *ws, int B, int H, int W,
                     int top_k, double cls_thres, int use_thres, double scale_in, T *xy, T *wh_out, T *box, T *score, int32_t *cell,
                     int32_t *count)
{
    if (!hm || !hs || (off && !os) || (wh && (!ws || !wh_out || !box)) || !xy || !score || !cell || !count || B < 1 || H < 1 || W < 1 ||
        top_k < 1 || top_k > 1024 || (int64_t)H * W > ((int64_t)1 << 30))
        return 1;
    const T thres = T(cls_thres), scale = T(scale_in);
    parallel_ranges(B, [=](int64_t b0, int64_t b1) {
        std::vector<T> s((size_t)H * W);
        std::vector<std::pair<T, int>> cand;
        for (int64_t b = b0; b < b1; ++b) {
            for (int row = 0; row < H; ++row)
                for (int col = 0; col < W; ++col)
                    s[(size_t)row * W + col] = T(1) / (T(1) + std::exp(-hm[b * hs[0] + row * hs[2] + col * hs[3]]));
            cand.clear();
            for (int row = 0; row < H; ++row)
                for (int col = 0; col < W; ++col) {
                    const T v = s[(size_t)row * W + col];
                    bool ok = v == v && (!use_thres || v > thres);
                    for (int dr = -1; dr <= 1 && ok; ++dr)
                        for (int dc = -1; dc <= 1 && ok; ++dc)
                            if (row + dr >= 0 && row + dr < H && col + dc >= 0 && col + dc < W)
                                ok = !(s[(size_t)(row + dr) * W + col + dc] > v);
                    if (ok) cand.emplace_back(v + T(0), row * W + col);
                }
            const int n = (int)cand.size(), m = std::min(n, top_k);
            std::partial_sort(cand.begin(), cand.begin() + m, cand.end(), [](const std::pair<T, int> &a, const std::pair<T, int> &c) {
                return a.first > c.first || (a.first == c.first && a.second > c.second);
            });
            count[b] = n;
            for (int r = 0; r < top_k; ++r) {
                const int64_t at = b * top_k + r;
                T x = T(0), y = T(0), w = T(0), h = T(0), x1 = T(0), y1 = T(0), x2 = T(0), y2 = T(0);
                if (r < m) {
                    const int c = cand[r].second, row = c / W, col = c - row * W;
                    T dx = T(0.5), dy = T(0.5);
                    if (off) {
                        const T *o = off + b * os[0] + row * os[2] + col * os[3];
                        dx = o[0];
                        dy = o[os[1]];
                    }
                    x = T(col) + dx;
                    y = T(row) + dy;
                    if (wh) {
                        const T *p = wh + b * ws[0] + row * ws[2] + col * ws[3];
                        w = p[0];
                        h = p[ws[1]];
                        const T half = T(0.5) * w, xl = x - half, yt = y - h, xr = x + half;
                        x1 = xl * scale;
                        y1 = yt * scale;
                        x2 = xr * scale;
                        y2 = y * scale;
                    }
                }
                xy[2 * at] = x;
                xy[2 * at + 1] = y;
                score[at] = r < m ? cand[r].first : T(0);
                cell[at] = r < m ? cand[r].second : 0;
                if (wh) {
                    wh_out[2 * at] = w;
                    wh_out[2 * at + 1] = h;
                    box[4 * at] = x1;
                    box[4 * at + 1] = y1;
                    box[4 * at + 2] = x2;
                    box[4 * at + 3] = y2;
                }
            }
        }
    });
    return 0;
}

}  // namespace

extern "C" {

#define MVDETR_PEAK_HOST_ENTRY(T, SFX)                                                                                            \
    int mvdetr_peak_detect_forward_host_##SFX(const T *heatmap, const int64_t *heatmap_stride, const T *offset,                    \
                                              const int64_t *offset_stride, const T *wh, const int64_t *wh_stride, int batch,      \
                                              int height, int width, int top_k, double cls_thres, int use_thres, double scale,     \
                                              T *xy, T *wh_out, T *box, T *score, int32_t *cell, int32_t *count)                   \
    {                                                                                                                            \
        return peak_detect_host<T>(heatmap, heatmap_stride, offset, offset_stride, wh, wh_stride, batch, height, width, top_k,     \
                                   cls_thres, use_thres, scale, xy, wh_out, box, score, cell, count);                              \
    }
MVDETR_PEAK_HOST_ENTRY(float, f32)
MVDETR_PEAK_HOST_ENTRY(double, f64)

}  // extern "C"

// ---- frame ingest ----------------------------------------------------------------------------------------------------------
// uint8 frames -> normalised, resized (and optionally perspective-augmented) float images: the contract of mvdetr_ingest_frames_*
// in include/mvdetr_ops.h.  Resize taps come from integers (floor and remainder of ((2i + 1) src - dst) / (2 dst)), the
// augmentation's source positions from an fp64 inverse; the blend runs in T on grey levels and ends with one multiply-add.
namespace {

template <typename T> inline void resize_tap_host(int i, int src, int dst, int &i0, T &lam)
{
    const int64_t num = (int64_t)(2 * i + 1) * src - dst, den = 2 * (int64_t)dst;
    if (num <= 0) {
        i0 = 0;
        lam = T(0);
        return;
    }
    i0 = (int)(num / den);
    lam = (T)(num - i0 * den) / (T)den;
}

template <typename T> inline T blend4_host(T p00, T p01, T p10, T p11, T wx, T wy)
{
    const T top = std::fma(wx, p01 - p00, p00), bot = std::fma(wx, p11 - p10, p10);
    return std::fma(wy, bot - top, top);
}

template <typename T>
inline void augmented_pixel_host(const uint8_t *frame, int64_t row_stride, int Hs, int Ws, const double *inv, bool inv_ok, T border, int xx,
                                 int yy, T *A)
{
    A[0] = A[1] = A[2] = border;
    const double u = inv[0] * xx + inv[1] * yy + inv[2], t = inv[3] * xx + inv[4] * yy + inv[5], w = inv[6] * xx + inv[7] * yy + inv[8];
    if (!inv_ok || !(w > 0.0)) return;
    const double px = u / w, py = t / w;
    if (!(px > -1.0 && px < (double)Ws && py > -1.0 && py < (double)Hs)) return;
    const double fx = std::floor(px), fy = std::floor(py);
    const T lx = (T)(px - fx), ly = (T)(py - fy);
    const int x0 = (int)fx, y0 = (int)fy;
    const bool vx0 = x0 >= 0, vx1 = x0 + 1 < Ws, vy0 = y0 >= 0, vy1 = y0 + 1 < Hs;
    const uint8_t *r0 = frame + (int64_t)std::max(y0, 0) * row_stride, *r1 = frame + (int64_t)std::min(y0 + 1, Hs - 1) * row_stride;
    const int c0 = std::max(x0, 0) * 3, c1 = std::min(x0 + 1, Ws - 1) * 3;
    for (int c = 0; c < 3; ++c)
        A[c] = blend4_host<T>(vy0 && vx0 ? (T)r0[c0 + c] : border, vy0 && vx1 ? (T)r0[c1 + c] : border,
                              vy1 && vx0 ? (T)r1[c0 + c] : border, vy1 && vx1 ? (T)r1[c1 + c] : border, lx, ly);
}

template <typename T>
int ingest_host(const uint8_t *frames, int64_t frame_stride, int64_t row_stride, const double *mats, const double *a_in, const double *b_in,
                int K, int Hs, int Ws, int Ho, int Wo, int nhwc, double border_in, T *out)
{
    if (K < 0 || Hs < 1 || Ws < 1 || Ho < 1 || Wo < 1 || Hs > 16384 || Ws > 16384 || Ho > 16384 || Wo > 16384 || K > 65535 ||
        row_stride < (int64_t)Ws * 3 || frame_stride < 0 || (K > 0 && (!frames || !out)))
        return 1;
    const T a[3] = {(T)a_in[0], (T)a_in[1], (T)a_in[2]}, b[3] = {(T)b_in[0], (T)b_in[1], (T)b_in[2]}, border = (T)border_in;
    std::vector<double> inv((size_t)K * 9, 0.0);
    std::vector<char> good(K, 0);
    if (mats)
        for (int k = 0; k < K; ++k) {
            good[k] = invert3(mats + (size_t)k * 9, &inv[(size_t)k * 9]);
            for (int i = 0; i < 9; ++i) good[k] = good[k] && std::isfinite(inv[(size_t)k * 9 + i]);
        }
    const double *invp = inv.data();
    const char *goodp = good.data();
    parallel_ranges((int64_t)K * Ho, [=](int64_t first, int64_t last) {
        for (int64_t u = first; u < last; ++u) {
            const int k = (int)(u / Ho), y = (int)(u % Ho);
            const uint8_t *frame = frames + (int64_t)k * frame_stride;
            int y0;
            T wy;
            resize_tap_host<T>(y, Hs, Ho, y0, wy);
            const int y1 = std::min(y0 + 1, Hs - 1);
            for (int x = 0; x < Wo; ++x) {
                int x0;
                T wx;
                resize_tap_host<T>(x, Ws, Wo, x0, wx);
                const int x1 = std::min(x0 + 1, Ws - 1);
                T A[4][3];
                if (mats) {
                    const double *iv = invp + (size_t)k * 9;
                    augmented_pixel_host<T>(frame, row_stride, Hs, Ws, iv, goodp[k], border, x0, y0, A[0]);
                    augmented_pixel_host<T>(frame, row_stride, Hs, Ws, iv, goodp[k], border, x1, y0, A[1]);
                    augmented_pixel_host<T>(frame, row_stride, Hs, Ws, iv, goodp[k], border, x0, y1, A[2]);
                    augmented_pixel_host<T>(frame, row_stride, Hs, Ws, iv, goodp[k], border, x1, y1, A[3]);
                } else {
                    const uint8_t *r0 = frame + (int64_t)y0 * row_stride, *r1 = frame + (int64_t)y1 * row_stride;
                    for (int c = 0; c < 3; ++c) {
                        A[0][c] = (T)r0[x0 * 3 + c];
                        A[1][c] = (T)r0[x1 * 3 + c];
                        A[2][c] = (T)r1[x0 * 3 + c];
                        A[3][c] = (T)r1[x1 * 3 + c];
                    }
                }
                for (int c = 0; c < 3; ++c) {
                    const T v = std::fma(blend4_host<T>(A[0][c], A[1][c], A[2][c], A[3][c], wx, wy), a[c], b[c]);
                    const int64_t at = nhwc ? (((int64_t)k * Ho + y) * Wo + x) * 3 + c : (((int64_t)k * 3 + c) * Ho + y) * Wo + x;
                    out[at] = v;
                }
            }
        }
    });
    return 0;
}

}  // namespace

extern "C" {

int mvdetr_ingest_frames_host_f32(const uint8_t *frames, int64_t frame_stride, int64_t row_stride, const double *mats, double a0,
                                  double a1, double a2, double b0, double b1, double b2, int k, int src_h, int src_w, int dst_h,
                                  int dst_w, int layout_nhwc, double border, float *out)
{
    const double a[3] = {a0, a1, a2}, b[3] = {b0, b1, b2};
    return ingest_host<float>(frames, frame_stride, row_stride, mats, a, b, k, src_h, src_w, dst_h, dst_w, layout_nhwc, border, out);
}
int mvdetr_ingest_frames_host_f64(const uint8_t *frames, int64_t frame_stride, int64_t row_stride, const double *mats, double a0,
                                  double a1, double a2, double b0, double b1, double b2, int k, int src_h, int src_w, int dst_h,
                                  int dst_w, int layout_nhwc, double border, double *out)
{
    const double a[3] = {a0, a1, a2}, b[3] = {b0, b1, b2};
    return ingest_host<double>(frames, frame_stride, row_stride, mats, a, b, k, src_h, src_w, dst_h, dst_w, layout_nhwc, border, out);
}

}  // extern "C"

// ---- training targets ------------------------------------------------------------------------------------------------------
// The host twin of frame_targets.hip: the contract of mvdetr_frame_targets_* on host memory, the per-object arithmetic shared
// with the kernel (frame_targets_core.h; this file is built with -ffp-contract=off).  Threads own maps for the slot lists, then
// rows of the heat maps.
extern "C" {

int mvdetr_frame_targets_host_f64(const double *coords, int is_boxes, const int32_t *count, const int64_t *pids, const double *mats,
                                  const double *shrink, const uint8_t *keep, const float *patch, int maps, int cap, int height,
                                  int width, int img_h, int img_w, int radius, int top_k, double reduce, float *heatmap,
                                  uint8_t *reg_mask, int64_t *idx, int64_t *pid, float *offset, float *wh)
{
    if (maps < 0 || maps > 65535 || cap < 1 || cap > MVDETR_FT_MAX_CAP || top_k < cap || height < 1 || width < 1 ||
        height > MVDETR_FT_MAX_DIM || width > MVDETR_FT_MAX_DIM || radius < 0 || radius > MVDETR_FT_MAX_RADIUS || !(reduce > 0.0))
        return 1;
    if ((!is_boxes && (mats || wh)) || (is_boxes && !wh) || (!mats && shrink) || (mats && (img_h < 1 || img_w < 1))) return 1;
    if (maps == 0) return 0;
    if (!coords || !count || !patch || !heatmap || !reg_mask || !idx || !pid || !offset) return 1;
    const int H = height, W = width, r = radius, side = 2 * r + 1;
    std::vector<int> centres((size_t)maps * cap * 2), filled(maps);          // per map: (cx, cy) of its slots, cx = -1: empty
    parallel_ranges(maps, [&](int64_t m0, int64_t m1) {
        for (int64_t m = m0; m < m1; ++m) {
            int n = std::min(std::max(count[m], 0), cap), used = 0;
            if (keep && !keep[m]) n = 0;
            int *cen = centres.data() + m * cap * 2;
            for (int i = 0; i < n; ++i) {
                const int64_t at = m * cap + i;
                double x, y, w = 0, h = 0;
                if (is_boxes) {
                    double b[4] = {coords[at * 4], coords[at * 4 + 1], coords[at * 4 + 2], coords[at * 4 + 3]};
                    if (mats && !ft_move_box(b, mats + m * 9, shrink ? shrink[m] : 1.0, (double)(img_w - 1), (double)(img_h - 1), b))
                        continue;
                    x = (b[0] + b[2]) / 2, y = b[3], w = b[2] - b[0], h = b[3] - b[1];
                } else {
                    x = coords[at * 2], y = coords[at * 2 + 1];
                }
                const FtSlot s = ft_slot(x, y, w, h, reduce, H, W);
                const int64_t o = m * top_k + used;
                cen[used * 2] = s.inside ? s.cx : -1;
                cen[used * 2 + 1] = s.cy;
                reg_mask[o] = s.inside ? 1 : 0;
                idx[o] = s.inside ? (int64_t)s.cy * W + s.cx : 0;
                pid[o] = s.inside && pids ? pids[at] : 0;
                offset[o * 2] = s.off_x, offset[o * 2 + 1] = s.off_y;
                if (wh) wh[o * 2] = s.wh_x, wh[o * 2 + 1] = s.wh_y;
                ++used;
            }
            for (int64_t o = m * top_k + used; o < (m + 1) * top_k; ++o) {
                reg_mask[o] = 0, idx[o] = 0, pid[o] = 0;
                offset[o * 2] = offset[o * 2 + 1] = 0.f;
                if (wh) wh[o * 2] = wh[o * 2 + 1] = 0.f;
            }
            filled[m] = used;
        }
    });
    parallel_ranges((int64_t)maps * H, [&](int64_t r0, int64_t r1) {
        for (int64_t row = r0; row < r1; ++row) {
            const int64_t m = row / H;
            const int y = (int)(row - m * H);
            float *out = heatmap + row * W;
            std::fill(out, out + W, 0.f);
            const int *cen = centres.data() + m * cap * 2;
            for (int s = 0; s < filled[m]; ++s) {
                const int cx = cen[s * 2], dy = y - cen[s * 2 + 1];
                if (cx < 0 || dy < -r || dy > r) continue;
                const float *p = patch + (dy + r) * side;
                for (int x = std::max(cx - r, 0); x <= std::min(cx + r, W - 1); ++x) out[x] = std::max(out[x], p[x - cx + r]);
            }
        }
    });
    return 0;
}

}  // extern "C"

// Frame ingest on the device: uint8 camera frames [K, Hs, Ws, 3] -> the trunk's normalised input [K, 3, Ho, Wo] (fp32 / fp16 /
// bf16; channels-last or NCHW) in ONE pass: optional perspective augmentation (cv2.warpPerspective's convention, constant border),
// ToTensor (/255), Normalize ((v - mean) / std) and the bilinear resize (F.interpolate, align_corners=False, no antialias) of the
// reference's dataset (multiview_detector/datasets/frameDataset.py:66-67,199-206; utils/image_utils.py:43).
//
// Arithmetic (include/mvdetr_ops.h has the contract):
//   * resize taps from INTEGERS: source position of output column x is ((2x + 1) Ws - Wo) / (2 Wo); its floor and remainder are an
//     integer division, the weight is remainder / (2 Wo), one rounded fp32 division of two exact numbers.  No fp32 position is formed.
//   * the blend runs on grey levels in fp32 (differences of two grey levels are exact) and the normalisation is one FMA at the
//     end, v * a_c + b_c with a_c = 1 / (255 std_c), b_c = -mean_c / std_c: the resize weights sum to 1, so this is the same value.
//   * the augmented image is never rounded to uint8: with a matrix, each of the 4 resize taps is itself a bilinear blend of 4
//     frame pixels around M^-1 (xx, yy, 1) (inverse, product and division in fp64), taps outside the frame = the border grey level.
//   * 16-bit outputs round once, on the store.
//
// Kernels.  A workgroup of 256 threads owns an output tile 128 columns wide; a lane produces PX adjacent pixels of one row (PX = 4
// for fp32, 8 for the 16-bit types: 48 bytes of channels-last output = three 16-byte stores, or one 16-byte store per NCHW plane).
//   ingest_identity_wide    no matrix.  The band of source rows / columns the tile needs is staged in LDS with aligned 16-byte loads
//                           (frame base, frame stride and row stride all multiples of 16; a chunk that would reach past the row's
//                           last byte is read byte by byte), then every tap is an LDS byte read.
//   ingest_identity_narrow  the same with byte loads (any base / strides: cropped views, odd row pitches).
//   ingest_identity_direct  no LDS: taps read from global memory.  Taken when the band of a tile does not fit 64 KiB of LDS
//                           (downscales beyond about 3x).
//   ingest_warp             with a matrix: 16 byte-triple gathers per output pixel straight from global memory (an affine
//                           footprint is compact and lives in L2).
// Stores are 16 bytes wide when `out` and its row pitch are 16-byte aligned and the lane's PX pixels are all inside the image;
// element by element otherwise.  Nothing here allocates or synchronises.
#include "common.h"
#include "half_types.h"
#include "../../include/mvdetr_ops.h"

#include <algorithm>
#include <atomic>

namespace mvdetr {

constexpr int ING_THREADS = 256;
constexpr int ING_TW = 128;                    // output columns per workgroup
constexpr int ING_LDS_MAX = 64 * 1024;
constexpr int ING_MAX_DIM = 16384;             // (2x + 1) * size stays far inside int32
enum { ING_DIRECT = 0, ING_NARROW = 1, ING_WIDE = 2 };

static std::atomic<const char *> g_ingest_last_kernel{"none"};

struct IngestArgs {
    const uint8_t *frames;
    int64_t frame_stride, row_stride;          // bytes
    const double *M;                           // [K, 9] destination <- source, or null
    float a[3], b[3];
    int K, Hs, Ws, Ho, Wo;
    int nhwc, wide_store;
    float border;
    int band_rows, pitch;                      // LDS band of the staged routes: rows and bytes per row (multiple of 16)
};

struct OutF32 {
    using T = float;
    static constexpr int PX = 4;
    static __device__ __forceinline__ float down(float f) { return f; }
};
template <typename C> struct OutHalf {
    using T = uint16_t;
    static constexpr int PX = 8;
    static __device__ __forceinline__ uint16_t down(float f) { return C::down(f); }
};

// floor and fraction of the bilinear resize's source position of output index i (size `src` -> `dst`), clamped below at 0
__device__ __forceinline__ void resize_tap(int i, int src, int dst, int &i0, float &lam)
{
    const int num = (2 * i + 1) * src - dst, den = 2 * dst;
    if (num <= 0) {
        i0 = 0;
        lam = 0.f;
        return;
    }
    i0 = num / den;
    lam = (float)(num - i0 * den) / (float)den;
}

__device__ __forceinline__ float blend4(float p00, float p01, float p10, float p11, float wx, float wy)
{
    const float top = fmaf(wx, p01 - p00, p00), bot = fmaf(wx, p11 - p10, p10);
    return fmaf(wy, bot - top, top);
}

// v[p][c], p < PX pixels from column x of row y of image k -> out
template <typename O>
__device__ __forceinline__ void store_pixels(const IngestArgs &g, typename O::T *out, int k, int y, int x, const float (&v)[O::PX][3])
{
    constexpr int PX = O::PX;
    using T = typename O::T;
    const bool full = g.wide_store && x + PX <= g.Wo;
    if (g.nhwc) {
        T *p = out + (((int64_t)k * g.Ho + y) * g.Wo + x) * 3;
        if (full) {
            if constexpr (sizeof(T) == 4) {
                float4 *q = reinterpret_cast<float4 *>(p);
                q[0] = make_float4(v[0][0], v[0][1], v[0][2], v[1][0]);
                q[1] = make_float4(v[1][1], v[1][2], v[2][0], v[2][1]);
                q[2] = make_float4(v[2][2], v[3][0], v[3][1], v[3][2]);
            } else {
                uint4 *q = reinterpret_cast<uint4 *>(p);
                uint32_t w[12];
#pragma unroll
                for (int i = 0; i < 12; ++i)
                    w[i] = (uint32_t)O::down(v[(2 * i) / 3][(2 * i) % 3]) | ((uint32_t)O::down(v[(2 * i + 1) / 3][(2 * i + 1) % 3]) << 16);
                q[0] = make_uint4(w[0], w[1], w[2], w[3]);
                q[1] = make_uint4(w[4], w[5], w[6], w[7]);
                q[2] = make_uint4(w[8], w[9], w[10], w[11]);
            }
        } else {
#pragma unroll
            for (int i = 0; i < PX; ++i)
                if (x + i < g.Wo) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) p[i * 3 + c] = O::down(v[i][c]);
                }
        }
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            T *p = out + (((int64_t)k * 3 + c) * g.Ho + y) * g.Wo + x;
            if (full) {
                if constexpr (sizeof(T) == 4) {
                    *reinterpret_cast<float4 *>(p) = make_float4(v[0][c], v[1][c], v[2][c], v[3][c]);
                } else {
                    uint32_t w[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) w[i] = (uint32_t)O::down(v[2 * i][c]) | ((uint32_t)O::down(v[2 * i + 1][c]) << 16);
                    *reinterpret_cast<uint4 *>(p) = make_uint4(w[0], w[1], w[2], w[3]);
                }
            } else {
#pragma unroll
                for (int i = 0; i < PX; ++i)
                    if (x + i < g.Wo) p[i] = O::down(v[i][c]);
            }
        }
    }
}

template <typename O, int STAGE> __global__ __launch_bounds__(ING_THREADS) void ingest_identity(IngestArgs g, typename O::T *out)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t ing_band[];
    constexpr int PX = O::PX, LANES_X = ING_TW / PX, TH = ING_THREADS / LANES_X;
    const int k = blockIdx.z, ty0 = blockIdx.y * TH, tx0 = blockIdx.x * ING_TW;
    const int lane_x = threadIdx.x % LANES_X, lane_y = threadIdx.x / LANES_X;
    const uint8_t *frame = g.frames + (int64_t)k * g.frame_stride;

    int band_y0 = 0, band_b0 = 0;              // first staged source row; first staged byte of a row
    if constexpr (STAGE != ING_DIRECT) {
        float unused;
        int band_y1, x_first, x_last;
        resize_tap(ty0, g.Hs, g.Ho, band_y0, unused);
        resize_tap(min(ty0 + TH, g.Ho) - 1, g.Hs, g.Ho, band_y1, unused);
        band_y1 = min(band_y1 + 1, g.Hs - 1);
        resize_tap(tx0, g.Ws, g.Wo, x_first, unused);
        resize_tap(min(tx0 + ING_TW, g.Wo) - 1, g.Ws, g.Wo, x_last, unused);
        x_last = min(x_last + 1, g.Ws - 1);
        const int rows = min(band_y1 - band_y0 + 1, g.band_rows);
        const int row_bytes = g.Ws * 3, b1 = (x_last + 1) * 3;
        if constexpr (STAGE == ING_WIDE) {
            band_b0 = (x_first * 3) & ~15;
            const int chunks = min((b1 - band_b0 + 15) >> 4, g.pitch >> 4);
            for (int i = threadIdx.x; i < rows * chunks; i += ING_THREADS) {
                const int r = i / chunks, j = i - r * chunks, at = band_b0 + 16 * j;
                const uint8_t *src = frame + (int64_t)(band_y0 + r) * g.row_stride + at;
                uint8_t *dst = ing_band + r * g.pitch + 16 * j;
                if (at + 16 <= row_bytes) {
                    *reinterpret_cast<uint4 *>(dst) = *reinterpret_cast<const uint4 *>(src);
                } else {
                    for (int t = 0; t < 16 && at + t < row_bytes; ++t) dst[t] = src[t];
                }
            }
        } else {
            band_b0 = x_first * 3;
            const int n = min(b1 - band_b0, g.pitch);
            for (int i = threadIdx.x; i < rows * n; i += ING_THREADS) {
                const int r = i / n, j = i - r * n;
                ing_band[r * g.pitch + j] = frame[(int64_t)(band_y0 + r) * g.row_stride + band_b0 + j];
            }
        }
        __syncthreads();
    }

    const int y = ty0 + lane_y, x = tx0 + lane_x * PX;
    if (y >= g.Ho || x >= g.Wo) return;
    int y0;
    float wy;
    resize_tap(y, g.Hs, g.Ho, y0, wy);
    const int y1 = min(y0 + 1, g.Hs - 1);
    float v[PX][3];
#pragma unroll
    for (int p = 0; p < PX; ++p) {
        int x0;
        float wx;
        resize_tap(min(x + p, g.Wo - 1), g.Ws, g.Wo, x0, wx);
        const int x1 = min(x0 + 1, g.Ws - 1);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float p00, p01, p10, p11;
            if constexpr (STAGE != ING_DIRECT) {
                const int r0 = (y0 - band_y0) * g.pitch - band_b0 + c, r1 = (y1 - band_y0) * g.pitch - band_b0 + c;
                p00 = (float)ing_band[r0 + x0 * 3];
                p01 = (float)ing_band[r0 + x1 * 3];
                p10 = (float)ing_band[r1 + x0 * 3];
                p11 = (float)ing_band[r1 + x1 * 3];
            } else {
                const uint8_t *r0 = frame + (int64_t)y0 * g.row_stride + c, *r1 = frame + (int64_t)y1 * g.row_stride + c;
                p00 = (float)r0[x0 * 3];
                p01 = (float)r0[x1 * 3];
                p10 = (float)r1[x0 * 3];
                p11 = (float)r1[x1 * 3];
            }
            v[p][c] = fmaf(blend4(p00, p01, p10, p11, wx, wy), g.a[c], g.b[c]);
        }
    }
    store_pixels<O>(g, out, k, y, x, v);
}

// The augmented image at integer position (xx, yy): the bilinear blend of the four frame pixels around M^-1 (xx, yy, 1), taps
// outside the frame = border; all border where the position is behind the camera (w <= 0) or not finite.
__device__ __forceinline__ void augmented_pixel(const IngestArgs &g, const uint8_t *frame, const double (&inv)[9], bool inv_ok, int xx,
                                                int yy, float (&A)[3])
{
    A[0] = A[1] = A[2] = g.border;
    const double u = fma(inv[0], (double)xx, fma(inv[1], (double)yy, inv[2]));
    const double t = fma(inv[3], (double)xx, fma(inv[4], (double)yy, inv[5]));
    const double w = fma(inv[6], (double)xx, fma(inv[7], (double)yy, inv[8]));
    if (!inv_ok || !(w > 0.0)) return;
    const double rw = 1.0 / w, px = u * rw, py = t * rw;
    if (!(px > -1.0 && px < (double)g.Ws && py > -1.0 && py < (double)g.Hs)) return;          // (NaN and inf fail too)
    const double fx = floor(px), fy = floor(py);
    const float lx = (float)(px - fx), ly = (float)(py - fy);
    const int x0 = (int)fx, y0 = (int)fy;
    const bool vx0 = x0 >= 0, vx1 = x0 + 1 < g.Ws, vy0 = y0 >= 0, vy1 = y0 + 1 < g.Hs;
    const uint8_t *r0 = frame + (int64_t)max(y0, 0) * g.row_stride, *r1 = frame + (int64_t)min(y0 + 1, g.Hs - 1) * g.row_stride;
    const int c0 = max(x0, 0) * 3, c1 = min(x0 + 1, g.Ws - 1) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float q00 = (float)r0[c0 + c], q01 = (float)r0[c1 + c], q10 = (float)r1[c0 + c], q11 = (float)r1[c1 + c];
        A[c] = blend4(vy0 && vx0 ? q00 : g.border, vy0 && vx1 ? q01 : g.border, vy1 && vx0 ? q10 : g.border,
                      vy1 && vx1 ? q11 : g.border, lx, ly);
    }
}

template <typename O> __global__ __launch_bounds__(ING_THREADS) void ingest_warp(IngestArgs g, typename O::T *out)
{
    constexpr int PX = O::PX, LANES_X = ING_TW / PX, TH = ING_THREADS / LANES_X;
    const int k = blockIdx.z;
    const int y = blockIdx.y * TH + threadIdx.x / LANES_X, x = blockIdx.x * ING_TW + (threadIdx.x % LANES_X) * PX;
    if (y >= g.Ho || x >= g.Wo) return;
    const uint8_t *frame = g.frames + (int64_t)k * g.frame_stride;
    // true inverse of the destination <- source matrix, fp64 (adjugate / determinant)
    const double *m = g.M + (int64_t)k * 9;
    const double m0 = m[0], m1 = m[1], m2 = m[2], m3 = m[3], m4 = m[4], m5 = m[5], m6 = m[6], m7 = m[7], m8 = m[8];
    const double c00 = m4 * m8 - m5 * m7, c01 = m5 * m6 - m3 * m8, c02 = m3 * m7 - m4 * m6;
    const double rdet = 1.0 / (m0 * c00 + m1 * c01 + m2 * c02);
    const double inv[9] = {c00 * rdet, (m2 * m7 - m1 * m8) * rdet, (m1 * m5 - m2 * m4) * rdet,
                           c01 * rdet, (m0 * m8 - m2 * m6) * rdet, (m2 * m3 - m0 * m5) * rdet,
                           c02 * rdet, (m1 * m6 - m0 * m7) * rdet, (m0 * m4 - m1 * m3) * rdet};
    bool inv_ok = true;
#pragma unroll
    for (int i = 0; i < 9; ++i) inv_ok = inv_ok && isfinite(inv[i]);

    int y0;
    float wy;
    resize_tap(y, g.Hs, g.Ho, y0, wy);
    const int y1 = min(y0 + 1, g.Hs - 1);
    float v[PX][3];
#pragma unroll
    for (int p = 0; p < PX; ++p) {
        int x0;
        float wx;
        resize_tap(min(x + p, g.Wo - 1), g.Ws, g.Wo, x0, wx);
        const int x1 = min(x0 + 1, g.Ws - 1);
        float A00[3], A01[3], A10[3], A11[3];
        augmented_pixel(g, frame, inv, inv_ok, x0, y0, A00);
        augmented_pixel(g, frame, inv, inv_ok, x1, y0, A01);
        augmented_pixel(g, frame, inv, inv_ok, x0, y1, A10);
        augmented_pixel(g, frame, inv, inv_ok, x1, y1, A11);
#pragma unroll
        for (int c = 0; c < 3; ++c) v[p][c] = fmaf(blend4(A00[c], A01[c], A10[c], A11[c], wx, wy), g.a[c], g.b[c]);
    }
    store_pixels<O>(g, out, k, y, x, v);
}

template <typename O>
static int ingest_launch(void *stream, const uint8_t *frames, int64_t frame_stride, int64_t row_stride, const double *M, float a0, float a1,
                         float a2, float b0, float b1, float b2, int K, int Hs, int Ws, int Ho, int Wo, int layout_nhwc, float border,
                         typename O::T *out)
{
    using T = typename O::T;
    if (K < 0 || Hs < 1 || Ws < 1 || Ho < 1 || Wo < 1 || Hs > ING_MAX_DIM || Ws > ING_MAX_DIM || Ho > ING_MAX_DIM || Wo > ING_MAX_DIM ||
        K > 65535 || row_stride < (int64_t)Ws * 3 || frame_stride < 0 || (K > 0 && (!frames || !out)))
        return 1;
    if (K == 0) return 0;
    constexpr int PX = O::PX, TH = ING_THREADS / (ING_TW / PX);
    IngestArgs g;
    g.frames = frames;
    g.frame_stride = frame_stride;
    g.row_stride = row_stride;
    g.M = M;
    g.a[0] = a0, g.a[1] = a1, g.a[2] = a2;
    g.b[0] = b0, g.b[1] = b1, g.b[2] = b2;
    g.K = K, g.Hs = Hs, g.Ws = Ws, g.Ho = Ho, g.Wo = Wo;
    g.nhwc = layout_nhwc ? 1 : 0;
    g.wide_store = aligned(out, 16) && ((int64_t)Wo * (g.nhwc ? 3 : 1) * (int64_t)sizeof(T)) % 16 == 0;
    g.border = border;
    g.band_rows = g.pitch = 0;
    const dim3 grid((unsigned)ceil_div(Wo, ING_TW), (unsigned)ceil_div(Ho, TH), (unsigned)K), block(ING_THREADS);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (M) {
        hipLaunchKernelGGL((ingest_warp<O>), grid, block, 0, st, g, out);
        g_ingest_last_kernel = "ingest_warp";
        return (int)hipGetLastError();
    }
    // the band of a tile.  The first tap of output i is floor(((2i + 1) S - D) / (2D)) (clamped at 0), so the first taps of outputs i and
    // i + n are at most floor(n S / D) + 1 apart (floor(a + b) - floor(a) <= floor(b) + 1); + 1 for the last output's second tap, + 1
    // to count both ends: n outputs touch at most floor((n - 1) S / D) + 3 source rows (columns).  The kernel clamps to it as well.
    const int64_t rows = std::min<int64_t>((int64_t)(TH - 1) * Hs / Ho + 3, Hs);
    const int64_t cols = std::min<int64_t>((int64_t)(ING_TW - 1) * Ws / Wo + 3, Ws);
    const int64_t pitch = (cols * 3 + 15 + 15) / 16 * 16;          // + up to 15 bytes in front of the first column (aligned loads)
    const int64_t lds = rows * pitch;
    if (lds > ING_LDS_MAX) {
        hipLaunchKernelGGL((ingest_identity<O, ING_DIRECT>), grid, block, 0, st, g, out);
        g_ingest_last_kernel = "ingest_identity_direct";
        return (int)hipGetLastError();
    }
    g.band_rows = (int)rows;
    g.pitch = (int)pitch;
    if (aligned(frames, 16) && frame_stride % 16 == 0 && row_stride % 16 == 0) {
        hipLaunchKernelGGL((ingest_identity<O, ING_WIDE>), grid, block, (size_t)lds, st, g, out);
        g_ingest_last_kernel = "ingest_identity_wide";
    } else {
        hipLaunchKernelGGL((ingest_identity<O, ING_NARROW>), grid, block, (size_t)lds, st, g, out);
        g_ingest_last_kernel = "ingest_identity_narrow";
    }
    return (int)hipGetLastError();
}

}  // namespace mvdetr

extern "C" {

int mvdetr_ingest_frames_f32(void *stream, const uint8_t *frames, int64_t frame_stride, int64_t row_stride, const double *M, float a0,
                             float a1, float a2, float b0, float b1, float b2, int K, int Hs, int Ws, int Ho, int Wo, int layout_nhwc,
                             float border, float *out)
{
    return mvdetr::ingest_launch<mvdetr::OutF32>(stream, frames, frame_stride, row_stride, M, a0, a1, a2, b0, b1, b2, K, Hs, Ws, Ho, Wo,
                                                 layout_nhwc, border, out);
}

int mvdetr_ingest_frames_f16(void *stream, const uint8_t *frames, int64_t frame_stride, int64_t row_stride, const double *M, float a0,
                             float a1, float a2, float b0, float b1, float b2, int K, int Hs, int Ws, int Ho, int Wo, int layout_nhwc,
                             float border, uint16_t *out)
{
    return mvdetr::ingest_launch<mvdetr::OutHalf<mvdetr::F16>>(stream, frames, frame_stride, row_stride, M, a0, a1, a2, b0, b1, b2, K, Hs,
                                                               Ws, Ho, Wo, layout_nhwc, border, out);
}

int mvdetr_ingest_frames_bf16(void *stream, const uint8_t *frames, int64_t frame_stride, int64_t row_stride, const double *M, float a0,
                              float a1, float a2, float b0, float b1, float b2, int K, int Hs, int Ws, int Ho, int Wo, int layout_nhwc,
                              float border, uint16_t *out)
{
    return mvdetr::ingest_launch<mvdetr::OutHalf<mvdetr::BF16>>(stream, frames, frame_stride, row_stride, M, a0, a1, a2, b0, b1, b2, K, Hs,
                                                                Ws, Ho, Wo, layout_nhwc, border, out);
}

const char *mvdetr_ingest_last_kernel(void) { return mvdetr::g_ingest_last_kernel.load(); }

}  // extern "C"

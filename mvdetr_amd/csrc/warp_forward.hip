// The perspective warp's forward kernels (fp32 / fp64, the fp32 LDS-patch kernel, the channel-last kernels, the two 16-bit
// kernels), the tiled transpose that prepares their layouts, and the launchers.  Which one a call runs: warp_route.h.
#include "half_types.h"
#include "warp_device.h"
#include "warp_launch.h"

namespace mvdetr {

template <typename T, bool NHWC>
__global__ __launch_bounds__(WARP_PIX *WARP_SUB) void warp_fwd(
    const T *__restrict__ src, const T *__restrict__ Mv, int N, int C, int h, int w, int H, int W,
    int nearest, T *__restrict__ dst)
{
    __shared__ float tile[NHWC && sizeof(T) == 4 ? WARP_PIX * (WARP_CH + 1) : 1];
    // the tile's geometry once per block, by its first wave (round 5: every wave used to run the fp64 inverse, the two
    // divisions and the footprint for its own copy of the 64 pixels -- ~300 instructions in front of 16 channels x 12)
    __shared__ WarpTexel<T> tex[WARP_PIX];
    const int lane = threadIdx.x & (WARP_PIX - 1);
    const int sub = threadIdx.x / WARP_PIX;
    WarpBlock wb;
    if (!warp_block(N, H, W, (C + WARP_CH - 1) / WARP_CH, wb)) return;
    const int n = wb.n, i = wb.i0 + lane / WARP_TW, j = wb.j0 + lane % WARP_TW;
    const int64_t pix = ((int64_t)n * H + i) * W + j;
    const int cbase = wb.group * WARP_CH;
    constexpr int CPT = WARP_CH / WARP_SUB;
    const bool live = i < H && j < W;
    if (sub == 0) tex[lane] = warp_texel(Mv + (int64_t)n * 9, i, j, h, w, live, nearest);
    __syncthreads();
    const WarpTexel<T> t = tex[lane];
    const bool v00 = t.valid & 1, v01 = t.valid & 2, v10 = t.valid & 4, v11 = t.valid & 8;
    const int64_t plane = (int64_t)h * w;
#pragma unroll 4
    for (int k = 0; k < CPT; ++k) {
        const int c = cbase + sub * CPT + k;
        T val = T(0);
        if (live && c < C && t.valid) {
            const T *sp = src + ((int64_t)n * C + c) * plane + t.o00;
            T a, b, cc, d;
            load_pair(sp, v00, v01, a, b);
            load_pair(sp + w, v10, v11, cc, d);
            val = t.w00 * a + t.w01 * b + t.w10 * cc + t.w11 * d;
        }
        if constexpr (!NHWC) {
            if (live && c < C) dst[(((int64_t)n * C + c) * H + i) * W + j] = val;
        } else if constexpr (sizeof(T) == 4) {
            tile[lane * (WARP_CH + 1) + sub * CPT + k] = (float)val;
        } else {
            if (live && c < C) dst[pix * C + c] = val;
        }
    }
    if constexpr (NHWC && sizeof(T) == 4) {
        __syncthreads();
        // 64 pixels x 64 channels -> rows of 64 consecutive channels per pixel
        const int ch = threadIdx.x & (WARP_CH - 1);
#pragma unroll 4
        for (int k = 0; k < WARP_PIX / WARP_SUB; ++k) {
            const int p = k * WARP_SUB + sub;
            const int pi = wb.i0 + p / WARP_TW, pj = wb.j0 + p % WARP_TW;
            if (pi < H && pj < W && cbase + ch < C)
                dst[(((int64_t)n * H + pi) * W + pj) * C + cbase + ch] = (T)tile[p * (WARP_CH + 1) + ch];
        }
    }
}

// ---- NCHW source -> NCHW destination through LDS source patches (fp32; round 5) -------------------------------------------
// warp_fwd<NCHW> issues one 8-byte gather per (pixel, channel, corner row): 1.2 M wave-level gathers at Wildtrack size, each
// touching 8 - 16 cache lines of which it uses a few bytes -- it runs at the rate of the texture-address / L1 pipeline (85 - 90 us,
// 30 % of the HBM roofline; computing the tile's fp64 geometry once per block instead of once per wave changed nothing).  The
// destination grid is denser than the source (360 x 120 from 160 x 90), so the pre-image of an 8 x 32 destination tile is a
// compact patch of ~8 x 16 texels per channel.  Here a workgroup = (8 x 32 tile, chunk of up to 32 channels): the four waves find
// the bounding box of their footprints, copy the patch rows of every channel of the chunk to LDS with LDS-DMA (16 bytes per lane,
// x aligned down to 4 texels: whole 64-byte row pieces, every byte of a fetched line used), and every lane blends its pixel's four
// corners from LDS -- four ds_read_b32, masked by the corner's validity (zero padding and mode='nearest' need no zero-filled
// border and multiply no unloaded value) -- and stores 128-byte rows.  The chunk shrinks with the patch (LDS budget / patch size);
// a tile whose patch would leave fewer than 4 channels per chunk (extreme magnification near the horizon) gathers from memory as
// warp_fwd does, in the same launch.
__global__ __launch_bounds__(256) void warp_fwd_nchw_patch(
    const float *__restrict__ src, const float *__restrict__ Mv, int N, int C, int h, int w, int H, int W,
    int nearest, float *__restrict__ dst)
{
    extern __shared__ __attribute__((aligned(16))) float patch[];       // [channel of the chunk][patch row][PWp]
    __shared__ int box[4][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tx = (W + WARP_PP_TW - 1) / WARP_PP_TW, ty = (H + WARP_PP_TH - 1) / WARP_PP_TH;
    const int groups = (C + WARP_PP_CH - 1) / WARP_PP_CH;
    int r = blockIdx.x;
    const int group = r % groups;
    r /= groups;
    const int j0 = (r % tx) * WARP_PP_TW;
    r /= tx;
    const int i0 = (r % ty) * WARP_PP_TH, n = r / ty;
    if (n >= N) return;
    const int i = i0 + tid / WARP_PP_TW, j = j0 + tid % WARP_PP_TW;
    const bool live = i < H && j < W;
    double sx = 0.0, sy = 0.0;
    if (live) source_position(Mv + (int64_t)n * 9, i, j, h, w, sx, sy);
    SrcCoord sc = make_coord(sx, sy, h, w, nearest);
    const bool use = live && sc.any;
    const bool v00 = use && sc.v00, v01 = use && sc.v01, v10 = use && sc.v10, v11 = use && sc.v11;
    const float w00 = (float)(sc.wy0 * sc.wx0), w01 = (float)(sc.wy0 * sc.wx1), w10 = (float)(sc.wy1 * sc.wx0), w11 = (float)(sc.wy1 * sc.wx1);

    // bounding box of the VALID corners (inside the image by construction)
    int xmin = 0x3fffffff, xmax = -0x3fffffff, ymin = 0x3fffffff, ymax = -0x3fffffff;
    if (v00 || v10) { xmin = min(xmin, sc.x0); xmax = max(xmax, sc.x0); }
    if (v01 || v11) { xmin = min(xmin, sc.x0 + 1); xmax = max(xmax, sc.x0 + 1); }
    if (v00 || v01) { ymin = min(ymin, sc.y0); ymax = max(ymax, sc.y0); }
    if (v10 || v11) { ymin = min(ymin, sc.y0 + 1); ymax = max(ymax, sc.y0 + 1); }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        xmin = min(xmin, __shfl_xor(xmin, o, 64));
        xmax = max(xmax, __shfl_xor(xmax, o, 64));
        ymin = min(ymin, __shfl_xor(ymin, o, 64));
        ymax = max(ymax, __shfl_xor(ymax, o, 64));
    }
    if (lane == 0) { box[wave][0] = xmin; box[wave][1] = xmax; box[wave][2] = ymin; box[wave][3] = ymax; }
    __syncthreads();
    xmin = min(min(box[0][0], box[1][0]), min(box[2][0], box[3][0]));
    xmax = max(max(box[0][1], box[1][1]), max(box[2][1], box[3][1]));
    ymin = min(min(box[0][2], box[1][2]), min(box[2][2], box[3][2]));
    ymax = max(max(box[0][3], box[1][3]), max(box[2][3], box[3][3]));

    const int c0 = group * WARP_PP_CH, cn = min(WARP_PP_CH, C - c0);
    const int64_t plane = (int64_t)h * w, oplane = (int64_t)H * W;
    float *const op = dst + ((int64_t)n * C + c0) * oplane + (int64_t)i * W + j;
    if (xmax < xmin) {
        // no pixel of the tile touches the source: zeros
        if (live)
            for (int c = 0; c < cn; ++c) op[c * oplane] = 0.f;
        return;
    }
    const int xs = xmin & ~3, PWp = ((xmax + 1 - xs) + 3) & ~3, PH = ymax - ymin + 1, PE = PH * PWp, Q = PWp >> 2;
    int chunk = WARP_PP_FLOATS / PE;
    chunk = chunk > cn ? cn : chunk;
    if (chunk < 4 && chunk < cn) {
        // the patch does not fit: per-lane gathers for this tile (warp_fwd's arithmetic)
        if (live) {
            const int64_t o00 = (int64_t)sc.y0 * w + sc.x0;
            for (int c = 0; c < cn; ++c) {
                float val = 0.f;
                if (use) {
                    const float *sp = src + ((int64_t)n * C + c0 + c) * plane + o00;
                    float a, b, cc, d;
                    load_pair(sp, v00, v01, a, b);
                    load_pair(sp + w, v10, v11, cc, d);
                    val = w00 * a + w01 * b + w10 * cc + w11 * d;
                }
                op[c * oplane] = val;
            }
        }
        return;
    }
    // this lane's corners inside a channel's patch (an invalid corner reads slot 0 and is masked)
    const int ry = sc.y0 - ymin, rx = sc.x0 - xs;
    const int r00 = v00 ? ry * PWp + rx : 0, r01 = v01 ? ry * PWp + rx + 1 : 0;
    const int r10 = v10 ? (ry + 1) * PWp + rx : 0, r11 = v11 ? (ry + 1) * PWp + rx + 1 : 0;
    // the view's channels c0.. through one buffer descriptor (the launcher checks that a view stays below 2^31 bytes)
    const __amdgpu_buffer_rsrc_t rv = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float *>(src + ((int64_t)n * C + c0) * plane), 0, (int)((unsigned)cn * (unsigned)plane * 4u), 0x00020000);
    for (int cb = 0; cb < cn; cb += chunk) {
        const int cc_n = min(chunk, cn - cb), items = cc_n * PH * Q;      // 16-byte pieces of this chunk's patches
        if (cb) __syncthreads();                                          // everyone is done reading the previous chunk
        for (int base = wave * 64; base < items; base += 256) {
            const int it = base + lane;
            const int ch = it / (PH * Q), rem = it - ch * (PH * Q), row = rem / Q, q = rem - row * Q;
            const unsigned vo = it < items ? (unsigned)(((cb + ch) * (int)plane + (ymin + row) * w + xs + 4 * q) * 4) : 0x80000000u;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rv, (__attribute__((address_space(3))) void *)(patch + base * 4), 16, (int)vo, 0, 0, 0);
        }
        __builtin_amdgcn_s_waitcnt(0x0F70);                               // vmcnt(0): this wave's copies have landed ...
        __syncthreads();                                                  // ... and everyone's
        if (live) {
            const float *pc = patch;
            float *o = op + (int64_t)cb * oplane;
#pragma unroll 4
            for (int c = 0; c < cc_n; ++c) {
                const float a = v00 ? pc[r00] : 0.f, b = v01 ? pc[r01] : 0.f, cq = v10 ? pc[r10] : 0.f, d = v11 ? pc[r11] : 0.f;
                *o = w00 * a + w01 * b + w10 * cq + w11 * d;
                pc += PE;
                o += oplane;
            }
        }
    }
}

// ---- channel-last source AND destination ---------------------------------------------------------------
// The layout a channels_last trunk hands over ([N,h,w,C] memory under an NCHW-shaped tensor) and the one the
// shadow transformer's tokens want.  The NCHW-source kernel above gathers 4-byte texels, one load
// instruction per (channel, corner row): at Wildtrack size ~10 M wave-level gathers, i.e. it runs at the
// texture-address rate (93 us vs 33 us for a copy of the same bytes).  With channels innermost a corner is a
// contiguous C-vector: a lane takes 16 bytes of it, the C/4 (fp32) lanes of a pixel read whole 512-byte rows,
// and a pixel's geometry is evaluated once (fp64) by one lane and shared through LDS instead of once per
// channel group.
template <typename T>
__global__ __launch_bounds__(WARP_CL_THREADS) void warp_fwd_cl(
    const T *__restrict__ src, const T *__restrict__ Mv, int N, int C, int h, int w, int H, int W,
    int nearest, T *__restrict__ dst)
{
    constexpr int VEC = 16 / (int)sizeof(T);
    __shared__ WarpTexel<T> tex[WARP_PIX];
    WarpBlock wb;
    if (!warp_block(N, H, W, 1, wb)) return;
    const int n = wb.n;
    if (threadIdx.x < WARP_PIX) {
        const int i = wb.i0 + threadIdx.x / WARP_TW, j = wb.j0 + threadIdx.x % WARP_TW;
        tex[threadIdx.x] = warp_texel(Mv + (int64_t)n * 9, i, j, h, w, i < H && j < W, nearest);
    }
    __syncthreads();
    const int chunks = C / VEC;                                   // 16-byte chunks per pixel
    const T *view = src + (int64_t)n * h * w * C;
    const int rowC = w * C;
    for (int item = threadIdx.x; item < WARP_PIX * chunks; item += WARP_CL_THREADS) {
        const int p = item / chunks, c = (item - p * chunks) * VEC;
        const int i = wb.i0 + p / WARP_TW, j = wb.j0 + p % WARP_TW;
        if (i >= H || j >= W) continue;
        const WarpTexel<T> t = tex[p];
        Pack<T, VEC> out = Pack<T, VEC>::zero();
        if (t.valid) {
            const T *sp = view + (int64_t)t.o00 * C + c;
            const Pack<T, VEC> z = Pack<T, VEC>::zero();
            const Pack<T, VEC> a = (t.valid & 1) ? Pack<T, VEC>::load(sp) : z;
            const Pack<T, VEC> b = (t.valid & 2) ? Pack<T, VEC>::load(sp + C) : z;
            const Pack<T, VEC> cc = (t.valid & 4) ? Pack<T, VEC>::load(sp + rowC) : z;
            const Pack<T, VEC> d = (t.valid & 8) ? Pack<T, VEC>::load(sp + rowC + C) : z;
#pragma unroll
            for (int k = 0; k < VEC; ++k) out.v[k] = t.w00 * a.v[k] + t.w01 * b.v[k] + t.w10 * cc.v[k] + t.w11 * d.v[k];
        }
        out.store(dst + (((int64_t)n * H + i) * W + j) * C + c);
    }
}

// Channel-last source -> NCHW destination (the reference's output layout, mvdetr.py:194): the same item loop as
// warp_fwd_cl, but the blended 16-byte chunks go to an LDS tile [pixel][channel] first and leave as whole 128-byte runs
// of 32 destination pixels per (channel, row) -- written channel by channel from registers they would be 4-byte
// stores 4*H*W bytes apart.  Destination tile = 2 rows x 32 columns; channels in groups of 128.
__global__ __launch_bounds__(WARP_CL_THREADS) void warp_fwd_cl_nchw(
    const float *__restrict__ src, const float *__restrict__ Mv, int N, int C, int h, int w, int H, int W,
    int nearest, float *__restrict__ dst)
{
    __shared__ WarpTexel<float> tex[WARP_PIX];
    __shared__ __attribute__((aligned(16))) float ot[WARP_PIX * WARP_NC_LD];
    const int tx = (W + WARP_NC_TW - 1) / WARP_NC_TW, ty = (H + WARP_NC_TH - 1) / WARP_NC_TH;
    const int b = blockIdx.x, n = b / (tx * ty), rem = b - n * tx * ty;
    const int i0 = (rem / tx) * WARP_NC_TH, j0 = (rem % tx) * WARP_NC_TW;
    if (threadIdx.x < WARP_PIX) {
        const int i = i0 + threadIdx.x / WARP_NC_TW, j = j0 + threadIdx.x % WARP_NC_TW;
        tex[threadIdx.x] = warp_texel(Mv + (int64_t)n * 9, i, j, h, w, i < H && j < W, nearest);
    }
    __syncthreads();
    const float *view = src + (int64_t)n * h * w * C;
    const int rowC = w * C;
    const bool vec_ok = (W & 3) == 0;
    for (int cg = 0; cg < C; cg += WARP_NC_CG) {
        const int cn = min(WARP_NC_CG, C - cg), chunks = cn / 4;
        for (int item = threadIdx.x; item < WARP_PIX * chunks; item += WARP_CL_THREADS) {
            const int p = item / chunks, c = (item - p * chunks) * 4;
            const WarpTexel<float> t = tex[p];
            float4 out = make_float4(0.f, 0.f, 0.f, 0.f);
            if (t.valid) {
                const float *sp = view + (int64_t)t.o00 * C + cg + c;
                const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
                const float4 a = (t.valid & 1) ? *reinterpret_cast<const float4 *>(sp) : z;
                const float4 bq = (t.valid & 2) ? *reinterpret_cast<const float4 *>(sp + C) : z;
                const float4 cc = (t.valid & 4) ? *reinterpret_cast<const float4 *>(sp + rowC) : z;
                const float4 d = (t.valid & 8) ? *reinterpret_cast<const float4 *>(sp + rowC + C) : z;
                out.x = t.w00 * a.x + t.w01 * bq.x + t.w10 * cc.x + t.w11 * d.x;
                out.y = t.w00 * a.y + t.w01 * bq.y + t.w10 * cc.y + t.w11 * d.y;
                out.z = t.w00 * a.z + t.w01 * bq.z + t.w10 * cc.z + t.w11 * d.z;
                out.w = t.w00 * a.w + t.w01 * bq.w + t.w10 * cc.w + t.w11 * d.w;
            }
            *reinterpret_cast<float4 *>(ot + p * WARP_NC_LD + c) = out;
        }
        __syncthreads();
        // (channel, tile row) segments of 32 pixels = 128 bytes, 8 lanes x float4 each
        for (int item = threadIdx.x; item < cn * WARP_NC_TH * 8; item += WARP_CL_THREADS) {
            const int part = item & 7, seg = item >> 3, r = seg % WARP_NC_TH, c = seg / WARP_NC_TH;
            const int i = i0 + r, j = j0 + part * 4;
            if (i >= H || j >= W) continue;
            const float *o = ot + (r * WARP_NC_TW + part * 4) * WARP_NC_LD + c;
            float *dp = dst + (((int64_t)n * C + cg + c) * H + i) * W + j;
            if (vec_ok && j + 4 <= W) {
                *reinterpret_cast<float4 *>(dp) = make_float4(o[0], o[WARP_NC_LD], o[2 * WARP_NC_LD], o[3 * WARP_NC_LD]);
            } else {
                for (int k = 0; k < 4 && j + k < W; ++k) dp[k] = o[k * WARP_NC_LD];
            }
        }
        __syncthreads();
    }
}

// ---- 16-bit storage (float16 / bfloat16), forward only (inference) ---------------------------------------------------------
// src and dst are 16-bit words, the matrices fp32; the source position is the same fp64 source_position / make_coord, the
// blend weights and the blend are fp32 (WarpTexel<float>: storage type and compute type are separate here), and every
// output element is rounded once, to nearest-even.  warp_fwd_cl_half is warp_fwd_cl with 8 channels (16 bytes) per lane:
// channel-last on both sides, the layout a channels_last trunk hands to the shadow transformer.
template <typename C>
__global__ __launch_bounds__(WARP_CL_THREADS) void warp_fwd_cl_half(
    const uint16_t *__restrict__ src, const float *__restrict__ Mv, int N, int Cn, int h, int w, int H, int W,
    int nearest, uint16_t *__restrict__ dst)
{
    constexpr int VEC = 8;
    __shared__ WarpTexel<float> tex[WARP_PIX];
    WarpBlock wb;
    if (!warp_block(N, H, W, 1, wb)) return;
    const int n = wb.n;
    if (threadIdx.x < WARP_PIX) {
        const int i = wb.i0 + threadIdx.x / WARP_TW, j = wb.j0 + threadIdx.x % WARP_TW;
        tex[threadIdx.x] = warp_texel(Mv + (int64_t)n * 9, i, j, h, w, i < H && j < W, nearest);
    }
    __syncthreads();
    const int chunks = Cn / VEC;                                  // 16-byte chunks per pixel
    const uint16_t *view = src + (int64_t)n * h * w * Cn;
    const int rowC = w * Cn;
    for (int item = threadIdx.x; item < WARP_PIX * chunks; item += WARP_CL_THREADS) {
        const int p = item / chunks, c = (item - p * chunks) * VEC;
        const int i = wb.i0 + p / WARP_TW, j = wb.j0 + p % WARP_TW;
        if (i >= H || j >= W) continue;
        const WarpTexel<float> t = tex[p];
        uint4 o = make_uint4(0u, 0u, 0u, 0u);
        if (t.valid) {
            const uint16_t *sp = view + (int64_t)t.o00 * Cn + c;
            float a[8], b[8], cc[8], d[8], r[8];
            up8<C>(load8_or_zero(sp, t.valid & 1, view), a);
            up8<C>(load8_or_zero(sp + Cn, t.valid & 2, view), b);
            up8<C>(load8_or_zero(sp + rowC, t.valid & 4, view), cc);
            up8<C>(load8_or_zero(sp + rowC + Cn, t.valid & 8, view), d);
#pragma unroll
            for (int k = 0; k < VEC; ++k) r[k] = warp_blend_half(t.w00, a[k], t.w01, b[k], t.w10, cc[k], t.w11, d[k]);
            o = down8<C>(r);
        }
        *reinterpret_cast<uint4 *>(dst + (((int64_t)n * H + i) * W + j) * Cn + c) = o;
    }
}

// The other three layout combinations (and channel counts / alignments the kernel above does not take): warp_fwd's mapping,
// an 8 x 8 tile of destination pixels x up to 64 channels split over the four waves, with 2-byte accesses through the
// element strides of either layout.
template <typename C>
__global__ __launch_bounds__(WARP_PIX *WARP_SUB) void warp_fwd_half(
    const uint16_t *__restrict__ src, const float *__restrict__ Mv, int N, int Cn, int h, int w, int H, int W,
    int nearest, int src_nhwc, int dst_nhwc, uint16_t *__restrict__ dst)
{
    __shared__ WarpTexel<float> tex[WARP_PIX];
    const int lane = threadIdx.x & (WARP_PIX - 1);
    const int sub = threadIdx.x / WARP_PIX;
    WarpBlock wb;
    if (!warp_block(N, H, W, (Cn + WARP_CH - 1) / WARP_CH, wb)) return;
    const int n = wb.n, i = wb.i0 + lane / WARP_TW, j = wb.j0 + lane % WARP_TW;
    const bool live = i < H && j < W;
    if (sub == 0) tex[lane] = warp_texel(Mv + (int64_t)n * 9, i, j, h, w, live, nearest);
    __syncthreads();
    if (!live) return;
    const WarpTexel<float> t = tex[lane];
    constexpr int CPT = WARP_CH / WARP_SUB;
    const int64_t plane = (int64_t)h * w, oplane = (int64_t)H * W;
    const int64_t s_c = src_nhwc ? 1 : plane, s_t = src_nhwc ? Cn : 1;            // element strides: channel, texel
    const int64_t d_c = dst_nhwc ? 1 : oplane, d_p = dst_nhwc ? Cn : 1;
    const uint16_t *view = src + (int64_t)n * Cn * plane + (int64_t)t.o00 * s_t;
    uint16_t *op = dst + (int64_t)n * Cn * oplane + ((int64_t)i * W + j) * d_p;
    const int c_begin = wb.group * WARP_CH + sub * CPT, c_end = min(Cn, c_begin + CPT);
    for (int c = c_begin; c < c_end; ++c) {
        uint16_t o = 0;
        if (t.valid) {
            const uint16_t *sp = view + c * s_c;
            const float a = (t.valid & 1) ? C::up(sp[0]) : 0.f, b = (t.valid & 2) ? C::up(sp[s_t]) : 0.f;
            const float cc = (t.valid & 4) ? C::up(sp[w * s_t]) : 0.f, d = (t.valid & 8) ? C::up(sp[w * s_t + s_t]) : 0.f;
            o = C::down(warp_blend_half(t.w00, a, t.w01, b, t.w10, cc, t.w11, d));
        }
        op[c * d_c] = o;
    }
}

// [n, rows, cols] -> [n, cols, rows] through a 64 x 64 LDS tile (reads and writes both in 256-byte runs): turns an NCHW
// feature map into the channel-last layout the fast warp kernels read (rows = C, cols = h*w) and back
// (rows = h*w, cols = C).
template <typename T>
__global__ __launch_bounds__(256) void transpose_tiles(const T *__restrict__ src, int rows, int cols, T *__restrict__ dst)
{
    __shared__ T tile[64][65];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int c0 = blockIdx.x * 64, r0 = blockIdx.y * 64;
    const int64_t base = (int64_t)blockIdx.z * rows * cols;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int r = r0 + ty + 4 * k, c = c0 + tx;
        if (r < rows && c < cols) tile[ty + 4 * k][tx] = src[base + (int64_t)r * cols + c];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int c = c0 + ty + 4 * k, r = r0 + tx;
        if (r < rows && c < cols) dst[base + (int64_t)c * rows + r] = tile[tx][ty + 4 * k];
    }
}

// ---- launchers -------------------------------------------------------------------------------------------------------------
template <typename C> static void warp_launch_fwd_half(const WarpCall &c, const WarpRoute &r)
{
    if (r.kind == WarpKind::fwd_cl_half) warp_launch_kernel<uint16_t, float>(warp_fwd_cl_half<C>, WARP_CL_THREADS, 0, c, r);
    else warp_launch_kernel<uint16_t, float>(warp_fwd_half<C>, WARP_PIX * WARP_SUB, 0, c, r, (int)r.src_nhwc, (int)r.dst_nhwc);
}

int warp_launch_forward(const WarpCall &c, const WarpRoute &r)
{
    switch (r.kind) {
    case WarpKind::fwd_nchw_patch: warp_launch_kernel<float, float>(warp_fwd_nchw_patch, 256, WARP_PP_FLOATS * 4, c, r); break;
    case WarpKind::fwd_cl_nchw: warp_launch_kernel<float, float>(warp_fwd_cl_nchw, WARP_CL_THREADS, 0, c, r); break;
    case WarpKind::fwd_half:
    case WarpKind::fwd_cl_half:
        if (c.type == WarpType::f16) warp_launch_fwd_half<F16>(c, r);
        else warp_launch_fwd_half<BF16>(c, r);
        break;
    default:
        // the kinds that exist for fp32 and fp64
        warp_for_type(c.type, [&](auto t) {
            using T = decltype(t);
            if (r.kind == WarpKind::fwd_cl) warp_launch_kernel<T, T>(warp_fwd_cl<T>, WARP_CL_THREADS, 0, c, r);
            else if (r.dst_nhwc) warp_launch_kernel<T, T>(warp_fwd<T, true>, WARP_PIX * WARP_SUB, 0, c, r);
            else warp_launch_kernel<T, T>(warp_fwd<T, false>, WARP_PIX * WARP_SUB, 0, c, r);
        });
    }
    return (int)hipGetLastError();
}

int warp_launch_transpose(hipStream_t st, int elem_size, const void *src, int n, int rows, int cols, void *dst)
{
    const dim3 grid((unsigned)((cols + 63) / 64), (unsigned)((rows + 63) / 64), (unsigned)n);
    if (elem_size == 4) hipLaunchKernelGGL((transpose_tiles<float>), grid, dim3(256), 0, st, static_cast<const float *>(src), rows, cols, static_cast<float *>(dst));
    else hipLaunchKernelGGL((transpose_tiles<double>), grid, dim3(256), 0, st, static_cast<const double *>(src), rows, cols, static_cast<double *>(dst));
    return (int)hipGetLastError();
}

}  // namespace mvdetr

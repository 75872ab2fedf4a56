// The backward of the Winograd F(2x2, 3x3) convolution of conv_winograd.hip (stride 1, padding = dilation, fp32, channel-last).
//
//   data gradient     the same convolution of grad_y with the weights flipped in both spatial axes and transposed in (C, K):
//                     winograd_weights_dgrad_f32 forms Ut[p][k][c] = (G g' G^T)[xi][nu], g'[i][j] = w[k][c][2 - i][2 - j], in fp64
//                     rounded once, and mvdetr_conv3x3_winograd_f32 runs on it with C and K exchanged.  No kernel of its own.
//   weight gradient   in the Winograd domain.  With V = B^T d B of a tile of x (as the forward forms it) and dM = A dY A^T of
//                     the same 2x2 tile of grad_y,
//                         dU[p][c][k] = sum over the tiles of V[p][tile][c] * dM[p][tile][k],      dw = G^T dU G
//                     sixteen GEMMs reduced over the tiles: 16 multiplications per (tile, c, k) against 36 of the direct form.
//
//   conv3x3_winograd_wgrad_f32   a unit is a 64-k x 64-c block of dU at all sixteen positions, run by a workgroup of 4 waves:
//       * every wave owns a 32-k x 32-c block of ALL sixteen products: 16 accumulators of v_mfma_f32_32x32x2_f32, so position
//         p of a (k, c) sits in the same lane and register of accumulator p and G^T dU G happens in registers;
//       * the reduction runs over the tile grid of the forward (conv_winograd.h: Shape, tile_grid, tile_pixel -- every
//         sub-lattice (y mod d, x mod d) its own grid) in chunks of 8 tiles = four k-steps of sixteen MFMAs.  Both operands are
//         transformed on the way into LDS, two buffers, one barrier per chunk: a lane loads one tile's 4x4 patch of x for two
//         input channels (sixteen 8-byte buffer loads) and its 2x2 tile of grad_y for two output channels (four), forms
//         B^T d B and A dY A^T, and writes the four nu of a row xi as one 16-byte slot: V and dM are [tile 8][xi 4][channel 64]
//         [nu 4], and one ds_read_b128 of each feeds four MFMAs;
//       * a pixel outside the image contributes ZERO, of x and of grad_y alike -- the overhanging row or column of an odd
//         extent, the tiles past the last image: its buffer offset lies beyond the resource's range, whose loads return zero.
//         (In the forward an overhanging output was merely not stored; here it would be summed.)  The resource's range ends
//         with the tensor;
//       * there are only (C / 64)(K / 64) units, so the chunk range is split over S workgroups per unit, each a contiguous
//         range of chunks; split s of a unit writes G^T dU G of its range to slice s of the workspace ([S][K][C][3][3]).
//   winograd_wgrad_reduce_f32    sums the S slices in index order and writes gw.  No atomics anywhere: for a given S the result
//                                is bit-identical from call to call.
#include "common.h"
#include "conv_winograd_device.h"
#include "../../include/mvdetr_ops.h"

#include <type_traits>

namespace mvdetr {

static std::atomic<int> g_winograd_wgrad_splits{0};                           // mvdetr_winograd_set_wgrad_splits: 0 = default
static std::atomic<int> g_winograd_last_wgrad_splits{0};

namespace wino {
namespace wgrad {

constexpr int CT = 8;                      // tiles per chunk: four k-steps of the 32x32x2 MFMA
constexpr int CB = 64;                     // channels of a unit, input and output
constexpr int OP_FLOATS = CT * 4 * CB * 4; // one operand of a chunk, [tile][xi][channel][nu]: 8,192 floats
constexpr int BUF_FLOATS = 2 * OP_FLOATS;  // dM first, then V
constexpr int LDS_BYTES = 2 * BUF_FLOATS * 4;                                 // two buffers = 131,072

// How a call is split (make_plan): `units` blocks of 64 x 64 channels, `chunks` chunks of 8 tiles, S splits of `per` chunks
// each (the last one `last`); the grid runs the units * S items round-robin
struct Plan {
    unsigned units, chunks, S, per, last, grid;
};

struct Args {
    unsigned items, S, per, chunks;
    int kblocks;
};

__global__ __launch_bounds__(256) void conv3x3_winograd_wgrad_f32(const float *__restrict__ x, const float *__restrict__ gy,
                                                                  float *__restrict__ part, const Shape s, const Args a)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int C = s.C, K = s.K, d = s.d, H = s.H, W = s.W;
    const unsigned txy = (unsigned)s.TX * (unsigned)s.TY;                     // tiles of one image

    // the loader's lane: tile `ltile` of the chunk, channels 2 cp and 2 cp + 1 of the unit's block, of x and of grad_y
    const int ltile = tid >> 5, cp = tid & 31;
    const int w_off = (ltile * 4 * CB + 2 * cp) * 4;                          // + (xi * CB + e) * 4; V: + OP_FLOATS
    // the wave's block: output channels wm * 32 .. of the unit (A operand, rows), input channels wn * 32 .. (B operand, columns);
    // k-step st reads tile 2 st + (lane >> 5)
    const int wm = wave & 1, wn = wave >> 1;
    const int a_off = ((lane >> 5) * 4 * CB + wm * 32 + (lane & 31)) * 4;     // + (2 st * 4 + xi) * CB * 4
    const int b_off = OP_FLOATS + ((lane >> 5) * 4 * CB + wn * 32 + (lane & 31)) * 4;

    for (unsigned item = blockIdx.x; item < a.items; item += gridDim.x) {
        const unsigned unit = item / a.S, split = item % a.S;
        const int kb = (int)(unit % (unsigned)a.kblocks), cb = (int)(unit / (unsigned)a.kblocks);
        const unsigned ch0 = split * a.per;
        const unsigned ch1 = ch0 + a.per < a.chunks ? ch0 + a.per : a.chunks;

        float2 raw[16], graw[4];
        // The loads of chunk `ch`.  Every per-lane offset is 32-bit and relative to the image of the chunk's first tile (the
        // host bounds the span of 8 tiles by the forward's bound for 64); the whole offset travels in the VGPR, so that one
        // outside the image, X_OUTSIDE, is beyond the range whatever else is added.
        auto load = [&](unsigned ch) {
            const unsigned t0 = ch * CT;
            const int n0 = (int)(t0 / txy);                                   // uniform
            const unsigned long long xleft = (unsigned long long)(s.N - n0) * H * W * C * 4ull;
            const unsigned long long gleft = (unsigned long long)(s.N - n0) * H * W * K * 4ull;
            const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc(
                const_cast<float *>(x + (size_t)n0 * H * W * C), 0, (int)(xleft < X_RANGE ? (unsigned)xleft : X_RANGE), 0x00020000);
            const __amdgpu_buffer_rsrc_t grsrc = __builtin_amdgcn_make_buffer_rsrc(
                const_cast<float *>(gy + (size_t)n0 * H * W * K), 0, (int)(gleft < X_RANGE ? (unsigned)gleft : X_RANGE), 0x00020000);
            int X, Y, n, y0, x0;
            tile_grid(s, t0 + ltile, X, Y, n);
            tile_pixel(s, X, Y, y0, x0);
            const bool tvalid = n < s.N;                                      // a tile past the last one is in image N or later
            const unsigned pix = ((unsigned)(n - n0) * H + y0) * W + x0;
            const unsigned base = (pix * C + cb * CB + 2 * cp) * 4u, cstep = (unsigned)d * C * 4u, rstep = cstep * W;
            bool oky[4], okx[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                oky[i] = tvalid & ((unsigned)(y0 + (i - 1) * d) < (unsigned)H);
                okx[i] = (unsigned)(x0 + (i - 1) * d) < (unsigned)W;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const unsigned row = base + (unsigned)(i - 1) * rstep;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const unsigned off = (oky[i] & okx[j]) ? row + (unsigned)(j - 1) * cstep : X_OUTSIDE;
                    raw[4 * i + j] = __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(xrsrc, (int)off, 0, 0));
                }
            }
            const unsigned gbase = (pix * K + kb * CB + 2 * cp) * 4u, gcstep = (unsigned)d * K * 4u, grstep = gcstep * W;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const unsigned off = (oky[1 + i] & okx[1 + j]) ? gbase + i * grstep + j * gcstep : X_OUTSIDE;
                    graw[2 * i + j] = __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(grsrc, (int)off, 0, 0));
                }
        };
        // B^T d B (rows first, as the forward) and A dY A^T of what load() fetched, into `buf`, in eight pieces that fit
        // behind a group of MFMAs each: piece q is row xi = q & 3 of channel e = q >> 2 of the lane's pair, of both operands
        auto xform_piece = [&](float *buf, int q) {
            const int e = q >> 2, xi = q & 3;
            const int ra = xi == 0 ? 0 : xi == 2 ? 2 : 1, rb = xi == 0 ? 2 : xi == 1 ? 2 : xi == 2 ? 1 : 3;   // t = d[ra] -/+ d[rb]
            float t[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float da = e ? raw[4 * ra + j].y : raw[4 * ra + j].x, db = e ? raw[4 * rb + j].y : raw[4 * rb + j].x;
                t[j] = xi == 1 ? da + db : da - db;
            }
            const f32x4 v = {t[0] - t[2], t[1] + t[2], t[2] - t[1], t[1] - t[3]};
            *reinterpret_cast<f32x4 *>(buf + OP_FLOATS + w_off + (xi * CB + e) * 4) = v;
            // A = (A^T)^T, A^T = [1 1 1 0; 0 1 -1 -1]: row xi of A dY is dY0, dY0 + dY1, dY0 - dY1, -dY1
            float g[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) g[k] = e ? graw[k].y : graw[k].x;
            const float r0 = xi == 0 ? g[0] : xi == 1 ? g[0] + g[2] : xi == 2 ? g[0] - g[2] : -g[2];
            const float r1 = xi == 0 ? g[1] : xi == 1 ? g[1] + g[3] : xi == 2 ? g[1] - g[3] : -g[3];
            const f32x4 m = {r0, r0 + r1, r0 - r1, -r1};
            *reinterpret_cast<f32x4 *>(buf + w_off + (xi * CB + e) * 4) = m;
        };

        f32x16 acc[16];

        load(ch0);
#pragma unroll
        for (int q = 0; q < 8; ++q) xform_piece(lds, q);
        __syncthreads();

        // One chunk = sixteen groups (k-step st = g >> 2, row xi = g & 3) of four MFMAs, one per nu.  Two sets of operand
        // registers: the two ds_read_b128 of group g + 1 are issued ahead of the MFMAs of group g.  The loads of the next
        // chunk go first, its transform and LDS writes behind the last eight groups; past the split's last chunk that chunk
        // is staged again, into a buffer nobody reads, so that the loop carries no branch.
        f32x4 fa[2], fb[2];
        auto read_ops = [&](const float *cur, int g, int set) {
            const int row = (2 * (g >> 2) * 4 + (g & 3)) * CB * 4;
            fa[set] = *reinterpret_cast<const f32x4 *>(cur + a_off + row);
            fb[set] = *reinterpret_cast<const f32x4 *>(cur + b_off + row);
        };
        // A split's first chunk is a copy of the chunk whose first k-step has a zero C operand: nothing is cleared, and the
        // accumulators are not live from one item to the next.
        int par = 0;
        unsigned ch = ch0;
        auto chunk = [&](auto first) {
            const float *const cur = lds + par * BUF_FLOATS;
            float *const nxt = lds + (par ^ 1) * BUF_FLOATS;
            load(ch + 1 < ch1 ? ch + 1 : ch);
            read_ops(cur, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                if (g < 15) read_ops(cur, g + 1, (g + 1) & 1);
#pragma unroll
                for (int nu = 0; nu < 4; ++nu) {
                    const int p = 4 * (g & 3) + nu;
                    if (decltype(first)::value && g < 4)
                        acc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[g & 1][nu], fb[g & 1][nu], f32x16{}, 0, 0, 0);
                    else
                        acc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[g & 1][nu], fb[g & 1][nu], acc[p], 0, 0, 0);
                }
                if (g >= 8) xform_piece(nxt, g - 8);
                __builtin_amdgcn_sched_barrier(0);
            }
            __syncthreads();                                                  // the next chunk is in LDS, this one is read
            par ^= 1;
        };
        chunk(std::true_type{});
        while (++ch < ch1) chunk(std::false_type{});

        // ---- G^T dU G in registers, then the stores: register r is output channel wm * 32 + (r & 3) + 8 (r >> 2) + 4 (lane >> 5) ----
        float *const dst = part + (size_t)split * K * C * 9 +
                           ((size_t)(kb * CB + wm * 32 + 4 * (lane >> 5)) * C + cb * CB + wn * 32 + (lane & 31)) * 9;
        // 18 wait states between the last MFMA's write and the hand-written reads of its registers
        asm volatile("s_nop 15\n\ts_nop 3");
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float m[16];
#pragma unroll
            for (int p = 0; p < 16; ++p) asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(m[p]) : "a"(acc[p][r]));
            float t[3][4];
#pragma unroll
            for (int nu = 0; nu < 4; ++nu) {
                const float h = 0.5f * (m[4 + nu] + m[8 + nu]);
                t[0][nu] = m[nu] + h;
                t[1][nu] = 0.5f * (m[4 + nu] - m[8 + nu]);
                t[2][nu] = h + m[12 + nu];
            }
            float *const o = dst + (size_t)((r & 3) + 8 * (r >> 2)) * C * 9;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const float h = 0.5f * (t[i][1] + t[i][2]);
                o[3 * i] = t[i][0] + h;
                o[3 * i + 1] = 0.5f * (t[i][1] - t[i][2]);
                o[3 * i + 2] = h + t[i][3];
            }
#pragma unroll
            for (int p = 0; p < 16; ++p) asm volatile("" : "+a"(acc[p]));
        }
    }
}

// gw[i] = part[0][i] + part[1][i] + ... in that order
__global__ __launch_bounds__(256) void winograd_wgrad_reduce_f32(const float *__restrict__ part, float *__restrict__ gw, int64_t n, int S)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float v = part[i];
    for (int sp = 1; sp < S; ++sp) v += part[(int64_t)sp * n + i];
    gw[i] = v;
}

// Ut[p = 4 xi + nu][k][c] = (G g' G^T)[xi][nu], g'[i][j] = weight[k][c][2 - i][2 - j], in fp64, rounded once: the forward's U of
// the flipped, transposed weights.  One thread per (k, c).
__global__ __launch_bounds__(256) void winograd_weights_dgrad_f32(const float *__restrict__ w, int C, int K, float *__restrict__ Ut)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)C * K) return;
    const float *g = w + i * 9;                                               // i = k * C + c
    double t[4][3];                                                           // G g'
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double g0 = g[8 - j], g1 = g[5 - j], g2 = g[2 - j];
        t[0][j] = g0;
        t[1][j] = 0.5 * (g0 + g1 + g2);
        t[2][j] = 0.5 * (g0 - g1 + g2);
        t[3][j] = g2;
    }
#pragma unroll
    for (int xi = 0; xi < 4; ++xi) {
        const double u[4] = {t[xi][0], 0.5 * (t[xi][0] + t[xi][1] + t[xi][2]), 0.5 * (t[xi][0] - t[xi][1] + t[xi][2]), t[xi][2]};
#pragma unroll
        for (int nu = 0; nu < 4; ++nu) Ut[(size_t)(4 * xi + nu) * C * K + i] = (float)u[nu];
    }
}

// The default S gives every CU about one workgroup (one fits: 128 KB of LDS): CUs / units, at least 1, and never more than
// there are chunks; mvdetr_winograd_set_wgrad_splits forces it, mvdetr_winograd_set_max_workgroups caps the CUs counted and
// the grid.  Every split gets `per` chunks but the last, which gets the rest (at least one).
static Plan make_plan(const Shape &s, int cus)
{
    Plan p;
    p.units = (unsigned)(s.C / CB) * (unsigned)(s.K / CB);
    p.chunks = (unsigned)(((uint64_t)s.tiles + CT - 1) / CT);
    const int cap = g_winograd_max_workgroups.load(), forced = g_winograd_wgrad_splits.load();
    unsigned wgs = (unsigned)(cus > 0 ? cus : 1);
    if (cap > 0 && wgs > (unsigned)cap) wgs = (unsigned)cap;
    unsigned S = forced > 0 ? (unsigned)forced : wgs / p.units;
    if (S < 1) S = 1;
    if (S > p.chunks) S = p.chunks;
    p.per = (p.chunks + S - 1) / S;
    p.S = (p.chunks + p.per - 1) / p.per;
    p.last = p.chunks - (p.S - 1) * p.per;
    const uint64_t items = (uint64_t)p.units * p.S;
    p.grid = (unsigned)(cap > 0 && items > (uint64_t)cap ? (uint64_t)cap : items);
    return p;
}

static bool shape_ok(int C, int K, int dilation) { return C % CB == 0 && K % CB == 0 && (dilation == 1 || dilation == 2 || dilation == 4); }

// The bounds on a shape, the forward's: 32-bit byte offsets from the image of a chunk's first tile, fewer than 2^31 tiles
static bool bounds_ok(Shape &s, int N, int H, int W, int C, int K, int dilation)
{
    return offsets_fit(H, W, C, K) && weights_fit(C, K) && tile_shape(s, N, H, W, C, K, dilation);
}

static bool overlap(const void *p, uint64_t pbytes, const void *q, uint64_t qbytes)
{
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return a < b + qbytes && b < a + pbytes;
}

static int entry(const float *x, const float *gy, float *gw, int N, int H, int W, int C, int K, int dilation, void *workspace,
                 int64_t workspace_bytes, void *stream)
{
    if (!x || !gy || !gw || N < 0 || H <= 0 || W <= 0 || C <= 0 || K <= 0 || workspace_bytes < 0) return (int)hipErrorInvalidValue;
    const uint64_t xb = (uint64_t)N * H * W * C * 4, gb = (uint64_t)N * H * W * K * 4, wb = (uint64_t)C * K * 36;
    if ((const float *)gw == x || (const float *)gw == gy || overlap(gw, wb, x, xb) || overlap(gw, wb, gy, gb))
        return (int)hipErrorInvalidValue;
    if (workspace && (overlap(workspace, (uint64_t)workspace_bytes, x, xb) || overlap(workspace, (uint64_t)workspace_bytes, gy, gb) ||
                      overlap(workspace, (uint64_t)workspace_bytes, gw, wb)))
        return (int)hipErrorInvalidValue;
    if (!shape_ok(C, K, dilation) || !aligned(x, 16) || !aligned(gy, 16) || !aligned(gw, 16) || !aligned(workspace, 16))
        return (int)hipErrorNotSupported;
    Shape s;
    if (!bounds_ok(s, N, H, W, C, K, dilation)) return (int)hipErrorNotSupported;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (N == 0) {
        const int rc = (int)hipMemsetAsync(gw, 0, wb, st);
        g_winograd_last_wgrad_splits = 0;
        return rc;
    }
    const Plan pl = make_plan(s, device_cus());
    if (!workspace || (uint64_t)workspace_bytes < (uint64_t)pl.S * wb) return (int)hipErrorNotSupported;
    static PerDevice<int> lds_attr;
    const int rc = lds_attr.get([] {
        return (int)hipFuncSetAttribute(reinterpret_cast<const void *>(conv3x3_winograd_wgrad_f32),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES);
    });
    if (rc != 0) return rc;
    const Args a{pl.units * pl.S, pl.S, pl.per, pl.chunks, K / CB};
    float *const part = static_cast<float *>(workspace);
    hipLaunchKernelGGL(conv3x3_winograd_wgrad_f32, dim3(pl.grid), dim3(256), LDS_BYTES, st, x, gy, part, s, a);
    const int64_t n = (int64_t)C * K * 9;
    hipLaunchKernelGGL(winograd_wgrad_reduce_f32, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, part, gw, n, (int)pl.S);
    g_winograd_last_wgrad_splits = (int)pl.S;
    g_winograd_last_kernel = "conv3x3_winograd_wgrad_f32";
    g_winograd_launches.fetch_add(1);
    return (int)hipGetLastError();
}

}  // namespace wgrad
}  // namespace wino
}  // namespace mvdetr

extern "C" int mvdetr_winograd_weights_dgrad_f32(const float *w, int C, int K, float *Ut, void *stream)
{
    using namespace mvdetr;
    if (!w || !Ut || C <= 0 || K <= 0) return (int)hipErrorInvalidValue;
    // the convolution that reads Ut has K input and C output channels
    if (C % 64 != 0 || K % 8 != 0 || !aligned(w, 4) || !aligned(Ut, 16) || (int64_t)C * K > (int64_t)1 << 26)
        return (int)hipErrorNotSupported;
    hipLaunchKernelGGL(wino::wgrad::winograd_weights_dgrad_f32, dim3((unsigned)(((int64_t)C * K + 255) / 256)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), w, C, K, Ut);
    g_winograd_last_kernel = "winograd_weights_dgrad_f32";
    g_winograd_launches.fetch_add(1);
    return (int)hipGetLastError();
}

extern "C" int mvdetr_conv3x3_winograd_wgrad_f32(const float *x, const float *gy, float *gw, int N, int H, int W, int C, int K,
                                                 int dilation, void *workspace, int64_t workspace_bytes, void *stream)
{
    return mvdetr::wino::wgrad::entry(x, gy, gw, N, H, W, C, K, dilation, workspace, workspace_bytes, stream);
}

extern "C" int mvdetr_winograd_set_wgrad_splits(int n) { return mvdetr::g_winograd_wgrad_splits.exchange(n > 0 ? n : 0); }

extern "C" int mvdetr_winograd_last_wgrad_splits(void) { return mvdetr::g_winograd_last_wgrad_splits.load(); }

extern "C" int mvdetr_winograd_wgrad_plan(int N, int H, int W, int C, int K, int dilation, int workgroups, int64_t *out)
{
    using namespace mvdetr;
    if (!out || N <= 0 || H <= 0 || W <= 0 || C <= 0 || K <= 0 || workgroups <= 0) return (int)hipErrorInvalidValue;
    wino::Shape s;
    if (!wino::wgrad::shape_ok(C, K, dilation) || !wino::wgrad::bounds_ok(s, N, H, W, C, K, dilation)) return (int)hipErrorNotSupported;
    const wino::wgrad::Plan p = wino::wgrad::make_plan(s, workgroups);
    out[0] = p.units; out[1] = p.chunks; out[2] = p.S; out[3] = p.per; out[4] = p.last;
    return 0;
}

extern "C" int64_t mvdetr_winograd_wgrad_workspace_bytes(int N, int H, int W, int C, int K, int dilation, int workgroups)
{
    int64_t out[5];
    if (mvdetr_winograd_wgrad_plan(N, H, W, C, K, dilation, workgroups, out) != 0) return -1;
    return out[2] * (int64_t)C * K * 36;
}

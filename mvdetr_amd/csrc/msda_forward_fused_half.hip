// Fused multi-scale deformable attention, forward, 16-bit storage (float16 / bfloat16) -- gfx950 (MI355X).
//
// The inference call MSDeformAttn makes in 16 bits: value and the module's ONE GEMM output `raw` (slice-interleaved,
// level outermost: per query [L][M/g][g*P*2 offsets | g*P logits], g = 32 / D heads per run -- the layout
// MultiScaleDeformableAttention.slice_major_rows(level_outer=True) gives the Linear) are READ in 16 bits, the
// reference points stay fp32 ([1 or B, L, Lq, 2], one per (query, level): a [0, 1] coordinate rounded to bfloat16 is
// +-0.7 px on a 180-wide map), softmax over the L*P logits and  loc = ref + offset / (W, H)  happen here in fp32, the
// bilinear taps are blended in fp32 and every output element is rounded once, to nearest-even, on the way out.
//
// Work mapping: a workgroup owns a small 2-D tile of neighbouring queries of one camera (level) x one 128-byte slice
// of the token row (64 channels: 4 heads of 16 channels or 2 of 32).  A lane owns 8 channels (16 bytes) of one query;
// the 2 (D = 16) or 4 (D = 32) lanes of a head compute that head's softmax redundantly -- the logits come out of the
// same cache lines for all of them -- so the kernel has no cross-lane step, no LDS and no barrier.  Taps are gathered
// straight from global memory: neighbouring queries hit neighbouring tokens, and the 8 lanes of a (query, slice) read
// one whole 128-byte line per corner.  Token rows narrower than 64 channels take one head per query slot instead.
//
// Shapes served: D 16 or 32, P = 4, L <= 16 levels OF EQUAL SHAPE, num_query == spatial_size.  The level shapes are
// device data: a call whose shapes / level_start_index are not L equal maps laid end to end gets NaN in every output
// element (nothing is read out of bounds); everything the host can see is refused with hipErrorNotSupported.
#include "common.h"
#include "half_types.h"
#include "msda_dispatch.h"
#include "../../include/mvdetr_ops.h"

namespace mvdetr {

constexpr int FH_THREADS = 256;
constexpr int FH_TW = 8;                                  // queries of a tile along x; its height is queries per workgroup / 8
constexpr int FH_P = 4;

template <typename C, int D>
__global__ __launch_bounds__(FH_THREADS) void msda_fwd_fused_half(
    const uint16_t *__restrict__ value, const int64_t *__restrict__ shapes, const int64_t *__restrict__ lsi,
    const float *__restrict__ ref, int64_t ref_bstride, const uint16_t *__restrict__ raw, int raw_q, int B, int S, int M,
    int L, int lpq, uint16_t *__restrict__ out)
{
    constexpr int G = 32 / D;                             // heads per run of the raw tensor
    constexpr int RUN = 12 * G;                           // elements of a run: G*P*2 offsets, then G*P logits
    const int H = (int)shapes[0], W = (int)shapes[1];
    const int64_t row = (int64_t)M * D;
    bool equal = H > 0 && W > 0 && (int64_t)H * W * L == (int64_t)S;
    for (int l = 0; l < L; ++l)
        equal = equal && shapes[2 * l] == H && shapes[2 * l + 1] == W && lsi[l] == (int64_t)l * H * W;
    if (!equal) {
        // not the promised shapes: NaN everywhere
        const uint32_t nan2 = down2<C>(__uint_as_float(0x7fc00000u), __uint_as_float(0x7fc00000u));
        const int64_t words = (int64_t)B * S * row / 2;
        uint32_t *o = reinterpret_cast<uint32_t *>(out);
        for (int64_t i = (int64_t)blockIdx.x * FH_THREADS + threadIdx.x; i < words; i += (int64_t)gridDim.x * FH_THREADS)
            o[i] = nan2;
        return;
    }
    const int HW = H * W;
    const int qpw = FH_THREADS / lpq, th = qpw / FH_TW;   // queries per workgroup; tile height
    const int slices = (int)(row / (8 * lpq));            // channel groups of 8 * lpq per token row
    const int tx = (W + FH_TW - 1) / FH_TW, ty = (H + th - 1) / th;
    const int64_t jobs = (int64_t)B * L * ty * tx * slices;
    const int sub = threadIdx.x % lpq, slot = threadIdx.x / lpq;
    const int qx_in = slot % FH_TW, qy_in = slot / FH_TW;
    const float fW = (float)W, fH = (float)H;
    const int runs_per_level = M / G;
    for (int64_t job = blockIdx.x; job < jobs; job += gridDim.x) {
        int64_t r = job;
        const int slice = (int)(r % slices);
        r /= slices;
        const int qx = (int)(r % tx) * FH_TW + qx_in;
        r /= tx;
        const int qy = (int)(r % ty) * th + qy_in;
        r /= ty;
        const int lq = (int)(r % L), b = (int)(r / L);
        if (qx >= W || qy >= H) continue;
        const int q = lq * HW + qy * W + qx;
        const int c0 = (slice * lpq + sub) * 8;           // this lane's 8 channels of the token row
        const int m = c0 / D, run = m / G, hd = m % G;
        const uint16_t *rq = raw + ((int64_t)b * S + q) * raw_q + run * RUN;       // level l: + l * runs_per_level * RUN
        const int lstep = runs_per_level * RUN;
        // softmax statistics of the head: maximum, then the sum of exp(logit - maximum)
        float mx = -INFINITY;
        for (int l = 0; l < L; ++l) {
            const Raw<4> lg = *reinterpret_cast<const Raw<4> *>(rq + l * lstep + G * 8 + hd * 4);
            mx = fmaxf(mx, fmaxf(fmaxf(C::up(lg.v[0]), C::up(lg.v[1])), fmaxf(C::up(lg.v[2]), C::up(lg.v[3]))));
        }
        float den = 0.f;
        for (int l = 0; l < L; ++l) {
            const Raw<4> lg = *reinterpret_cast<const Raw<4> *>(rq + l * lstep + G * 8 + hd * 4);
            den += (expf(C::up(lg.v[0]) - mx) + expf(C::up(lg.v[1]) - mx)) + (expf(C::up(lg.v[2]) - mx) + expf(C::up(lg.v[3]) - mx));
        }
        const float inv = 1.f / den;
        const uint16_t *vb = value + (int64_t)b * S * row + c0;
        const float *rp = ref + (int64_t)b * ref_bstride + (int64_t)q * 2;
        float acc[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = 0.f;
        for (int l = 0; l < L; ++l) {
            const float2 rf = *reinterpret_cast<const float2 *>(rp + (int64_t)l * S * 2);
            const uint16_t *rl = rq + l * lstep;
            const Raw<4> oa = *reinterpret_cast<const Raw<4> *>(rl + hd * 8);
            const Raw<4> ob = *reinterpret_cast<const Raw<4> *>(rl + hd * 8 + 4);
            const Raw<4> lg = *reinterpret_cast<const Raw<4> *>(rl + G * 8 + hd * 4);
            const float ox[4] = {C::up(oa.v[0]), C::up(oa.v[2]), C::up(ob.v[0]), C::up(ob.v[2])};
            const float oy[4] = {C::up(oa.v[1]), C::up(oa.v[3]), C::up(ob.v[1]), C::up(ob.v[3])};
            const float lgt[4] = {C::up(lg.v[0]), C::up(lg.v[1]), C::up(lg.v[2]), C::up(lg.v[3])};
            const uint16_t *plane = vb + (int64_t)l * HW * row;
#pragma unroll
            for (int p = 0; p < FH_P; ++p) {
                // the module's arithmetic: loc = ref + offset / (W, H); the core's: loc * size - 0.5
                const float x = (rf.x + ox[p] / fW) * fW - 0.5f;
                const float y = (rf.y + oy[p] / fH) * fH - 0.5f;
                const float a = expf(lgt[p] - mx) * inv;
                const bool in = y > -1.f && x > -1.f && y < fH && x < fW;          // (false for NaN / inf positions)
                const Footprint<float> f = footprint(in ? y : 0.f, in ? x : 0.f, H, W);
                const uint16_t *r0 = plane + ((int64_t)f.y0 * W + f.x0) * row;
                const uint16_t *r1 = r0 + (int64_t)W * row;
                const uint4 c00 = load8_or_zero(r0, in && f.vy0 && f.vx0, vb);
                const uint4 c01 = load8_or_zero(r0 + row, in && f.vy0 && f.vx1, vb);
                const uint4 c10 = load8_or_zero(r1, in && f.vy1 && f.vx0, vb);
                const uint4 c11 = load8_or_zero(r1 + row, in && f.vy1 && f.vx1, vb);
                const float w00 = f.wy0 * f.wx0 * a, w01 = f.wy0 * f.wx1 * a;
                const float w10 = f.wy1 * f.wx0 * a, w11 = f.wy1 * f.wx1 * a;
                float v00[8], v01[8], v10[8], v11[8];
                up8<C>(c00, v00);
                up8<C>(c01, v01);
                up8<C>(c10, v10);
                up8<C>(c11, v11);
#pragma unroll
                for (int i = 0; i < 8; ++i) acc[i] += w00 * v00[i] + w01 * v01[i] + w10 * v10[i] + w11 * v11[i];
            }
        }
        *reinterpret_cast<uint4 *>(out + ((int64_t)b * S + q) * row + c0) = down8<C>(acc);
    }
}

static bool fused_half_dims_ok(int B, int S, int M, int D, int L, int Lq, int P)
{
    if (B <= 0 || S <= 0 || M <= 0 || L <= 0) return false;
    if ((D != 16 && D != 32) || P != FH_P || L > 16 || Lq != S || S % L) return false;
    if (M % (32 / D)) return false;                                               // whole runs of the raw tensor
    return (int64_t)S * M * L * 12 <= 0x7fffffffLL && (int64_t)S * M * D <= 0x7fffffffLL;
}

template <typename C>
static int fused_half_entry(void *stream, const uint16_t *value, const int64_t *shapes, const int64_t *lsi, const float *ref,
                            int64_t ref_bstride, const uint16_t *raw, int raw_q, int B, int S, int M, int D, int L, int P,
                            uint16_t *out)
{
    if (B < 0 || S < 0 || M <= 0 || D <= 0 || L <= 0 || P <= 0 || ref_bstride < 0) return (int)hipErrorInvalidValue;
    if ((int64_t)B * S == 0) return 0;
    if (!value || !shapes || !lsi || !ref || !raw || !out) return (int)hipErrorInvalidValue;
    if (raw_q == 0) raw_q = M * L * P * 3;
    if (raw_q < M * L * P * 3) return (int)hipErrorInvalidValue;
    // 16-byte accesses of value / out, 8-byte accesses of raw (a run of a 32-channel head starts 24 bytes after the last)
    // and of the reference points
    if (!fused_half_dims_ok(B, S, M, D, L, S, P) || !aligned(value, 16) || !aligned(raw, 16) || !aligned(out, 16) ||
        !aligned(ref, 8) || raw_q % 4 || ref_bstride % 2)
        return (int)hipErrorNotSupported;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int chunks = M * D / 8;                                                  // 16-byte chunks of a token row
    const int lpq = chunks % 8 == 0 ? 8 : D / 8;                                   // lanes per (query, workgroup): a 128-byte slice, or one head
    static PerDevice<int> cus_of;
    const int cus = cus_of.get([] {
        int dev = 0, n = 256;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) n = 256;
        return n;
    });
    // (the number of jobs depends on the map shape, which is device data: the kernel strides over its jobs, and a
    // workgroup too many finds none)
    int64_t blocks = ((int64_t)B * S * chunks + FH_THREADS - 1) / FH_THREADS;
    if (blocks > (int64_t)cus * 8) blocks = (int64_t)cus * 8;
    const void *fn = D == 16 ? reinterpret_cast<const void *>(&msda_fwd_fused_half<C, 16>)
                             : reinterpret_cast<const void *>(&msda_fwd_fused_half<C, 32>);
    static PerDevice<KernelResources> res_of[2];
    const KernelResources res = res_of[D == 32].get([fn] { return kernel_resources(fn); });
    msda_note_forward_kernel("msda_fwd_fused_half", &res);
    if (D == 16)
        hipLaunchKernelGGL((msda_fwd_fused_half<C, 16>), dim3((unsigned)blocks), dim3(FH_THREADS), 0, st, value, shapes, lsi, ref,
                           ref_bstride, raw, raw_q, B, S, M, L, lpq, out);
    else
        hipLaunchKernelGGL((msda_fwd_fused_half<C, 32>), dim3((unsigned)blocks), dim3(FH_THREADS), 0, st, value, shapes, lsi, ref,
                           ref_bstride, raw, raw_q, B, S, M, L, lpq, out);
    return (int)hipGetLastError();
}

}  // namespace mvdetr

extern "C" {

int mvdetr_msda_fused_half_supported(int batch, int spatial_size, int num_heads, int channels, int num_levels, int num_query,
                                     int num_point)
{
    return mvdetr::fused_half_dims_ok(batch, spatial_size, num_heads, channels, num_levels, num_query, num_point) ? 1 : 0;
}

int mvdetr_msda_forward_fused_f16(void *stream, const uint16_t *value, const int64_t *spatial_shapes,
                                  const int64_t *level_start_index, const float *reference_points, int64_t ref_batch_stride,
                                  const uint16_t *raw, int raw_query_stride, int batch, int spatial_size, int num_heads,
                                  int channels, int num_levels, int num_point, uint16_t *out)
{
    return mvdetr::fused_half_entry<mvdetr::F16>(stream, value, spatial_shapes, level_start_index, reference_points,
                                                 ref_batch_stride, raw, raw_query_stride, batch, spatial_size, num_heads,
                                                 channels, num_levels, num_point, out);
}

int mvdetr_msda_forward_fused_bf16(void *stream, const uint16_t *value, const int64_t *spatial_shapes,
                                   const int64_t *level_start_index, const float *reference_points, int64_t ref_batch_stride,
                                   const uint16_t *raw, int raw_query_stride, int batch, int spatial_size, int num_heads,
                                   int channels, int num_levels, int num_point, uint16_t *out)
{
    return mvdetr::fused_half_entry<mvdetr::BF16>(stream, value, spatial_shapes, level_start_index, reference_points,
                                                  ref_batch_stride, raw, raw_query_stride, batch, spatial_size, num_heads,
                                                  channels, num_levels, num_point, out);
}

}  // extern "C"

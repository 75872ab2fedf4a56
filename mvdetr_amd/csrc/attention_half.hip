// Fused multi-head attention in 16-bit storage (float16 / bfloat16), forward only -- gfx950 (MI355X).
//   out[b,h,i,:] = sum_j softmax_j(scale * q[b,h,i,:] . k[b,h,j,:]) * v[b,h,j,:],  scale = 1 / sqrt(D), D = 16 or 32,
// no dropout, no lse, no masks.  q, k, v, out are raw 16-bit words addressed by the element strides (batch, head, token)
// of the fp32 entries with the channel contiguous; every row starts 16-byte aligned.  The house contract of half_types.h:
// 16-bit storage, fp32 arithmetic, ONE rounding on the way out.
//
// attn_fwd_mfma_half<Conv, D, NQW> is attn_fwd_mfma (attention.hip) on v_mfma_f32_32x32x16_{f16,bf16}: a workgroup =
// 2 NQW waves = 32 NQW queries of one (batch, head); wave w owns 32 queries (w % NQW) and one 32-key half (w / NQW) of every
// 64-key tile pair (K row-major and V transposed in LDS, double-buffered, the next pair's global loads in flight during the
// MFMAs).  Lane (r = lane & 31, h = lane >> 5):
//   S^T = K Q^T   A = K[key r][channel 16 s + 8 h + j] (one 16-byte LDS read per 16 channels), B = the lane's own query row
//                 (registers, the same channels).  Products of 16-bit numbers are exact in fp32 and the accumulator is fp32:
//                 S is what the fp32 kernel computes on the upcast inputs.  The lane holds S^T[key crow(e, h)][query r].
//   softmax       fp32, online, in registers: exp2 of scores already reduced by the running maximum, as in attn_fwd_mfma.
//   O^T += V^T P^T  the probabilities are the B operand straight from their registers: element j of k-step s is register
//                 8 s + j, i.e. key crow(8 s + j, h), and V^T lies in LDS with key x at column tpos(x) = 16 h + e, so the A
//                 operand of k-step s is 16 contiguous bytes at column 16 h + 8 s.  P is NOT rounded to 16 bits once (that
//                 alone is 2^-9 / 2^-12 of every term): it is split into hi = rn16(P) and lo = rn16(P - hi), one MFMA each on
//                 the same V operand, which leaves 2^-18 (bf16) / 2^-22 (fp16) of P.
//   fp16 range    P <= 1, so hi is a subnormal half below 2^-14 and lo nearly always; nothing here depends on what the MFMA
//                 does with subnormal operands: P is scaled by 2^14 (l, the row sum, with it: the final o / l does not see
//                 it), a hi below 2^-14 is sent to 0 (the lo term then carries that probability whole), and lo is scaled by
//                 another 2^11 into an accumulator of its own, folded in as o_hi + 2^-11 o_lo before the merge.  Both scalings
//                 are by powers of two: exact.  What is lost is below 2^-39 of the row's largest probability.
//   tails         keys >= Sk are zeros in LDS (load8_or_zero: memory is not touched) and their scores are -inf before the
//                 maximum; query rows >= Sq are clamped for the load and never stored.
// No scratch, no atomics; every output element is owned by one lane: bit-reproducible run to run.
#include "../../include/mvdetr_ops.h"
#include "attention.h"
#include "half_mfma.h"

namespace mvdetr {

struct AttnHalfP {
    int B, H, Sq, Sk;
    int64_t q[3], k[3], v[3], o[3];                          // element strides: batch, head, token
};

__device__ __forceinline__ int ah_tpos(int x) { return 16 * ((x >> 2) & 1) + (x & 3) + 4 * (x >> 3); }

constexpr float AH_LOG2E = 1.4426950408889634f;
constexpr float AH_P_SCALE = 16384.f;                        // 2^14: fp16 probabilities (module comment)

// registers 8 s .. 8 s + 7 of p as the hi and lo fragments of k-step s (fp16: p carries AH_P_SCALE, lo HALF_LO_SCALE more)
template <typename Conv> __device__ __forceinline__ void ah_split(const floatx16 &p, int s, uint4 &hi, uint4 &lo)
{
    uint32_t wh[4], wl[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) split2<Conv, false>(p[8 * s + 2 * j], p[8 * s + 2 * j + 1], wh[j], wl[j]);
    hi = make_uint4(wh[0], wh[1], wh[2], wh[3]);
    lo = make_uint4(wl[0], wl[1], wl[2], wl[3]);
}

// A 64-key tile pair of K and of V in registers: item f < 64 D / 8 is 8 channels of a K row, the next 64 D / 8 of a V row.
template <int D, int NT> struct AttnHalfTile {
    static constexpr int C8 = D / 8, ITEMS = 64 * C8, N = (2 * ITEMS + NT - 1) / NT, LDK = D + 8, LDV = 40;
    uint4 v[N];
    __device__ __forceinline__ void fetch(const uint16_t *kb, int64_t ks, const uint16_t *vb, int64_t vs, int key0, int Sk, int t)
    {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const int f = t + NT * i, g = f & (ITEMS - 1), key = g / C8, c8 = g - key * C8;
            const bool isv = f >= ITEMS;
            const bool ok = f < 2 * ITEMS && key0 + key < Sk;
            const uint16_t *base = isv ? vb : kb;
            v[i] = load8_or_zero(base + (int64_t)(key0 + key) * (isv ? vs : ks) + 8 * c8, ok, base);
        }
    }
    // K: row-major [2][32][D + 8]; V: transposed [2][D][40], key x of a half at column tpos(x)
    __device__ __forceinline__ void put(uint16_t (*sk)[32][LDK], uint16_t (*sv)[D][LDV], int t) const
    {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const int f = t + NT * i, g = f & (ITEMS - 1), key = g / C8, c8 = g - key * C8;
            if (f >= 2 * ITEMS) continue;
            if (f < ITEMS) {
                *reinterpret_cast<uint4 *>(&sk[key >> 5][key & 31][8 * c8]) = v[i];
            } else {
                const int pos = ah_tpos(key & 31);
                uint16_t(*dst)[LDV] = sv[key >> 5];
                const uint32_t w[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    dst[8 * c8 + 2 * j][pos] = (uint16_t)(w[j] & 0xffffu);
                    dst[8 * c8 + 2 * j + 1][pos] = (uint16_t)(w[j] >> 16);
                }
            }
        }
    }
};

template <typename Conv, int D, int NQW>
__global__ __launch_bounds__(128 * NQW) void attn_fwd_mfma_half(const uint16_t *__restrict__ q, const uint16_t *__restrict__ k,
                                                                 const uint16_t *__restrict__ v, uint16_t *__restrict__ out,
                                                                 AttnHalfP p)
{
    constexpr int NT = 128 * NQW, KST = D / 16;
    constexpr bool FP16 = std::is_same<Conv, F16>::value;
    using Tile = AttnHalfTile<D, NT>;
    __shared__ __attribute__((aligned(16))) uint16_t sK[2][2][32][Tile::LDK];      // [buffer][half] K tile [key][d]
    __shared__ __attribute__((aligned(16))) uint16_t sVt[2][2][D][Tile::LDV];      // V tile transposed [d][tpos(key)]
    __shared__ float sMerge[NQW][18][64];                                          // the second key half's O, max, sum
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
    const int qw = wave % NQW, ks = wave / NQW;
    const int b = blockIdx.z, hd = blockIdx.y;
    const int q0 = blockIdx.x * (32 * NQW) + qw * 32, qi = q0 + r;
    const bool active = q0 < p.Sq, qv = qi < p.Sq;
    const uint16_t *kb = k + b * p.k[0] + hd * p.k[1];
    const uint16_t *vb = v + b * p.v[0] + hd * p.v[1];
    const float scale = 1.f / sqrtf((float)D), c2 = scale * AH_LOG2E;

    uint4 qr[KST];                                           // channels 16 s + 8 h .. + 7 of the lane's query
    {
        const uint16_t *qp = q + b * p.q[0] + hd * p.q[1] + (int64_t)(qv ? qi : 0) * p.q[2];
#pragma unroll
        for (int s = 0; s < KST; ++s) qr[s] = *reinterpret_cast<const uint4 *>(qp + 16 * s + 8 * h);
    }
    floatx16 o, o2;                                          // o2: the fp16 lo term's accumulator (unused for bf16)
#pragma unroll
    for (int e = 0; e < 16; ++e) o[e] = o2[e] = 0.f;
    float m = -3.0e38f, l = 0.f;

    const int nt = (p.Sk + 63) / 64;
    Tile tile;
    tile.fetch(kb, p.k[2], vb, p.v[2], 0, p.Sk, t);
    tile.put(sK[0], sVt[0], t);
    __syncthreads();
    for (int kt = 0; kt < nt; ++kt) {
        const int buf = kt & 1, key0 = kt * 64 + ks * 32;
        if (kt + 1 < nt) tile.fetch(kb, p.k[2], vb, p.v[2], (kt + 1) * 64, p.Sk, t);
        if (active && key0 < p.Sk) {
            floatx16 s;
#pragma unroll
            for (int e = 0; e < 16; ++e) s[e] = 0.f;
#pragma unroll
            for (int c = 0; c < KST; ++c)
                s = mfma16<Conv>(*reinterpret_cast<const uint4 *>(&sK[buf][ks][r][16 * c + 8 * h]), qr[c], s);
            if (key0 + 32 > p.Sk) {
#pragma unroll
                for (int e = 0; e < 16; ++e)
                    if (key0 + mfma_crow(e, h) >= p.Sk) s[e] = -INFINITY;
            }
            float mx = s[0];
#pragma unroll
            for (int e = 1; e < 16; ++e) mx = fmaxf(mx, s[e]);
            mx = fmaxf(mx, __shfl_xor(mx, 32));
            const float mn = fmaxf(m, mx);
            const float alpha = __builtin_amdgcn_exp2f((m - mn) * c2);
            float ls = 0.f;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                s[e] = __builtin_amdgcn_exp2f((s[e] - mn) * c2);
                if (FP16) s[e] *= AH_P_SCALE;
                ls += s[e];
            }
            l = l * alpha + ls;
            m = mn;
            if (__any(alpha != 1.f)) {                       // (no lane's maximum moved: most tiles after the first few)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    o[e] *= alpha;
                    if (FP16) o2[e] *= alpha;
                }
            }
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const uint4 a = *reinterpret_cast<const uint4 *>(&sVt[buf][ks][r & (D - 1)][16 * h + 8 * c]);
                uint4 hi, lo;
                ah_split<Conv>(s, c, hi, lo);
                o = mfma16<Conv>(a, hi, o);
                if (FP16)
                    o2 = mfma16<Conv>(a, lo, o2);
                else
                    o = mfma16<Conv>(a, lo, o);
            }
        }
        if (kt + 1 < nt) tile.put(sK[buf ^ 1], sVt[buf ^ 1], t);
        __syncthreads();
    }
    if (FP16) {
#pragma unroll
        for (int e = 0; e < 16; ++e) o[e] += o2[e] * (1.f / HALF_LO_SCALE);
    }
    if (ks == 1) {
#pragma unroll
        for (int e = 0; e < 16; ++e) sMerge[qw][e][lane] = o[e];
        sMerge[qw][16][lane] = m;
        sMerge[qw][17][lane] = l;
    }
    __syncthreads();
    if (ks == 1 || !qv) return;
    {
        // (a half that saw no key has m = -3e38 and l = 0: its weight underflows to 0)
        const float m1 = sMerge[qw][16][lane], l1 = sMerge[qw][17][lane];
        const float mt = fmaxf(m, m1);
        const float a0 = __builtin_amdgcn_exp2f((m - mt) * c2), a1 = __builtin_amdgcn_exp2f((m1 - mt) * c2);
#pragma unroll
        for (int e = 0; e < 16; ++e) o[e] = o[e] * a0 + sMerge[qw][e][lane] * a1;
        l = l * a0 + l1 * a1;
    }
    l += __shfl_xor(l, 32);
    const float inv_l = 1.f / l;
    // registers 4 g .. 4 g + 3 are channels 8 g + 4 h .. + 3 of the lane's query: one 8-byte store each
    uint16_t *op = out + b * p.o[0] + hd * p.o[1] + (int64_t)qi * p.o[2];
#pragma unroll
    for (int g = 0; g < D / 8; ++g)
        *reinterpret_cast<uint2 *>(op + 8 * g + 4 * h) = make_uint2(down2<Conv>(o[4 * g] * inv_l, o[4 * g + 1] * inv_l),
                                                                    down2<Conv>(o[4 * g + 2] * inv_l, o[4 * g + 3] * inv_l));
}

// queries per workgroup: 128 (NQW = 4) or 64 (NQW = 2), four lanes per query.  mvdetr_attn_half_set_query_tile forces one
// (tests, tools); 0 = by the shape (attn_route).  (At 2,700 tokens x 8 heads 128 is the faster of the two although it fills only
// 176 of 256 compute units: docs/notes/attention_half.md.)
std::atomic<int> g_ah_query_tile{0};

template <typename Conv> static void attn_launch_half(const AttnCall &c)
{
    const AttnRoute &r = c.r;
    AttnHalfP p;
    p.B = c.p.B; p.H = c.p.H; p.Sq = c.p.Sq; p.Sk = c.p.Sk;
    for (int j = 0; j < 3; ++j) p.q[j] = c.p.q[j], p.k[j] = c.p.k[j], p.v[j] = c.p.v[j], p.o[j] = c.p.o[j];
    const dim3 grid(r.grid.x, r.grid.y, r.grid.z);
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(4 * r.tile), 0, c.st, (const uint16_t *)c.q, (const uint16_t *)c.k, (const uint16_t *)c.v,
                           (uint16_t *)c.out, p);
    };
    if (r.D == 16) launch(r.tile == 64 ? attn_fwd_mfma_half<Conv, 16, 2> : attn_fwd_mfma_half<Conv, 16, 4>);
    else launch(r.tile == 64 ? attn_fwd_mfma_half<Conv, 32, 2> : attn_fwd_mfma_half<Conv, 32, 4>);
}

int attn_launch_forward_half(const AttnCall &c)
{
    if (c.type == AttnType::f16) attn_launch_half<F16>(c);
    else attn_launch_half<BF16>(c);
    return (int)hipGetLastError();
}

}  // namespace mvdetr

using namespace mvdetr;

extern "C" {

int mvdetr_attn_half_set_query_tile(int queries)
{
    if (queries != 0 && queries != 64 && queries != 128) return -1;
    return g_ah_query_tile.exchange(queries);
}

#define MVDETR_ATTN_HALF_ENTRY(SFX, TYPE)                                                                                    \
    int mvdetr_attn_forward_##SFX(void *stream, const uint16_t *q, const uint16_t *k, const uint16_t *v, const int64_t *strides, \
                                  int batch, int heads, int sq, int sk, int head_dim, uint16_t *out)                         \
    {                                                                                                                        \
        return attn_entry(AttnEntry::forward_half, AttnCall{(hipStream_t)stream, TYPE, nullptr, q, k, v, out, nullptr, nullptr, nullptr, \
                                                            nullptr, nullptr, {}, {}}, strides, batch, heads, sq, sk, head_dim, 0.0, 0); \
    }

MVDETR_ATTN_HALF_ENTRY(f16, AttnType::f16)
MVDETR_ATTN_HALF_ENTRY(bf16, AttnType::bf16)

}  // extern "C"

// Multi-scale deformable attention for deformable-ENCODER calls: the locality probe the forward tile kernels and the two-kernel
// backward launch in front of themselves -- gfx950 (MI355X).  What it writes and who reads it: msda_dispatch.h.
// (The grad_value kernels that lived here: docs/notes/backward_kernels_rounds_1_to_5.md.)
#include "common.h"
#include "msda_dispatch.h"
#include "msda_tile.h"

namespace mvdetr {

// Samples MSDA_PROBE_SAMPLES taps spread over the whole call -- block b samples head b % M -- and counts those within
// MSDA_PROBE_RADIUS pixels of their own query's cell (equal level shapes assumed; with unequal ones the count is ignored
// anyway); per head it also sums the displacement of the sampled taps from their cells (msda_dispatch.h).
__global__ __launch_bounds__(256) void msda_locality_probe(const float *__restrict__ loc, const int64_t *__restrict__ shapes,
                                                           int B, int S, int M, int L, int *__restrict__ probe)
{
    __shared__ int red[4][3];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int H = (int)shapes[0], W = (int)shapes[1];
    const int head = blockIdx.x % M;
    const int64_t per_head = (int64_t)B * S * L * TILE_P;     // taps of one head
    // a fixed odd stride walks the (query, level, point) space of the block's head evenly
    const int64_t u = (int64_t)(((unsigned long long)i * 0x9E3779B97F4A7C15ull) % (unsigned long long)per_head);
    const int64_t bq = u / ((int64_t)L * TILE_P);
    const int64_t t = (bq * M + head) * L * TILE_P + (u - bq * L * TILE_P);
    const int cell = (int)((bq % S) % ((int64_t)H * W));
    const float x = loc[2 * t] * (float)W - 0.5f, y = loc[2 * t + 1] * (float)H - 0.5f;
    const float dx = x - (float)(cell % W), dy = y - (float)(cell / W);
    const bool in = i < MSDA_PROBE_SAMPLES;
    const bool hit = in && fabsf(dx) <= MSDA_PROBE_RADIUS && fabsf(dy) <= MSDA_PROBE_RADIUS;
    const bool near = in && fabsf(dx) <= 16.f && fabsf(dy) <= 16.f;      // (NaN: false)
    int sx = near ? (int)rintf(dx * 16.f) : 0, sy = near ? (int)rintf(dy * 16.f) : 0, sn = near ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sx += __shfl_xor(sx, o, 64);
        sy += __shfl_xor(sy, o, 64);
        sn += __shfl_xor(sn, o, 64);
    }
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = sx; red[threadIdx.x >> 6][1] = sy; red[threadIdx.x >> 6][2] = sn; }
    const int n = __syncthreads_count(hit);
    if (threadIdx.x == 0) {
        if (n) atomicAdd(probe, n);
        if (head < MSDA_PROBE_MAXHEADS) {
            atomicAdd(probe + 1 + 3 * head, red[0][0] + red[1][0] + red[2][0] + red[3][0]);
            atomicAdd(probe + 1 + 3 * head + 1, red[0][1] + red[1][1] + red[2][1] + red[3][1]);
            atomicAdd(probe + 1 + 3 * head + 2, red[0][2] + red[1][2] + red[2][2] + red[3][2]);
        }
    }
}

int msda_launch_locality_probe(hipStream_t st, const float *loc, const int64_t *shapes, int B, int S, int M, int L, int *probe)
{
    hipError_t e = hipMemsetAsync(probe, 0, MSDA_PROBE_INTS * sizeof(int), st);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(msda_locality_probe, dim3(MSDA_PROBE_SAMPLES / 256), dim3(256), 0, st, loc, shapes, B, S, M, L, probe);
    return (int)hipGetLastError();
}

}  // namespace mvdetr

// What an instruction beside v_mfma_f32_32x32x2_f32 costs, at one and at two waves per SIMD (gfx950).
//
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 tools/mfma_issue_probe.hip -o tools/mfma_issue_probe
//   timeout -k 10 60 tools/mfma_issue_probe          (run once; the table belongs in profiles/mfma_f32_issue_probe.txt)
//
// Every SIMD issues the same MFMAs in every cell: 2,000 rounds of sixteen MFMAs on independent accumulators, from one wave
// with sixteen accumulators (256 threads per workgroup) or from two waves with eight each (512 threads).  Behind every MFMA
// sit F fillers of one kind: v_add_f32, ds_read2st64_b32 or ds_read_b128, the reads conflict-free on LDS the kernel fills
// itself.  256 workgroups, one per CU (96 KB of LDS each), no global memory beyond one result word that is never written.
// Prints ns per MFMA per SIMD; a bare MFMA is 64 cycles.  conv3x3_winograd_f32 (mvdetr_amd/csrc/conv_winograd.hip) is the
// one-wave case: docs/notes/conv_winograd.md.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <utility>

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using f32x2 = __attribute__((ext_vector_type(2))) float;
typedef __attribute__((address_space(3))) float lds_float;

constexpr int ROUNDS = 2000, MFMAS = 16, LDS_BYTES = 96 * 1024, FILLED = 8192, GRID = 256;
static const char *const kKinds[3] = {"v_add_f32", "ds_read2st64_b32", "ds_read_b128"};

#define CHECK(e)                                                                                  \
    do {                                                                                          \
        const hipError_t rc_ = (e);                                                               \
        if (rc_ != hipSuccess) {                                                                  \
            std::fprintf(stderr, "%s: %s\n", #e, hipGetErrorString(rc_));                         \
            std::exit(1);                                                                         \
        }                                                                                         \
    } while (0)

template <int KIND, int F, int THREADS>
__global__ __launch_bounds__(THREADS) void probe(float *out)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int NACC = MFMAS * 256 / THREADS;                               // 16 per wave, or 8 for each wave of a pair
    for (int i = threadIdx.x; i < FILLED; i += THREADS) lds[i] = 1.0f + (float)(i & 7);
    __syncthreads();
    const unsigned lane = threadIdx.x & 63;
    const unsigned base = (unsigned)(size_t)(lds_float *)lds;
    const unsigned a32 = base + lane * 4, a128 = base + lane * 16;            // a lane's own bank(s): no conflict
    const float av = lds[lane], bv = lds[64 + lane];
    f32x16 acc[NACC];
#pragma unroll
    for (int a = 0; a < NACC; ++a) acc[a] = f32x16{};
    float f[4] = {av, bv, av + bv, av - bv};
    f32x2 r2[4] = {};
    f32x4 r4[4] = {};
#pragma unroll 1
    for (int round = 0; round < ROUNDS; ++round) {
#pragma unroll
        for (int a = 0; a < NACC; ++a) {
            acc[a] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[a], 0, 0, 0);
#pragma unroll
            for (int k = 0; k < F; ++k) {
                if (KIND == 0) asm volatile("v_add_f32 %0, %0, %1" : "+v"(f[k]) : "v"(bv));
                if (KIND == 1) asm volatile("ds_read2st64_b32 %0, %1 offset0:%2 offset1:%3" : "+v"(r2[k]) : "v"(a32), "n"(2 * k), "n"(2 * k + 1));
                if (KIND == 2) asm volatile("ds_read_b128 %0, %1 offset:%2" : "+v"(r4[k]) : "v"(a128), "n"(1024 * k));
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    // every result ends in an empty statement where it is (summed up, the 256 accumulator registers are copied out at
    // once and the allocator spills inside the loop to make room)
#pragma unroll
    for (int k = 0; k < 4; ++k) asm volatile("" ::"v"(f[k]), "v"(r2[k]), "v"(r4[k]));
#if defined(__HIP_DEVICE_COMPILE__)                                           // (register classes of the device)
#pragma unroll
    for (int a = 0; a < NACC; ++a) {
        if (NACC == 16) asm volatile("" ::"a"(acc[a]));
        else asm volatile("" ::"v"(acc[a]));
    }
#endif
    if (av == -1.5f) out[0] = bv;                                             // (LDS holds 1 .. 8: never)
}

template <int KIND, int F, int THREADS>
static float ns_per_mfma(float *out, hipEvent_t e0, hipEvent_t e1)
{
    const auto kernel = probe<KIND, F, THREADS>;
    CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES));
    hipLaunchKernelGGL(kernel, dim3(GRID), dim3(THREADS), LDS_BYTES, 0, out);     // once unmeasured
    CHECK(hipEventRecord(e0, 0));
    hipLaunchKernelGGL(kernel, dim3(GRID), dim3(THREADS), LDS_BYTES, 0, out);
    CHECK(hipEventRecord(e1, 0));
    CHECK(hipEventSynchronize(e1));
    CHECK(hipGetLastError());
    float ms = 0.f;
    CHECK(hipEventElapsedTime(&ms, e0, e1));
    return ms * 1e6f / ((float)ROUNDS * MFMAS);
}

template <int KIND, int THREADS, int... F>
static void row(float *out, hipEvent_t e0, hipEvent_t e1, std::integer_sequence<int, F...>)
{
    std::printf("%-18s %d waves/SIMD ", kKinds[KIND], THREADS / 256);
    const float ns[] = {ns_per_mfma<KIND, F, THREADS>(out, e0, e1)...};
    for (const float v : ns) std::printf(" %7.2f", v);
    std::printf("   per filler %+6.2f\n", (ns[sizeof...(F) - 1] - ns[0]) / (float)(sizeof...(F) - 1));
}

int main()
{
    float *out = nullptr;
    hipEvent_t e0, e1;
    CHECK(hipMalloc(&out, sizeof(float)));
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    std::printf("# ns per v_mfma_f32_32x32x2_f32 per SIMD, %d rounds x %d MFMAs, %d workgroups; F fillers behind every MFMA\n", ROUNDS, MFMAS, GRID);
    std::printf("# filler             waves          F = 0       1       2       3       4   (last - first) / 4\n");
    const std::make_integer_sequence<int, 5> fs;
    row<0, 256>(out, e0, e1, fs);
    row<0, 512>(out, e0, e1, fs);
    row<1, 256>(out, e0, e1, fs);
    row<1, 512>(out, e0, e1, fs);
    row<2, 256>(out, e0, e1, fs);
    row<2, 512>(out, e0, e1, fs);
    CHECK(hipDeviceSynchronize());
    CHECK(hipFree(out));
    return 0;
}

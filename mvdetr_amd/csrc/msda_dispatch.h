// Internal dispatch between the MSDA kernel variants, forward and backward (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "msda_backward_route.h"
#include "msda_forward_route.h"
#include "msda_tile.h"

namespace mvdetr {

// name of the kernel the last forward on this thread launched (bench / tests only; set by the launchers)
// what the code object says about a kernel (hipFuncGetAttributes): registers per lane, scratch (spill) bytes per lane,
// static LDS bytes.  Queried once per instantiation by the launchers and reported through
// mvdetr_msda_last_forward_resources().
struct KernelResources {
    int num_regs, scratch_bytes, static_lds_bytes;
};
inline KernelResources kernel_resources(const void *func)
{
    hipFuncAttributes at;
    if (hipFuncGetAttributes(&at, func) != hipSuccess) return KernelResources{-1, -1, -1};
    return KernelResources{at.numRegs, (int)at.localSizeBytes, (int)at.sharedSizeBytes};
}
void msda_note_forward_kernel(const char *name, const KernelResources *res = nullptr);

// options of a camera-grouped launch (MsdaFwdCall::opts, the kernels' `opts` argument)
#define GROUP_OPT_NO_SHIFT 1      // keep the windows centred on the tile (A/B knob MVDETR_MSDA_WINDOW_SHIFT=0)
#define GROUP_OPT_BLOCKS 2        // XCD k takes a 2-D block of the tile grid instead of a band of the job list
#define GROUP_OPT_STANDDOWN 4     // (msda_fwd_group2, public contract) a job whose taps are far from its cells gathers instead

// One fp32 forward call as every launcher below receives it (host only, never a kernel parameter).  The public and the fused
// contract share the kernels' argument slots: loc / aw hold final sampling locations and attention weights (ref_mode 0, ref
// unused), or the raw offsets and logits next to reference points [.., Lq, L, P, 2] (ref_mode 1) or one reference point per
// (query, level) (ref_mode 2).  stats: where the training entry wants its softmax statistics, or null.  probe:
// msda_launch_locality_probe's scratch, or null (no probe)
struct MsdaFwdCall {
    hipStream_t st;
    const float *value;
    const int64_t *shapes, *lsi;
    const float *loc, *aw;
    const float *ref;
    int64_t ref_bstride;
    SamplingLayout lay;
    QueryLevels qr;
    int ref_mode;
    int B, S, M, D, L;
    float *out, *stats;
    const int *probe;
    int opts;
};

// The launchers of msda_forward_route.h's routes; which of them a call takes is decided there, they only pick the instantiation
// from D, L and ref_mode.
// LDS-tiled encoder kernel (msda_forward_tile.hip)
int msda_forward_tile(const MsdaFwdCall &c);
// camera-grouped kernels: 6 / 7 cameras, software-pipelined (msda_forward_group.hip); 9..16 cameras, 4 lane groups x up to 4
// cameras (msda_forward_group_many.hip)
int msda_forward_group2(const MsdaFwdCall &c);
int msda_forward_group_many(const MsdaFwdCall &c);
// the fused training forward's statistics -- (maximum, 1 / sum exp) of a (query, head)'s L x P logits -- for calls whose forward
// kernel does not write them itself (the camera-grouped kernels do): msda_forward_tile.hip
int msda_softmax_stats(hipStream_t st, const float *logits, SamplingLayout lay, int64_t queries, int M, int L, float *stats);

// One backward call as every launcher below receives it (host only, never a kernel parameter).  The public and the fused
// contract share the kernels' argument slots: loc / aw hold sampling locations and attention weights, or (fused) the raw
// offsets+logits tensor and the forward's softmax statistics; grad_loc / grad_aw their gradients, or grad_raw and null.
// ref, ref_bstride, raw_q, out_fwd: null / 0 for the public contract.
struct MsdaBwdCall {
    hipStream_t st;
    const float *go, *value;
    const int64_t *shapes, *lsi;
    const float *loc, *aw;
    const float *ref;
    int64_t ref_bstride;
    int raw_q;
    const float *out_fwd;
    bool fused;
    int B, S, M, D, L;
    float *grad_value, *grad_loc, *grad_aw;
};

// The launchers of msda_backward_route.h's routes; which of them a call takes is decided there, they only pick the instantiation.
// grad_value through token-major fixed-point LDS windows (msda_backward_value_tok.hip).  probe: msda_launch_locality_probe's
// scratch (public contract), or null
int msda_backward_value_tok(const MsdaBwdCall &c, const int *probe);
// grad_sampling_loc / grad_attn_weight (fused: grad_raw) from LDS-staged value windows (msda_backward_sampling.hip): the resident
// or the level-groups kernel.  probe null: the kernel takes its own sample and skips the tiles the grad_value kernel took along
int msda_backward_sampling(const MsdaBwdCall &c, MsdaBwdSampling which, const int *probe);
// the same for 6 / 7 levels of 16-channel heads on the raw tensor (msda_backward_fused.hip)
int msda_backward_fused_sampling(const MsdaBwdCall &c);
// the whole encoder-shaped fp32 backward in ONE kernel (msda_backward_onepass.hip): 16-channel heads; no probe, no scratch.
// opts: bit 0 = stand-down (a far job computes its taps in the lane-group formulation)
int msda_backward_onepass(const MsdaBwdCall &c, int opts);
// the grad_value half of the same kernel alone (no value window, no dot products): units of L level jobs, guessed fixed-point
// scale, in-kernel window shift and stand-down; job order from MVDETR_MSDA_BWD_ORDER
int msda_backward_scatter(const MsdaBwdCall &c, int opts);
// the one-pass kernel with grad_value summed in 64-bit fixed point (one binary point per call): bit-reproducible run to run.  Opt-in
// (mvdetr_msda_set_backward_deterministic / MVDETR_MSDA_BWD_DETERMINISTIC=1); scratch of 8 bytes per value element, cached per (device, stream)
int msda_backward_deterministic(const MsdaBwdCall &c);
int msda_release_det_scratch();

// device-side locality probe (msda_locality_probe.hip) shared by the kernels of a call (stream-ordered scratch of MSDA_PROBE_INTS ints):
//   probe[0]              how many of MSDA_PROBE_SAMPLES sampled taps lie within MSDA_PROBE_RADIUS pixels of their own query cell
//   probe[1 + 3 m + 0..2] for head m (< MSDA_PROBE_MAXHEADS): sum of the sampled taps' x / y displacement from their own cell in
//                         1/16 px, and how many were summed (those within 16 px) -- where that head's taps lie.  MSDeformAttn's
//                         offset bias is a ray per head (ms_deform_attn.py:64-69), so windows centred on the cell lose the
//                         far points of the ray; the LDS-tiled backward kernels shift their windows by msda_probe_shift().
#define MSDA_PROBE_SAMPLES 16384
#define MSDA_PROBE_RADIUS 5.5f
// a call stands down to the generic formulation when fewer than 1 / MSDA_PROBE_NEAR_DIV of the sampled taps are near (round 4's
// noise sweep: with a half, the backward left the windows at a spread of 6 px, 3.08 ms where they take 1.93; a quarter keeps them)
#ifndef MSDA_PROBE_NEAR_DIV
#define MSDA_PROBE_NEAR_DIV 4
#endif
#define MSDA_PROBE_MAXHEADS 64
#define MSDA_PROBE_INTS (1 + 3 * MSDA_PROBE_MAXHEADS)
#define MSDA_PROBE_MAXSHIFT 3
__device__ __forceinline__ void msda_probe_shift(const int *__restrict__ probe, int head, int &sx, int &sy)
{
    sx = sy = 0;
    if (!probe || head >= MSDA_PROBE_MAXHEADS) return;
    const int n = probe[1 + 3 * head + 2];
    if (n <= 0) return;
    const float inv = 1.f / (16.f * (float)n);
    sx = max(-MSDA_PROBE_MAXSHIFT, min(MSDA_PROBE_MAXSHIFT, (int)rintf((float)probe[1 + 3 * head] * inv)));
    sy = max(-MSDA_PROBE_MAXSHIFT, min(MSDA_PROBE_MAXSHIFT, (int)rintf((float)probe[1 + 3 * head + 1] * inv)));
}
// The same two answers WITHOUT a probe launch (round 5): every wave of a workgroup reduces ONE sample of the job -- 64 lanes'
// worth of (cell, 4 points) locations of camera 0, the job's head and one level, the same sample in every wave -- to the mean
// tap displacement (the window shift) and to whether fewer than 1 / MSDA_PROBE_NEAR_DIV of the sampled taps lie within
// MSDA_PROBE_RADIUS pixels of their own cell (`far`: the job computes its taps in the lane-group formulation instead of
// staging windows).  All waves see the same data and do the same arithmetic: the results are workgroup-uniform without LDS
// or a barrier.  la / lb: the lane's four normalised (x, y) locations; have: the lane holds a cell of the map.
// The tile whose sample decides: the grad_value kernel's (msda_backward_onepass.hip) -- the sampling kernels' 4 x 8 jobs are
// nested in it and repeat ITS sample (first 64 cells, camera 0, level 0), so that both kernels of a backward agree on which
// (tile, head) stand down: the grad_value kernel then computes all three gradients of such a tile in the lane-group
// formulation and the sampling kernel skips it.
#define MSDA_SAMPLE_TH 4
#define MSDA_SAMPLE_TW 16
__device__ __forceinline__ void msda_job_sample(const float4 &la, const float4 &lb, bool have, int qx, int qy, float fW, float fH,
                                                int &shx, int &shy, bool &far)
{
    float sx = 0.f, sy = 0.f, sn = 0.f, snear = 0.f, scnt = 0.f;
    if (have) {
        const float mx = 0.25f * ((la.x + la.z) + (lb.x + lb.z)) * fW - 0.5f - (float)qx;
        const float my = 0.25f * ((la.y + la.w) + (lb.y + lb.w)) * fH - 0.5f - (float)qy;
        if (mx == mx && my == my && fabsf(mx) < 64.f && fabsf(my) < 64.f) { sx = mx; sy = my; sn = 1.f; }
        const float ox_ = (float)qx + 0.5f, oy_ = (float)qy + 0.5f, rr = MSDA_PROBE_RADIUS;
        snear = (float)((fabsf(la.x * fW - ox_) < rr && fabsf(la.y * fH - oy_) < rr) + (fabsf(la.z * fW - ox_) < rr && fabsf(la.w * fH - oy_) < rr) +
                        (fabsf(lb.x * fW - ox_) < rr && fabsf(lb.y * fH - oy_) < rr) + (fabsf(lb.z * fW - ox_) < rr && fabsf(lb.w * fH - oy_) < rr));
        scnt = 4.f;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sx += __shfl_xor(sx, o, 64);
        sy += __shfl_xor(sy, o, 64);
        sn += __shfl_xor(sn, o, 64);
        snear += __shfl_xor(snear, o, 64);
        scnt += __shfl_xor(scnt, o, 64);
    }
    const float tx = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, sx)));
    const float ty = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, sy)));
    const float tn = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, sn)));
    const float tl = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, snear)));
    const float tc = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, scnt)));
    shx = shy = 0;
    if (tn > 0.f) {
        shx = max(-MSDA_PROBE_MAXSHIFT, min(MSDA_PROBE_MAXSHIFT, (int)rintf(tx / tn)));
        shy = max(-MSDA_PROBE_MAXSHIFT, min(MSDA_PROBE_MAXSHIFT, (int)rintf(ty / tn)));
    }
    far = tl * (float)MSDA_PROBE_NEAR_DIV < tc;
}
int msda_launch_locality_probe(hipStream_t st, const float *loc, const int64_t *shapes, int B, int S, int M, int L, int *hits);

}  // namespace mvdetr

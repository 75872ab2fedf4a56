// The device text that the forward Winograd kernels of conv_winograd.hip (and the data gradient, which runs on them) share, each
// piece once: the constants and types of a chunk and of the store, and those parts of the store and of the loader that compile
// to the same instructions as a function as they did written out in every kernel --
//   out_range, out_window      the buffer resources of a unit's outputs and residual
//   out_offsets                a lane's four output offsets: its tile's descriptor plus its channel, saturating
//   bn_fold_channel            the BatchNorm constants of the lane's output channel
//   u_lane_offset              the lane's constant of the LDS-DMA of U with the rotation of the 16-channel wave block
// What is NOT here, because as a shared function it changes the kernels' compiled code (docs/notes/conv_winograd.md has each
// form that was tried): a loader tile's sixteen offsets and descriptor, A^T M A with the epilogue and the stores, the
// hand-written accumulator reads, the transform pieces and operand addresses of the 16-channel wave block, the persistent frame.
// (conv_winograd_backward.hip, the weight gradient, takes the vector types from here.)
#pragma once
#include "bn_epilogue.h"
#include "conv_winograd.h"

namespace mvdetr {
namespace wino {

constexpr int CC = 8;                      // input channels per chunk
constexpr int U_FLOATS = 16 * CC * KB;     // the U slice of a chunk, [p][c][k]: 8,192 floats, first in an LDS buffer

// An output element that is not stored, in a tile's descriptor: the lane's channel is added with unsigned saturation, so it
// stays beyond every range, and a buffer store (or a residual load) at it does nothing
constexpr unsigned Y_NONE = 0xFFFFFFFFu;

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned;

typedef __attribute__((address_space(3))) void lds_void;

// What the output store applies (MODE 0: nothing, and none of this is read).  res has y's [N, H, W, K] geometry.
struct Epilogue {
    BnVectors bn, bn2;
    const float *res;
};

// ---- the store ----------------------------------------------------------------------------------------------------------------
// y (and the residual) of the unit whose first tile is in image n0 and whose channel block is kb go through buffer resources
// that start at that image and channel and end with the tensor: a lane's byte offset is its tile's descriptor plus its channel.
// Raw buffer accesses as for x: an element that is not stored has an offset past the range, for which nothing is written or
// read.  out_range: the bytes from there to the tensor's end, capped at X_RANGE; out_window: the resource of y or of the residual.
__device__ __forceinline__ int out_range(int N, int H, int W, int K, int n0, int kb)
{
    const unsigned long long left = ((unsigned long long)(N - n0) * H * W * K - (unsigned)(kb * KB)) * 4ull;
    return (int)(left < X_RANGE ? (unsigned)left : X_RANGE);
}

__device__ __forceinline__ __amdgpu_buffer_rsrc_t out_window(const float *p, int H, int W, int K, int n0, int kb, int range)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p + (size_t)n0 * H * W * K + kb * KB), 0, range, 0x00020000);
}

// A tile's descriptor plus the lane's channel `kcol` of the block: Y_NONE plus anything saturates
__device__ __forceinline__ void out_offsets(const u32x4 &dsc, int kcol, unsigned (&o4)[4])
{
#pragma unroll
    for (int e = 0; e < 4; ++e) o4[e] = __builtin_elementwise_add_sat(dsc[e], (unsigned)kcol * 4u);
}

// The folded BatchNorm constants of output channel k (MODE 3: bt holds both shifts, bs2 the residual's scale)
template <int MODE>
__device__ __forceinline__ void bn_fold_channel(const Epilogue &ep, int k, float &bs, float &bt, float &bs2)
{
    bn_fold1(ep.bn, k, bs, bt);
    if (MODE == 3) {
        float bt2;
        bn_fold1(ep.bn2, k, bs2, bt2);
        bt = bt + bt2;
    }
}

// ---- the 16-channel wave block (half-unit and 8-wave kernels) ----------------------------------------------------------------
// The lane's constant of the LDS-DMA of U, in bytes: 16 bytes of position tid >> 7, channel c = (tid >> 4) & 7 of the chunk, for LDS
// column (tid & 15) * 4, which holds output channel (column - 16 (c & 1)) mod 64 of the slice (the rotation: conv_winograd.hip)
__device__ __forceinline__ unsigned u_lane_offset(int tid, int C, int K)
{
    return ((unsigned)((tid >> 7) * C + ((tid >> 4) & 7)) * K + ((((tid & 15) * 4) - 16 * ((tid >> 4) & 1)) & 63)) * 4u;
}

}  // namespace wino
}  // namespace mvdetr

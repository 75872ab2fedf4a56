// One perspective-warp call as the C ABI entries of warp_perspective.hip fill it, and the launchers of warp_forward.hip and
// warp_backward.hip they switch into.  A launcher picks the instantiation and launches: what a call may ask for is checked by
// warp_route() (warp_route.h), once, before any of them runs.
#pragma once
#include "common.h"
#include "warp_route.h"

namespace mvdetr {

enum class WarpType { f16, bf16, f32, f64 };

struct WarpCall {
    hipStream_t st;
    WarpType type;
    const void *in;             // the source (forward) or grad_dst (backward)
    const void *M;              // [N, 3, 3] in the tensor's type (float for the 16-bit types)
    void *out;                  // the destination or grad_src
    void *plan;                 // the caller's plan buffer (plan and planned entries)
    int N, C, h, w, H, W;
    uint64_t tag;               // the tagged backward: version tag of the matrices (0: none)
    WarpKnobs knobs;
};

// The argument list most warp kernels share -- (in, M, N, C, h, w, H, W, nearest, [extra ...,] out) -- on the route's grid.
// T: the tensors' storage type, MT: the matrices' type.
template <typename T, typename MT, typename Kernel, typename... Extra>
inline void warp_launch_kernel(Kernel kernel, int threads, size_t lds, const WarpCall &c, const WarpRoute &r, Extra... extra)
{
    hipLaunchKernelGGL(kernel, dim3((unsigned)r.grid), dim3(threads), lds, c.st, static_cast<const T *>(c.in), static_cast<const MT *>(c.M),
                       c.N, c.C, c.h, c.w, c.H, c.W, r.nearest, extra..., static_cast<T *>(c.out));
}

// f(float()) or f(double()): the instantiation of a call of the fp32 / fp64 entries
template <typename F> inline void warp_for_type(WarpType type, F f)
{
    if (type == WarpType::f32) f(float());
    else f(double());
}

// every forward kind
int warp_launch_forward(const WarpCall &c, const WarpRoute &r);
// warp_bwd / warp_bwd_cl into a zeroed grad_src
int warp_launch_scatter(const WarpCall &c, const WarpRoute &r);
// the geometry pass into `plan`; the gather from `plan`; both with the plan in the stream's scratch (reused while c.tag stays)
int warp_launch_plan(const WarpCall &c, char *plan);
int warp_launch_gather(const WarpCall &c, const WarpRoute &r, char *plan);
int warp_launch_gather_scratch(const WarpCall &c, const WarpRoute &r);
// [n, rows, cols] -> [n, cols, rows], elements of 4 or 8 bytes
int warp_launch_transpose(hipStream_t st, int elem_size, const void *src, int n, int rows, int cols, void *dst);

}  // namespace mvdetr

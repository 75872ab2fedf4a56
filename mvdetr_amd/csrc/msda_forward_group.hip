// Multi-scale deformable attention forward, fused + camera-grouped LDS-tiled kernel -- gfx950 (MI355X).
//
// What bounds msda_fwd_tile is the window staging: every (tile, slice, QUERY level) workgroup copies the
// same L source windows into LDS -- 1.35 GB of L2->LDS traffic per launch at Wildtrack size against 0.28 GB
// of algorithmic bytes -- and pays two barriers per level for 4 taps per lane.  In MVDeTr all levels
// (cameras) have the same shape and a cell's queries of all L cameras sample the same windows, so here one
// workgroup owns a (tile, slice) and walks ALL NG = L query levels per staged window: staging, window writes
// and barriers drop by L, the taps per barrier rise by L.  That needs the sampling data of (camera, level)
// when level's window is resident, which the reference layout [Lq, M, L, P] scatters over the tensor; the
// fused path's level-major raw layout [Lq, L, M, P] (a row permutation of the module's Linear) makes it one
// contiguous run per query -- that is where this kernel pays (170 -> 128 us); on the reference layout it is
// only marginally ahead of the tile kernel (188 vs 197 us).
//
// Lane = (cell, half slice) as in the tile kernel, but with NG accumulator sets (one per camera) and NG
// online-softmax states.  The window copy is synchronous (its latency is now amortised over NG x 4 taps),
// which is what frees the registers for the accumulators.
//
// Shapes live on the device, so the kernel itself checks that the levels are equal; if they are not, the
// same launch runs the tile kernel's body instead (msda_tile_body.h) -- no second launch, no host knowledge.
#include "msda_group2_kernel.h"

namespace mvdetr {

#ifdef MVDETR_GROUP_TRACE
__device__ unsigned long long *g_group_trace = nullptr;
#endif

// reads in flight ahead of the FMAs in msda_fwd_group2's tap stream, in pairs (measured at Wildtrack size: 2 and 3 alike, 4
// slower -- registers)
constexpr int GROUP2_DEPTH = 2;

// 6 / 7 cameras: the software-pipelined kernel (msda_group2_kernel.h) for every entry -- fused (raw offsets / logits, one
// or P reference points per (query, level)) and the public contract (final locations / weights)
template <typename Cfg, int L>
static int group2_of_ref_mode(const MsdaFwdCall &c)
{
    return c.ref_mode == 2 ? launch_group2<Cfg, L, 2, GROUP2_DEPTH>(c) : c.ref_mode ? launch_group2<Cfg, L, 1, GROUP2_DEPTH>(c)
                                                                                    : launch_group2<Cfg, L, 0, GROUP2_DEPTH>(c);
}

int msda_forward_group2(const MsdaFwdCall &c)
{
    if (c.D == 16 && c.L == 7) return group2_of_ref_mode<GWide16, 7>(c);
    if (c.D == 16 && c.L == 6) return group2_of_ref_mode<GWide16, 6>(c);
    if (c.D == 32 && c.L == 7) return group2_of_ref_mode<GWide32, 7>(c);
    if (c.D == 32 && c.L == 6) return group2_of_ref_mode<GWide32, 6>(c);
    return (int)hipErrorInvalidValue;
}

}  // namespace mvdetr

#ifdef MVDETR_GROUP_TRACE
// trace builds only: (re)arm the stamp table (zeroed device memory of `workgroups` x 4 x GROUP_TRACE_SLOTS words, or NULL)
extern "C" int mvdetr_debug_group_trace_arm(unsigned long long *table)
{
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(mvdetr::g_group_trace), &table, sizeof(table));
}
#endif

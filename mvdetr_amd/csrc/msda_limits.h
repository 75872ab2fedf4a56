// Shape limits of the LDS-tiled MSDA kernels that host-side dispatch needs as well.  Plain C++ (no HIP): the one definition both
// the kernels (through msda_tile.h / msda_backward_sampling.hip) and msda_backward_route.h read.
#pragma once

namespace mvdetr {

constexpr int TILE_MAX_LEVELS = 16;     // 64-bit miss mask = L * P bits with P == 4
constexpr int TILE_P = 4;
// msda_bwd_sampling_resident: head width, and the levels whose value windows stay in LDS together
constexpr int RS_D = 16, RS_MAXL = 7;

}  // namespace mvdetr

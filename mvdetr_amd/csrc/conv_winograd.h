// What the Winograd F(2x2, 3x3) kernels of conv_winograd.hip (forward) and conv_winograd_backward.hip (weight gradient) share:
// the tile grid of a shape -- every sub-lattice (y mod d, x mod d) of an image has its own grid of 2x2 output tiles -- the
// buffer-load constants, the host entries' offset bounds and CU count, and the process-wide bookkeeping behind
// mvdetr_winograd_last_kernel / _launch_count / _set_max_workgroups.  (The device text they share: conv_winograd_device.h.)
#pragma once
#include "common.h"

#include <atomic>

namespace mvdetr {

extern std::atomic<const char *> g_winograd_last_kernel;
extern std::atomic<int64_t> g_winograd_launches;
extern std::atomic<int> g_winograd_max_workgroups;                            // 0: one per CU (mvdetr_winograd_set_max_workgroups)

namespace wino {

constexpr int TILES = 64;                  // 2x2 output tiles per workgroup
constexpr int KB = 64;                     // output channels per workgroup

// Range of the x buffer resource and the offset of a pixel outside the image (beyond it: the load returns zero)
constexpr unsigned X_RANGE = 0xFFFFFFF0u, X_OUTSIDE = 0xFFFFFFF8u;

struct Shape {
    int N, H, W, C, K, d;
    int py[5], px[5];                      // tile rows (columns) of the sub-lattice rows (columns) before sy (sx): prefix sums of
                                           // th(sy) = (ceil((H - sy) / d) + 1) / 2, zero where H <= sy; py[sy] = TY for sy >= d
    int TY, TX;                            // tile grid of one image: all its sub-lattices
    unsigned tiles;                        // N * TY * TX
    int kblocks;                           // K / 64
    unsigned units;                        // ceil(tiles / 64) * kblocks: 64 tiles x 64 output channels each
    // A workgroup's next unit is G units on (G: the grid): its channel block moves by gr = G % kblocks, and its tile
    // block by G / kblocks, one more where the channel block wraps.  Those two strides of 64 * (G / kblocks + i) tiles
    // as (columns, rows, images) of the tile grid, columns < TX and rows < TY: a position follows by addition.
    int gr;
    int dX0, dY0, dn0, dX1, dY1, dn1;
};

// Where tile `t` sits in the tile grid: column X, row Y, image n (n >= N past the last tile).  Two divisions: once per
// workgroup and lane, for its first unit.
__device__ __forceinline__ void tile_grid(const Shape &s, unsigned t, int &X, int &Y, int &n)
{
    X = (int)(t % (unsigned)s.TX);
    const unsigned r = t / (unsigned)s.TX;
    Y = (int)(r % (unsigned)s.TY);
    n = (int)(r / (unsigned)s.TY);
}

// The same tile of the workgroup's next unit (carry: its channel block wrapped), by addition
__device__ __forceinline__ void tile_step(const Shape &s, bool carry, int &X, int &Y, int &n)
{
    X += carry ? s.dX1 : s.dX0;
    const bool cx = X >= s.TX;
    X -= cx ? s.TX : 0;
    Y += (carry ? s.dY1 : s.dY0) + (cx ? 1 : 0);
    const bool cy = Y >= s.TY;
    Y -= cy ? s.TY : 0;
    n += (carry ? s.dn1 : s.dn0) + (cy ? 1 : 0);
}

// Top-left OUTPUT pixel (y0, x0) of the tile at (X, Y) of the tile grid
__device__ __forceinline__ void tile_pixel(const Shape &s, int X, int Y, int &y0, int &x0)
{
    // the sub-lattice by three compares against the prefix sums (an empty one has the prefix of the next: never chosen)
    const int sy = (Y >= s.py[1]) + (Y >= s.py[2]) + (Y >= s.py[3]);
    const int sx = (X >= s.px[1]) + (X >= s.px[2]) + (X >= s.px[3]);
    const int ty = Y - (Y >= s.py[3] ? s.py[3] : Y >= s.py[2] ? s.py[2] : Y >= s.py[1] ? s.py[1] : 0);
    const int tx = X - (X >= s.px[3] ? s.px[3] : X >= s.px[2] ? s.px[2] : X >= s.px[1] ? s.px[1] : 0);
    y0 = sy + 2 * ty * s.d;
    x0 = sx + 2 * tx * s.d;
}

// The tile grid of a shape and its units; false where there are 2^31 tiles or units or more
inline bool tile_shape(Shape &s, int N, int H, int W, int C, int K, int dilation)
{
    s.N = N; s.H = H; s.W = W; s.C = C; s.K = K; s.d = dilation;
    // every sub-lattice's own tile grid: th(sy) = (ceil((H - sy) / d) + 1) / 2 tile rows, none where H <= sy
    s.py[0] = s.px[0] = 0;
    for (int i = 0; i < 4; ++i) {
        s.py[i + 1] = s.py[i] + (i < dilation && i < H ? ((H - i + dilation - 1) / dilation + 1) / 2 : 0);
        s.px[i + 1] = s.px[i] + (i < dilation && i < W ? ((W - i + dilation - 1) / dilation + 1) / 2 : 0);
    }
    s.TY = s.py[4];
    s.TX = s.px[4];
    const int64_t tiles = (int64_t)N * s.TY * s.TX;
    s.kblocks = K / KB;
    const int64_t blocks = (tiles + TILES - 1) / TILES * s.kblocks;
    if (tiles >= (int64_t)1 << 31 || blocks >= (int64_t)1 << 31) return false;
    s.tiles = (unsigned)tiles;
    s.units = (unsigned)blocks;
    return true;
}

// A lane's byte offsets are 32-bit and count from the image of its workgroup's first tile: 64 tiles span at most
// 256 / (H W) + 2 images (a tile covers at most 4 pixels of one).  C and K are multiples of 8, so the bound keeps every offset
// into x, y or grad_y below 2^32 - 64, under the range of the kernels' buffer resources (X_RANGE)
inline bool offsets_fit(int H, int W, int C, int K) { return (256 + 2 * (int64_t)H * W) * (C > K ? C : K) < (int64_t)1 << 30; }

// U is staged through a buffer resource too, with 32-bit byte offsets from the slice's first column: 64 C K bytes
// (mvdetr_winograd_weights_f32 makes no U above 2^26 elements of (c, k))
inline bool weights_fit(int C, int K) { return (int64_t)C * K < (int64_t)1 << 26; }

// The CUs of the current device: one persistent workgroup each (one fits).  256 where the runtime does not say.
inline int device_cus()
{
    static PerDevice<int> cus_of;
    return cus_of.get([] {
        int dev = 0, n = 256;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
            n = 256;
        return n;
    });
}

}  // namespace wino
}  // namespace mvdetr

// Winograd F(2x2, 3x3) convolution in exact fp32 on the MFMA units, for the ResNet trunk's wide 3x3 convolutions
// (stride 1, padding = dilation, no bias, channel-last activations).
//
//   Y = A^T [ sum_c (G g G^T) .* (B^T d B) ] A          per 2x2 output tile and output channel
//
// The sixteen element-wise products over the input channels are sixteen GEMMs  M_p[tile, k] = sum_c V_p[tile, c] U_p[c, k]
// (p = 4 xi + nu, the position inside the 4x4 transformed tile): 2.25x fewer multiplications than the direct form.
//
//   winograd_weights_f32   U[p][c][k] = (G g G^T)[xi][nu], formed in fp64 and rounded once; runs once per weight tensor.
//   conv3x3_winograd_f32   one launch: a unit of work is 64 tiles x 64 output channels x all 16 positions, run by a workgroup
//                          of 4 waves.
//       * the grid is persistent: G = min(units, CUs) workgroups (140 KB of LDS: one per CU), workgroup g runs the units
//         g, g + G, ... in that order -- no counter, no atomics.  Its chunk pipeline runs through all of them: the staging
//         side, two chunks ahead, has its own (unit, chunk) cursor, so the input loads and LDS-DMA of a unit's first chunks
//         are in flight while the unit before it is stored, and only the first unit pays a cold prologue.  Only the first
//         unit pays divisions too: the host splits the stride of G units into columns, rows and images of the tile grid, and
//         a workgroup's next unit follows by addition;
//       * the store is four buffer stores per accumulator register at byte offsets from a per-tile descriptor in LDS, an
//         element outside the image at an offset that saturates beyond the buffer's range: no branches, no 64-bit addresses;
//       * every wave owns a 32-tile x 32-channel block of ALL sixteen products: 16 accumulators of v_mfma_f32_32x32x2_f32 =
//         256 registers per lane (one wave per SIMD; the fp32 MFMA reaches its issue rate from one wave with independent
//         accumulators), so A^T M A happens in registers -- position p of a (tile, channel) sits in the same lane and
//         register of accumulator p -- and nothing but the result is ever stored.  A unit's first MFMA per position has a
//         zero C operand, so nothing is cleared, and the store reads each accumulator register exactly once;
//       * the input channels go by in chunks of 8: B^T d B is formed on the way into LDS (each lane transforms two channels
//         of one tile from 16 8-byte loads), the U slice of the chunk is staged beside it; two LDS buffers, one barrier per
//         chunk.  With one wave per SIMD every instruction that is not an MFMA costs its issue slots in full (measured:
//         docs/notes/conv_winograd.md), so the loop is built to need few of them -- buffer loads that return zero outside
//         the image, the four positions of a row of a transformed tile as one 16-byte LDS slot (one ds_write_b128, one
//         ds_read_b128), every LDS row reached by an instruction offset, LDS-DMA of U in the buffer form with scalar
//         addressing -- and deals them out at most one LDS read and one piece of the other work behind every MFMA;
//       * dilation d: the convolution is d*d independent undilated ones on the sub-lattices (y mod d, x mod d); a tile is
//         (image, sub-lattice, tile row, tile column) and its pixels are d apart -- no copies.  Every sub-lattice has its
//         own tile grid, ceil(rows / 2) x ceil(columns / 2) of its own extent: an image's tiles form one TY x TX grid, the
//         sub-lattice rows stacked along Y and the sub-lattice columns along X, with no tile wholly outside the image.  A
//         tile may still hang over the edge by one pixel, which reads as zero and is never stored.
//   conv3x3_winograd_w16x2_f32   the same persistent kernel on wave blocks of 32 tiles x 16 channels (v_mfma_f32_16x16x4_f32):
//                          8 waves, two per SIMD, so that one wave's loads, transform, LDS traffic and waits issue beside the
//                          other's MFMAs.  The same units, order of channels and bits; the host's table says which of the two a
//                          (C, K, dilation) runs (mvdetr_winograd_set_variant overrides it).
//   conv3x3_winograd_w16_f32     HALF units (32 tiles x 64 channels, 4 waves of the same wave block), one per workgroup, for the
//                          units of a launch's last, mostly empty round: a second launch behind the persistent one.
//   No atomics, no split over the input channels: the result is deterministic.
//
// Where each part lives: conv_winograd.h has the tile grid of a shape, the buffer-load constants and what the two host entries
// share (offset bounds, CU count); conv_winograd_device.h the chunk's and the store's constants and types and the device functions
// that all kernels call (out_range / out_window, out_offsets, bn_fold_channel, u_lane_offset); this file the three kernels and the
// host side: the family table (family_of), make_plan, launch<MODE, RELU> behind a [mode][relu] table, conv_entry, the C ABI.
#include "common.h"
#include "conv_winograd_device.h"
#include "../../include/mvdetr_ops.h"

#include <atomic>
#include <type_traits>

namespace mvdetr {

std::atomic<const char *> g_winograd_last_kernel{"none"};
static std::atomic<const char *> g_winograd_last_epilogue{"none"};
std::atomic<int64_t> g_winograd_launches{0};
std::atomic<int> g_winograd_max_workgroups{0};                                // 0: one per CU (mvdetr_winograd_set_max_workgroups)
static std::atomic<int> g_winograd_tail{1};                                   // mvdetr_winograd_set_tail
static std::atomic<int> g_winograd_last_tail_units{0};
static std::atomic<int> g_winograd_variant{0};                                // mvdetr_winograd_set_variant
static std::atomic<int> g_winograd_last_variant{0};
static std::atomic<int> g_winograd_schedule{0};                               // mvdetr_winograd_set_schedule
static std::atomic<int> g_winograd_last_schedule{0};

namespace wino {

// (TILES = 64 tiles and KB = 64 output channels per workgroup, the tile grid and its Shape: conv_winograd.h)
// V in LDS is [channel 8][xi 4][column 72][nu 4]: the four nu of a row xi of one (tile, channel) are one 16-byte slot, written
// by one ds_write_b128 and read by one ds_read_b128.  The column of tile t in the rows of channel pair cp is t + 2 cp (72
// columns: 8 of padding), which keeps the four channel pairs that eight lanes write together on different banks and is
// an instruction offset where it is read (the channel pair is the k-step there); xi and the channel are instruction
// offsets too, so the writes, the A reads and the B reads take one address register each.
constexpr int VCOLS = TILES + 8;
constexpr int VROW = VCOLS * 4;            // floats per (channel, xi) row of V: 1,152 bytes
constexpr int V_FLOATS = CC * 4 * VROW;    // 9,216
constexpr int BUF_FLOATS = U_FLOATS + V_FLOATS;   // U first: every instruction offset of both stays below 64 KB (V) and
                                                  // 255 rows of 256 bytes (U)
constexpr int TINFO_SLOTS = 4;             // units whose tiles' output descriptors are kept at a time (a power of two)
constexpr int LDS_BYTES = 2 * BUF_FLOATS * 4 + TINFO_SLOTS * TILES * 16;      // two buffers + the descriptors = 143,360

// MODE 0: y = conv(x).  1: y = act(bn(conv)).  2: act(bn(conv) + res).  3: act(bn(conv) + bn2(res)).  The arithmetic after
// the convolution is bn_act_cl's (bn_epilogue.h), element for element: the same bits as the pass over a stored y.
template <int MODE, bool RELU>
__global__ __launch_bounds__(256) void conv3x3_winograd_f32(const float *__restrict__ x, const float *__restrict__ U,
                                                            float *__restrict__ y, const Shape s, const Epilogue ep)
{
    // ONE shared array: two {U, V} buffers, then four units' tiles' output descriptors: the byte offsets of a tile's four
    // outputs from the unit's first image, channel 0 of the unit's block, Y_NONE for one that is not stored
    extern __shared__ __attribute__((aligned(16))) float lds[];
    u32x4 *const tinfo = reinterpret_cast<u32x4 *>(lds + 2 * BUF_FLOATS);

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);               // uniform: LDS-DMA targets by scalar arithmetic
    const int C = s.C, K = s.K, d = s.d, H = s.H, W = s.W;
    const int chunks = C / CC;
    // The grid is persistent: workgroup g runs the units g, g + G, g + 2 G, ... (G = gridDim.x <= s.units), a unit being
    // what a workgroup used to be.  Units that share a 64-channel slice of U are 'kblocks' apart: with 8 (or 4, 2, 1)
    // slices, consecutive ids being dealt round-robin over the 8 XCDs, each XCD's L2 serves one slice, and with G a
    // multiple of kblocks a workgroup keeps its slice -- which nothing below relies on.
    const unsigned G = gridDim.x;

    // ---- the staging side: the unit and chunk whose loads are issued next ---------------------------------------------------
    // Every per-lane offset is 32-bit and relative to the image of the unit's first tile (the host bounds the span of one
    // unit's 64 tiles).  The loader's tile: lane group of 4 = one tile, its 4 channel pairs.
    const int ltile = tid >> 2, cp = tid & 3;
    unsigned off[16];                                                         // BYTE offset of pixel (i, j), channel pair cp
    __amdgpu_buffer_rsrc_t xrsrc;                                             // the unit's image block, in SGPRs
    __amdgpu_buffer_rsrc_t ursrc;                                             // the unit's 64-channel slice of U, likewise
    // A unit's place: its channel block and the tile-grid position of its first tile (uniform: SGPRs), one for the staging
    // side and one for the store.  Found by division for the workgroup's first unit, by addition for every other: the
    // next unit is G units on, whose stride over the tile grid the host has split into columns, rows and images.
    struct Place { int kb, X, Y, n; };
    auto next_unit = [&](Place &p) {
        p.kb += s.gr;
        const bool carry = p.kb >= s.kblocks;
        p.kb -= carry ? s.kblocks : 0;
        tile_step(s, carry, p.X, p.Y, p.n);
        return carry;
    };
    Place sp, cpl;                                                            // staging side, compute side
    sp.kb = (int)(blockIdx.x % (unsigned)s.kblocks);
    tile_grid(s, blockIdx.x / (unsigned)s.kblocks * TILES, sp.X, sp.Y, sp.n);
    cpl = sp;
    int lX, lY, ln;                                                           // the loader's tile of the staged unit
    tile_grid(s, blockIdx.x / (unsigned)s.kblocks * TILES + ltile, lX, lY, ln);
    // Entering the staged unit: its offsets, bases, and the output descriptors of its tiles into slot 'slot' of tinfo.  The
    // staging side is at most two units ahead of the one whose store reads its slot (C = 8: one chunk per unit), and a
    // barrier lies between any store and the write that is four units later: four slots.
    auto enter_unit = [&](int slot) {
        const int n0 = sp.n;
        xrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(x + (size_t)n0 * H * W * C), 0, (int)X_RANGE, 0x00020000);
        // the slice starts at its first column of U and the range ends with U (the host bounds U below X_RANGE)
        ursrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(U + sp.kb * KB), 0,
                                                  (int)(((unsigned)(16 * C) * K - sp.kb * KB) * 4u), 0x00020000);
        int y0, x0;
        tile_pixel(s, lX, lY, y0, x0);
        const bool tvalid = ln < s.N;                                         // a tile past the last one is in image N or later
        const unsigned pix = ((unsigned)(ln - n0) * H + y0) * W + x0;         // the tile's first output pixel
        // pixel (i, j) of the tile's 4x4 input patch: rows and columns by addition, four row and four column tests
        const unsigned base = (pix * C + 2 * cp) * 4u, cstep = (unsigned)d * C * 4u, rstep = cstep * W;
        bool oky[4], okx[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            oky[i] = tvalid & ((unsigned)(y0 + (i - 1) * d) < (unsigned)H);
            okx[i] = (unsigned)(x0 + (i - 1) * d) < (unsigned)W;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const unsigned row = base + (unsigned)(i - 1) * rstep;
#pragma unroll
            for (int j = 0; j < 4; ++j) off[4 * i + j] = (oky[i] & okx[j]) ? row + (unsigned)(j - 1) * cstep : X_OUTSIDE;   // selects
        }
        if (cp == 0) {
            // every tile starts inside the image; one that hangs over the edge has no second row or column
            const bool in = tvalid & (y0 < H) & (x0 < W), right = in & (x0 + d < W), below = in & (y0 + d < H);
            const unsigned o = pix * (unsigned)K * 4u, dx = (unsigned)d * K * 4u, dy = dx * W;
            tinfo[slot * TILES + ltile] = u32x4{in ? o : Y_NONE, right ? o + dx : Y_NONE, below ? o + dy : Y_NONE,
                                                (right & below) ? o + dy + dx : Y_NONE};
        }
    };
    unsigned su = blockIdx.x;                                                 // staging cursor: unit, its ordinal & 3, chunk
    int sslot = 0, sc = 0;
    // One position further in the workgroup's (unit, chunk) sequence; past its end the last chunk is staged again, into
    // buffers nobody reads.  All of it is uniform: scalar arithmetic and one uniform branch.
    auto advance = [&] {
        if (sc + 1 < chunks) {
            ++sc;
        } else if (su + G < s.units) {
            su += G;
            sslot = (sslot + 1) & (TINFO_SLOTS - 1);
            sc = 0;
            tile_step(s, next_unit(sp), lX, lY, ln);
            enter_unit(sslot);
        }
    };
    enter_unit(0);

    // ---- U staging by LDS-DMA: the chunk's [16][8][64] slice is 8 x 16 bytes per lane, LDS image in lane order ---------------
    // float index f = r * 1024 + tid * 4 of the image [p][c][k]:  p = 2 r + (tid >> 7), c = (tid >> 4) & 7, k = (tid & 15) * 4
    const unsigned uoff = ((unsigned)((tid >> 7) * C + ((tid >> 4) & 7)) * K + (tid & 15) * 4) * 4u;   // bytes
    const unsigned ustep = 2u * C * K * 4u;                                   // two positions further per r, bytes

    // The x loads are raw buffer loads: the uniform base (image block + chunk) travels in SGPRs, the lane's 32-bit byte
    // offset in one VGPR, and a pixel outside the image has an offset past the buffer's range, for which the hardware
    // returns zero -- no per-lane 64-bit addresses, no selects.  (Valid offsets end below 2^32 - 64: the host's bound.)
    float2 raw[16];
    auto load_x = [&](int c0, int e) {
        const auto v = __builtin_amdgcn_raw_buffer_load_b64(xrsrc, (int)off[e], c0 * 4, 0);
        static_assert(sizeof(v) == 8, "two floats");
        raw[e] = __builtin_bit_cast(float2, v);
    };
    auto load_u = [&](int c0, float *ubuf, int r) {
        // the buffer form, as the x loads: chunk and position pair in the scalar offset, the lane's constant in one VGPR
        __builtin_amdgcn_raw_ptr_buffer_load_lds(ursrc, (lds_void *)(ubuf + r * 1024 + wave * 256), 16, (int)uoff,
                                                 (int)((unsigned)c0 * K * 4u + r * ustep), 0, 0);
    };
    // One sixteenth of a chunk's loads: the 16 x loads go first (two per piece), the 8 LDS-DMA of U behind them.
    auto load_piece = [&](int c0, float *ubuf, int q) {
        if (q < 8) {
            load_x(c0, 2 * q);
            load_x(c0, 2 * q + 1);
        } else {
            load_u(c0, ubuf, q - 8);
        }
    };

    // B^T d B of the lane's tile and channel pair, in 16 pieces that fit between two MFMAs each:
    //   pieces 4 xi + {0, 1}   the row combinations tx/ty of row xi
    //   pieces 4 xi + {2, 3}   the four values of row xi of one channel, one 16-byte store -> V[buf][2 cp + e][xi][ltile + 2 cp]
    float tx[4], ty[4];
    const int v_off = U_FLOATS + 2 * cp * 4 * VROW + (ltile + 2 * cp) * 4;
    auto xform_piece = [&](float *vbuf, int u) {
        const int xi = u / 4, s = u % 4;
        const int ra = xi == 0 ? 0 : 1, rb = xi == 3 ? 3 : 2;                 // t = d[ra] -/+ d[rb]
        if (s < 2) {
#pragma unroll
            for (int j = 2 * s; j < 2 * s + 2; ++j) {
                const float2 a = raw[4 * ra + j], b = raw[4 * rb + j];
                if (xi == 0 || xi == 3) { tx[j] = a.x - b.x; ty[j] = a.y - b.y; }     // d0 - d2, d1 - d3
                else if (xi == 1) { tx[j] = a.x + b.x; ty[j] = a.y + b.y; }           // d1 + d2
                else { tx[j] = b.x - a.x; ty[j] = b.y - a.y; }                        // d2 - d1
            }
            return;
        }
        // (four adds straight into the four registers of the store: the Makefile keeps this file from the SLP vectoriser
        // and from vector-combine, which pair x with y and then pay four copies per store)
        const float *const t = s == 2 ? tx : ty;
        const f32x4 v = {t[0] - t[2], t[1] + t[2], t[2] - t[1], t[1] - t[3]};
        *reinterpret_cast<f32x4 *>(vbuf + v_off + ((s - 2) * 4 + xi) * VROW) = v;
    };

    // ---- the wave's block of the sixteen products -----------------------------------------------------------------------------
    const int wm = wave & 1, wn = wave >> 1;                                  // 32-tile block, 32-channel block
    // k-step s, row xi: channel 2 s + (lane >> 5), column tile + 2 s: + (8 s + xi) * VROW + 8 s
    const int a_off = U_FLOATS + (lane >> 5) * 4 * VROW + (wm * 32 + (lane & 31)) * 4;
    const int b_off = (lane >> 5) * KB + wn * 32 + (lane & 31);             // + (p * CC + 2 s) * KB
    f32x16 acc[16];

    // Two sets of operand registers, by the parity of the k-step: while the sixteen MFMAs of one k-step issue, the
    // operands of the next one are read, at most one LDS instruction behind every MFMA: the four positions of a row xi
    // of V are one ds_read_b128; positions p and p + 1 are eight rows (2,048 bytes) apart in U, which is one
    // ds_read2st64_b32 (a lane needs one float of each 16-byte granule of U: nothing wider exists).  Twelve reads a k-step.
    float fa[2][16], fb[2][16];
    auto read_piece = [&](const float *buf, int st, int q) {
        const int par = st & 1;
        if (q < 4) {
            const f32x4 v = *reinterpret_cast<const f32x4 *>(buf + a_off + (8 * st + q) * VROW + 8 * st);
#pragma unroll
            for (int nu = 0; nu < 4; ++nu) fa[par][4 * q + nu] = v[nu];
        } else if (q < 12) {
            const int p = 2 * (q - 4);
            fb[par][p] = buf[b_off + (p * CC + 2 * st) * KB];
            fb[par][p + 1] = buf[b_off + ((p + 1) * CC + 2 * st) * KB];
        }
    };
    auto mfma = [&](int p, int par) { acc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[par][p], fb[par][p], acc[p], 0, 0, 0); };

    // prologue: the first position (unit, chunk 0) into buffer 0; then the second position's loads, and the operands of the
    // first k-step
    {
#pragma unroll
        for (int q = 0; q < 16; ++q) load_piece(0, lds, q);
#pragma unroll
        for (int u = 0; u < 16; ++u) xform_piece(lds, u);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                      // this wave's LDS-DMA has landed
        __syncthreads();
        advance();
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            read_piece(lds, 0, q);
            load_piece(sc * CC, lds + BUF_FLOATS, q);
        }
    }

    // One chunk = four groups of sixteen MFMAs (k-steps 0..3), one MFMA per position, and behind the first twelve MFMAs of a
    // group one LDS read of the next k-step's operands, plus one piece of the other work where there is some.  With one
    // wave per SIMD nothing else hides the issue slots of that other work (profiles/conv_winograd_loop_ab.txt), so it is
    // spread evenly and kept short:
    //   k-step 0   nothing else: the next chunk's loads, issued a group earlier, get this group too (2,048 cycles)
    //   k-step 1   the first half of the next chunk's B^T d B and its LDS writes, behind the last eight MFMAs
    //   k-step 2   the second half, behind the first eight
    //   barrier    every wave's V writes and LDS-DMA of the next chunk are done, all reads of this chunk are done
    //   k-step 3   its reads are the NEXT chunk's k-step 0; the loads of the chunk after it, into the buffer this chunk left
    // The loop runs over the positions (unit, chunk) of ALL the workgroup's units, and the staging side, two positions
    // ahead, has a cursor of its own: the last chunks of a unit issue the x loads and the LDS-DMA of the next unit's first
    // chunks, which fly over the stores between the two.  The k-steps carry no branch: the two uniform ones, the staging
    // side entering a unit and the store behind a unit's last chunk, sit at the top and at the bottom of an iteration.
    // A unit's first chunk is a copy of the chunk whose k-step 0 has a zero C operand: the accumulators are not live from
    // one unit to the next, and nothing is cleared.
    const int kcol = wn * 32 + (lane & 31);                                   // the lane stores ONE output channel of a unit
    float bs = 1.f, bt = 0.f, bs2 = 0.f;                                      // its folded BatchNorm constants ...
    int kb_folded = -1;                                                       // ... which are those of this channel block
    unsigned cu = blockIdx.x;                                                 // compute cursor: unit, its ordinal & 3,
    int cslot = 0, par = 0;                                                   // and the LDS buffer the position is in
    auto chunk = [&](auto first) {
        advance();
        float *const cur = lds + par * BUF_FLOATS;
        float *const nxt = lds + (par ^ 1) * BUF_FLOATS;
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int p = 0; p < 16; ++p) {
            if (decltype(first)::value) acc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[0][p], fb[0][p], f32x16{}, 0, 0, 0);
            else mfma(p, 0);
            read_piece(cur, 1, p);
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int p = 0; p < 16; ++p) {
            mfma(p, 1);
            read_piece(cur, 2, p);
            if (p >= 8) xform_piece(nxt, p - 8);
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int p = 0; p < 16; ++p) {
            mfma(p, 0);
            read_piece(cur, 3, p);
            if (p < 8) xform_piece(nxt, 8 + p);
            __builtin_amdgcn_sched_barrier(0);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
#pragma unroll
        for (int p = 0; p < 16; ++p) {
            mfma(p, 1);
            read_piece(nxt, 0, p);
            load_piece(sc * CC, cur, p);
            __builtin_amdgcn_sched_barrier(0);
        }
        par ^= 1;
    };
    do {
        chunk(std::true_type{});
        if (chunks > 1) {                                                     // (a zero-trip `for` has the allocator spill)
            int ch = 1;
            do chunk(std::false_type{});
            while (++ch < chunks);
        }

        // ---- behind the unit's last chunk: A^T M A in registers, then the stores -------------------------------------------------
        // The operands of the next position's first k-step are already in registers and its loads in flight.
        const int kb = cpl.kb, n0 = cpl.n;
        // y (and the residual) through a buffer resource that starts at the unit's first image and channel and ends with
        // the tensor: a lane's byte offset is its tile's descriptor plus its channel, and Y_NONE plus anything saturates
        const int yrange = out_range(s.N, H, W, K, n0, kb);
        const __amdgpu_buffer_rsrc_t yrsrc = out_window(y, H, W, K, n0, kb, yrange);
        // accumulator register r holds tile wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5): an instruction offset
        const u32x4 *const ti = tinfo + cslot * TILES + wm * 32 + 4 * (lane >> 5);
        auto offsets = [&](int r, unsigned (&o4)[4]) {
            const u32x4 dsc = ti[(r & 3) + 8 * (r >> 2)];
out_offsets(dsc, kcol, o4);
        };
        // The BatchNorm constants of channel kb * 64 + kcol, folded when the workgroup's channel block changes: once per
        // launch where the grid is a multiple of kblocks.
        if (MODE >= 1 && kb != kb_folded) {
            bn_fold_channel<MODE>(ep, kb * KB + kcol, bs, bt, bs2);
            kb_folded = kb;
        }
        // The residual: 4 values per accumulator register, requested four registers' worth at a time and one such batch
        // ahead of its use (the staged chunk and the next unit's offsets are live here: no room for all 64 at once).  Raw
        // buffer loads as for x: the byte offsets of the stores below, and an element that is not stored gets an offset
        // past the buffer's range, for which nothing is read.  The range ends with the tensor.
        float q[2][4][4];
        __amdgpu_buffer_rsrc_t rrsrc;
        if (MODE >= 2) rrsrc = out_window(ep.res, H, W, K, n0, kb, yrange);
        auto load_res = [&](int b) {
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                unsigned o4[4];
                offsets(4 * b + rr, o4);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    q[b & 1][rr][e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rrsrc, (int)o4[e], 0, 0));
            }
        };
        if (MODE >= 2) {
            load_res(0);
            __builtin_amdgcn_sched_barrier(0);
        }
        // The accumulator reads below are written out by hand, so the wait states between the last MFMA's write and a
        // read of its registers are too: 18 for a 16-pass MFMA, whatever the compiler puts between the two.
        asm volatile("s_nop 15\n\ts_nop 3");
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            if (MODE >= 2 && r % 4 == 0 && r + 4 < 16) {
                load_res(r / 4 + 1);
                __builtin_amdgcn_sched_barrier(0);                            // issued ahead of the stores of batch r / 4
            }
            unsigned o4[4];                                                   // the accumulator's row = the tile
            offsets(r, o4);
            // Register r of the sixteen accumulators, read one by one: left to the compiler, an element of an accumulator
            // costs a copy of all its sixteen registers, 4,096 reads per unit where 256 are needed.
            float m[16];
#pragma unroll
            for (int p = 0; p < 16; ++p) asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(m[p]) : "a"(acc[p][r]));
            float s0[4], s1[4];
#pragma unroll
            for (int nu = 0; nu < 4; ++nu) {
                s0[nu] = m[nu] + m[4 + nu] + m[8 + nu];
                s1[nu] = m[4 + nu] - m[8 + nu] - m[12 + nu];
            }
            float y00 = s0[0] + s0[1] + s0[2], y01 = s0[1] - s0[2] - s0[3];
            float y10 = s1[0] + s1[1] + s1[2], y11 = s1[1] - s1[2] - s1[3];
            if (MODE >= 1) {
                constexpr int RES = MODE - 1;
                const float *const qr = q[(r >> 2) & 1][r & 3];
                y00 = bn_finish<RES, RELU>(bn_apply(y00, bs, bt), RES ? qr[0] : 0.f, bs2);
                y01 = bn_finish<RES, RELU>(bn_apply(y01, bs, bt), RES ? qr[1] : 0.f, bs2);
                y10 = bn_finish<RES, RELU>(bn_apply(y10, bs, bt), RES ? qr[2] : 0.f, bs2);
                y11 = bn_finish<RES, RELU>(bn_apply(y11, bs, bt), RES ? qr[3] : 0.f, bs2);
            }
            // four buffer stores, no branch: one at Y_NONE is dropped
            const float y4[4] = {y00, y01, y10, y11};
#pragma unroll
            for (int e = 0; e < 4; ++e)
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, y4[e]), yrsrc, (int)o4[e], 0, 0);
            // one register's sixteen reads at a time, and the accumulators stay where the MFMAs left them: copied out all at
            // once they take the whole VGPR file, and the allocator then spills the loop's operands to make room
#pragma unroll
            for (int p = 0; p < 16; ++p) asm volatile("" : "+a"(acc[p]));
            __builtin_amdgcn_sched_barrier(0);
        }
        cu += G;
        next_unit(cpl);
        cslot = (cslot + 1) & (TINFO_SLOTS - 1);
    } while (cu < s.units);
    // the loads of the last k-step 3 are nobody's, but an LDS-DMA must not outlive the workgroup's LDS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// ---- the half unit: 32 tiles x 64 output channels, for the units of a launch's last, mostly empty round ------------------------
// The persistent kernel's unit is indivisible, so a remainder of `rem` units keeps rem CUs busy for a whole unit time while
// the others idle.  This kernel runs a unit as two workgroups of half the tiles each, on twice the CUs in about half the
// time, and the host (conv_entry) launches it behind the main one for the remainder alone.
//   * a wave owns 32 tiles x 16 channels of all sixteen products on v_mfma_f32_16x16x4_f32: 16 positions x 2 blocks of 16
//     tiles = 32 accumulators of 4 registers, 128 per lane.  Position p of a (tile, channel) is again one lane and register
//     of accumulator p, so A^T M A stays in registers.  Both fp32 MFMAs are fmaf chains in the order of k, and the channels
//     go by in the same order: the bits of conv3x3_winograd_f32.
//   * one half unit per workgroup, found by division; no persistence (a tail has at most one workgroup per CU).
//   * a chunk of 8 channels is two k-steps of 32 MFMAs.  The loader has one (tile, channel) per lane, the channel fastest:
//     sixteen 4-byte buffer loads, 32 adds, four ds_write_b128; the chunk's U slice is 8 LDS-DMA per lane, as above.
//   * V in LDS is [channel 8][xi 4][column 40][nu 4], the column of tile t in the rows of channel c being t + 2 (c >> 1).
//     ds_read_b128 is served in groups of 16 lanes that mix two channels of a k-step (k = lane >> 4): lanes 0-3, 12-15 of
//     channel k with lanes 4-11 of channel k + 1, on 64 banks.  Those are disjoint only where the two channels have the same
//     shift, so the shift goes by channel PAIR, and the eight lanes of a ds_write_b128 group (32 banks) meet two by two:
//     16 LDS cycles for an instruction that takes 13 to issue.
//   * U in LDS is [p][c][64] with the row of an odd channel rotated by 16 floats: a B operand is one float per lane, lanes
//     0-15 of channel k and 16-31 of channel k + 1 in one group of ds_read_b32 on 32 banks.  The rotation is free: the
//     LDS-DMA writes in lane order and the lane chooses what it fetches.
namespace w16 {
constexpr int HT = 32;                     // tiles of a half unit
constexpr int VCOLS = HT + 8;
constexpr int VROW = VCOLS * 4;            // floats per (channel, xi) row of V: 640 bytes; a channel is 640 floats = 10 x 64 banks
constexpr int V_FLOATS = CC * 4 * VROW;    // 5,120
constexpr int BUF_FLOATS = U_FLOATS + V_FLOATS;
constexpr int LDS_BYTES = 2 * BUF_FLOATS * 4 + HT * 16;                       // two buffers + the descriptors = 107,008
}  // namespace w16

// Half unit j of the launch is tile half j & 1 of unit `unit0 + j / 2`; one wholly past the last tile stores nothing.
template <int MODE, bool RELU>
__global__ __launch_bounds__(256) void conv3x3_winograd_w16_f32(const float *__restrict__ x, const float *__restrict__ U,
                                                                float *__restrict__ y, const Shape s, const Epilogue ep,
                                                                const unsigned unit0)
{
    constexpr int HT = w16::HT, VROW = w16::VROW, BUF_FLOATS = w16::BUF_FLOATS;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    u32x4 *const tinfo = reinterpret_cast<u32x4 *>(lds + 2 * BUF_FLOATS);

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);               // the wave's quarter of the 64 channels
    const int C = s.C, K = s.K, d = s.d, H = s.H, W = s.W;
    const int chunks = C / CC;
    const unsigned unit = unit0 + (blockIdx.x >> 1);
    const int kb = (int)(unit % (unsigned)s.kblocks);
    const unsigned t0 = unit / (unsigned)s.kblocks * TILES + (blockIdx.x & 1) * HT;
    if (t0 >= s.tiles) return;                                                // uniform: before any barrier

    // ---- the loader's (tile, channel): offsets, bases and the tile's output descriptor, as in conv3x3_winograd_f32 -------
    const int ltile = tid >> 3, lc = tid & 7;
    int X0, Y0, n0, lX, lY, ln;
    tile_grid(s, t0, X0, Y0, n0);
    tile_grid(s, t0 + ltile, lX, lY, ln);
    const __amdgpu_buffer_rsrc_t xrsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(x + (size_t)n0 * H * W * C), 0, (int)X_RANGE, 0x00020000);
    const __amdgpu_buffer_rsrc_t ursrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float *>(U + kb * KB), 0, (int)(((unsigned)(16 * C) * K - kb * KB) * 4u), 0x00020000);
    unsigned off[16];                                                         // BYTE offset of pixel (i, j), channel lc
    {
        int y0, x0;
        tile_pixel(s, lX, lY, y0, x0);
        const bool tvalid = ln < s.N;
        const unsigned pix = ((unsigned)(ln - n0) * H + y0) * W + x0;
        const unsigned base = (pix * C + lc) * 4u, cstep = (unsigned)d * C * 4u, rstep = cstep * W;
        bool oky[4], okx[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            oky[i] = tvalid & ((unsigned)(y0 + (i - 1) * d) < (unsigned)H);
            okx[i] = (unsigned)(x0 + (i - 1) * d) < (unsigned)W;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const unsigned row = base + (unsigned)(i - 1) * rstep;
#pragma unroll
            for (int j = 0; j < 4; ++j) off[4 * i + j] = (oky[i] & okx[j]) ? row + (unsigned)(j - 1) * cstep : X_OUTSIDE;
        }
        if (lc == 0) {
            const bool in = tvalid & (y0 < H) & (x0 < W), right = in & (x0 + d < W), below = in & (y0 + d < H);
            const unsigned o = pix * (unsigned)K * 4u, dx = (unsigned)d * K * 4u, dy = dx * W;
            tinfo[ltile] = u32x4{in ? o : Y_NONE, right ? o + dx : Y_NONE, below ? o + dy : Y_NONE,
                                 (right & below) ? o + dy + dx : Y_NONE};
        }
    }

    // ---- U by LDS-DMA: float f = r * 1024 + tid * 4 of the LDS image is p = 2 r + (tid >> 7), c = (tid >> 4) & 7, column
    // (tid & 15) * 4, which holds output channel (column - 16 (c & 1)) mod 64 of the slice
    const unsigned uoff = u_lane_offset(tid, C, K);
    const unsigned ustep = 2u * C * K * 4u;
    float raw[16];
    auto load_piece = [&](int c0, float *ubuf, int q) {                       // 16 x loads, then the 8 LDS-DMA of U
        if (q < 16)
            raw[q] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xrsrc, (int)off[q], c0 * 4, 0));
        else if (q < 24)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(ursrc, (lds_void *)(ubuf + (q - 16) * 1024 + wave * 256), 16, (int)uoff,
                                                     (int)((unsigned)c0 * K * 4u + (q - 16) * ustep), 0, 0);
    };
    // B^T d B of the lane's (tile, channel) in 16 pieces: 4 xi + {0, 1} the row combination of row xi, 4 xi + {2, 3} its four
    // values and their one 16-byte store -> V[buf][lc][xi][ltile + 2 (lc >> 1)]
    float t[4];
    f32x4 v4;
    const int v_off = U_FLOATS + lc * 4 * VROW + (ltile + 2 * (lc >> 1)) * 4;
    auto xform_piece = [&](float *vbuf, int u) {
        const int xi = u / 4, q = u % 4;
        const int ra = xi == 0 ? 0 : 1, rb = xi == 3 ? 3 : 2;                 // t = d[ra] -/+ d[rb]
        if (q < 2) {
#pragma unroll
            for (int j = 2 * q; j < 2 * q + 2; ++j) {
                const float a = raw[4 * ra + j], b = raw[4 * rb + j];
                t[j] = (xi == 0 || xi == 3) ? a - b : xi == 1 ? a + b : b - a;
            }
        } else if (q == 2) {
            v4[0] = t[0] - t[2];
            v4[1] = t[1] + t[2];
        } else {
            v4[2] = t[2] - t[1];
            v4[3] = t[1] - t[3];
            *reinterpret_cast<f32x4 *>(vbuf + v_off + xi * VROW) = v4;
        }
    };

    // ---- the wave's block: tile 16 h + (lane & 15) and channel 4 st + (lane >> 4) of k-step st for A, the same channel's
    // row of U and output channel 16 wave + (lane & 15) for B
    const int kk = lane >> 4;
    const int a_off = U_FLOATS + kk * 4 * VROW + ((lane & 15) + 2 * (kk >> 1)) * 4;     // + (16 st + xi) VROW + (16 h + 4 st) 4
    const int b_off = kk * KB + ((wave * 16 + (lane & 15) + 16 * (kk & 1)) & 63);       // + (p CC + 4 st) KB
    f32x4 acc[16][2];
    float fa[2][2][16], fb[2][16];                                            // [set][tile block][p], [set][p]
    auto read_piece = [&](const float *buf, int st, int set, int q) {         // 8 ds_read_b128, 8 ds_read2st64_b32
        if (q < 8) {
            const int xi = q >> 1, h = q & 1;
            const f32x4 v = *reinterpret_cast<const f32x4 *>(buf + a_off + (16 * st + xi) * VROW + (16 * h + 4 * st) * 4);
#pragma unroll
            for (int nu = 0; nu < 4; ++nu) fa[set][h][4 * xi + nu] = v[nu];
        } else if (q < 16) {
            const int p = 2 * (q - 8);
            fb[set][p] = buf[b_off + (p * CC + 4 * st) * KB];
            fb[set][p + 1] = buf[b_off + ((p + 1) * CC + 4 * st) * KB];
        }
    };

    // prologue: chunk 0 into buffer 0, then the loads of chunk 1 and the operands of the first k-step
    int sc = 0;                                                               // the chunk staged next (the last one again past the end)
    auto advance = [&] { sc = sc + 1 < chunks ? sc + 1 : sc; };
#pragma unroll
    for (int q = 0; q < 24; ++q) load_piece(0, lds, q);
#pragma unroll
    for (int u = 0; u < 16; ++u) xform_piece(lds, u);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    advance();
#pragma unroll
    for (int q = 0; q < 24; ++q) {
        read_piece(lds, 0, 0, q);
        load_piece(sc * CC, lds + BUF_FLOATS, q);
    }

    // One chunk = two k-steps of 32 MFMAs (position p, tile block h: consecutive ones never share an accumulator).
    //   k-step 0   the reads of k-step 1, then the next chunk's B^T d B and its LDS writes
    //   barrier    the next chunk's V and U are in LDS, every read of this chunk is done
    //   k-step 1   the reads of the next chunk's k-step 0, and the loads of the chunk after it into the buffer this one left
    int par = 0;
    auto chunk = [&](auto first) {
        float *const cur = lds + par * BUF_FLOATS;
        float *const nxt = lds + (par ^ 1) * BUF_FLOATS;
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int m = 0; m < 32; ++m) {
            const int p = m >> 1, h = m & 1;
            acc[p][h] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[0][h][p], fb[0][p], decltype(first)::value ? f32x4{} : acc[p][h], 0, 0, 0);
            if (m < 16) read_piece(cur, 1, 1, m);
            else xform_piece(nxt, m - 16);
            __builtin_amdgcn_sched_barrier(0);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        advance();
#pragma unroll
        for (int m = 0; m < 32; ++m) {
            const int p = m >> 1, h = m & 1;
            acc[p][h] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[1][h][p], fb[1][p], acc[p][h], 0, 0, 0);
            read_piece(nxt, 0, 0, m);
            load_piece(sc * CC, cur, m);
            __builtin_amdgcn_sched_barrier(0);
        }
        par ^= 1;
    };
    chunk(std::true_type{});
    if (chunks > 1) {
        int ch = 1;
        do chunk(std::false_type{});
        while (++ch < chunks);
    }

    // ---- A^T M A in registers, then the stores: register r of tile block h is tile 16 h + 4 (lane >> 4) + r ----------------
    const int kcol = wave * 16 + (lane & 15);
    float bs = 1.f, bt = 0.f, bs2 = 0.f;
    if (MODE >= 1) {
        bn_fold_channel<MODE>(ep, kb * KB + kcol, bs, bt, bs2);
    }
    const unsigned long long left = ((unsigned long long)(s.N - n0) * H * W * K - (unsigned)(kb * KB)) * 4ull;
    const int yrange = (int)(left < X_RANGE ? (unsigned)left : X_RANGE);
    const __amdgpu_buffer_rsrc_t yrsrc =
        __builtin_amdgcn_make_buffer_rsrc(y + (size_t)n0 * H * W * K + kb * KB, 0, yrange, 0x00020000);
    __amdgpu_buffer_rsrc_t rrsrc;
    if (MODE >= 2)
        rrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(ep.res + (size_t)n0 * H * W * K + kb * KB), 0, yrange,
                                                  0x00020000);
    const u32x4 *const ti = tinfo + 4 * (lane >> 4);
    unsigned o4[8][4];
    float q4[8][4];
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const u32x4 dsc = ti[16 * (b >> 2) + (b & 3)];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            o4[b][e] = __builtin_elementwise_add_sat(dsc[e], (unsigned)kcol * 4u);
            if (MODE >= 2) q4[b][e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rrsrc, (int)o4[b][e], 0, 0));
        }
    }
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const int h = b >> 2, r = b & 3;
        float s0[4], s1[4];
#pragma unroll
        for (int nu = 0; nu < 4; ++nu) {
            s0[nu] = acc[nu][h][r] + acc[4 + nu][h][r] + acc[8 + nu][h][r];
            s1[nu] = acc[4 + nu][h][r] - acc[8 + nu][h][r] - acc[12 + nu][h][r];
        }
        float y00 = s0[0] + s0[1] + s0[2], y01 = s0[1] - s0[2] - s0[3];
        float y10 = s1[0] + s1[1] + s1[2], y11 = s1[1] - s1[2] - s1[3];
        if (MODE >= 1) {
            constexpr int RES = MODE - 1;
            y00 = bn_finish<RES, RELU>(bn_apply(y00, bs, bt), RES ? q4[b][0] : 0.f, bs2);
            y01 = bn_finish<RES, RELU>(bn_apply(y01, bs, bt), RES ? q4[b][1] : 0.f, bs2);
            y10 = bn_finish<RES, RELU>(bn_apply(y10, bs, bt), RES ? q4[b][2] : 0.f, bs2);
            y11 = bn_finish<RES, RELU>(bn_apply(y11, bs, bt), RES ? q4[b][3] : 0.f, bs2);
        }
        const float y4[4] = {y00, y01, y10, y11};
#pragma unroll
        for (int e = 0; e < 4; ++e)
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, y4[e]), yrsrc, (int)o4[b][e], 0, 0);
    }
    // the loads of the last k-step 1 are nobody's, but an LDS-DMA must not outlive the workgroup's LDS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// ---- the 8-wave unit: the persistent kernel on the 16-channel wave block, two waves per SIMD -----------------------------------
// The unit, the persistent grid, the staging cursor, the descriptors and the store are conv3x3_winograd_f32's.  Wave w owns
// tile half w / 4 and channel quarter w % 4 of the unit (waves w and w + 4 share a SIMD): 32 tiles x 16 channels of all sixteen
// products, 128 accumulator registers, pinned to AGPRs; the other 128 registers hold the operands in two sets of eight positions
// (16 + 8 registers each), the loader's sixteen pixels and offsets.  A chunk is four half k-steps of 16 MFMAs:
//   k-step 0, positions 0-7     the reads of positions 8-15
//   k-step 0, positions 8-15    the reads of k-step 1, positions 0-7; the first half of the next chunk's B^T d B
//   k-step 1, positions 0-7     the reads of positions 8-15; the second half
//   barrier
//   k-step 1, positions 8-15    the x loads of the chunk after next, the reads of the next chunk's first set, the LDS-DMA of U
// The loader has one (tile, channel) per lane as in the half-unit kernel; V keeps 72 columns, U is 4 LDS-DMA per lane.
//
// That is DEAL 0, and under schedule 1 (lockstep) all eight waves run it: both waves of a SIMD issue their sixteen x loads and
// four LDS-DMA in the same half k-step.  The memory work of a chunk may sit elsewhere without another barrier, LDS buffer or
// bit of the result: with c the chunk a wave computes, buf[c & 1] its operands' buffer and the barrier of c between its third
// and fourth half k-step (h0 .. h3),
//   V of chunk c + 1   -> buf[(c + 1) & 1], last read before the barrier of c - 1, first read in h3(c): anywhere in h3(c - 1) .. h2(c)
//   U of chunk c + 2   -> buf[c & 1], last read before the barrier of c, first read in h3(c + 1): issued in h3(c) .. h1(c + 1), under
//                         the vmcnt(0) before the barrier of c + 1
//   x of chunk c + 2   -> raw[], once the transform of chunk c + 1 has read it, landed by the transform's first piece
// DEAL 1 (early) is the program of waves 4-7 under schedule 2 (de-phased; waves 0-3 keep deal 0), at priority 1:
//   h0(c)   the reads; U of chunk c + 1, under the staging cursor of before this chunk's advance(); the second half of the
//           transform of chunk c + 1
//   h1(c)   the reads; the x loads of chunk c + 2
//   h2(c)   the reads
//   barrier
//   h3(c)   eight bare MFMAs beside the other role's loads, then the reads and the first half of the transform of chunk c + 2
// Both deals have the same barrier statement, once per chunk, and the same trip counts, so every wave arrives at every barrier.
// The whole kernel under one deal.  A role's program is a copy of ALL of it, setup included, behind the kernel's one branch
// (ROLES: this is one of two copies), so that no vector register is live across the other role's loop: not the thread index
// either, which a copy takes from its wave's number and the lane count, in a statement of its own that cannot be hoisted.
template <int MODE, bool RELU, int DEAL, bool ROLES>
__device__ __forceinline__ void conv3x3_winograd_w16x2_deal(const float *__restrict__ x, const float *__restrict__ U,
                                                            float *__restrict__ y, const Shape &s, const Epilogue &ep,
                                                            const int wave)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    u32x4 *const tinfo = reinterpret_cast<u32x4 *>(lds + 2 * BUF_FLOATS);

    int lane = threadIdx.x & 63;
    if (ROLES) asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0 ; deal %1" : "=v"(lane) : "n"(DEAL));
    const int tid = wave * 64 + lane;
    const int C = s.C, K = s.K, d = s.d, H = s.H, W = s.W;
    const int chunks = C / CC;
    const unsigned G = gridDim.x;

    // ---- the staging side, as in conv3x3_winograd_f32; the loader's lane is one tile and ONE channel ------------------------------
    const int ltile = tid >> 3, lc = tid & 7;
    unsigned off[16];
    __amdgpu_buffer_rsrc_t xrsrc;
    __amdgpu_buffer_rsrc_t ursrc;
    struct Place { int kb, X, Y, n; };
    auto next_unit = [&](Place &p) {
        p.kb += s.gr;
        const bool carry = p.kb >= s.kblocks;
        p.kb -= carry ? s.kblocks : 0;
        tile_step(s, carry, p.X, p.Y, p.n);
        return carry;
    };
    Place sp, cpl;
    sp.kb = (int)(blockIdx.x % (unsigned)s.kblocks);
    tile_grid(s, blockIdx.x / (unsigned)s.kblocks * TILES, sp.X, sp.Y, sp.n);
    cpl = sp;
    int lX, lY, ln;
    tile_grid(s, blockIdx.x / (unsigned)s.kblocks * TILES + ltile, lX, lY, ln);
    auto enter_unit = [&](int slot) {
        const int n0 = sp.n;
        xrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(x + (size_t)n0 * H * W * C), 0, (int)X_RANGE, 0x00020000);
        ursrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(U + sp.kb * KB), 0,
                                                  (int)(((unsigned)(16 * C) * K - sp.kb * KB) * 4u), 0x00020000);
        int y0, x0;
        tile_pixel(s, lX, lY, y0, x0);
        const bool tvalid = ln < s.N;
        const unsigned pix = ((unsigned)(ln - n0) * H + y0) * W + x0;
        const unsigned base = (pix * C + lc) * 4u, cstep = (unsigned)d * C * 4u, rstep = cstep * W;
        bool oky[4], okx[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            oky[i] = tvalid & ((unsigned)(y0 + (i - 1) * d) < (unsigned)H);
            okx[i] = (unsigned)(x0 + (i - 1) * d) < (unsigned)W;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const unsigned row = base + (unsigned)(i - 1) * rstep;
#pragma unroll
            for (int j = 0; j < 4; ++j) off[4 * i + j] = (oky[i] & okx[j]) ? row + (unsigned)(j - 1) * cstep : X_OUTSIDE;
        }
        if (lc == 0) {
            const bool in = tvalid & (y0 < H) & (x0 < W), right = in & (x0 + d < W), below = in & (y0 + d < H);
            const unsigned o = pix * (unsigned)K * 4u, dx = (unsigned)d * K * 4u, dy = dx * W;
            tinfo[slot * TILES + ltile] = u32x4{in ? o : Y_NONE, right ? o + dx : Y_NONE, below ? o + dy : Y_NONE,
                                                (right & below) ? o + dy + dx : Y_NONE};
        }
    };
    unsigned su = blockIdx.x;
    int sslot = 0, sc = 0;
    auto advance = [&] {
        if (sc + 1 < chunks) {
            ++sc;
        } else if (su + G < s.units) {
            su += G;
            sslot = (sslot + 1) & (TINFO_SLOTS - 1);
            sc = 0;
            tile_step(s, next_unit(sp), lX, lY, ln);
            enter_unit(sslot);
        }
    };
    enter_unit(0);

    // U by LDS-DMA, 4 x 16 bytes per lane: float f = r * 2048 + tid * 4 of the LDS image is p = 4 r + (tid >> 7), c = (tid >> 4) & 7,
    // column (tid & 15) * 4, which holds output channel (column - 16 (c & 1)) mod 64 (the rotation of the half-unit kernel)
    const unsigned uoff = u_lane_offset(tid, C, K);
    const unsigned ustep = 4u * C * K * 4u;
    float raw[16];
    auto load_x = [&](int c0, int e) {
        raw[e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xrsrc, (int)off[e], c0 * 4, 0));
    };
    auto load_u = [&](int c0, float *ubuf, int r) {
        __builtin_amdgcn_raw_ptr_buffer_load_lds(ursrc, (lds_void *)(ubuf + r * 2048 + wave * 256), 16, (int)uoff,
                                                 (int)((unsigned)c0 * K * 4u + r * ustep), 0, 0);
    };
    float t[4];
    f32x4 v4;
    const int v_off = U_FLOATS + lc * 4 * VROW + (ltile + 2 * (lc >> 1)) * 4;
    auto xform_piece = [&](float *vbuf, int u) {
        const int xi = u / 4, q = u % 4;
        const int ra = xi == 0 ? 0 : 1, rb = xi == 3 ? 3 : 2;
        if (q < 2) {
#pragma unroll
            for (int j = 2 * q; j < 2 * q + 2; ++j) {
                const float a = raw[4 * ra + j], b = raw[4 * rb + j];
                t[j] = (xi == 0 || xi == 3) ? a - b : xi == 1 ? a + b : b - a;
            }
        } else if (q == 2) {
            v4[0] = t[0] - t[2];
            v4[1] = t[1] + t[2];
        } else {
            v4[2] = t[2] - t[1];
            v4[3] = t[1] - t[3];
            *reinterpret_cast<f32x4 *>(vbuf + v_off + xi * VROW) = v4;
        }
    };

    // ---- the wave's block ------------------------------------------------------------------------------------------------------
    const int th = wave >> 2, wq = wave & 3, kk = lane >> 4;
    const int a_off = U_FLOATS + kk * 4 * VROW + (th * 32 + (lane & 15) + 2 * (kk >> 1)) * 4;
    const int b_off = kk * KB + ((wq * 16 + (lane & 15) + 16 * (kk & 1)) & 63);
    f32x4 acc[16][2];
    float fa[2][2][8], fb[2][8];                                              // [set = position half][tile block][position], [set][position]
    // the eight reads of half k-step hs (k-step hs >> 1, positions 8 (hs & 1) ..): in the order the MFMAs need them
    auto read_piece = [&](const float *buf, int hs, int q) {
        const int st = hs >> 1, half = hs & 1;
        if ((q & 2) == 0) {
            const int xl = q >> 2, h = q & 1;
            const f32x4 v = *reinterpret_cast<const f32x4 *>(buf + a_off + (16 * st + 2 * half + xl) * VROW + (16 * h + 4 * st) * 4);
#pragma unroll
            for (int nu = 0; nu < 4; ++nu) fa[half][h][4 * xl + nu] = v[nu];
        } else {
            const int pl = 4 * (q >> 2) + 2 * (q & 1), p = 8 * half + pl;
            fb[half][pl] = buf[b_off + (p * CC + 4 * st) * KB];
            fb[half][pl + 1] = buf[b_off + ((p + 1) * CC + 4 * st) * KB];
        }
    };
    auto mfma = [&](int hs, int m, auto first) {
        const int half = hs & 1, pl = m >> 1, h = m & 1, p = 8 * half + pl;
        if (decltype(first)::value) acc[p][h] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[half][h][pl], fb[half][pl], f32x4{}, 0, 0, 0);
        else acc[p][h] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[half][h][pl], fb[half][pl], acc[p][h], 0, 0, 0);
    };

    // prologue
    {
#pragma unroll
        for (int q = 0; q < 16; ++q) load_x(0, q);
#pragma unroll
        for (int r = 0; r < 4; ++r) load_u(0, lds, r);
#pragma unroll
        for (int u = 0; u < 16; ++u) xform_piece(lds, u);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        advance();
#pragma unroll
        for (int q = 0; q < 16; ++q) load_x(sc * CC, q);
        if (DEAL == 1) {                                                      // the first half of chunk 1's transform; its U in h0
#pragma unroll
            for (int u = 0; u < 8; ++u) xform_piece(lds + BUF_FLOATS, u);
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) load_u(sc * CC, lds + BUF_FLOATS, r);
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) read_piece(lds, 0, q);
    }

    const int kcol = wq * 16 + (lane & 15);
    float bs = 1.f, bt = 0.f, bs2 = 0.f;
    int kb_folded = -1;
    unsigned cu = blockIdx.x;
    int cslot = 0, par = 0;
    // One chunk under deal D (above).  Deal 0 moves the staging cursor at the top, to the chunk after next; deal 1 behind h0,
    // whose LDS-DMA is still the next chunk's.
    auto chunk = [&](auto first, auto deal) {
        constexpr int D = decltype(deal)::value;
        if (D == 0) advance();
        float *const cur = lds + par * BUF_FLOATS;
        float *const nxt = lds + (par ^ 1) * BUF_FLOATS;
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int m = 0; m < 16; ++m) {
            mfma(0, m, first);
            if (m < 8) read_piece(cur, 1, m);
            if (D == 1 && m < 4) load_u(sc * CC, nxt, m);
            if (D == 1 && m >= 8) xform_piece(nxt, m);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (D != 0) {
            advance();
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int m = 0; m < 16; ++m) {
            mfma(1, m, first);
            if (m < 8) {
                read_piece(cur, 2, m);
            } else if (D == 1) {
                load_x(sc * CC, 2 * (m - 8));
                load_x(sc * CC, 2 * (m - 8) + 1);
            } else {
                xform_piece(nxt, m - 8);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int m = 0; m < 16; ++m) {
            mfma(2, m, std::false_type{});
            if (m < 8) read_piece(cur, 3, m);
            else if (D == 0) xform_piece(nxt, m);
            __builtin_amdgcn_sched_barrier(0);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
#pragma unroll
        for (int m = 0; m < 16; ++m) {
            mfma(3, m, std::false_type{});
            if (D == 0) {
                if (m < 8) {
                    load_x(sc * CC, 2 * m);
                    load_x(sc * CC, 2 * m + 1);
                } else {
                    read_piece(nxt, 0, m - 8);
                    if (m < 12) load_u(sc * CC, cur, m - 8);
                }
            } else if (m >= 8) {                                              // bare MFMAs behind the barrier, beside the other role's loads
                read_piece(nxt, 0, m - 8);
                xform_piece(cur, m - 8);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        par ^= 1;
    };
    // the chunks of one unit: every deal has the same trips, and the barrier above is their one barrier statement
    auto unit_chunks = [&](auto deal) {
        chunk(std::true_type{}, deal);
        if (chunks > 1) {
            int ch = 1;
            do chunk(std::false_type{}, deal);
            while (++ch < chunks);
        }
    };
    // the units of this workgroup under one deal: a role runs its own copy of the whole loop, store included
    auto units = [&](auto deal) {
        do {
            unit_chunks(deal);

            // ---- the store: conv3x3_winograd_f32's, over 2 tile blocks x 4 registers ------------------------------------------------
            const int kb = cpl.kb, n0 = cpl.n;
            const int yrange = out_range(s.N, H, W, K, n0, kb);
            const __amdgpu_buffer_rsrc_t yrsrc = out_window(y, H, W, K, n0, kb, yrange);
            // register r of tile block h is tile 32 (w / 4) + 16 h + 4 (lane >> 4) + r
            const u32x4 *const ti = tinfo + cslot * TILES + th * 32 + 4 * (lane >> 4);
            auto offsets = [&](int b, unsigned (&o4)[4]) {
                const u32x4 dsc = ti[16 * (b >> 2) + (b & 3)];
out_offsets(dsc, kcol, o4);
            };
            if (MODE >= 1 && kb != kb_folded) {
                bn_fold_channel<MODE>(ep, kb * KB + kcol, bs, bt, bs2);
                kb_folded = kb;
            }
            // the second block's residual: behind the first block's first row, or (a role copy with two BatchNorms, which has a
            // register less) behind its third
            constexpr int RES1_AT = ROLES && MODE == 3 ? 2 : 0;
            float q[2][4][4];                                                     // the residual of one tile block, one block ahead
            __amdgpu_buffer_rsrc_t rrsrc;
            if (MODE >= 2) rrsrc = out_window(ep.res, H, W, K, n0, kb, yrange);
            auto load_res = [&](int h) {
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    unsigned o4[4];
                    offsets(4 * h + rr, o4);
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        q[h][rr][e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rrsrc, (int)o4[e], 0, 0));
                }
            };
            if (MODE >= 2) {
                load_res(0);
                __builtin_amdgcn_sched_barrier(0);
            }
            // 18 wait states between the last MFMA's write and the hand-written reads of its registers (more than an 8-pass MFMA needs)
            asm volatile("s_nop 15\n\ts_nop 3");
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                const int h = b >> 2, r = b & 3;
                if (MODE >= 2 && b == RES1_AT) {
                    load_res(1);
                    __builtin_amdgcn_sched_barrier(0);
                }
                unsigned o4[4];
                offsets(b, o4);
                float m[16];
#pragma unroll
                for (int p = 0; p < 16; ++p) asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(m[p]) : "a"(acc[p][h][r]));
                float s0[4], s1[4];
#pragma unroll
                for (int nu = 0; nu < 4; ++nu) {
                    s0[nu] = m[nu] + m[4 + nu] + m[8 + nu];
                    s1[nu] = m[4 + nu] - m[8 + nu] - m[12 + nu];
                }
                float y00 = s0[0] + s0[1] + s0[2], y01 = s0[1] - s0[2] - s0[3];
                float y10 = s1[0] + s1[1] + s1[2], y11 = s1[1] - s1[2] - s1[3];
                if (MODE >= 1) {
                    constexpr int RES = MODE - 1;
                    const float *const qr = q[h][r];
                    y00 = bn_finish<RES, RELU>(bn_apply(y00, bs, bt), RES ? qr[0] : 0.f, bs2);
                    y01 = bn_finish<RES, RELU>(bn_apply(y01, bs, bt), RES ? qr[1] : 0.f, bs2);
                    y10 = bn_finish<RES, RELU>(bn_apply(y10, bs, bt), RES ? qr[2] : 0.f, bs2);
                    y11 = bn_finish<RES, RELU>(bn_apply(y11, bs, bt), RES ? qr[3] : 0.f, bs2);
                }
                const float y4[4] = {y00, y01, y10, y11};
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, y4[e]), yrsrc, (int)o4[e], 0, 0);
#pragma unroll
                for (int p = 0; p < 16; ++p) asm volatile("" : "+a"(acc[p][0]), "+a"(acc[p][1]));
                __builtin_amdgcn_sched_barrier(0);
            }
            cu += G;
            next_unit(cpl);
            cslot = (cslot + 1) & (TINFO_SLOTS - 1);
        } while (cu < s.units);
    };
    units(std::integral_constant<int, DEAL>{});
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

template <int MODE, bool RELU, int SCHED>
__global__ __launch_bounds__(512) void conv3x3_winograd_w16x2_f32(const float *__restrict__ x, const float *__restrict__ U,
                                                                  float *__restrict__ y, const Shape s, const Epilogue ep)
{
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (SCHED == 2 && wave >= 4) {                                            // wave-uniform: one scalar branch
        __builtin_amdgcn_s_setprio(1);
        conv3x3_winograd_w16x2_deal<MODE, RELU, 1, true>(x, U, y, s, ep, wave);
    } else {
        conv3x3_winograd_w16x2_deal<MODE, RELU, 0, SCHED == 2>(x, U, y, s, ep, wave);
    }
}

// U[p = 4 xi + nu][c][k] = (G g G^T)[xi][nu] of weight[k][c][3][3], in fp64, rounded once.  One thread per (c, k).
__global__ __launch_bounds__(256) void winograd_weights_f32(const float *__restrict__ w, int C, int K, float *__restrict__ U)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)C * K) return;
    const int k = (int)(i % K), c = (int)(i / K);
    const float *g = w + ((size_t)k * C + c) * 9;
    double t[4][3];                                                           // G g
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double g0 = g[j], g1 = g[3 + j], g2 = g[6 + j];
        t[0][j] = g0;
        t[1][j] = 0.5 * (g0 + g1 + g2);
        t[2][j] = 0.5 * (g0 - g1 + g2);
        t[3][j] = g2;
    }
#pragma unroll
    for (int xi = 0; xi < 4; ++xi) {
        const double u[4] = {t[xi][0], 0.5 * (t[xi][0] + t[xi][1] + t[xi][2]), 0.5 * (t[xi][0] - t[xi][1] + t[xi][2]), t[xi][2]};
#pragma unroll
        for (int nu = 0; nu < 4; ++nu) U[((size_t)(4 * xi + nu) * C + c) * K + k] = (float)u[nu];
    }
}

// One launch of one instantiation (its dynamic-LDS attribute is set once per device): the persistent kernel over the units
// [0, s.units) -- variant 1: 4 waves on the 32-channel block, 2: 8 waves on the 16-channel block -- then, where tail_units > 0,
// the half-unit kernel over the 2 * tail_units halves of the units behind them
template <int MODE, bool RELU>
static int launch(hipStream_t st, unsigned blocks, const float *x, const float *U, float *y, const Shape &s, const Epilogue &ep,
                  int variant, int schedule, unsigned tail_units)
{
    static PerDevice<int> lds_attr;
    const int rc = lds_attr.get([] {
        const void *const kernels[4] = {reinterpret_cast<const void *>(conv3x3_winograd_w16_f32<MODE, RELU>),
                                        reinterpret_cast<const void *>(conv3x3_winograd_f32<MODE, RELU>),
                                        reinterpret_cast<const void *>(conv3x3_winograd_w16x2_f32<MODE, RELU, 1>),
                                        reinterpret_cast<const void *>(conv3x3_winograd_w16x2_f32<MODE, RELU, 2>)};
        for (int i = 0; i < 4; ++i) {
            const int a = (int)hipFuncSetAttribute(kernels[i], hipFuncAttributeMaxDynamicSharedMemorySize, i ? LDS_BYTES : w16::LDS_BYTES);
            if (a != 0) return a;
        }
        return 0;
    });
    if (rc != 0) return rc;
    if (variant == 2 && schedule == 2)
        hipLaunchKernelGGL((conv3x3_winograd_w16x2_f32<MODE, RELU, 2>), dim3(blocks), dim3(512), LDS_BYTES, st, x, U, y, s, ep);
    else if (variant == 2)
        hipLaunchKernelGGL((conv3x3_winograd_w16x2_f32<MODE, RELU, 1>), dim3(blocks), dim3(512), LDS_BYTES, st, x, U, y, s, ep);
    else
        hipLaunchKernelGGL((conv3x3_winograd_f32<MODE, RELU>), dim3(blocks), dim3(256), LDS_BYTES, st, x, U, y, s, ep);
    if (tail_units)
        hipLaunchKernelGGL((conv3x3_winograd_w16_f32<MODE, RELU>), dim3(2 * tail_units), dim3(256), w16::LDS_BYTES, st, x, U, y, s,
                           ep, s.units);
    return 0;
}

// [mode][relu], trunk_epilogue's names
static const char *const kEpilogueNames[4][2] = {
    {"none", "none"}, {"bn", "bn_relu"}, {"bn_add", "bn_add_relu"}, {"bn_bn_add", "bn_bn_add_relu"}};

static bool bn_ok(const BnVectors &b)
{
    return b.mean && b.var && aligned(b.mean, 4) && aligned(b.var, 4) && aligned(b.gamma, 4) && aligned(b.beta, 4);
}

// What the modes 0 / 1 of the three setters choose for a (C, K, dilation): each flag is set where that side measured faster in
// every repetition of tools/conv_bench.py; a shape that is not listed has none.
//   tail        the last round runs as half units (--tail, profiles/conv_winograd_w16_shapes.txt)
//   eight_wave  the persistent launch is the 8-wave kernel (--variant, the same file)
//   dephased    an 8-wave launch runs the de-phased schedule (--schedule, profiles/conv_winograd_dephase_shapes.txt)
struct Family {
    int C, K, d;
    bool tail, eight_wave, dephased;
};

static Family family_of(int C, int K, int d)
{
    static const Family table[] = {{64, 64, 1, true, true, true},    {128, 128, 1, true, true, true},  {128, 256, 1, true, true, false},
                                   {256, 256, 1, true, true, true},  {256, 256, 2, true, true, true},  {256, 512, 2, false, true, true},
                                   {512, 512, 1, true, true, true},  {512, 512, 4, false, true, true}};
    for (const Family &f : table)
        if (f.C == C && f.K == K && f.d == d) return f;
    return Family{C, K, d, false, false, false};
}

// The schedule of an 8-wave launch of this shape under the current mode: 1 lockstep, 2 de-phased
static int schedule_of(int C, int K, int d)
{
    const int v = g_winograd_schedule.load();
    return v ? v : family_of(C, K, d).dephased ? 2 : 1;
}

// How a call is split: G persistent workgroups run the units [0, R G) and, where the rest is a tail, 2 rem half units run
// the units [R G, units).  Otherwise (half_units = 0) the persistent kernel runs them all.
struct Plan {
    unsigned units, G, R, rem, half_units;
    int variant;                           // 1: conv3x3_winograd_f32, 2: conv3x3_winograd_w16x2_f32
};

static Plan make_plan(const Shape &s, int cus)
{
    Plan p;
    p.units = s.units;
    const int cap = g_winograd_max_workgroups.load();
    p.G = s.units < (unsigned)cus ? s.units : (unsigned)cus;
    if (cap > 0 && p.G > (unsigned)cap) p.G = (unsigned)cap;
    p.R = s.units / p.G;
    p.rem = s.units % p.G;
    const Family f = family_of(s.C, s.K, s.d);
    const int tail = g_winograd_tail.load();
    const bool on = p.rem > 0 && (tail == 2 || (tail == 1 && 2 * p.rem <= p.G && f.tail));
    p.half_units = on ? 2 * p.rem : 0;
    const int v = g_winograd_variant.load();
    p.variant = v ? v : f.eight_wave ? 2 : 1;
    return p;
}

// mode 0: the convolution alone (ep unread).  1..3: with the epilogue in the store.
static int conv_entry(const float *x, const float *U, float *y, int N, int H, int W, int C, int K, int dilation, int mode,
                      bool relu, const Epilogue &ep, void *stream)
{
    if (!x || !U || !y || x == y || N < 0 || H <= 0 || W <= 0 || C <= 0 || K <= 0 || mode < 0 || mode > 3) return (int)hipErrorInvalidValue;
    if (mode >= 1 && !bn_ok(ep.bn)) return (int)hipErrorInvalidValue;
    if (mode == 3 && !bn_ok(ep.bn2)) return (int)hipErrorInvalidValue;
    if (C % 8 != 0 || K % 64 != 0 || !(dilation == 1 || dilation == 2 || dilation == 4) || !aligned(x, 16) ||
        !aligned(U, 16) || !aligned(y, 16) || (mode >= 2 && !aligned(ep.res, 16)))
        return (int)hipErrorNotSupported;
    if (!offsets_fit(H, W, C, K) || !weights_fit(C, K)) return (int)hipErrorNotSupported;
    if (mode >= 2) {
        // the residual is read while other workgroups store y: their byte ranges may not meet
        const uintptr_t r0 = reinterpret_cast<uintptr_t>(ep.res), y0 = reinterpret_cast<uintptr_t>(y);
        const uintptr_t bytes = (uintptr_t)N * H * W * K * 4;
        if (r0 < y0 + bytes && y0 < r0 + bytes) return (int)hipErrorInvalidValue;
    }
    if (N == 0) return 0;
    Shape s;
    if (!tile_shape(s, N, H, W, C, K, dilation)) return (int)hipErrorNotSupported;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    // the persistent grid: one workgroup per CU (one fits), each running every G-th unit; fewer under the tests' cap
    const Plan pl = make_plan(s, device_cus());
    const unsigned nb = pl.G;
    if (pl.half_units) s.units = pl.R * pl.G;                                 // what the persistent kernel runs; the tail starts there
    // the stride from a workgroup's unit to its next one (nb units on), over the tile grid
    s.gr = (int)(nb % (unsigned)s.kblocks);
    const auto stride = [&](int64_t tile_blocks, int &dX, int &dY, int &dn) {
        const int64_t t = tile_blocks * TILES, r = t / s.TX;
        dX = (int)(t % s.TX);
        dY = (int)(r % s.TY);
        dn = (int)(r / s.TY);
    };
    stride(nb / (unsigned)s.kblocks, s.dX0, s.dY0, s.dn0);
    stride(nb / (unsigned)s.kblocks + 1, s.dX1, s.dY1, s.dn1);
    const unsigned tu = pl.half_units / 2;
    const int sch = pl.variant == 2 ? schedule_of(C, K, dilation) : 1;       // the 4-wave kernel has one program
    // [mode][relu]; mode 0 has no activation
    static constexpr decltype(&launch<0, false>) kLaunch[4][2] = {{launch<0, false>, launch<0, false>},
                                                                  {launch<1, false>, launch<1, true>},
                                                                  {launch<2, false>, launch<2, true>},
                                                                  {launch<3, false>, launch<3, true>}};
    const int rc = kLaunch[mode][relu ? 1 : 0](st, nb, x, U, y, s, ep, pl.variant, sch, tu);
    if (rc != 0) return rc;
    g_winograd_last_tail_units = (int)tu;
    g_winograd_last_variant = pl.variant;
    g_winograd_last_schedule = sch;
    g_winograd_last_kernel = "conv3x3_winograd_f32";
    g_winograd_last_epilogue = kEpilogueNames[mode][mode && relu ? 1 : 0];
    g_winograd_launches.fetch_add(1);
    return (int)hipGetLastError();
}

}  // namespace wino
}  // namespace mvdetr

extern "C" int mvdetr_winograd_weights_f32(const float *w, int C, int K, float *U, void *stream)
{
    using namespace mvdetr;
    if (!w || !U || C <= 0 || K <= 0) return (int)hipErrorInvalidValue;
    if (C % 8 != 0 || K % 64 != 0 || !aligned(w, 4) || !aligned(U, 16) || (int64_t)C * K > (int64_t)1 << 26)
        return (int)hipErrorNotSupported;
    hipLaunchKernelGGL(wino::winograd_weights_f32, dim3((unsigned)(((int64_t)C * K + 255) / 256)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), w, C, K, U);
    g_winograd_last_kernel = "winograd_weights_f32";
    g_winograd_launches.fetch_add(1);
    return (int)hipGetLastError();
}

extern "C" int mvdetr_conv3x3_winograd_f32(const float *x, const float *U, float *y, int N, int H, int W, int C, int K,
                                           int dilation, void *stream)
{
    return mvdetr::wino::conv_entry(x, U, y, N, H, W, C, K, dilation, 0, false, mvdetr::wino::Epilogue{}, stream);
}

extern "C" int mvdetr_conv3x3_winograd_bn_act_f32(const float *x, const float *U, float *y, int N, int H, int W, int C, int K,
                                                  int dilation, const float *mean, const float *var, const float *gamma,
                                                  const float *beta, float eps, const float *res, const float *res_mean,
                                                  const float *res_var, const float *res_gamma, const float *res_beta,
                                                  float res_eps, int relu, void *stream)
{
    using namespace mvdetr;
    const bool res_bn = res_mean || res_var || res_gamma || res_beta;
    if (res_bn && !res) return (int)hipErrorInvalidValue;
    const wino::Epilogue ep{BnVectors{mean, var, gamma, beta, eps}, BnVectors{res_mean, res_var, res_gamma, res_beta, res_eps}, res};
    return wino::conv_entry(x, U, y, N, H, W, C, K, dilation, !res ? 1 : res_bn ? 3 : 2, relu != 0, ep, stream);
}

extern "C" const char *mvdetr_winograd_last_kernel(void) { return mvdetr::g_winograd_last_kernel.load(); }

extern "C" const char *mvdetr_winograd_last_epilogue(void) { return mvdetr::g_winograd_last_epilogue.load(); }

extern "C" int64_t mvdetr_winograd_launch_count(void) { return mvdetr::g_winograd_launches.load(); }

extern "C" int mvdetr_winograd_set_max_workgroups(int n) { return mvdetr::g_winograd_max_workgroups.exchange(n > 0 ? n : 0); }

extern "C" int mvdetr_winograd_set_tail(int mode) { return mvdetr::g_winograd_tail.exchange(mode == 0 || mode == 2 ? mode : 1); }

extern "C" int mvdetr_winograd_set_variant(int v) { return mvdetr::g_winograd_variant.exchange(v == 1 || v == 2 ? v : 0); }

extern "C" int mvdetr_winograd_last_variant(void) { return mvdetr::g_winograd_last_variant.load(); }

extern "C" int mvdetr_winograd_set_schedule(int v) { return mvdetr::g_winograd_schedule.exchange(v == 1 || v == 2 ? v : 0); }

extern "C" int mvdetr_winograd_last_schedule(void) { return mvdetr::g_winograd_last_schedule.load(); }

extern "C" int mvdetr_winograd_schedule_of(int C, int K, int dilation) { return mvdetr::wino::schedule_of(C, K, dilation); }

extern "C" int mvdetr_winograd_last_tail_units(void) { return mvdetr::g_winograd_last_tail_units.load(); }

extern "C" int mvdetr_winograd_plan(int N, int H, int W, int C, int K, int dilation, int workgroups, int64_t *out)
{
    using namespace mvdetr;
    if (!out || N <= 0 || H <= 0 || W <= 0 || C <= 0 || K <= 0 || workgroups <= 0) return (int)hipErrorInvalidValue;
    wino::Shape s;
    if (C % 8 != 0 || K % 64 != 0 || !(dilation == 1 || dilation == 2 || dilation == 4) ||
        !wino::tile_shape(s, N, H, W, C, K, dilation))
        return (int)hipErrorNotSupported;
    const wino::Plan p = wino::make_plan(s, workgroups);
    out[0] = p.units; out[1] = p.G; out[2] = p.R; out[3] = p.rem; out[4] = p.half_units; out[5] = p.variant;
    return 0;
}

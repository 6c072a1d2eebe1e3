// Hole filling of the finished mosaic (sucre_mosaic_fill_*): a bounded push-pull over a pyramid of the grid.  A pure grid
// operation: it reads no image and issues no atomic, every cell is written by exactly one lane, and every number is formed by a
// fixed chain of float32 operations -- the same bits on every run, as the rest of the mosaic (mosaic.h).  The library's
// -ffp-contract=off and IEEE divide hold: ONE IEEE operation per step below, every product rounded before its add.
//
// Levels.  Level 0 is the mosaic, H_0 = Hm, W_0 = Wm; H_(l+1) = (H_l + 1) >> 1, W likewise; the caller gives L = `levels` in
// 1..24 (engine.mosaic_fill_levels: the smallest L >= 1 with gsd 2^L >= R, in float64, capped at the first level that is 1x1).
// A RECORD is 8 float32 = 32 bytes: c[0..2] for J, c[3..5] for the raw colour as float, w, g.  The pyramid holds the levels
// 1..L, each row-major and 256-byte aligned (fill_pyramid_bytes); level 0 is read in place from J, raw and source: no copy.
//   level 0   a cell is VALID (w = 1) when source >= 0 and its three J channels are finite: c = its J and raw values.
//             Otherwise w = 0 and every c counts as +0.0f (a measured cell with a non-finite J contributes nothing).
//   pull      l -> l+1, the children (2y+dy, 2x+dx) in the order (0,0), (0,1), (1,0), (1,1); a child outside the level is a
//             record of zeros; all four terms are always added:
//               Wt  = ((w0 + w1) + w2) + w3
//               S_k = ((w0 c0_k + w1 c1_k) + w2 c2_k) + w3 c3_k
//             Wt > 0: c_k = S_k / Wt, w = Wt 0.25f, g = l+1.  Otherwise the record is all +0.0f: wherever w == 0, c is stored
//             as +0.0f, so the sign of every zero that enters a sum is pinned (a valid -0.0f gives -0.0f + 0.0f = +0.0f).
//   push      l = L-1 .. 0, in place; level l+1 is complete by then (level L as pulled).  A cell with w > 0 is untouched.
//             For a cell (y, x) with w == 0: py = y >> 1, ny = clamp(py + (y & 1 ? 1 : -1), 0, H_(l+1) - 1); px, nx likewise.
//             Taps, in this order: (py,px) k = 9/16, (py,nx) 3/16, (ny,px) 3/16, (ny,nx) 1/16; a_i = k_i when the tap's
//             w > 0, otherwise 0:
//               A   = ((a0 + a1) + a2) + a3
//               S_k = ((a0 c0_k + a1 c1_k) + a2 c2_k) + a3 c3_k
//             A > 0: c_k = S_k / A, w = 1, g = the largest g of the taps with a_i > 0.  Otherwise the cell stays empty.
//   outputs   (level 0's push writes them for EVERY cell, no record):
//             J_filled    a measured cell (source >= 0): J bit for bit, finite or not; a filled cell: c[0..2]; an unfilled
//                         one: the NaN 0x7fc00000
//             raw_filled  measured: raw; filled: (uint8)rintf(fminf(fmaxf(c[3+k], 0), 255)); unfilled: 0
//             fill_level  measured: 0; filled: g, in 1..L -- the coarsest level its value drew on; unfilled: -1
// What follows from the taps (asserted by tests/mosaic_fill_ref.py on random masks): every empty cell within Chebyshev distance
// 2^(L-1) cells of a valid cell is filled, and no cell at 3 x 2^L cells or more from every valid cell is.
//
// Kernels: one lane per destination cell, workgroups of 64 x 4 cells (a wave: 64 consecutive cells of a row), the tile from a
// linear workgroup index; records move as two 16-byte loads or stores, a wave's 64 records of a row as 2 KiB contiguous.  The
// level-0 side is not vectorised: J and raw are 12- and 3-byte cells with 4- and 1-byte alignment, read and written as three
// dwords and three bytes per lane, contiguous across a wave's row.  No LDS.  One launch per level and direction: 2 L launches.  A pull reads every record of its source level once (the 2 x 2 children
// of a lane are two 64-byte runs) and writes a quarter as many; a push reads a level's own records, for its empty cells the
// four taps (served by the cache: neighbours share them), and writes the empty cells alone.
// Measured on one MI355X (tools/mosaic_fill_time.py, profiles/mosaic_fill_time.txt; 65 resident images of 1080p, warm): at the
// default gsd, 2181 x 916 cells, L = 3: pull 0.025 ms for the 79 MB it must move (3.2 TB/s, from arrays the phases before have
// just written), push 0.029 ms for 78 MB (level 0 in and out, no tap) to 117 MB (every record read whole): 2.7 to 4.0 TB/s; the
// gather phase of the same run: 0.65 ms.  At half the gsd, 4362 x 1831 cells, L = 4: 0.069 ms (321 MB) and 0.103 ms (314 to
// 472 MB) against 0.71 ms.  8 to 10 microseconds per launch at the default gsd, near a launch's floor: the optional
// single-workgroup tail for the coarse levels was not built.
#pragma once
#include "launch.h"

namespace sucre {

constexpr int kFillMaxLevels = 24;       // Hm, Wm <= 2^24: level 24 is 1x1 at the latest
constexpr uint32_t kFillTileW = 64, kFillTileH = 4;   // cells of a workgroup

struct FillRecord {
    float c[6];
    float w, g;
};
static_assert(sizeof(FillRecord) == 32, "a record is two 16-byte accesses");

struct FillBase {   // level 0, read in place
    const uint32_t *J;   // the floats' bit patterns: a measured cell is copied, not computed with
    const uint8_t *raw;
    const int32_t *source;
};

struct FillOut {
    uint32_t *J;
    uint8_t *raw;
    int32_t *level;
};

inline int fill_next(int n) { return (n + 1) >> 1; }
inline size_t fill_level_bytes(int H, int W) { return align_up((size_t)H * (size_t)W * sizeof(FillRecord), 256); }
inline size_t fill_pyramid_bytes(int Hm, int Wm, int levels) {
    size_t bytes = 0;
    for (int l = 1, H = Hm, W = Wm; l <= levels; ++l) {
        H = fill_next(H); W = fill_next(W);
        bytes += fill_level_bytes(H, W);
    }
    return bytes;
}
inline uint64_t fill_blocks(int H, int W) {
    return (uint64_t)((W + kFillTileW - 1) / kFillTileW) * (uint64_t)((H + kFillTileH - 1) / kFillTileH);
}

// Levels 1..L from level 0 (L launches on s), and back down to the three outputs (L launches).  The caller has checked that every
// level's workgroups fit a launch.
hipError_t launch_fill_pull(int Hm, int Wm, int levels, const FillBase &base, void *pyramid, hipStream_t s);
hipError_t launch_fill_push(int Hm, int Wm, int levels, const FillBase &base, void *pyramid, const FillOut &out, hipStream_t s);

}  // namespace sucre

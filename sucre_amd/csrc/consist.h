// Cross-view colour consistency of restored images (sucre_view_consistency): does the restored J of the target agree with
// the restored J of its neighbours on the seabed they both see -- and better than the raw pictures did?
//
// For every view k and every target pixel p1 the match is match_pixel()'s (match_pixel.h: the very function match_kernel and
// match_map_kernel call, so the matched set IS sucre_match_map's); the pair is VALID when neither a = J_target[p1] nor
// b = J_k[p2] holds a NaN in any channel (plot_J's rule, sucre.py:86-87).  Over the valid pairs:
//   count (H,W) int32         views with a valid pair at the pixel
//   ssd   (H,W,3) float32     sum over k (ascending) of (a_c - b_c)^2, fmaf(d, d, acc)
//   stats (n_views,26) float64  [0] matches, [1] valid pairs, [2:14] sum d^2, a^2, b^2, a b of J (three channels each),
//                             [14:26] the same four sums of the raw colours k / 255 of the same pixels of the same pairs
//
// One workgroup per 16x16 target tile, one lane per pixel: wave w owns rows 4 w .. 4 w + 3 of the tile (sixteen adjacent lanes
// gather from sixteen adjacent pixels of a row, match_kernel's arrangement) and walks the views in order on its own -- no
// barrier, no LDS.  count and ssd stay in the owning lane's registers and are stored once.  Per (tile, view) every wave's two
// pair counts come from ballots and always go to scratch (4 bytes); its 24 float32 sums go through the fixed-shape tree of
// handoff.h and are written by lane 0 only where the wave has a valid pair in the view -- the common case for most (tile, view)
// pairs of a survey is none.  The second kernel reads the count words first; it adds a tile's four waves in float32, in wave
// order -- the float32 sum of the (16x16 tile, view) pair -- and every view's tiles in float64 in a fixed order
// (residual_view_sum_kernel's).  No atomics, no map in memory: two calls give the same bits.
// Measured on one MI355X, 1080p target against 64 neighbours (tools/consistency_time.py, profiles/consistency_time.txt): 1.48 ms
// for the first kernel, 0.14 ms for the second, against 0.72 ms for match_kernel on the same views.  What did not pay: a wave
// per whole tile with four pixels per lane (157 VGPRs, 3 waves per SIMD instead of 6: 2.93 against 2.77 ms, both with the view
// table read through vector loads -- see consist.hip; the table, not the occupancy, was what cost).
#pragma once
#include "launch.h"

namespace sucre {

constexpr int kConsistSums = 24;          // float32 sums per (tile, view): {d^2, a^2, b^2, a b} x {R, G, B} of J, then of the raw colours
constexpr int kConsistStats = 2 + kConsistSums;   // columns of a view's row

// scratch: uint32 [n_views][n_tiles][4 waves] (matches | valid pairs << 16; both <= 64), then float [n_views][n_tiles][4 waves][24]
inline size_t consist_counts_bytes(int n_tiles, int n_views) { return (size_t)n_tiles * n_views * 4 * sizeof(uint32_t); }
inline size_t consist_scratch_bytes(int n_tiles, int n_views) {
    return consist_counts_bytes(n_tiles, n_views) + (size_t)n_tiles * n_views * 4 * kConsistSums * sizeof(float);
}

hipError_t launch_consistency(int H, int W, int n_views, const sucre_view_t &target, const sucre_view_t *views_dev, const float *J_target,
                              const float *const *J_views, int32_t *count, float *ssd, double *stats, void *scratch, hipStream_t s);

}  // namespace sucre

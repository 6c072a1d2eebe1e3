// View-supported surface of the seabed mosaic (sucre_mosaic_support, sucre_mosaic_support_top, sucre_mosaic_cull_supported): the
// surface of surface.h is a plain minimum, so ONE spurious high sample -- a fish, a diver's fin, one view's bad depth patch --
// owns its cell and culls the seabed under it.  Such outliers come per IMAGE, not per sample (a fish in one image puts dozens of
// samples into a cell), so a median over samples is the wrong robustness.  Here the surface of a cell is the highest level that at
// least M DIFFERENT images reach, and what stands more than T ABOVE it goes the way of what lies more than T below it.
//
// A sample: a pixel that takes part (mosaic_member, mosaic_pixel) and has a cell (mosaic_cell); a_n is the float32 of surface.h; a
// sample whose a_n is a NaN adds nothing.  ordinal: the image's position in the request -- A VIEW LISTED TWICE HAS TWO ORDINALS AND
// COUNTS TWICE.
//   key64     = (uint64)order_key(a_n) << 32 | ordinal
//   level 0   of a cell: the minimum key64 over all its samples
//   level r   the minimum over the samples whose ordinal is not the ordinal (low word) of one of the levels 0 .. r-1 of the cell
// so the levels are the per-image tops of the cell in ascending (height key, ordinal) order, one per image; an exact height tie
// goes to the earlier image.  A level that finds no sample stays all ones, and so do all levels above it.
//   n = the levels of the cell that are not all ones (0 <= n <= M), m = min(M, n)
//   top[cell]            = the high word of level m-1 for n >= 1 (the uint32 key of surface.h's top: key_value, the `surface`
//                          output and the DEM picture work unchanged), all ones for n = 0
//   support[cell]        = n                     surface_source[cell] = the low word of level m-1, -1 for n = 0
// A CELL SEEN BY FEWER THAN M IMAGES RESTS ON THE LOWEST OF ITS PER-IMAGE TOPS, not on the plain minimum.
// The two-sided cull: d = a_n - key_value(top[cell]), one float32 subtraction; culled BELOW when d > T (surface.h's rule), culled
// ABOVE when d < -T; a cell whose top is all ones culls nothing.
//   - The sample that defines the supported top has d = 0 and is never culled: the set of filled cells, n_filled, the bounds and
//     the grid stay those of a run without the flag.
//   - M = 1: the supported top is the plain minimum, no sample lies above it, and every output equals surface.h's bit for bit.
//   - All state is integer minima and integer counts: the same bits in any order of arrival, any batch split, any schedule and
//     either atomic form.
//   - THE LIMIT: an error shared by M or more images passes, and a real feature that only ONE image sees and that stands more than
//     T above what M images agree on is removed.
//
// support      the walk of mosaic.h (one lane per pixel, 32 images per launch), one pass over ALL images per level, level r after
//              level r-1 has seen them all.  rank: (n_levels, Hm Wm) uint64, all ones at the start.  A lane of level r reads the
//              cell's levels 0 .. r-1 (8-byte loads of final words, rank[(size_t)level Hm Wm + cell]) and returns when level r-1
//              is all ones or one of the low words is its own ordinal; unless SUCRE_MOSAIC_PLAIN_ATOMIC is given it then loads
//              level r's word and skips the atomic when the stored key is not above its own (the splat's filter: a stale value
//              can only be larger); else the splat's 64-bit atomicMin.  No LDS, no scratch.
// support_top  one lane per cell, no image read: top, support, surface_source from the n_levels words of the cell.
// cull         surface.h's cull with the second side (surface.hip's one kernel, the side a template argument; launch_mosaic_cull
//              with two_sided): the same J_out copy in the same layout; culled (uint32 per cell)
//              counts the samples culled below, culled_above those culled above; counts (uint64 x 3): culled below, culled above,
//              samples with a cell, by the 32-blocks-per-workgroup scheme, at most one atomic per counter and workgroup.
// Registers (gfx950, -O3; the build's support.rpt, the cull's in surface.rpt): support 10 VGPR / 58 SGPR in both forms, support_top
// 9 / 24, the two-sided cull 12 / 70, its counting form 17 / 84 (the one-sided 12 / 68 and 17 / 78, 32 bytes of LDS); 8 waves per SIMD everywhere, no scratch, LDS only in the counting cull (48 bytes).
// Measured on one MI355X, 65 resident images of 1080p, 74 pixels per cell, in ONE run (tools/mosaic_support_time.py,
// profiles/mosaic_support_time.txt), next to the splat's 0.87 ms, sucre_mosaic_surface's 0.75 ms and invert_kernel's 0.61 ms in
// the same run: levels 0, 1, 2, 3 take 0.77, 0.92, 1.04 and 1.15 ms with the load ahead of the atomic -- 0.89 to 1.33 of the splat:
// the same atomic behind the same filter, and 0.12 ms per level read below, one scattered 8-byte load per lane -- and 2.6-2.8 ms
// with the plain 64-bit atomic for every pixel (the load is kept as the default); support_top 0.02 ms; the two-sided cull 0.82 ms,
// 0.85-0.87 ms with its three counts (1.38 ms with 49 % of the samples culled), against 0.78 ms for surface.h's in the same run.
// Not built: the single-pass k-smallest form -- one pass that keeps the M smallest per-image keys of a cell in one update (a CAS
// loop over M words, or a 128-bit word for M = 2) instead of M passes of one atomicMin each.
#pragma once
#include "surface.h"

namespace sucre {

constexpr int kSupportMax = 4;          // the most views a supported surface asks for (SUCRE_MOSAIC_SUPPORT_MAX)
static_assert(kSupportMax == SUCRE_MOSAIC_SUPPORT_MAX, "the most supporting views is public");

// Level `level` of the ranks over images[0 .. n): the launches of a phase of mosaic.h; rank: lowered at that level, read below it.
hipError_t launch_mosaic_support(bool plain, void *table, int n_images, const sucre_mosaic_image_t *images, int first_ordinal,
                                 const MosaicGrid &grid, int level, unsigned long long *rank, hipStream_t s);

// The supported top of every cell from its n_levels rank words (one launch); support, source: may be NULL.
hipError_t launch_mosaic_support_top(const MosaicGrid &grid, int n_levels, const unsigned long long *rank, uint32_t *top, int32_t *support,
                                     int32_t *source, hipStream_t s);

}  // namespace sucre

// Surface test of the seabed mosaic (sucre_mosaic_surface, sucre_mosaic_cull): a per-cell top height along the mosaic's own viewing
// direction, and the samples that lie too far below it taken out of every later phase.  The phases of mosaic.h decide by range
// alone, the least water between camera and seabed, so a camera close to a LOWER surface -- the seabed under a ledge, the foot of
// a wall seen obliquely, a view whose depth map is off -- beats a camera further from the surface above it, and the blend mixes
// both layers into one colour.  The top height is also the height product next to the ortho picture (a DEM).
//
// For a pixel that takes part (mosaic_member, mosaic_pixel) and has a cell (mosaic_cell), float32, one IEEE operation per step:
//   a_n = dot3(e3, wP)                            e3: row 2 of the axes; wP: the very wP that a_s and a_t are formed from
// e3 looks the way the cameras look, so SMALLER IS HIGHER.
//   top[cell] = key_value(min order_key(a_n))     over all such pixels of all images (order_key.h: the integer image of the float
//                                                 order, so -0.0 lies below +0.0 and the minimum has one bit pattern; a pixel whose
//                                                 a_n is a NaN adds nothing)
// A sample is CULLED when a_n - top[cell] > T: one subtraction, one comparison, T = float32(T) formed on the host, T > 0.  A culled
// pixel is a NON-MEMBER for everything after that -- splat, resolve, gather, accumulate, the feather's map, the band split --: the
// cull writes a copy of the image's J with the NaN 0x7fc00000 in all three channels of every culled pixel (and of every pixel that
// was no member before), every other pixel's J bit for bit, and the phases of mosaic.h and bands.h get that copy as the image's J.
// Their kernels are not changed.  The bounds and the grid (lo, Wm, Hm) are those of ALL members, as without the test: cells stay
// comparable between runs.
//   - A cell's top sample is never culled (a_n - a_n = 0 <= T), so the set of filled cells does not change.
//   - An integer min and an integer count are order-free: the same bits in any order, batch split and schedule.
//   - A T that culls nothing leaves every output of the other phases identical bit for bit (the copy IS J at the members).
// The feather then fades towards a culled region as it does towards a NaN patch: it is a seam.
// THE SURFACE IS A PLAIN MINIMUM: one spurious high sample -- a fish, a bad depth -- owns its cell and culls the seabed under it
// (the best view has the same weakness with the nearest sample).  The remedy is support.h: the top that M different images reach,
// and a cull on both sides of it -- this file's cull kernel with its second side compiled in --; its M = 1 is this surface bit for bit.
//
// surface  the walk of mosaic.h (one lane per pixel, 32 images per launch): atomicMin(top[cell], order_key(a_n)), uint32 per cell,
//          empty: all ones.  Unless SUCRE_MOSAIC_PLAIN_ATOMIC is given, top[cell] is loaded first and the atomic skipped when the
//          stored key is not above the lane's (the splat's filter: a stale value can only be larger than the current one).
// cull     one lane per pixel on the same walk.  J_out: a buffer in the band buffers' layout (bands.h, band_bytes): image i's
//          (H,W,3) block starts at PIXEL 256 sum_(j<i) ceil(H_j W_j / 256), so a lane finds its pixel behind its launch's first
//          pixel; the pixels between two images are not written.  culled (uint32 per cell, or NULL): a culled sample adds 1 to its
//          cell, a no-return integer atomic.  counts (uint64 x 2, or NULL): culled samples, samples with a cell.  With counts a
//          workgroup walks 32 consecutive 256-pixel blocks of the launch, one after the other (still one lane per pixel of a block),
//          sums its waves' ballots as it goes and adds to each counter at most once: two atomics per 8192 pixels.  With two per
//          256 pixels every workgroup's atomics met on one cache line -- 6.4 ms against 0.82 ms without the counters, the bounds
//          phase's finding (mosaic.h).  A cell whose top is still all ones culls nothing.
// Measured on one MI355X, 65 resident images of 1080p, 74 pixels per cell, in ONE run (tools/mosaic_surface_time.py,
// profiles/mosaic_surface_time.txt), next to the splat's 0.86 ms and invert_kernel's 0.60 ms in the same run: the surface phase
// 0.79 ms with the load ahead of the atomic -- 0.92 of the splat, a narrower atomic behind the same filter, as expected -- and
// 2.38 ms with the plain 32-bit atomic for every pixel (3.0 x; the load is kept as the default); over tops that are final already
// 0.56 against 2.39 ms.  The cull 0.77-0.80 ms, 1.3 x invert_kernel (it moves 28 bytes per pixel against that kernel's 19: 1.47 by
// the bytes), 0.82 ms with its counts.  With every second depth map scaled by 1.01 and T = 0.005 m -- 49 % of the samples culled,
// 65 M per-cell adds into 1.7 M cells -- the cull with its counts takes 1.38 ms, without them 0.77 ms; the surface phase 0.71 ms.
// The cull is run again for every phase and batch (one buffer, no copy of the request is held): four phases of a blended mosaic
// add about 3.2 ms to the accumulate's 23.8 ms.
// Not built: the accumulate's run sums ahead of the surface's atomic (adjacent lanes that share a cell) -- behind the filter only a
// cell's first arrivals reach the atomic at all, and the phase already runs below the splat.
#pragma once
#include "mosaic.h"

namespace sucre {

struct MosaicCull {   // what a cull launch writes besides J_out
    uint32_t *culled;               // per cell: culled (two-sided: culled below); or NULL
    uint32_t *culled_above;         // two-sided, per cell: culled above; or NULL.  Not read by the one-sided cull
    unsigned long long *counts;     // culled samples, samples with a cell -- two-sided: culled below, culled above, samples with a
                                    // cell --; or NULL
};

// The surface phase over images[0 .. n): the launches of a phase of mosaic.h; top: lowered.
hipError_t launch_mosaic_surface(bool plain, void *table, int n_images, const sucre_mosaic_image_t *images, int first_ordinal,
                                 const MosaicGrid &grid, uint32_t *top, hipStream_t s);

// The cull over images[0 .. n) into J_out (band_bytes of bands.h for the same images); top: read.  two_sided: support.h's cull, the
// same kernel with its second side and its third counter.
hipError_t launch_mosaic_cull(bool two_sided, void *table, int n_images, const sucre_mosaic_image_t *images, int first_ordinal,
                              const MosaicGrid &grid, const uint32_t *top, float tol, float *J_out, const MosaicCull &out, hipStream_t s);

}  // namespace sucre

// Multi-band blend of the seabed mosaic (sucre_mosaic_band_*): every image is split into K detail bands and a residual in SOURCE
// space, every band is blended by the blend's own accumulate (mosaic.h, "The blend", "The feather": the kernel takes any float32
// image as J, signed values included) with a transition that halves with every finer band, and one pass over the cells adds the
// K + 1 blended bands.  The low frequencies of a cell are then the consensus of every view that saw it -- what is wrong with a far
// view's water model is smooth --, the fine detail comes from the view that saw it through the least water -- what is wrong with
// a far view's detail, amplified noise and depth error, is fine-grained (Burt & Adelson 1983 with this project's weight).
//
// THE STACK of an image, K in 1..kBandsMax = 6; its members are mosaic_member's (mosaic.h).  Float32, one IEEE operation per step:
//   S_0 = min(max(J, -1024), 1024) at members       the clamp the accumulate applies anyway; an infinity becomes finite, so the
//                                                   members of every band are the members of J
//   level j -> j+1, step s = 2^j: a 3-tap [1, 2, 1] a-trous filter each way, normalised over the members.  With a(u,v) = S_j at a
//   member and +0.0f elsewhere and outside the image, m(u,v) the same with 1 and 0:
//     Nh(u,v) = (a(u-s,v) + 2 a(u,v)) + a(u+s,v)        Ah likewise in integers
//     N(u,v)  = (Nh(u,v-s) + 2 Nh(u,v)) + Nh(u,v+s)     A likewise, 0..16; a member has A >= 4
//     S_(j+1) = N / (float)A                            IEEE divide
//   D_j = S_j - S_(j+1), j = 0..K-1
// and at a non-member every S and every D is the NaN 0x7fc00000 in all three channels.  The factor 2 is exact, so a contracted FMA
// would give the same bits as the two operations; all four terms are always added, so signed zeros are pinned.  The stack is
// D_0 .. D_(K-1), S_K: it depends on the image's own depth and J alone, and a constant image has D_j = 0 exactly.
//
// THE BUFFER of one band of one call (band_bytes): image i's (H,W,3) float32 block starts at PIXEL 256 sum_(j<i) ceil(H_j W_j / 256)
// -- the feather map's placement (mosaic.h) with 12 bytes per pixel, so the lane of the walk finds its pixel behind its launch's
// first pixel without a pointer per image.  The pixels between two images are not written.
//
// The split kernel: one lane per pixel on the walk's row segments (a wave's lanes hold consecutive pixels of a row, so every tap
// row is a coalesced load), the fused nine-point form evaluated in the separable order above; no intermediate buffer, no LDS.
// Level 0 reads depth and J and forms S_0 on the fly (every tap is clamped where it is read); from level 1 on a NaN in S_in marks a
// non-member.  A tap outside the image is not read.
//
// The combine pass, one lane per cell, reads no image: acc_bands holds n_bands = K + 1 accumulators of the blend's layout, band j
// at slice j, the residual last.  For a cell whose residual has a count (word 7) > 0:
//   B_j = mosaic_quotient(acc_j,c, wsum_j)                the normalise pass's quotient, the same function
//   J_multiband_c = (..((B_K + B_(K-1)) + B_(K-2)) ..) + B_0     float32, coarse to fine
// Empty cells are not touched.  EVERY FILLED CELL HAS wsum_j >= 4 IN EVERY BAND: the cell's winner has d = 0, so t = 1 whatever the
// band's H_j, and its feather factor is f >= 1 / F_j >= 1 / 1024 (mosaic.h, "The feather"), so its wq >= 4.
#pragma once
#include "mosaic.h"

namespace sucre {

constexpr int kBandsMax = 6;            // detail bands of a stack (SUCRE_MOSAIC_BANDS_MAX): steps 1 .. 32
static_assert(kBandsMax == SUCRE_MOSAIC_BANDS_MAX, "the largest band count is public");

// The pixels of one band buffer of images[0 .. n), every image rounded up to whole workgroups (feather_words: the same count).
inline size_t band_bytes(int n_images, const sucre_mosaic_image_t *images) { return feather_words(n_images, images) * 3 * sizeof(float); }

// One level of the stack over images[0 .. n) (one launch per 32 images, plus the table's): S_in NULL for level 0.
hipError_t launch_band_split(void *table, int n_images, const sucre_mosaic_image_t *images, int level, const float *S_in, float *S_out,
                             float *D_out, hipStream_t s);

// The per-cell sum of the n_bands blended bands (one launch).
hipError_t launch_band_combine(const MosaicGrid &grid, int n_bands, const long long *acc_bands, float *J_out, hipStream_t s);

}  // namespace sucre

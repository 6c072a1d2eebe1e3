// Seabed mosaic of restored images (sucre_mosaic_*): a best-view ortho splat.  Every pixel of every image is dropped onto a
// plane grid; the pixel seen through the LEAST water wins its cell.  No float atomics: the optional blend
// ("The blend" below) sums in fixed point.  Cells no pixel lands in stay empty here; closing them is fill.h.  Range alone decides
// here; a test of the samples' height along e3 ahead of every phase, which hands the phases a culled copy of J, is surface.h.
//
// A pixel p = v W + u of image i (its ordinal: the position in the request) TAKES PART when d > 0 and J[p] holds no NaN in any
// channel (plot_J's rule, sucre.py:86-87).  Then, all in float32 with explicit FMAs (the library is built with
// -ffp-contract=off and IEEE divide / sqrt):
//   cP = unproject(Kinv, u, v, d)                 match_pixel.h, sfm.py:90-93
//   z  = sqrtf(cP.x cP.x + cP.y cP.y + cP.z cP.z) the range, invert.h's chain for the same quantity
//   wP = rigid(R, t, cP)                          match_pixel.h, sfm.py:49-55
//   a_s = dot3(e1, wP), a_t = dot3(e2, wP)        e1, e2: rows 0 and 1 of the mosaic's axes
//   q_s = (a_s - lo_s) / gsd, q_t = (a_t - lo_t) / gsd;  the pixel is dropped unless 0 <= q_s < Wm and 0 <= q_t < Hm;
//   cell = (int)q_t * Wm + (int)q_s
// The WINNER of a cell is the pixel with the lexicographically smallest (bits of z, ordinal, p): z > 0, so its bit pattern
// orders like its value; ties on z to the bit go to the earlier image, ties within an image to the lower pixel index.  The rule
// does not depend on the order in which pixels arrive: two runs give the same bits.
//
// Four phases, one entry each (a caller with several ranks can all-reduce bounds, keys and pixel words between them):
//   bounds   min / max of a_s, a_t over the pixels that take part: reduced per wave (shuffles) and per workgroup (LDS), then at
//            most ONE atomicMin / atomicMax per workgroup on each of four order_key words (order_key.h), skipped when a load of
//            the word shows that it has passed the workgroup's extreme already (as the splat's filter: a stale value is safe)
//   splat    atomicMin of (uint64)bits(z) << 32 | ordinal into key[cell] (empty: all ones; below 2^63, a valid int64 as well).
//            Unless SUCRE_MOSAIC_PLAIN_ATOMIC is given, key[cell] is loaded first and the atomic skipped when the stored key is
//            already smaller: a stale value can only be larger than the current one, so nothing that could win is skipped
//   resolve  a pixel whose key equals key[cell] does atomicMin(pix[cell], p) (uint32; empty: all ones)
//   gather   the pixel with the cell's key AND pix[cell] == p writes the cell's five outputs: exactly one per filled cell
// Every phase forms a pixel's numbers with the same function (mosaic_pixel), so the phases agree on who takes part and where.
// Walk (invert_kernel's): one lane per pixel, rows contiguous across the lanes, workgroup b of the grid finds its image by
// bisecting the first-workgroup column of a device table of up to 32 images; the image's camera is wave-uniform and read with
// scalar loads (SGPR-resident, as CamDev is for a single target).
// Measured on one MI355X, 65 resident images of 1080p, 74 pixels per cell (tools/mosaic_time.py, profiles/mosaic_time.txt): bounds
// 0.97 ms, splat 0.86 ms, resolve 0.59 ms, gather 0.61 ms, against 0.58-0.62 ms for invert_kernel on the same images.  The plain
// 64-bit atomic min for every pixel: 2.77 ms (48 G atomics/s; 25 G/s at 1176 pixels per cell) -- the load ahead of it is kept.  The
// bounds phase without ITS load: 12.0 ms (every workgroup's four atomics land on one cache line).
//
// The blend (sucre_mosaic_accumulate, sucre_mosaic_normalize): a range-weighted mean of ALL the pixels of a cell, next to the
// best-view outputs.  A float sum would depend on the order of arrival; a sum of integers does not, so the weights and the
// colours are quantised first and summed with 64-bit integer atomics: the same bits in any order and any batch split.
// After the splat key[cell] >> 32 holds the bits of zmin, the cell's smallest range.  A pixel that takes part (mosaic_pixel)
// and has a cell (mosaic_cell), with range z, float32, one IEEE operation per step (inv_h = 1 / H from the host, H the blend depth):
//   d    = z - zmin                                >= 0; 0 for the winner and its ties
//   t    = fmaxf(1 - d inv_h, 0)                   the product rounded, then the difference
//   wq   = (int)rintf((t t) 4096)                  0 .. 4096; 4096 for the winner
//   Jq_c = (int64)rintf(fminf(fmaxf(J_c, -1024), 1024) 1048576)     |Jq_c| <= 2^30; an infinity is clamped too
// A pixel with wq == 0 adds nothing.  Every other one adds into its cell's eight int64 words (kMosaicAccWords; cell-major, 64
// bytes per cell, so one sample's adds land in one 64-byte request):
//   words 0..2  wq Jq_c     words 3..5  wq rgb_c (the raw uint8 colours)     word 6  wq     word 7  1, the sample count
// with no-return, agent-scope, relaxed 64-bit atomic adds.  THE BOUND: with fewer than 2^20 samples in a cell every sum stays below
// 2^20 x 2^12 x 2^30 = 2^62.  The count has a word of its own, so a cell that reaches 2^20 samples shows in word 7 whatever has
// become of the other words; the caller checks the largest count after the normalise pass (engine.Mosaic.normalize).
// Unless SUCRE_MOSAIC_PLAIN_ATOMIC is given, the lanes of a wave -- consecutive pixels of a row -- first sum over every run of
// adjacent lanes with one cell (a segmented suffix sum by shuffles: 11 words, 6 steps) and the run's first lane issues the eight
// atomics for the run; integer sums, so the words end up the same to the bit.
// The normalise pass, one lane per cell, no atomics, reads no image; for a cell with word 7 > 0:
//   J_blend_c = (float)(((double)acc_c / (double)wsum) 2^-20)     raw_blend_c = (uint8)((2 racc_c + wsum) / (2 wsum))
//   weight = (float)((double)wsum 2^-12)                            samples = count (2^31 - 1 when above)
// (int64 -> double: the compiler's conversion, correctly rounded, as numpy's astype is; IEEE double division.)  Empty cells are
// not touched.  As H -> 0 the blend tends to the best-view mosaic quantised to 2^-20, as H -> infinity to the plain mean.
// Measured on the shape above (profiles/mosaic_blend_time.txt; H = 0.5 m, 119 M samples): accumulate 23.8 ms with the run sums,
// 47.7 ms with the plain atomics (7.5 against 58.2 ms at 1176 pixels per cell), against the splat's 0.87 ms in the same run -- a
// sum can skip none of its atomics --; normalise 0.04 ms.
//
// The feather (sucre_mosaic_feather, sucre_mosaic_accumulate_feathered): one more factor in the blend's weight, which falls to
// nothing towards the edge of an image's footprint -- the frame of the image, a NaN patch of J, a hole of the depth map -- so that
// the blended colour no longer steps where a view ends.  A pixel is a MEMBER of its image when it takes part (mosaic_member, the
// rule of mosaic_pixel: one function).  For a member (u, v) of an H x W image and a feather width of F source pixels, 1 <= F <= 1024:
//   D2    = min over integer (u', v') that are non-members OR lie outside [0,W) x [0,H) of (u - u')^2 + (v - v')^2
//   dist2 = min(D2, F^2)                           uint32; 0 for a non-member; >= 1 for a member (the frame just outside counts)
// in exact integers, separably; integer min is order-free, so any schedule gives the same bits:
//   columns  g(u,v) = min(F, distance along column u to the nearest non-member), rows -1 and H counting as non-members; uint16,
//            0 for a non-member.  One lane per column walks down (reads depth and J, writes the distance to the one above) and
//            then up (reads and lowers g alone); a wave's lanes touch consecutive addresses.  One launch per 32 images
//   rows     dist2(u,v) = min(F^2, min over |dx| < F of dx^2 + g(u+dx, v)^2), a column outside the image having g = 0.  One lane
//            per pixel, a workgroup per 256-column segment of a row; the segment and F - 1 columns of halo on each side are
//            staged in LDS (256 + 2 x 1023 uint16 at most); each lane scans dx outwards and stops once dx^2 >= its best so far
// The capped form is exact: a nearest non-member with |dx| < F and |dy| < F is found, any other one has D2 >= F^2.
// THE BUFFER of one call (feather_bytes): image i's dist2 words, row-major H x W, start at word 256 sum_(j<i) ceil(H_j W_j / 256)
// -- so the lane of mosaic_walk reads word blockIdx.x 256 + threadIdx.x behind its launch's first word: one coalesced load, no
// pointer per image --; the uint16 g scratch sits behind all the words, image i's at the same index.  6 bytes per (padded) pixel.
// The weight, float32, one IEEE operation per step (inv_F = float32(1) / float32(F), formed on the host):
//   f  = dist2 >= F^2 ? 1.0f : sqrtf((float)dist2) inv_F
//   wq = (int)rintf(((t t) f) 4096)                t as in the blend; 0 <= wq <= 4096
// and everything after wq is the blend's: the Jq clamp, the eight words, the run sums, the 2^62 bound, the normalise pass.
// EVERY FILLED CELL STILL HAS A BLEND: its winner has t = 1 and f >= 1 / F >= 1 / 1024, so wq >= 4, wsum > 0 and samples >= 1 --
// which is why F stops at 1024 (a filled cell has wsum >= 4 here, not >= 4096).  F = 1 IS THE UNFEATHERED BLEND TO THE BIT: every
// member has dist2 >= 1 = F^2, so f = 1 and (t t) 1.0f is t t.
// Measured on the shape above in one run (tools/mosaic_feather_time.py, profiles/mosaic_feather_time.txt): the map 2.6 ms at F = 16
// and 64, 3.1 ms at F = 1024, 2.2 ms of it the column pass (the floor at F = 1: one wave per 64 columns walks 1080 rows); the
// feathered accumulate 23.8, 23.5 and 21.9 ms against 23.8 ms unfeathered.  Not built: the row pass's workgroup shortcut (a window
// that holds only g = F writes F^2 at once).
#pragma once
#include "launch.h"

namespace sucre {

constexpr int kMosaicSet = 16;          // table entries per set launch (by value: 16 x 128 bytes of kernel arguments)
constexpr int kMosaicLaunch = 32;       // images per phase launch (the bisection: 5 steps)
constexpr uint32_t kMosaicBlockPx = 256;   // one lane per pixel

struct MosaicImage {   // sucre_mosaic_image_t with its reserved words put to use
    const float *depth;
    const uint8_t *rgb;
    const float *J;
    int32_t H, W;
    float Kinv[9], R[9], t[3];
    uint32_t block0;    // the image's first workgroup in ITS launch's grid
    int32_t ordinal;
    int32_t pad;
};
static_assert(sizeof(MosaicImage) == sizeof(sucre_mosaic_image_t) && sizeof(MosaicImage) == 128, "the device table entry is the public struct");

struct MosaicGrid {   // sucre_mosaic_grid_t
    float axes[9];
    float gsd, lo_s, lo_t;
    int32_t Hm, Wm;
};
static_assert(sizeof(MosaicGrid) == sizeof(sucre_mosaic_grid_t), "the grid is the public struct");

struct MosaicOut {   // the five outputs of sucre_mosaic_gather
    float *J;
    uint8_t *raw;
    int32_t *source, *pixel;
    float *range;
};

struct MosaicBlend {   // the four outputs of sucre_mosaic_normalize
    float *J;
    uint8_t *raw;
    float *weight;
    int32_t *samples;
};

constexpr int kMosaicAccWords = 8;      // int64 words per cell of the blend's accumulator (SUCRE_MOSAIC_ACC_WORDS)
static_assert(kMosaicAccWords == SUCRE_MOSAIC_ACC_WORDS, "the accumulator's layout is public");

enum MosaicPhase { kMosaicBounds, kMosaicSplat, kMosaicSplatPlain, kMosaicResolve, kMosaicGather };

inline size_t mosaic_table_bytes(int n_images) { return align_up((size_t)n_images * sizeof(MosaicImage), 256); }
inline uint64_t mosaic_blocks(int H, int W) { return ((uint64_t)H * (uint64_t)W + kMosaicBlockPx - 1) / kMosaicBlockPx; }

constexpr int kFeatherMax = 1024;       // the widest feather (SUCRE_MOSAIC_FEATHER_MAX): the winner's wq stays >= 4
static_assert(kFeatherMax == SUCRE_MOSAIC_FEATHER_MAX, "the widest feather is public");

struct MosaicFeather {   // what a feathered accumulate launch reads (all zeros for an unfeathered one, which reads none of it)
    const uint32_t *dist2;   // the first word of the launch's first image
    uint32_t f2;             // F^2
    float inv_f;             // 1 / F
};

// The words of the map of images[0 .. n), every image rounded up to whole workgroups; the g scratch holds as many uint16.
inline size_t feather_words(int n_images, const sucre_mosaic_image_t *images) {
    size_t words = 0;
    for (int i = 0; i < n_images; ++i) words += (size_t)mosaic_blocks(images[i].H, images[i].W) * kMosaicBlockPx;
    return words;
}
inline size_t feather_bytes(int n_images, const sucre_mosaic_image_t *images) { return feather_words(n_images, images) * 6; }

// One phase over images[0 .. n): ceil(n / 32) launches (plus the table's set launches) on s.  Only the arguments of the phase
// are read: bounds (kMosaicBounds), key (splat: written; resolve, gather: read), pix (resolve: written; gather: read), out (gather).
hipError_t launch_mosaic(MosaicPhase phase, void *table, int n_images, const sucre_mosaic_image_t *images, int first_ordinal,
                         const MosaicGrid &grid, uint32_t *bounds, unsigned long long *key, uint32_t *pix, const MosaicOut &out,
                         hipStream_t s);

// The feather's map of images[0 .. n) into `feather` (feather_bytes; two launches per 32 images, plus the table's).
hipError_t launch_mosaic_feather(void *table, int n_images, const sucre_mosaic_image_t *images, int feather_px, void *feather,
                                 hipStream_t s);

// The blend's accumulate phase over images[0 .. n) (the same launches as a phase above; key: read, acc: added to) and its
// per-cell pass (one launch).  `feather`: NULL, or what a feathered phase reads -- dist2 the map as launch_mosaic_feather left it
// for the same call's images in the same order, made with this F or a larger one (bands.h blends every band from one map).
hipError_t launch_mosaic_accumulate(bool plain, void *table, int n_images, const sucre_mosaic_image_t *images, int first_ordinal,
                                    const MosaicGrid &grid, const unsigned long long *key, float inv_h, const MosaicFeather *feather,
                                    unsigned long long *acc, hipStream_t s);
hipError_t launch_mosaic_normalize(const MosaicGrid &grid, const long long *acc, const MosaicBlend &out, hipStream_t s);

// ---- what every translation unit that walks images shares (mosaic.hip, bands.hip): one copy of each ----

// Whether a pixel takes part, from its depth and its three restored channels: the one statement of the rule (the feather's column
// pass and the band split form their members with it too).
__device__ __forceinline__ bool mosaic_member(float d, float J0, float J1, float J2) {
    return d > 0.0f && J0 == J0 && J1 == J1 && J2 == J2;
}

// The image of this workgroup: the last one whose first workgroup is not behind blockIdx.x (wave-uniform: scalar loads).
__device__ __forceinline__ const MosaicImage *mosaic_block_image(const MosaicImage *__restrict__ table, int n_images) {
    int lo = 0, hi = n_images - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].block0 <= blockIdx.x) lo = mid;
        else hi = mid - 1;
    }
    return table + lo;
}

// The same for a kernel whose workgroups each walk several of the grid's 256-pixel blocks: the image of `block`.  A second copy on
// purpose: handing blockIdx.x to this form moves the loop's entry branches in every existing kernel, and their code stays as it is.
__device__ __forceinline__ const MosaicImage *mosaic_block_image_at(const MosaicImage *__restrict__ table, int n_images, uint32_t block) {
    int lo = 0, hi = n_images - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].block0 <= block) lo = mid;
        else hi = mid - 1;
    }
    return table + lo;
}

// A blended colour from its fixed-point sum and weight sum: the quotient of the normalise pass and of the band combine.
__device__ __forceinline__ float mosaic_quotient(long long acc, long long wsum) {
    return (float)(((double)acc / (double)wsum) * 0x1p-20);
}

// The table entries of images[l0 .. l0 + nl), one launch's, written to entries[l0 ..) by set launches on s (by value: nothing is
// copied from the host); returns the workgroups of that launch (the caller has checked that every launch's grid fits).
uint32_t mosaic_set_launch(MosaicImage *entries, int l0, int nl, const sucre_mosaic_image_t *images, int first_ordinal, hipStream_t s);

// The launches of one phase over images[0 .. n): per 32 images, the table's set launches, then launch(workgroups, table, images).
template <typename Launch>
static void mosaic_for_each_launch(void *table, int n_images, const sucre_mosaic_image_t *images, int first_ordinal, hipStream_t s,
                                   Launch launch) {
    auto *entries = static_cast<MosaicImage *>(table);
    for (int l0 = 0; l0 < n_images; l0 += kMosaicLaunch) {
        const int nl = n_images - l0 < kMosaicLaunch ? n_images - l0 : kMosaicLaunch;
        launch(mosaic_set_launch(entries, l0, nl, images, first_ordinal, s), entries + l0, nl);
    }
}

}  // namespace sucre

// Colour consensus across views of the seabed mosaic (sucre_mosaic_reject_claim, sucre_mosaic_reject_sums,
// sucre_mosaic_reject_consensus, sucre_mosaic_reject_cull): the samples whose COLOUR is not what the other images saw at that spot,
// taken out ahead of the splat.  surface.h and support.h test a sample's height along the view axis, gains_mosaic.h finds one
// scalar per image; a fish, a fin, a caustic band or a particle cloud is not in the rendered depth maps at all -- such a sample
// carries the seabed's height and its own colour, wins best-view cells, enters the blend with a weight near 1 and biases the gain
// sums.  The remedy has the shape support.h uses for heights: robustness by views, not by samples.
//
// A SAMPLE is a pixel that takes part and has a cell (mosaic_member / mosaic_pixel / mosaic_cell, the walk of mosaic_walk.h: one lane
// per pixel, 32 images per launch, ordinal = first_ordinal + index).  The J seen is the surface-culled copy when there is a surface
// test, never the gained one: the rejection runs before the splat and before the gains.  Everything is integer state, or one IEEE
// operation per step in the stated format: the same bits in any order of arrival, any batch split and either atomic form.
//
// claim      over ALL images.  Per cell kRejectSlots = 8 words, slot_ord (cells, 8) uint32, all ones when free, and slot_over
//            (cells) uint32, a 0 / 1 flag.  After the pass a cell's words hold the 8 smallest distinct ordinals that reach it,
//            ascending, free words last, and slot_over[cell] = 1 exactly when a ninth distinct ordinal reaches it.  A lane carries
//            v = its ordinal from slot 0 upward and calls old = atomicMin(&slot[s], v):
//              old == v   stop (the value is there)
//              old >  v   the slot now holds v; stop when old was free, else carry v = old on to slot s + 1
//              old <  v   go on to slot s + 1 with the same v
//            and a value carried past slot 7 sets the flag.
//            THE PROOF that the end state is the sorted prefix whatever the schedule.  (a) Words only fall: atomicMin is the only
//            write.  (b) Slot s + 1 is written only by a lane that has just seen slot s hold less than what it writes -- it passed
//            slot s (old < v) or left its v there and carries the larger old -- and by (a) slot s stays below that value for good:
//            at EVERY moment slot s < slot s + 1 unless slot s + 1 is free.  So the words of a cell are strictly ascending at all
//            times, free words (the largest value) last, and no ordinal stands in two words.  (c) A value is never lost: each step
//            leaves the set {words} + {values lanes carry} unchanged except where it drops a copy of a value that a word holds at
//            that moment (old == v) -- if that word is displaced later its value goes on in the displacing lane's register -- and
//            where it drops a value past slot 7.  (d) A value dropped past slot 7 has seen, at each of the eight slots, a smaller
//            value stand there; by (a) all eight final words are smaller than it.  When every lane has stopped nothing is carried,
//            so by (c) the final words are the distinct ordinals that reached the cell less the dropped ones, by (d) every dropped
//            one exceeds all of them, by (b) they are ascending: the 8 smallest, and fewer than 8 only when nothing was dropped.
//            The flag is set exactly when a value was dropped: exactly when more than 8 distinct ordinals reach the cell.
//            THE DEFAULT FORM puts a plain load of the cell's 32 bytes ahead of the chain.  Every loaded word is a value the word
//            held at some moment, so by (a) it is not below the word's current value, whenever each of the eight was read.  Own
//            ordinal among them: it has been inserted (c keeps it), the lane does nothing.  All eight smaller than the own: the
//            current eight are smaller too and by (b) distinct, eight other ordinals below this one reach the cell, so this is a
//            ninth: the flag, set behind a plain test of it, and no atomic on the words.  Otherwise the lane enters the chain at
//            the first loaded word larger than its own: the words before it are below the own ordinal now as then, and the chain
//            from slot 0 would pass each of them.  The proof above holds for a chain entered there.  Only the first lane of a run
//            of adjacent lanes that share a cell acts: a workgroup has one image, so the run's lanes carry one value.
//            SUCRE_MOSAIC_PLAIN_ATOMIC: every sample walks the whole chain from slot 0, no load, no run.
// sums       over ALL images, once the claim has seen every image (the words are final: plain loads).  A sample whose ordinal is
//            one of its cell's eight adds 1 and Xq_c = gain_quantise(J_c) (gains_mosaic.h: 2^-14, clamp +-8) to that slot's four
//            int64 words of slot_sum (cells, 8, 4): n, sum Xq x 3; a sample of any other image adds nothing.  run_sum over runs of
//            adjacent lanes that share a cell (mosaic_walk.h), as the direct gain solve's slots; SUCRE_MOSAIC_PLAIN_ATOMIC: every
//            sample for itself.  |Xq| <= 2^17: a cell's words stay below 2^17 n.
// consensus  one pass over the cells, no image is read.  k = the occupied slots (a prefix).  k < kRejectMinViews = 3: source -1,
//            ref NaN, views k -- two images cannot say which of them is wrong.  Otherwise the slots are ordered by mean brightness,
//            exactly, in integers: Y_a = S_a,0 + S_a,1 + S_a,2; a comes before b when Y_a n_b < Y_b n_a, or on equality when
//            ord_a < ord_b.  The reference is the slot at index (k - 1) / 2 of that order, the lower median: source = its ordinal,
//            views = k, ref_c = (float)(((double)S_c / (double)n) 2^-14) -- one divide, one exact scaling, one rounding.  One scalar
//            ranks the images and all three channels come from that ONE image, so its own samples have a reference they define.
//            THE BOUND: |Y_a| <= 3 2^17 n_a, so |Y_a n_b| <= 3 2^17 n_a n_b < 2^59 while every n < 2^20.  The kernel counts the
//            slots with n >= 2^20 (`big`, one 64-bit word) and leaves their cells without a reference; the caller stops the run on a
//            count above 0 (engine.Mosaic.finish_reject names the count and --mosaic-gsd, the blend's rule).
// cull       surface.h's cull with another test: J_out is a copy of the images' J in the band buffers' layout (bands.h).  A pixel
//            gets the NaN 0x7fc00000 in every channel when it does not take part, or when its cell has a reference, its ordinal is
//            not source[cell], and fabsf(J_c - ref_c) > T in any channel: one float32 subtraction and one comparison, T = float32(T)
//            formed on the host, T > 0.  rejected (uint32 per cell, or NULL): a rejected sample adds 1 to its cell.  counts (rows
//            of kGainRowWords int64 words per ordinal, two used; or NULL): samples in cells that have a reference, samples
//            rejected -- the counting form of surface.h with gains_mosaic.h's flush: a workgroup walks 32 consecutive 256-pixel
//            blocks, sums in registers and adds when the image changes and at the end.
// CONSEQUENCES.  The reference image's samples never go, and a cell without a reference rejects nothing: every cell keeps a sample,
// so the filled cells, the bounds and the grid are those of a run without the test.  A T that rejects nothing leaves every output of
// the later phases bit for bit (the copy IS J at the members).  An image outside an overflowed cell's eight does not vote but is
// tested like any other.  T must exceed the offsets the gain compensation will remove afterwards: there is no second rejection.
//
// Memory: 32 + 256 + 4 = 292 bytes per cell for slot_ord, slot_sum and slot_over, freed after the consensus; 24 bytes per cell stay
// (ref 12, source 4, views 4, rejected 4) and the caller's copy of the flags (engine.Mosaic: one byte); 12 bytes per padded pixel
// of the largest batch for the copy.
// Resources (gfx950, the build's reject.rpt): claim 14 VGPRs (9 plain), sums 22 (16 plain), cull 12 (33 and 64 bytes of LDS with
// its counts): 8 waves per SIMD; consensus 151 VGPRs, 3 waves per SIMD (eight slots' counts, sums and 56 pairs of 64-bit products
// in registers; one lane per cell, once per mosaic).  No LDS otherwise, no scratch.
// Measured on one MI355X, 65 resident images of 1080p, 1.81 M reached cells, 1.59 M of them reached by 3 images or more and 1.18 M
// by more than 8, 6.6 of a reached cell's 8 slots held on average, in ONE run (tools/mosaic_reject_time.py,
// profiles/mosaic_reject_time.txt), next to the splat's 0.86 ms, sucre_mosaic_gain_span's 2.45 ms, sucre_mosaic_gain_slots' 5.28 ms
// and sucre_mosaic_cull's 0.81 ms in the same run.  The claim 1.00 ms behind its load with one lane per run, 0.74 ms over words that
// are final already, 31.0 ms with every sample walking the whole chain (31 x: eight returning atomics per pixel on words that 74
// pixels of 65 images share).  The expectation was the span's time: REFUTED, 0.41 x -- faster: the span's max word rises with every
// image, so its filter passes an atomic per (image, cell) at least, while here one lane per run loads the cell and, from the ninth
// image of a cell on, finds eight smaller words and issues no atomic on them.  The sums 4.34 ms with the run sums, 8.20 ms with every sample
// for itself; expected near gain_slots: HELD, 0.82 x (the same four adds per run; no claim, a final slot found by one load).  The
// consensus 0.14 ms.  The cull 1.04 ms, 1.39 ms with its counts; expected near sucre_mosaic_cull: HELD, 1.28 x (12 more bytes per
// sample: the cell's source and reference, 16, against the top's 4).  At T = 0.05 on images whose factors span 0.9 .. 1.1, 27 % of the tested samples go.
// The whole phase adds about 6.5 ms once, and the cull about 1 ms to every later phase and batch.  ("near": within a factor of
// 1.5 either way, fixed in the tool before the run.)
// Not built: a second rejection after the gains; the direct gain solve on these deterministic slots (gains_direct.h keeps its
// claim by arrival); a per-channel median (three references per cell would mix images); multi-rank mosaics -- slot_ord (min-merge
// of the sorted words), slot_sum (sum) and rejected (sum) are the tensors an all-reduce would combine.
#pragma once
#include "gains_mosaic.h"

namespace sucre {

constexpr int kRejectSlots = 8;           // words per cell (SUCRE_MOSAIC_REJECT_SLOTS)
static_assert(kRejectSlots == SUCRE_MOSAIC_REJECT_SLOTS, "the slots' layout is public");
constexpr int kRejectMinViews = 3;        // images a consensus takes (SUCRE_MOSAIC_REJECT_MIN_VIEWS)
static_assert(kRejectMinViews == SUCRE_MOSAIC_REJECT_MIN_VIEWS, "the consensus' rule is public");
constexpr int kRejectSlotWords = 4;       // int64 words per slot: n, sum Xq x 3
constexpr int kRejectCountWords = 2;      // int64 words per image of the cull's counts (row: kGainRowWords)
constexpr uint32_t kRejectSlotFree = 0xffffffffu;
constexpr long long kRejectMaxSamples = 1ll << 20;   // of one image in one cell: the consensus' products stay below 2^59

struct MosaicReject {   // what a reject cull launch writes besides J_out
    uint32_t *rejected;             // per cell, or NULL
    unsigned long long *counts;     // per ordinal a row of kGainRowWords: samples in cells with a reference, samples rejected; or NULL
};

// The claim over images[0 .. n): the launches of a phase of mosaic.h; slot_ord: lowered; slot_over: set.
hipError_t launch_mosaic_reject_claim(bool plain, void *table, int n_images, const sucre_mosaic_image_t *images, int first_ordinal,
                                      const MosaicGrid &grid, uint32_t *slot_ord, uint32_t *slot_over, hipStream_t s);

// The sums over images[0 .. n); slot_ord: read (final); slot_sum: added to.
hipError_t launch_mosaic_reject_sums(bool plain, void *table, int n_images, const sucre_mosaic_image_t *images, int first_ordinal,
                                     const MosaicGrid &grid, const uint32_t *slot_ord, unsigned long long *slot_sum, hipStream_t s);

// The consensus over the grid's cells (one launch); ref (cells, 3), source, views: written; big: added to.
hipError_t launch_mosaic_reject_consensus(const MosaicGrid &grid, const uint32_t *slot_ord, const long long *slot_sum, float *ref,
                                          int32_t *source, int32_t *views, unsigned long long *big, hipStream_t s);

// The cull over images[0 .. n) into J_out (band_bytes of bands.h for the same images); ref, source: read.
hipError_t launch_mosaic_reject_cull(void *table, int n_images, const sucre_mosaic_image_t *images, int first_ordinal,
                                     const MosaicGrid &grid, const float *ref, const int32_t *source, float tol, float *J_out,
                                     const MosaicReject &out, hipStream_t s);

}  // namespace sucre

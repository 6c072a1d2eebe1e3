// The direct solve of the mosaic's gain compensation (sucre_mosaic_gain_slots, sucre_mosaic_gain_pairs, sucre_mosaic_gain_diag): the
// rounds of gains_mosaic.h are a Jacobi-style relaxation of  E = sum over shared cells, over their samples, of (g_i X - m_cell)^2,
// and a slow drift along a chain of N images -- a lawn-mower transect with a drifting strobe -- takes them on the order of N^2
// rounds.  This is the same objective solved exactly, once.  Eliminating m (the cell's mean of g X) leaves, per channel, a quadratic
// form  E = g^T A g  with
//   A_ii = Q_i - P_ii      A_ij = -P_ij      P_ij = sum over cells k of S_ik S_jk / N_k      Q_i = sum X^2
// where S_ik is the sum of image i's quantised colours X = gain_quantise(J) (gains_mosaic.h: the one clamp / quantise helper) in
// cell k and N_k the cell's sample count.  The device forms P and Q as integers; the host solves (engine.mosaic_gain_solve_direct,
// float64: (A + mu diag Q) g = mu Q, the Brown-Lowe prior (g - 1)^2 scaled to the data term, then the gauge and the clamp of the
// rounds' solve).  The direct solve replaces the FIRST round's solve; the remaining rounds and the measuring pass run unchanged.
//
// Every kernel sees the images' J as the gain kernels see them (the culled copy when there is a surface test; never the gained one)
// and walks as mosaic.h's phases do (mosaic_walk.h, mosaic_member / mosaic_pixel / mosaic_cell, 32 images per launch).  All state
// is integer and order-free: any order of arrival, any batch split and either atomic form give the same bits -- with ONE proviso,
// which nothing downstream can see: WHICH slot of a cell an image holds depends on arrival (a reader sorts a cell's slots by ordinal).
//
// slots  after the span, over ALL images.  Per cell kGainSlots = 8 slots (SUCRE_MOSAIC_GAIN_SLOTS): slot_ord (cells, 8) uint32, all
//        ones when free; slot_sum (cells, 8, 4) int64: n, sum Xq x 3; slot_over (cells) uint32, a 0 / 1 flag.  Only a sample whose
//        cell is shared (span lo < hi) takes part.  It scans the cell's slots from the first: a slot that holds its ordinal is its
//        own (a claimed slot never changes, so a plain load that finds the own ordinal needs no atomic); a free one it claims with
//        atomicCAS (and takes also when the CAS finds that another lane of the same image has just claimed it); a slot held by
//        another image it passes, for good.  So an ordinal holds at most one slot, the occupied slots are a prefix, and a sample
//        that passes all eight sets slot_over[cell] = 1: the cell OVERFLOWS exactly when more than eight different ordinals reach
//        it, whatever the order.  A flag and not a count: a count would depend on which images came first.  Which images hold the
//        slots of an overflowed cell depends on arrival too, and NOTHING may read them.  The sample then adds 1 and Xq_c to its
//        slot.  Unless SUCRE_MOSAIC_PLAIN_ATOMIC, the lanes of a wave first sum over runs of adjacent lanes with one cell (a
//        workgroup has one image): the accumulate's segmented suffix sum (run_sum, mosaic_walk.h), on 4 words instead of 11, and
//        one lane per run finds the slot and adds.
// pairs  one pass over the cells, no image is read.  For a cell that is shared and not overflowed: N = sum n_a over the occupied
//        slots, and for every pair of occupied slots a <= b (a = b too), with i = min(ord), j = max(ord), per channel
//          pairs[i][j][c] += llrint(((double)S_a,c (double)S_b,c) / (double)N)      pairs[i][j][3] += 1
//        ONE IEEE multiply, one divide, one round to nearest even; no contraction is possible (the build has -ffp-contract=off, and
//        a product feeding a quotient has no fused form); the conversions are exact, |S| < 2^37.  pairs is (n, n, 4) int64, zeroed
//        by the caller; only the upper triangle is written.
//        THE BOUND: |S_a| <= 2^17 n_a, so |S_a S_b / N| <= 2^34 n_a n_b / N <= 2^34 min(n_a, n_b); summed over the cells of a pair
//        that is at most 2^34 times the samples of the smaller image, 2^26 (gains_mosaic.h refuses a larger image before any
//        launch; it stands), plus half a unit of rounding per cell: no word passes 2^60 + 2^26.
//        Every cell in the overlap of images i and j adds to the same words; global atomics per cell would meet on one cache line
//        (the finding of the bounds phase and of the sums: 12 x and 2.5 x there).  So a workgroup walks a tile of
//        kPairTileCells consecutive cells and keeps its pair sums in an LDS open-addressing table: key i << 12 | j (ordinals stay
//        below 4096), four int64 words per entry, ds 64-bit atomic adds, linear probing from a multiplicative hash; a lane that
//        finds neither its key nor a free entry within 32 probes (or the whole table) adds to global memory directly -- the same
//        integer add.
//        When the walk ends, one set of global atomics per occupied entry.  `table_entries`: the table's size, a power of two up
//        to kPairTableMax = 512 (18 KB of LDS), 0 for that; the tests force the overflow path with 1 and 2.
//        SUCRE_MOSAIC_PLAIN_ATOMIC: global atomics per cell and pair, for the tests and the timing.
// diag   per image four int64 words in a 128-byte row (kGainRowWords, as the sums): n_i and sum Xq^2 x 3 over the image's samples
//        in cells that are shared and not overflowed.  The counting form of sucre_mosaic_gain_sums and its flush (gain_flush,
//        gains_mosaic.h): registers across 32 blocks, then wave, then LDS, then four atomics; SUCRE_MOSAIC_PLAIN_ATOMIC: one set
//        per 256 pixels.  Xq^2 <= 2^34 and 2^26 pixels: no word passes 2^60.
//
// Memory: 32 + 256 + 4 = 292 bytes per cell for the slots, 32 n^2 bytes for the pairs, 128 n for the diag; allocated only when the
// direct solve is asked for (engine.Mosaic refuses a request beyond 0.8 of the free device memory before it allocates).
// Resources (gfx950, the build's gains_direct.rpt): slots 16 VGPRs (12 plain), pairs 56 and 18432 bytes of LDS (58 and none plain),
// diag 39 and 128 bytes of LDS; 8 waves per SIMD, no scratch.
// Measured on one MI355X, 65 resident images of 1080p, 1.69 M shared cells, in ONE run (tools/mosaic_gain_direct_time.py,
// profiles/mosaic_gain_direct_time.txt), next to the splat's 0.87 ms, the blend's accumulate at H = 0.5 m, 23.8 ms, and a whole round
// of the relaxation, 28.9 ms.  The slots 5.30 ms with the run sums, 9.51 ms with every sample for itself; the expectation was about
// half an accumulate (they write four words per sample where it writes eight): HELD, 0.22 x.  The pairs 0.34 ms with the table,
// 14.3 ms with global atomics per cell and pair: 42 x, the cache-line finding once more.  The diag 0.81 ms in the counting form,
// 1.29 ms with one set per 256 pixels.  The host solve of three 65 x 65 systems 0.28 ms (host clock).  The whole direct phase, resets,
// copies to the host and solve included, 6.95 ms; the expectation was below one round: HELD, 0.24 x.
// NOT expected: that survey is dense (13 x 5 cameras; 7.0 of a shared cell's 8 slots are held on average) and 1.18 M of its 1.69 M
// shared cells hold more than 8 images and are left out -- the pairs' time above is that of the remaining 0.5 M cells --, so the solve sees only
// the thinner edges of the overlap: one direct solve takes the RMS disagreement from 0.034 / 0.031 / 0.031 to 0.020 / 0.013 / 0.013
// where three rounds reach 0.015 / 0.0041 / 0.0035.  Without a drift, on dense overlap, the rounds are the better tool; the flow
// runs the remaining R - 1 rounds after the direct solve for that reason.  On the crafted chain of 12 views (tests/
// mosaic_gain_direct_crafted.py) the spread of gain x factor falls from 0.710 to 1.3e-4 in the one solve; 8 rounds leave 0.468.
// Not built: more than eight slots per cell, or a sampled subset of an overflowed cell's images; the solve on the device.
#pragma once
#include "gains_mosaic.h"

namespace sucre {

constexpr int kGainSlots = 8;             // slots per cell (SUCRE_MOSAIC_GAIN_SLOTS)
static_assert(kGainSlots == SUCRE_MOSAIC_GAIN_SLOTS, "the slots' layout is public");
constexpr int kGainSlotWords = 4;         // int64 words per slot: n, sum Xq x 3
constexpr int kGainPairWords = 4;         // int64 words per pair: P x 3, the cells the pair shares
constexpr int kGainDiagWords = 4;         // int64 words per image of the diag: n, sum Xq Xq x 3 (row: kGainRowWords)
constexpr uint32_t kGainSlotFree = 0xffffffffu;
constexpr int kPairTableMax = 512;        // entries of the pairs' LDS table: 512 x (4 + 32) bytes = 18 KB
constexpr uint32_t kPairTileCells = 4096; // consecutive cells a workgroup of the pairs walks: 16 per lane

// The slots over images[0 .. n): the launches of a phase of mosaic.h; span: read; slot_ord, slot_sum, slot_over: claimed / added to / set.
hipError_t launch_mosaic_gain_slots(bool plain, void *table, int n_images, const sucre_mosaic_image_t *images, int first_ordinal,
                                    const MosaicGrid &grid, const uint32_t *span, uint32_t *slot_ord, unsigned long long *slot_sum,
                                    uint32_t *slot_over, hipStream_t s);

// The pairs over the grid's cells (one launch); pairs: (n_ordinals, n_ordinals, 4), added to.  table_entries: a power of two in
// 1 .. kPairTableMax.
hipError_t launch_mosaic_gain_pairs(bool plain, const MosaicGrid &grid, const uint32_t *span, const uint32_t *slot_ord,
                                    const long long *slot_sum, const uint32_t *slot_over, int n_ordinals, unsigned long long *pairs,
                                    int table_entries, hipStream_t s);

// The diag over images[0 .. n); span, slot_over: read; diag: rows of kGainRowWords words, added to.
hipError_t launch_mosaic_gain_diag(bool plain, void *table, int n_images, const sucre_mosaic_image_t *images, int first_ordinal,
                                   const MosaicGrid &grid, const uint32_t *span, const uint32_t *slot_over, unsigned long long *diag,
                                   hipStream_t s);

}  // namespace sucre

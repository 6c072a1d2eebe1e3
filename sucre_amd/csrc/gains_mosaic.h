// Per-image gain compensation of the seabed mosaic (sucre_mosaic_gain_span, sucre_mosaic_gain_apply, sucre_mosaic_gain_sums): one
// gain per image and channel, found from the cells that two or more images share, applied to every image's J ahead of resolve,
// gather, accumulate and the bands.  The phases of mosaic.h decide WHICH samples enter a cell and with what weight; none of them
// asks whether two images agree on the colour of the same seabed.  Images restored with a water model each carry a residual cast
// each, the best view shows the offsets as seams, and the blend hides them only with a depth so wide that it averages the far
// views' noise into every cell.  Removing the offset at its source makes every later stage's job smaller.
//
// THE MODEL.  Over the gains g (per image i and channel) and the cell means m, minimise
//   E = sum over shared cells, over their samples s, of (g_i(s) J_s - m_cell)^2
// by exact block-coordinate descent: with g fixed m is the plain mean of g J over the cell; with m fixed g_i = sum(J m) / sum(J J)
// over the image's samples in shared cells.  One ROUND is one such pair; the host solves (engine.mosaic_gain_solve, float64) and
// fixes the gauge -- the overlap-weighted mean gain is 1 -- and the limit, 1/L <= g <= L.  The rounds are a Jacobi-style
// relaxation: what overlapping images disagree on (the seams) goes in a few rounds; a slow drift along a chain of N images takes
// on the order of N^2 rounds and is not what this is for: gains_direct.h solves the same objective exactly, once, for that.
//
// Every kernel takes the image's J as the phases after the surface test see it (the culled copy when there is one), walks as
// mosaic.h's phases do (mosaic_walk.h: one lane per pixel, 32 images per launch, ordinal = first_ordinal + index) and forms a
// pixel's membership and cell with mosaic_member / mosaic_pixel / mosaic_cell: one copy of each.  Integer sums and integer minima
// only, so the same bits in any order of arrival, any batch split and either atomic form.
//
// span   once, after the splat: per cell two uint32 words, span[2 cell] = min and span[2 cell + 1] = max of the ordinals of the
//        samples that take part and have a cell (empty: all ones, 0).  atomicMin / atomicMax, each behind a load that filters it
//        (the splat's way: a stale value is only less extreme than the current one); SUCRE_MOSAIC_PLAIN_ATOMIC: both atomics for
//        every sample.  A cell is SHARED when lo < hi: two different ordinals reach it (a view listed twice has two).
// A PASS at gains G ((n, 3) float32 on the device, row = ordinal; all 1.0f before round 1):
// apply  one lane per pixel, J'_c = J_c G[ordinal][c]: ONE float32 multiply, a NaN stays a NaN.  J_out has the band buffers'
//        layout (bands.h, band_bytes: image i's block starts at PIXEL 256 sum_(j<i) ceil(H_j W_j / 256)), like the cull's.  The
//        image's row of G is wave-uniform (scalar loads).  A lane reads and writes its own pixel alone, so an image's J may BE its
//        block of J_out (the culled copy gained in place); any other overlap is refused.
// refer- the blend's own accumulate (mosaic.h), unchanged, over the J' images into a zeroed accumulator of its eight words per
// ence   cell, with inv_h = 0x1p-126f: d inv_h < 2^-25 for every range below 2^101 m, so t = 1 and wq = 4096 for every sample --
//        the plain per-sample mean.  m_c = mosaic_quotient(acc_c, acc_6), the blend's quotient.  Word 7 counts the samples; the
//        caller refuses a cell with 2^20 or more (the blend's bound).
// sums   over the ORIGINAL (un-gained) J.  For a sample that takes part, has a cell and whose cell is shared, in float32 with one
//        IEEE operation per step (gain_quantise: the one clamp / quantise helper):
//          Xq_c = (int64)rintf(fminf(fmaxf(J_c, -8), 8) 16384)      Mq_c the same of m_c      Yq_c the same of J_c G[i][c]
//          Rq_c = Yq_c - Mq_c
//        and the sample adds into its image's ten int64 words (kGainWords; the row of ordinal i at word 16 i: rows are padded to 128
//        bytes so that two images' atomics never meet on one cache line):
//          word 0  1      words 1..3  Xq_c Mq_c      words 4..6  Xq_c Xq_c      words 7..9  Rq_c Rq_c
//        THE BOUND: |Xq|, |Mq| <= 2^17 and |Rq| <= 2^18 (an infinity is clamped too), so with H W <= 2^26 pixels in an image no word
//        passes 2^62; a larger image is refused before any launch.
//        A per-image reduction, in the cull's counting form (surface.h): a workgroup walks 32 consecutive 256-pixel blocks of the
//        launch, keeps the ten sums per lane in registers, and when the image changes or the walk ends reduces them in the wave
//        (shuffles), in the workgroup (LDS) and issues ten atomics -- ten per 8192 pixels of an image.  One set per 256 pixels
//        puts every workgroup's atomics of an image on one cache line, the finding of the bounds phase and of the cull's counters
//        (12.0 against 0.97 ms, 6.4 against 0.82 ms).  SUCRE_MOSAIC_PLAIN_ATOMIC: that form, one set per 256-pixel block, for the
//        tests: integer adds, the same words.
// The disagreement the rounds remove is rms_c = sqrt(sum_i word(7 + c) / sum_i word 0) / 16384 at the gains of the pass.
//
// Memory: 8 bytes per cell for span, 64 for the reference accumulator; 12 bytes per padded pixel of the largest batch for J'.
// Resources (gfx950, the build's gains_mosaic.rpt): span 9 VGPRs, apply 8, sums 60 and 320 bytes of LDS; 8 waves per SIMD, no scratch.
// Measured on one MI355X, 65 resident images of 1080p, 74 pixels per cell, 1.69 M of 1.81 M reached cells shared, in ONE run
// (tools/mosaic_gains_time.py, profiles/mosaic_gains_time.txt), next to the splat's 0.87 ms, invert_kernel's 0.62 ms and the blend's
// accumulate at H = 0.5 m, 23.8 ms, in the same run.  The span 2.48 ms behind its loads, 5.90 ms with the plain atomics, 0.65 ms
// over words that are final already.  The expectation was the surface phase's 0.79 ms: REFUTED, 3 x -- a minimum of heights is
// settled by a cell's first few arrivals, but the images arrive in ascending ordinal, so EVERY image raises the max word of every
// cell it reaches and the filter on that side passes one atomic per (image, cell) at least.  It runs once per mosaic and stays.
// The apply 0.59 ms, below the cull's 0.78 (no geometry, no cell; 24 bytes per pixel): as expected.  The sums 1.29 ms in the
// counting form against 3.26 ms with one set of atomics per 256 pixels (2.5 x: the cache-line finding once more), 1.6 x the cull
// with its counts -- it reads 40 bytes of the cell's accumulator and span per sample on top of the pixel.  The reference accumulate
// 26.7 ms (every sample has a weight, none is dropped at wq = 0: 1.12 x the blend's), a whole round with the solve 29.0 ms: the
// reused accumulate is 92 % of a round, as expected.  Three rounds and the measuring pass: 116 ms on this survey, whose RMS
// disagreement in the shared cells falls from 0.034 / 0.031 / 0.031 to 0.015 / 0.0041 / 0.0035 (R / G / B; factors 0.9 .. 1.1).
// Not built: run sums of adjacent lanes ahead of the span's atomics (a wave's lanes share cells; it would take the max side's
// (image, cell) atomics down by the pixels per cell and image); a 4-word reference pass (the reference reuses the blend's
// accumulate and pays for its three raw-colour words); multi-rank mosaics -- span (min / max), the reference accumulator (sum) and the sums
// (sum) are the tensors an all-reduce would combine.
#pragma once
#include "mosaic.h"

namespace sucre {

constexpr int kGainWords = 10;          // int64 words per image of the sums (SUCRE_MOSAIC_GAIN_WORDS)
static_assert(kGainWords == SUCRE_MOSAIC_GAIN_WORDS, "the sums' layout is public");
constexpr int kGainRowWords = 16;       // an image's row of the sums: 128 bytes
constexpr uint64_t kGainMaxPixels = 1ull << 26;   // H W of an image the sums take: no word passes 2^62

// The float32 clamp / quantise of the sums: one IEEE operation per step; a NaN comes out as -8 (fmaxf drops it), an infinity as +-8.
__device__ __forceinline__ long long gain_quantise(float x) {
    return (long long)rintf(fminf(fmaxf(x, -8.0f), 8.0f) * 16384.0f);
}

__device__ __forceinline__ long long wave_sum_i64(long long x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    return x;
}

// The workgroup's kWords sums into the row of `ordinal`, and the lanes' registers back to zero.  Every lane of the workgroup calls it.
// (The ten sums of a pass, and the four words per image of the direct solve's diag, gains_direct.h.)
template <int kWords>
__device__ __forceinline__ void gain_flush(long long (&w)[kWords], long long (&part)[4][kWords], int ordinal,
                                           unsigned long long *__restrict__ sums) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < kWords; ++i) {
        const long long x = wave_sum_i64(w[i]);
        if (lane == 0) part[wave][i] = x;
        w[i] = 0;
    }
    __syncthreads();
    if (threadIdx.x < kWords) {
        const int i = threadIdx.x;
        const long long x = (part[0][i] + part[1][i]) + (part[2][i] + part[3][i]);
        if (x) __hip_atomic_fetch_add(sums + (size_t)ordinal * kGainRowWords + i, (unsigned long long)x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();   // part is written again by the next flush
}

// The span pass over images[0 .. n): the launches of a phase of mosaic.h; span: lowered / raised.
hipError_t launch_mosaic_gain_span(bool plain, void *table, int n_images, const sucre_mosaic_image_t *images, int first_ordinal,
                                   const MosaicGrid &grid, uint32_t *span, hipStream_t s);

// J_out = J x gains[ordinal] over images[0 .. n) (band_bytes of bands.h for the same images).
hipError_t launch_mosaic_gain_apply(void *table, int n_images, const sucre_mosaic_image_t *images, int first_ordinal, const float *gains,
                                    float *J_out, hipStream_t s);

// The ten sums per image over images[0 .. n); span, acc (the reference accumulator), gains: read; sums: added to.
hipError_t launch_mosaic_gain_sums(bool plain, void *table, int n_images, const sucre_mosaic_image_t *images, int first_ordinal,
                                   const MosaicGrid &grid, const uint32_t *span, const long long *acc, const float *gains,
                                   unsigned long long *sums, hipStream_t s);

}  // namespace sucre

// Per-image gain compensation of the seabed mosaic for gfx950 (sucre_mosaic_gain_span, sucre_mosaic_gain_apply,
// sucre_mosaic_gain_sums; the description: gains_mosaic.h).
#include "gains_mosaic.h"
#include "mosaic_walk.h"

namespace sucre {

constexpr uint32_t kGainSumBlocks = 32;   // 256-pixel blocks per workgroup of the sums' counting form (the cull's, surface.hip)

template <bool kPlain>
__global__ __launch_bounds__(256) void mosaic_gain_span_kernel(const MosaicImage *__restrict__ table, int n_images, const MosaicGrid g,
                                                               uint32_t *__restrict__ span) {
    const MosaicImage *__restrict__ im;
    uint32_t p;
    MosaicPixel m;
    const bool in = mosaic_walk(table, n_images, g, &im, &p, &m);
    size_t cell = 0;
    if (!in || !mosaic_cell(g, m, &cell)) return;
    const uint32_t mine = (uint32_t)im->ordinal;
    uint32_t *lo = span + cell * 2, *hi = lo + 1;
    // a stale value is only less extreme than the current one: whatever is skipped here could not have moved the word
    if (kPlain || __hip_atomic_load(lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > mine) atomicMin(lo, mine);
    if (kPlain || __hip_atomic_load(hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < mine) atomicMax(hi, mine);
}

// One lane per pixel; the lane's pixel of J_out sits where the lane sits in the launch (the cull's layout).  The three channels are
// read before the first is written: the image's J may be this very block of J_out.
__global__ __launch_bounds__(256) void mosaic_gain_apply_kernel(const MosaicImage *__restrict__ table, int n_images,
                                                                const float *__restrict__ gains, float *J_out) {
    const MosaicImage *__restrict__ im = mosaic_block_image(table, n_images);
    const uint32_t n_px = (uint32_t)im->H * (uint32_t)im->W;
    const uint32_t p = (blockIdx.x - im->block0) * kMosaicBlockPx + threadIdx.x;
    if (p >= n_px) return;
    const float *__restrict__ row = gains + (size_t)im->ordinal * 3;   // wave-uniform
    const float g0 = row[0], g1 = row[1], g2 = row[2];
    const float *pj = im->J + (size_t)p * 3;
    const float j0 = pj[0], j1 = pj[1], j2 = pj[2];
    float *o = J_out + ((size_t)blockIdx.x * kMosaicBlockPx + threadIdx.x) * 3;
    o[0] = j0 * g0; o[1] = j1 * g1; o[2] = j2 * g2;
}

// kPlain: a workgroup per 256-pixel block, one set of atomics each.  Otherwise a workgroup walks kGainSumBlocks consecutive blocks
// and flushes when the image changes (the block's image is workgroup-uniform) and at the end.
template <bool kPlain>
__global__ __launch_bounds__(256) void mosaic_gain_sums_kernel(const MosaicImage *__restrict__ table, int n_images, const MosaicGrid g,
                                                               const uint32_t *__restrict__ span, const long long *__restrict__ acc,
                                                               const float *__restrict__ gains, unsigned long long *__restrict__ sums,
                                                               uint32_t n_blocks) {
    __shared__ long long part[4][kGainWords];
    constexpr uint32_t per = kPlain ? 1u : kGainSumBlocks;
    const uint32_t b0 = blockIdx.x * per;
    const uint32_t b1 = n_blocks - b0 < per ? n_blocks : b0 + per;
    long long w[kGainWords];
#pragma unroll
    for (int i = 0; i < kGainWords; ++i) w[i] = 0;
    const MosaicImage *__restrict__ cur = mosaic_block_image_at(table, n_images, b0);
    for (uint32_t block = b0; block < b1; ++block) {
        const MosaicImage *__restrict__ im;
        uint32_t p;
        MosaicPixel m;
        const bool in = mosaic_walk_at(table, n_images, g, block, &im, &p, &m);
        if (im != cur) {
            gain_flush(w, part, cur->ordinal, sums);
            cur = im;
        }
        size_t cell = 0;
        if (!in || !mosaic_cell(g, m, &cell)) continue;
        if (!(span[cell * 2] < span[cell * 2 + 1])) continue;   // not shared
        const float *__restrict__ row = gains + (size_t)im->ordinal * 3;   // wave-uniform
        const long long *__restrict__ a = acc + cell * kMosaicAccWords;
        const long long wsum = a[6];
        w[0] += 1;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const long long xq = gain_quantise(m.J[c]);
            const long long mq = gain_quantise(mosaic_quotient(a[c], wsum));
            const long long yq = gain_quantise(m.J[c] * row[c]);
            const long long rq = yq - mq;
            w[1 + c] += xq * mq;
            w[4 + c] += xq * xq;
            w[7 + c] += rq * rq;
        }
    }
    gain_flush(w, part, cur->ordinal, sums);
}

hipError_t launch_mosaic_gain_span(bool plain, void *table, int n_images, const sucre_mosaic_image_t *images, int first_ordinal,
                                   const MosaicGrid &grid, uint32_t *span, hipStream_t s) {
    mosaic_for_each_launch(table, n_images, images, first_ordinal, s, [&](uint32_t nb, const MosaicImage *entries, int nl) {
        if (plain) hipLaunchKernelGGL((mosaic_gain_span_kernel<true>), dim3(nb), dim3(256), 0, s, entries, nl, grid, span);
        else hipLaunchKernelGGL((mosaic_gain_span_kernel<false>), dim3(nb), dim3(256), 0, s, entries, nl, grid, span);
    });
    return hipGetLastError();
}

hipError_t launch_mosaic_gain_apply(void *table, int n_images, const sucre_mosaic_image_t *images, int first_ordinal, const float *gains,
                                    float *J_out, hipStream_t s) {
    size_t base = 0;   // floats ahead of this launch's first pixel
    mosaic_for_each_launch(table, n_images, images, first_ordinal, s, [&](uint32_t nb, const MosaicImage *entries, int nl) {
        hipLaunchKernelGGL(mosaic_gain_apply_kernel, dim3(nb), dim3(256), 0, s, entries, nl, gains, J_out + base);
        base += (size_t)nb * kMosaicBlockPx * 3;
    });
    return hipGetLastError();
}

hipError_t launch_mosaic_gain_sums(bool plain, void *table, int n_images, const sucre_mosaic_image_t *images, int first_ordinal,
                                   const MosaicGrid &grid, const uint32_t *span, const long long *acc, const float *gains,
                                   unsigned long long *sums, hipStream_t s) {
    mosaic_for_each_launch(table, n_images, images, first_ordinal, s, [&](uint32_t nb, const MosaicImage *entries, int nl) {
        if (plain)
            hipLaunchKernelGGL((mosaic_gain_sums_kernel<true>), dim3(nb), dim3(256), 0, s, entries, nl, grid, span, acc, gains, sums, nb);
        else
            hipLaunchKernelGGL((mosaic_gain_sums_kernel<false>), dim3((nb + kGainSumBlocks - 1) / kGainSumBlocks), dim3(256), 0, s, entries, nl,
                               grid, span, acc, gains, sums, nb);
    });
    return hipGetLastError();
}

}  // namespace sucre

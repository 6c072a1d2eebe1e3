// Surface test of the seabed mosaic for gfx950 (sucre_mosaic_surface, sucre_mosaic_cull and, with its second side,
// sucre_mosaic_cull_supported; the description: surface.h, of the second side: support.h).
#include "surface.h"
#include "mosaic_walk.h"
#include "order_key.h"

namespace sucre {

template <bool kPlain>
__global__ __launch_bounds__(256) void mosaic_surface_kernel(const MosaicImage *__restrict__ table, int n_images, const MosaicGrid g,
                                                             uint32_t *__restrict__ top) {
    const MosaicImage *__restrict__ im;
    uint32_t p;
    MosaicPixel m;
    const bool in = mosaic_walk(table, n_images, g, &im, &p, &m);
    size_t cell = 0;
    if (!in || !mosaic_cell(g, m, &cell) || m.a_n != m.a_n) return;
    const uint32_t mine = order_key(m.a_n);
    if constexpr (!kPlain) {
        // a stale value can only be larger than the current one: whatever is skipped here could not have lowered the word
        if (__hip_atomic_load(top + cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= mine) return;
    }
    atomicMin(top + cell, mine);
}

// One lane per pixel; the lane's pixel of J_out: mosaic_store_copy.  kTwoSided (support.h): a sample more than tol ABOVE its cell's
// top goes too, and is counted apart.  kCount: every workgroup's atomics land on one cache line (measured: 6.4 ms for 65 images of
// 1080p against 0.82 ms without the counters, the bounds phase's finding), so a workgroup of the counting form walks
// kMosaicCountBlocks consecutive 256-pixel blocks of the grid, one after the other, sums its waves' ballots as it goes and adds to
// each counter -- culled below, (two-sided: culled above,) samples with a cell -- at most once at the end.
template <bool kCount, bool kTwoSided>
__global__ __launch_bounds__(256) void mosaic_cull_kernel(const MosaicImage *__restrict__ table, int n_images, const MosaicGrid g,
                                                          const uint32_t *__restrict__ top, float tol, float *__restrict__ J_out,
                                                          const MosaicCull out, uint32_t n_blocks) {
    constexpr int kWords = kTwoSided ? 3 : 2;
    const uint32_t b0 = kCount ? blockIdx.x * kMosaicCountBlocks : blockIdx.x;
    const uint32_t b1 = kCount ? (n_blocks - b0 < kMosaicCountBlocks ? n_blocks : b0 + kMosaicCountBlocks) : b0 + 1;
    uint32_t n_below = 0, n_above = 0, n_cell = 0;   // of this wave
    for (uint32_t block = b0; block < b1; ++block) {
        const MosaicImage *__restrict__ im;
        uint32_t p;
        MosaicPixel m;
        const bool in = mosaic_walk_at(table, n_images, g, block, &im, &p, &m);
        const bool inside = p < (uint32_t)im->H * (uint32_t)im->W;
        size_t cell = 0;
        const bool has_cell = in && mosaic_cell(g, m, &cell);
        bool below = false, above = false;
        if (has_cell) {
            const uint32_t k = top[cell];
            if (k != ~0u) {   // a cell the surface phase has not seen culls nothing
                const float d = m.a_n - key_value(k);
                below = d > tol;
                if constexpr (kTwoSided) above = d < -tol;
            }
        }
        if (inside) mosaic_store_copy(J_out, block, in && !below && !above, m);
        if (below && out.culled) __hip_atomic_fetch_add(out.culled + cell, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if constexpr (kTwoSided) {
            if (above && out.culled_above) __hip_atomic_fetch_add(out.culled_above + cell, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if constexpr (kCount) {
            n_below += (uint32_t)__popcll(__ballot(below));
            if constexpr (kTwoSided) n_above += (uint32_t)__popcll(__ballot(above));
            n_cell += (uint32_t)__popcll(__ballot(has_cell));
        }
    }
    if constexpr (kCount) {
        __shared__ uint32_t part[4][kWords];
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        if (lane == 0) {
            part[wave][0] = n_below;
            if constexpr (kTwoSided) part[wave][1] = n_above;
            part[wave][kWords - 1] = n_cell;
        }
        __syncthreads();
        if (threadIdx.x < kWords) {
            const uint32_t x = (part[0][threadIdx.x] + part[1][threadIdx.x]) + (part[2][threadIdx.x] + part[3][threadIdx.x]);
            if (x) __hip_atomic_fetch_add(out.counts + threadIdx.x, (unsigned long long)x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

hipError_t launch_mosaic_surface(bool plain, void *table, int n_images, const sucre_mosaic_image_t *images, int first_ordinal,
                                 const MosaicGrid &grid, uint32_t *top, hipStream_t s) {
    mosaic_for_each_launch(table, n_images, images, first_ordinal, s, [&](uint32_t nb, const MosaicImage *entries, int nl) {
        if (plain) hipLaunchKernelGGL((mosaic_surface_kernel<true>), dim3(nb), dim3(256), 0, s, entries, nl, grid, top);
        else hipLaunchKernelGGL((mosaic_surface_kernel<false>), dim3(nb), dim3(256), 0, s, entries, nl, grid, top);
    });
    return hipGetLastError();
}

template <bool kTwoSided>
static hipError_t launch_cull(void *table, int n_images, const sucre_mosaic_image_t *images, int first_ordinal, const MosaicGrid &grid,
                              const uint32_t *top, float tol, float *J_out, const MosaicCull &out, hipStream_t s) {
    return mosaic_for_each_cull_launch(table, n_images, images, first_ordinal, s, out.counts != nullptr, J_out,
                                       [&](dim3 blocks, const MosaicImage *entries, int nl, float *J_launch, uint32_t nb) {
        if (out.counts)
            hipLaunchKernelGGL((mosaic_cull_kernel<true, kTwoSided>), blocks, dim3(256), 0, s, entries, nl, grid, top, tol, J_launch, out, nb);
        else
            hipLaunchKernelGGL((mosaic_cull_kernel<false, kTwoSided>), blocks, dim3(256), 0, s, entries, nl, grid, top, tol, J_launch, out, nb);
    });
}

hipError_t launch_mosaic_cull(bool two_sided, void *table, int n_images, const sucre_mosaic_image_t *images, int first_ordinal,
                              const MosaicGrid &grid, const uint32_t *top, float tol, float *J_out, const MosaicCull &out, hipStream_t s) {
    return two_sided ? launch_cull<true>(table, n_images, images, first_ordinal, grid, top, tol, J_out, out, s)
                     : launch_cull<false>(table, n_images, images, first_ordinal, grid, top, tol, J_out, out, s);
}

}  // namespace sucre

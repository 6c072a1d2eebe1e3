// View-supported surface of the seabed mosaic for gfx950 (sucre_mosaic_support, sucre_mosaic_support_top; the description:
// support.h.  The two-sided cull of sucre_mosaic_cull_supported is surface.hip's cull kernel with its second side).
#include "support.h"
#include "mosaic_walk.h"
#include "order_key.h"

namespace sucre {

constexpr unsigned long long kNoRank = ~0ull;

// One lane per pixel, one level per launch.  The levels below `level` are final (earlier passes over all images): plain loads.
template <bool kPlain>
__global__ __launch_bounds__(256) void mosaic_support_kernel(const MosaicImage *__restrict__ table, int n_images, const MosaicGrid g,
                                                             int level, unsigned long long *rank) {
    const MosaicImage *__restrict__ im;
    uint32_t p;
    MosaicPixel m;
    const bool in = mosaic_walk(table, n_images, g, &im, &p, &m);
    size_t cell = 0;
    if (!in || !mosaic_cell(g, m, &cell) || m.a_n != m.a_n) return;
    const size_t n_cells = (size_t)g.Hm * (size_t)g.Wm;
    const uint32_t ordinal = (uint32_t)im->ordinal;
    unsigned long long below = 0;   // the level under this one; a level that is all ones has nothing but all ones above it
    for (int r = 0; r < level; ++r) {
        below = rank[(size_t)r * n_cells + cell];
        if ((uint32_t)below == ordinal) return;   // this image holds a lower level of the cell already
    }
    if (below == kNoRank) return;
    const unsigned long long mine = ((unsigned long long)order_key(m.a_n) << 32) | (unsigned long long)ordinal;
    unsigned long long *word = rank + (size_t)level * n_cells + cell;
    if constexpr (!kPlain) {
        // a stale value can only be larger than the current one: whatever is skipped here could not have lowered the word
        if (__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= mine) return;
    }
    atomicMin(word, mine);
}

// One lane per cell: the last level that holds something, of the first n_levels.
__global__ __launch_bounds__(256) void mosaic_support_top_kernel(size_t n_cells, int n_levels, const unsigned long long *__restrict__ rank,
                                                                 uint32_t *__restrict__ top, int32_t *__restrict__ support,
                                                                 int32_t *__restrict__ source) {
    const size_t cell = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (cell >= n_cells) return;
    unsigned long long last = kNoRank;
    int n = 0;
    for (int r = 0; r < n_levels; ++r) {
        const unsigned long long w = rank[(size_t)r * n_cells + cell];
        if (w == kNoRank) break;
        last = w;
        n = r + 1;
    }
    top[cell] = (uint32_t)(last >> 32);   // all ones for an empty cell
    if (support) support[cell] = n;
    if (source) source[cell] = n ? (int32_t)(uint32_t)last : -1;
}

hipError_t launch_mosaic_support(bool plain, void *table, int n_images, const sucre_mosaic_image_t *images, int first_ordinal,
                                 const MosaicGrid &grid, int level, unsigned long long *rank, hipStream_t s) {
    mosaic_for_each_launch(table, n_images, images, first_ordinal, s, [&](uint32_t nb, const MosaicImage *entries, int nl) {
        if (plain) hipLaunchKernelGGL((mosaic_support_kernel<true>), dim3(nb), dim3(256), 0, s, entries, nl, grid, level, rank);
        else hipLaunchKernelGGL((mosaic_support_kernel<false>), dim3(nb), dim3(256), 0, s, entries, nl, grid, level, rank);
    });
    return hipGetLastError();
}

hipError_t launch_mosaic_support_top(const MosaicGrid &grid, int n_levels, const unsigned long long *rank, uint32_t *top, int32_t *support,
                                     int32_t *source, hipStream_t s) {
    const size_t n_cells = (size_t)grid.Hm * (size_t)grid.Wm;   // the caller has checked that the workgroups fit a launch
    hipLaunchKernelGGL(mosaic_support_top_kernel, dim3((uint32_t)((n_cells + 255) / 256)), dim3(256), 0, s, n_cells, n_levels, rank, top,
                       support, source);
    return hipGetLastError();
}

}  // namespace sucre

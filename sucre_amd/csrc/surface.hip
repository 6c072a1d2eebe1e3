// Surface test of the seabed mosaic for gfx950 (sucre_mosaic_surface, sucre_mosaic_cull; the description: surface.h).
#include "surface.h"
#include "mosaic_walk.h"
#include "order_key.h"

namespace sucre {

constexpr uint32_t kCullCountBlocks = 32;   // 256-pixel blocks per workgroup of the cull's counting form

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

// One lane per pixel; the lane's pixel of J_out sits where the lane sits in the launch: pixel block 256 + threadIdx.x behind `J_out`.
// kCount: every workgroup's two atomics land on one cache line (measured: 6.4 ms for 65 images of 1080p against 0.82 ms without the
// counters, the bounds phase's finding), so a workgroup of the counting form walks kCullCountBlocks consecutive 256-pixel blocks
// of the grid, one after the other, sums its waves' ballots as it goes and adds to each counter at most once at the end.
template <bool kCount>
__global__ __launch_bounds__(256) void mosaic_cull_kernel(const MosaicImage *__restrict__ table, int n_images, const MosaicGrid g,
                                                          const uint32_t *__restrict__ top, float tol, float *__restrict__ J_out,
                                                          const MosaicCull out, uint32_t n_blocks) {
    const uint32_t b0 = kCount ? blockIdx.x * kCullCountBlocks : blockIdx.x;
    const uint32_t b1 = kCount ? (n_blocks - b0 < kCullCountBlocks ? n_blocks : b0 + kCullCountBlocks) : b0 + 1;
    uint32_t n_culled = 0, n_cell = 0;   // of this wave
    for (uint32_t block = b0; block < b1; ++block) {
        const MosaicImage *__restrict__ im;
        uint32_t p;
        MosaicPixel m;
        const bool in = mosaic_walk_at(table, n_images, g, block, &im, &p, &m);
        const bool inside = p < (uint32_t)im->H * (uint32_t)im->W;
        size_t cell = 0;
        const bool has_cell = in && mosaic_cell(g, m, &cell);
        bool cull = false;
        if (has_cell) {
            const uint32_t k = top[cell];
            cull = k != ~0u && m.a_n - key_value(k) > tol;   // a cell the surface phase has not seen culls nothing
        }
        if (inside) {
            const bool keep = in && !cull;
            const float none = __uint_as_float(0x7fc00000u);
            float *__restrict__ o = J_out + ((size_t)block * kMosaicBlockPx + threadIdx.x) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) o[c] = keep ? m.J[c] : none;
        }
        if (cull && out.culled) __hip_atomic_fetch_add(out.culled + cell, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if constexpr (kCount) {
            n_culled += (uint32_t)__popcll(__ballot(cull));
            n_cell += (uint32_t)__popcll(__ballot(has_cell));
        }
    }
    if constexpr (kCount) {
        __shared__ uint32_t part[4][2];
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        if (lane == 0) { part[wave][0] = n_culled; part[wave][1] = n_cell; }
        __syncthreads();
        if (threadIdx.x < 2) {
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

hipError_t launch_mosaic_cull(void *table, int n_images, const sucre_mosaic_image_t *images, int first_ordinal, const MosaicGrid &grid,
                              const uint32_t *top, float tol, float *J_out, const MosaicCull &out, hipStream_t s) {
    size_t base = 0;   // floats ahead of this launch's first pixel
    mosaic_for_each_launch(table, n_images, images, first_ordinal, s, [&](uint32_t nb, const MosaicImage *entries, int nl) {
        if (out.counts)
            hipLaunchKernelGGL((mosaic_cull_kernel<true>), dim3((nb + kCullCountBlocks - 1) / kCullCountBlocks), dim3(256), 0, s, entries, nl, grid,
                               top, tol, J_out + base, out, nb);
        else
            hipLaunchKernelGGL((mosaic_cull_kernel<false>), dim3(nb), dim3(256), 0, s, entries, nl, grid, top, tol, J_out + base, out, nb);
        base += (size_t)nb * kMosaicBlockPx * 3;
    });
    return hipGetLastError();
}

}  // namespace sucre

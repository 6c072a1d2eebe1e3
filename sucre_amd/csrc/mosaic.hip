// Seabed mosaic of restored images for gfx950 (sucre_mosaic_*; the description: mosaic.h).
#include "mosaic_walk.h"
#include "order_key.h"

namespace sucre {

struct MosaicEntries { MosaicImage e[kMosaicSet]; };

// Entries of the table handed over by value: the library performs no host-to-device copy (invert_set_kernel's way).
__global__ void mosaic_set_kernel(MosaicImage *dst, const MosaicEntries src, int n) {
    if ((int)threadIdx.x < n) dst[threadIdx.x] = src.e[threadIdx.x];
}

template <int kPhase>
__global__ __launch_bounds__(256) void mosaic_kernel(const MosaicImage *__restrict__ table, int n_images, const MosaicGrid g,
                                                     uint32_t *__restrict__ bounds, unsigned long long *__restrict__ key,
                                                     uint32_t *__restrict__ pix, const MosaicOut out) {
    const MosaicImage *__restrict__ im;
    uint32_t p;
    MosaicPixel m;
    const bool in = mosaic_walk(table, n_images, g, &im, &p, &m);

    if constexpr (kPhase == kMosaicBounds) {
        // words 0, 1: min of a_s, a_t; words 2, 3: max -- as the min of the complemented key, so that one reduction serves all four
        __shared__ uint32_t part[4][4];
        uint32_t k[4] = {~0u, ~0u, ~0u, ~0u};
        if (in) { k[0] = order_key(m.a_s); k[1] = order_key(m.a_t); k[2] = ~k[0]; k[3] = ~k[1]; }
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            k[i] = wave_min_u32(k[i]);
            if (lane == 0) part[wave][i] = k[i];
        }
        __syncthreads();
        if (threadIdx.x < 4) {
            const int i = threadIdx.x;
            uint32_t x = part[0][i];
#pragma unroll
            for (int w = 1; w < 4; ++w) x = part[w][i] < x ? part[w][i] : x;
            // A workgroup without a pixel that takes part adds nothing; nor does one whose extreme the word has passed already
            // (a stale value is only less extreme than the current one, so nothing that could move the word is skipped).
            // Measured: half a million workgroups' atomics on four words of one cache line serialise -- 12.0 ms for 65 images
            // of 1080p without this load, against the 0.58 ms of a streaming pass over the same images.
            if (x != ~0u) {
                const uint32_t seen = __hip_atomic_load(bounds + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (i < 2) { if (x < seen) atomicMin(bounds + i, x); }
                else if (~x > seen) atomicMax(bounds + i, ~x);
            }
        }
    } else {
        size_t cell = 0;
        if (!in || !mosaic_cell(g, m, &cell)) return;
        const unsigned long long mine = ((unsigned long long)__float_as_uint(m.z) << 32) | (unsigned long long)(uint32_t)im->ordinal;
        if constexpr (kPhase == kMosaicSplat || kPhase == kMosaicSplatPlain) {
            if constexpr (kPhase == kMosaicSplat) {
                // a stale value can only be larger than the current one: whatever is skipped here could not have won
                if (__hip_atomic_load(key + cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= mine) return;
            }
            atomicMin(key + cell, mine);
        } else if constexpr (kPhase == kMosaicResolve) {
            if (key[cell] == mine) atomicMin(pix + cell, p);
        } else {
            if (key[cell] != mine || pix[cell] != p) return;
            const uint32_t k0 = global_ptr(im->rgb)[(size_t)p * 3], k1 = global_ptr(im->rgb)[(size_t)p * 3 + 1],
                           k2 = global_ptr(im->rgb)[(size_t)p * 3 + 2];
            out.J[cell * 3] = m.J[0]; out.J[cell * 3 + 1] = m.J[1]; out.J[cell * 3 + 2] = m.J[2];
            out.raw[cell * 3] = (uint8_t)k0; out.raw[cell * 3 + 1] = (uint8_t)k1; out.raw[cell * 3 + 2] = (uint8_t)k2;
            out.source[cell] = im->ordinal;
            out.pixel[cell] = (int32_t)p;
            out.range[cell] = m.z;
        }
    }
}

// ---- the blend (mosaic.h, "The blend"): fixed-point sums per cell, then one pass over the cells ----

// kFeather: the weight takes one more factor, f of the pixel's capped squared border distance (mosaic.h, "The feather").  The
// lane's word of the map sits where the lane sits in the launch: word blockIdx.x 256 + threadIdx.x of `feather.dist2`.
template <bool kPlain, bool kFeather>
__global__ __launch_bounds__(256) void mosaic_accumulate_kernel(const MosaicImage *__restrict__ table, int n_images, const MosaicGrid g,
                                                                const unsigned long long *__restrict__ key, float inv_h,
                                                                unsigned long long *__restrict__ acc, const MosaicFeather feather) {
    const MosaicImage *__restrict__ im;
    uint32_t p;
    MosaicPixel m;
    const bool in = mosaic_walk(table, n_images, g, &im, &p, &m);
    size_t cell = 0;
    int32_t wq = 0;
    if (in && mosaic_cell(g, m, &cell)) {
        const float zmin = __uint_as_float((uint32_t)(key[cell] >> 32));   // an unsplatted cell: NaN, and fmaxf gives weight 0
        const float d = m.z - zmin;
        const float t = fmaxf(1.0f - d * inv_h, 0.0f);
        if constexpr (kFeather) {
            const uint32_t d2 = global_ptr(feather.dist2)[(size_t)blockIdx.x * kMosaicBlockPx + threadIdx.x];
            const float f = d2 >= feather.f2 ? 1.0f : sqrtf((float)d2) * feather.inv_f;
            wq = (int32_t)rintf(((t * t) * f) * 4096.0f);
        } else {
            wq = (int32_t)rintf((t * t) * 4096.0f);
        }
    }
    // (no lane leaves before the shuffles of the aggregated form)
    long long jq[3] = {0, 0, 0};
    uint32_t rq[3] = {0, 0, 0};
    if (wq > 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            jq[c] = (long long)wq * (long long)rintf(fminf(fmaxf(m.J[c], -1024.0f), 1024.0f) * 1048576.0f);
            rq[c] = (uint32_t)wq * (uint32_t)global_ptr(im->rgb)[(size_t)p * 3 + c];
        }
    }
    uint32_t wsum = (uint32_t)wq, count = wq > 0 ? 1u : 0u;
    bool issue = wq > 0;
    if constexpr (!kPlain) {
        // Lanes hold consecutive pixels of a row, so runs of adjacent lanes share a cell: one lane per run adds the run's sums.
        // Integer adds: the same bits as one add per lane.  Within a wave the colour sums stay below 64 x 4096 x 255 < 2^26.
        const int lane = threadIdx.x & 63;
        const uint32_t id_lo = wq > 0 ? (uint32_t)cell : ~0u, id_hi = wq > 0 ? (uint32_t)((uint64_t)cell >> 32) : ~0u;   // cells stay below 2^48
        const uint32_t before_lo = (uint32_t)__shfl_up((int)id_lo, 1), before_hi = (uint32_t)__shfl_up((int)id_hi, 1);
        const bool head = lane == 0 || wq <= 0 || before_lo != id_lo || before_hi != id_hi;
        const unsigned long long heads = __ballot(head);
        const unsigned long long above = (heads >> lane) >> 1;   // heads of the lanes after this one
        const int left = above ? __ffsll((long long)above) : 64 - lane;
#pragma unroll
        for (int c = 0; c < 3; ++c) { jq[c] = run_sum(jq[c], left); rq[c] = run_sum(rq[c], left); }
        wsum = run_sum(wsum, left);
        count = run_sum(count, left);
        issue = head && wq > 0;
    }
    if (!issue) return;
    unsigned long long *a = acc + cell * kMosaicAccWords;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        __hip_atomic_fetch_add(a + c, (unsigned long long)jq[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(a + 3 + c, (unsigned long long)rq[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __hip_atomic_fetch_add(a + 6, (unsigned long long)wsum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(a + 7, (unsigned long long)count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One lane per cell: the sums of a filled cell become its four outputs; an empty cell's outputs are not touched.
__global__ __launch_bounds__(256) void mosaic_normalize_kernel(size_t n_cells, const long long *__restrict__ acc, const MosaicBlend out) {
    const size_t cell = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (cell >= n_cells) return;
    const long long *a = acc + cell * kMosaicAccWords;
    const long long wsum = a[6], count = a[7];
    if (count <= 0) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        out.J[cell * 3 + c] = mosaic_quotient(a[c], wsum);
        out.raw[cell * 3 + c] = (uint8_t)((2 * a[3 + c] + wsum) / (2 * wsum));
    }
    out.weight[cell] = (float)((double)wsum * 0x1p-12);
    out.samples[cell] = count > 0x7fffffffll ? 0x7fffffff : (int32_t)count;
}

// ---- the feather (mosaic.h, "The feather"): the capped squared distance of every member to the nearest non-member ----

// Columns: one lane per column walks down and then up; the lanes of a wave touch consecutive addresses of a row.  blockIdx.y: the
// image of the launch; blockIdx.x: its 64-column strip (a workgroup past the image's width leaves).
__global__ __launch_bounds__(64) void feather_columns_kernel(const MosaicImage *__restrict__ table, uint32_t F, uint16_t *__restrict__ g) {
    const MosaicImage *__restrict__ im = table + blockIdx.y;
    const uint32_t W = (uint32_t)im->W, H = (uint32_t)im->H, u = blockIdx.x * 64 + threadIdx.x;
    if (u >= W) return;
    const auto *depth = global_ptr(im->depth);
    const auto *J = global_ptr(im->J);
    uint16_t *__restrict__ gi = g + (size_t)im->block0 * kMosaicBlockPx;
    uint32_t run = 0;   // rows since the last non-member, capped; the row above the image is one
#pragma unroll 4
    for (uint32_t v = 0; v < H; ++v) {
        const size_t p = (size_t)v * W + u;
        const bool in = mosaic_member(depth[p], J[p * 3], J[p * 3 + 1], J[p * 3 + 2]);
        run = in ? (run < F ? run + 1 : F) : 0;
        gi[p] = (uint16_t)run;
    }
    run = 0;            // and so is the row below it
#pragma unroll 4
    for (uint32_t v = H; v-- > 0;) {
        const size_t p = (size_t)v * W + u;
        const uint32_t down = gi[p];
        run = down ? (run < F ? run + 1 : F) : 0;
        if (run < down) gi[p] = (uint16_t)run;
    }
}

// Rows: one lane per pixel, a workgroup per 256-column segment of a row (blockIdx.x: the segment, .y: the row, .z: the image; a
// workgroup past the image leaves, all its lanes together).  The segment and its F - 1 columns of halo on either side are
// staged in LDS, a column outside the image as 0; each lane then scans outwards and stops once dx^2 cannot improve its minimum.
__global__ __launch_bounds__(256) void feather_rows_kernel(const MosaicImage *__restrict__ table, uint32_t F, const uint16_t *__restrict__ g,
                                                           uint32_t *__restrict__ dist2) {
    __shared__ uint16_t win[kMosaicBlockPx + 2 * (kFeatherMax - 1)];
    const MosaicImage *__restrict__ im = table + blockIdx.z;
    const uint32_t W = (uint32_t)im->W, H = (uint32_t)im->H, v = blockIdx.y, u0 = blockIdx.x * kMosaicBlockPx;
    if (v >= H || u0 >= W) return;
    const size_t row = (size_t)im->block0 * kMosaicBlockPx + (size_t)v * W;
    const uint32_t halo = F - 1, n = kMosaicBlockPx + 2 * halo;
    for (uint32_t i = threadIdx.x; i < n; i += kMosaicBlockPx) {
        const uint32_t u = u0 + i - halo;   // wraps below 0: then it is not below W either
        win[i] = u < W ? g[row + u] : (uint16_t)0;
    }
    __syncthreads();
    const uint32_t u = u0 + threadIdx.x;
    if (u >= W) return;
    const uint32_t c = halo + threadIdx.x, g0 = win[c], F2 = F * F;
    uint32_t best = g0 * g0 < F2 ? g0 * g0 : F2;
    for (uint32_t dx = 1; dx < F && dx * dx < best; ++dx) {
        const uint32_t a = win[c - dx], b = win[c + dx], m = a < b ? a : b, d = dx * dx + m * m;
        best = d < best ? d : best;
    }
    dist2[row + u] = best;
}

template <int kPhase>
static void mosaic_launch(uint32_t n_blocks, hipStream_t s, const MosaicImage *table, int n, const MosaicGrid &g, uint32_t *bounds,
                          unsigned long long *key, uint32_t *pix, const MosaicOut &out) {
    hipLaunchKernelGGL((mosaic_kernel<kPhase>), dim3(n_blocks), dim3(256), 0, s, table, n, g, bounds, key, pix, out);
}

uint32_t mosaic_set_launch(MosaicImage *entries, int l0, int nl, const sucre_mosaic_image_t *images, int first_ordinal, hipStream_t s) {
    uint64_t block0 = 0;
    for (int i0 = l0; i0 < l0 + nl; i0 += kMosaicSet) {
        MosaicEntries src = {};
        const int n = l0 + nl - i0 < kMosaicSet ? l0 + nl - i0 : kMosaicSet;
        for (int j = 0; j < n; ++j) {
            const sucre_mosaic_image_t &im = images[i0 + j];
            MosaicImage &e = src.e[j];
            e.depth = im.depth; e.rgb = im.rgb; e.J = im.J; e.H = im.H; e.W = im.W;
            for (int q = 0; q < 9; ++q) { e.Kinv[q] = im.Kinv[q]; e.R[q] = im.R[q]; }
            for (int q = 0; q < 3; ++q) e.t[q] = im.t[q];
            e.block0 = (uint32_t)block0;
            e.ordinal = first_ordinal + i0 + j;
            block0 += mosaic_blocks(im.H, im.W);
        }
        hipLaunchKernelGGL(mosaic_set_kernel, dim3(1), dim3(64), 0, s, entries + i0, src, n);
    }
    return (uint32_t)block0;
}

hipError_t launch_mosaic(MosaicPhase phase, void *table, int n_images, const sucre_mosaic_image_t *images, int first_ordinal,
                         const MosaicGrid &grid, uint32_t *bounds, unsigned long long *key, uint32_t *pix, const MosaicOut &out,
                         hipStream_t s) {
    mosaic_for_each_launch(table, n_images, images, first_ordinal, s, [&](uint32_t nb, const MosaicImage *entries, int nl) {
        switch (phase) {
            case kMosaicBounds: mosaic_launch<kMosaicBounds>(nb, s, entries, nl, grid, bounds, key, pix, out); break;
            case kMosaicSplat: mosaic_launch<kMosaicSplat>(nb, s, entries, nl, grid, bounds, key, pix, out); break;
            case kMosaicSplatPlain: mosaic_launch<kMosaicSplatPlain>(nb, s, entries, nl, grid, bounds, key, pix, out); break;
            case kMosaicResolve: mosaic_launch<kMosaicResolve>(nb, s, entries, nl, grid, bounds, key, pix, out); break;
            case kMosaicGather: mosaic_launch<kMosaicGather>(nb, s, entries, nl, grid, bounds, key, pix, out); break;
        }
    });
    return hipGetLastError();
}

hipError_t launch_mosaic_accumulate(bool plain, void *table, int n_images, const sucre_mosaic_image_t *images, int first_ordinal,
                                    const MosaicGrid &grid, const unsigned long long *key, float inv_h, const MosaicFeather *feather,
                                    unsigned long long *acc, hipStream_t s) {
    MosaicFeather f = feather ? *feather : MosaicFeather{};
    mosaic_for_each_launch(table, n_images, images, first_ordinal, s, [&](uint32_t nb, const MosaicImage *entries, int nl) {
        if (!feather) {
            if (plain) hipLaunchKernelGGL((mosaic_accumulate_kernel<true, false>), dim3(nb), dim3(256), 0, s, entries, nl, grid, key, inv_h, acc, f);
            else hipLaunchKernelGGL((mosaic_accumulate_kernel<false, false>), dim3(nb), dim3(256), 0, s, entries, nl, grid, key, inv_h, acc, f);
            return;
        }
        if (plain) hipLaunchKernelGGL((mosaic_accumulate_kernel<true, true>), dim3(nb), dim3(256), 0, s, entries, nl, grid, key, inv_h, acc, f);
        else hipLaunchKernelGGL((mosaic_accumulate_kernel<false, true>), dim3(nb), dim3(256), 0, s, entries, nl, grid, key, inv_h, acc, f);
        f.dist2 += (size_t)nb * kMosaicBlockPx;   // the map of the next launch's first image
    });
    return hipGetLastError();
}

hipError_t launch_mosaic_feather(void *table, int n_images, const sucre_mosaic_image_t *images, int feather_px, void *feather,
                                 hipStream_t s) {
    auto *dist2 = static_cast<uint32_t *>(feather);
    auto *g = reinterpret_cast<uint16_t *>(dist2 + feather_words(n_images, images));
    size_t base = 0;   // words ahead of this launch's first image
    int first = 0;     // that image
    mosaic_for_each_launch(table, n_images, images, 0, s, [&](uint32_t nb, const MosaicImage *entries, int nl) {
        int Hmax = 0, Wmax = 0;
        for (int i = first; i < first + nl; ++i) {
            Hmax = images[i].H > Hmax ? images[i].H : Hmax;
            Wmax = images[i].W > Wmax ? images[i].W : Wmax;
        }
        hipLaunchKernelGGL(feather_columns_kernel, dim3((uint32_t)(Wmax + 63) / 64, (uint32_t)nl), dim3(64), 0, s, entries, (uint32_t)feather_px,
                           g + base);
        hipLaunchKernelGGL(feather_rows_kernel, dim3((uint32_t)(Wmax + kMosaicBlockPx - 1) / kMosaicBlockPx, (uint32_t)Hmax, (uint32_t)nl),
                           dim3(256), 0, s, entries, (uint32_t)feather_px, g + base, dist2 + base);
        base += (size_t)nb * kMosaicBlockPx;
        first += nl;
    });
    return hipGetLastError();
}

hipError_t launch_mosaic_normalize(const MosaicGrid &grid, const long long *acc, const MosaicBlend &out, hipStream_t s) {
    const size_t n_cells = (size_t)grid.Hm * (size_t)grid.Wm;   // the caller has checked that the workgroups fit a launch
    hipLaunchKernelGGL(mosaic_normalize_kernel, dim3((uint32_t)((n_cells + 255) / 256)), dim3(256), 0, s, n_cells, acc, out);
    return hipGetLastError();
}

}  // namespace sucre

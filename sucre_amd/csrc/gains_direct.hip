// The direct solve of the mosaic's gain compensation for gfx950 (sucre_mosaic_gain_slots, sucre_mosaic_gain_pairs,
// sucre_mosaic_gain_diag; the description: gains_direct.h).
#include "gains_direct.h"
#include "mosaic_walk.h"

namespace sucre {

constexpr uint32_t kGainDiagBlocks = 32;   // 256-pixel blocks per workgroup of the diag's counting form (the sums', gains_mosaic.hip)
constexpr uint32_t kPairKeyFree = 0xffffffffu;   // a key is i << 12 | j < 2^24
constexpr int kPairProbes = 32;            // entries a lane looks at before it takes the table for full

__device__ __forceinline__ bool gain_cell_shared(const uint32_t *__restrict__ span, size_t cell) {
    return span[cell * 2] < span[cell * 2 + 1];
}

// The slot of `mine` in the cell's eight, claimed if need be; kGainSlots when eight other images hold them (gains_direct.h, "slots").
__device__ __forceinline__ int gain_slot_of(uint32_t *so, uint32_t mine) {
    int k = 0;
    for (; k < kGainSlots; ++k) {
        uint32_t cur = __hip_atomic_load(so + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == kGainSlotFree) cur = atomicCAS(so + k, kGainSlotFree, mine);   // the word before: free (claimed now), or its holder
        if (cur == mine || cur == kGainSlotFree) break;
    }
    return k;
}

template <bool kPlain>
__global__ __launch_bounds__(256) void mosaic_gain_slots_kernel(const MosaicImage *__restrict__ table, int n_images, const MosaicGrid g,
                                                                const uint32_t *__restrict__ span, uint32_t *slot_ord,
                                                                unsigned long long *__restrict__ slot_sum, uint32_t *slot_over) {
    const MosaicImage *__restrict__ im;
    uint32_t p;
    MosaicPixel m;
    const bool in = mosaic_walk(table, n_images, g, &im, &p, &m);
    size_t cell = 0;
    const bool part = in && mosaic_cell(g, m, &cell) && gain_cell_shared(span, cell);
    // (no lane leaves before the shuffles of the aggregated form)
    uint32_t count = part ? 1u : 0u;
    int xq[3] = {0, 0, 0};
    if (part) {
#pragma unroll
        for (int c = 0; c < 3; ++c) xq[c] = (int)gain_quantise(m.J[c]);   // |Xq| <= 2^17: a wave's run stays below 2^23
    }
    bool issue = part;
    if constexpr (!kPlain) {
        // Lanes hold consecutive pixels of ONE image, so runs of adjacent lanes share a cell: one lane per run claims and adds.
        const int lane = threadIdx.x & 63;
        const uint32_t id_lo = part ? (uint32_t)cell : ~0u, id_hi = part ? (uint32_t)((uint64_t)cell >> 32) : ~0u;   // cells stay below 2^48
        const uint32_t before_lo = (uint32_t)__shfl_up((int)id_lo, 1), before_hi = (uint32_t)__shfl_up((int)id_hi, 1);
        const bool head = lane == 0 || !part || before_lo != id_lo || before_hi != id_hi;
        const unsigned long long heads = __ballot(head);
        const unsigned long long above = (heads >> lane) >> 1;   // heads of the lanes after this one
        const int left = above ? __ffsll((long long)above) : 64 - lane;
#pragma unroll
        for (int c = 0; c < 3; ++c) xq[c] = run_sum(xq[c], left);
        count = run_sum(count, left);
        issue = head && part;
    }
    if (!issue) return;
    const int k = gain_slot_of(slot_ord + cell * kGainSlots, (uint32_t)im->ordinal);
    if (k == kGainSlots) {
        if (__hip_atomic_load(slot_over + cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) atomicOr(slot_over + cell, 1u);
        return;
    }
    unsigned long long *w = slot_sum + (cell * kGainSlots + (size_t)k) * kGainSlotWords;
    __hip_atomic_fetch_add(w, (unsigned long long)count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
    for (int c = 0; c < 3; ++c)
        __hip_atomic_fetch_add(w + 1 + c, (unsigned long long)(long long)xq[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The LDS table of the pairs: `entries` of its kPairTableMax are in use (a power of two; `bits` its logarithm).
struct PairTable {
    uint32_t key[kPairTableMax];
    unsigned long long word[kPairTableMax][kGainPairWords];
};

__device__ __forceinline__ void pair_add_global(unsigned long long *__restrict__ pairs, int n, uint32_t i, uint32_t j, const long long (&v)[3],
                                                unsigned long long cells) {
    unsigned long long *w = pairs + ((size_t)i * (size_t)n + j) * kGainPairWords;
#pragma unroll
    for (int c = 0; c < 3; ++c) __hip_atomic_fetch_add(w + c, (unsigned long long)v[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(w + 3, cells, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One pair's three quotients and its cell: into the workgroup's table, or, when the lane finds neither its key nor a free entry
// within kPairProbes entries (or the whole table), into global memory -- the same integer add.
template <bool kPlain>
__device__ __forceinline__ void pair_add(PairTable &t, int entries, int bits, unsigned long long *__restrict__ pairs, int n, uint32_t i,
                                         uint32_t j, const long long (&v)[3]) {
    if constexpr (!kPlain) {
        const uint32_t key = i << 12 | j, mask = (uint32_t)entries - 1;
        const uint32_t h = bits ? (key * 2654435761u) >> (32 - bits) : 0u;
        const int probes = entries < kPairProbes ? entries : kPairProbes;
        for (int s = 0; s < probes; ++s) {
            const uint32_t at = (h + (uint32_t)s) & mask;
            uint32_t cur = __hip_atomic_load(&t.key[at], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (cur == kPairKeyFree) cur = atomicCAS(&t.key[at], kPairKeyFree, key);
            if (cur == key || cur == kPairKeyFree) {
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    __hip_atomic_fetch_add(&t.word[at][c], (unsigned long long)v[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __hip_atomic_fetch_add(&t.word[at][3], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                return;
            }
        }
    }
    pair_add_global(pairs, n, i, j, v, 1ull);
}

// One lane per cell, kPairTileCells consecutive cells per workgroup.  A cell's slots are read where they lie (292 bytes of the
// lane's own: no register array, no scratch); the occupied slots are a prefix of the eight.
template <bool kPlain>
__global__ __launch_bounds__(256) void mosaic_gain_pairs_kernel(size_t n_cells, const uint32_t *__restrict__ span,
                                                                const uint32_t *__restrict__ slot_ord, const long long *__restrict__ slot_sum,
                                                                const uint32_t *__restrict__ slot_over, int n,
                                                                unsigned long long *__restrict__ pairs, int entries, int bits) {
    __shared__ PairTable t;
    if constexpr (!kPlain) {
        for (int e = threadIdx.x; e < entries; e += 256) {
            t.key[e] = kPairKeyFree;
#pragma unroll
            for (int w = 0; w < kGainPairWords; ++w) t.word[e][w] = 0;
        }
        __syncthreads();
    }
    const size_t cell0 = (size_t)blockIdx.x * kPairTileCells;
    for (uint32_t step = 0; step < kPairTileCells; step += 256) {
        const size_t cell = cell0 + step + threadIdx.x;
        if (cell >= n_cells || !gain_cell_shared(span, cell) || slot_over[cell] != 0) continue;
        const uint32_t *__restrict__ so = slot_ord + cell * kGainSlots;
        const long long *__restrict__ ss = slot_sum + cell * (kGainSlots * kGainSlotWords);
        int held = 0;
        long long N = 0;
        for (; held < kGainSlots && so[held] != kGainSlotFree; ++held) N += ss[held * kGainSlotWords];
        if (N <= 0) continue;
        const double dN = (double)N;
        for (int a = 0; a < held; ++a) {
            const uint32_t oa = so[a];
            const double sa0 = (double)ss[a * kGainSlotWords + 1], sa1 = (double)ss[a * kGainSlotWords + 2],
                         sa2 = (double)ss[a * kGainSlotWords + 3];
            for (int b = a; b < held; ++b) {
                const uint32_t ob = so[b];
                const uint32_t i = oa < ob ? oa : ob, j = oa < ob ? ob : oa;
                if (j >= (uint32_t)n) continue;   // no ordinal of a checked call: never index past the pairs
                const long long v[3] = {llrint((sa0 * (double)ss[b * kGainSlotWords + 1]) / dN),
                                        llrint((sa1 * (double)ss[b * kGainSlotWords + 2]) / dN),
                                        llrint((sa2 * (double)ss[b * kGainSlotWords + 3]) / dN)};
                pair_add<kPlain>(t, entries, bits, pairs, n, i, j, v);
            }
        }
    }
    if constexpr (!kPlain) {
        __syncthreads();
        for (int e = threadIdx.x; e < entries; e += 256) {
            const uint32_t key = t.key[e];
            if (key == kPairKeyFree) continue;
            const long long v[3] = {(long long)t.word[e][0], (long long)t.word[e][1], (long long)t.word[e][2]};
            pair_add_global(pairs, n, key >> 12, key & 4095u, v, t.word[e][3]);
        }
    }
}

// kPlain: a workgroup per 256-pixel block, one set of atomics each.  Otherwise a workgroup walks kGainDiagBlocks consecutive blocks
// and flushes when the image changes and at the end (mosaic_gain_sums_kernel's form, on four words).
template <bool kPlain>
__global__ __launch_bounds__(256) void mosaic_gain_diag_kernel(const MosaicImage *__restrict__ table, int n_images, const MosaicGrid g,
                                                               const uint32_t *__restrict__ span, const uint32_t *__restrict__ slot_over,
                                                               unsigned long long *__restrict__ diag, uint32_t n_blocks) {
    __shared__ long long part[4][kGainDiagWords];
    constexpr uint32_t per = kPlain ? 1u : kGainDiagBlocks;
    const uint32_t b0 = blockIdx.x * per;
    const uint32_t b1 = n_blocks - b0 < per ? n_blocks : b0 + per;
    long long w[kGainDiagWords];
#pragma unroll
    for (int i = 0; i < kGainDiagWords; ++i) w[i] = 0;
    const MosaicImage *__restrict__ cur = mosaic_block_image_at(table, n_images, b0);
    for (uint32_t block = b0; block < b1; ++block) {
        const MosaicImage *__restrict__ im;
        uint32_t p;
        MosaicPixel m;
        const bool in = mosaic_walk_at(table, n_images, g, block, &im, &p, &m);
        if (im != cur) {
            gain_flush(w, part, cur->ordinal, diag);
            cur = im;
        }
        size_t cell = 0;
        if (!in || !mosaic_cell(g, m, &cell)) continue;
        if (!gain_cell_shared(span, cell) || slot_over[cell] != 0) continue;
        w[0] += 1;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const long long xq = gain_quantise(m.J[c]);
            w[1 + c] += xq * xq;
        }
    }
    gain_flush(w, part, cur->ordinal, diag);
}

hipError_t launch_mosaic_gain_slots(bool plain, void *table, int n_images, const sucre_mosaic_image_t *images, int first_ordinal,
                                    const MosaicGrid &grid, const uint32_t *span, uint32_t *slot_ord, unsigned long long *slot_sum,
                                    uint32_t *slot_over, hipStream_t s) {
    mosaic_for_each_launch(table, n_images, images, first_ordinal, s, [&](uint32_t nb, const MosaicImage *entries, int nl) {
        if (plain)
            hipLaunchKernelGGL((mosaic_gain_slots_kernel<true>), dim3(nb), dim3(256), 0, s, entries, nl, grid, span, slot_ord, slot_sum, slot_over);
        else
            hipLaunchKernelGGL((mosaic_gain_slots_kernel<false>), dim3(nb), dim3(256), 0, s, entries, nl, grid, span, slot_ord, slot_sum, slot_over);
    });
    return hipGetLastError();
}

hipError_t launch_mosaic_gain_pairs(bool plain, const MosaicGrid &grid, const uint32_t *span, const uint32_t *slot_ord,
                                    const long long *slot_sum, const uint32_t *slot_over, int n_ordinals, unsigned long long *pairs,
                                    int table_entries, hipStream_t s) {
    const size_t n_cells = (size_t)grid.Hm * (size_t)grid.Wm;
    const uint32_t nb = (uint32_t)((n_cells + kPairTileCells - 1) / kPairTileCells);   // Hm Wm < 2^43, so nb < 2^31: checked by the caller
    int bits = 0;
    while ((1 << bits) < table_entries) ++bits;
    if (plain)
        hipLaunchKernelGGL((mosaic_gain_pairs_kernel<true>), dim3(nb), dim3(256), 0, s, n_cells, span, slot_ord, slot_sum, slot_over, n_ordinals,
                           pairs, table_entries, bits);
    else
        hipLaunchKernelGGL((mosaic_gain_pairs_kernel<false>), dim3(nb), dim3(256), 0, s, n_cells, span, slot_ord, slot_sum, slot_over, n_ordinals,
                           pairs, table_entries, bits);
    return hipGetLastError();
}

hipError_t launch_mosaic_gain_diag(bool plain, void *table, int n_images, const sucre_mosaic_image_t *images, int first_ordinal,
                                   const MosaicGrid &grid, const uint32_t *span, const uint32_t *slot_over, unsigned long long *diag,
                                   hipStream_t s) {
    mosaic_for_each_launch(table, n_images, images, first_ordinal, s, [&](uint32_t nb, const MosaicImage *entries, int nl) {
        if (plain)
            hipLaunchKernelGGL((mosaic_gain_diag_kernel<true>), dim3(nb), dim3(256), 0, s, entries, nl, grid, span, slot_over, diag, nb);
        else
            hipLaunchKernelGGL((mosaic_gain_diag_kernel<false>), dim3((nb + kGainDiagBlocks - 1) / kGainDiagBlocks), dim3(256), 0, s, entries, nl,
                               grid, span, slot_over, diag, nb);
    });
    return hipGetLastError();
}

}  // namespace sucre

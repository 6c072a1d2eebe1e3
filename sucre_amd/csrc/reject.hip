// Colour consensus across views of the seabed mosaic for gfx950 (sucre_mosaic_reject_claim, sucre_mosaic_reject_sums,
// sucre_mosaic_reject_consensus, sucre_mosaic_reject_cull; the description and the proof of the claim: reject.h).
#include "reject.h"
#include "mosaic_walk.h"

namespace sucre {

// Whether this lane is the first of a run of adjacent lanes of its wave that share `cell` (`part`: the lane has one).  Every lane of
// the wave calls it.  `left`: lanes from this one to the end of its run, this one included.
__device__ __forceinline__ bool reject_run_head(bool part, size_t cell, int *left) {
    const int lane = threadIdx.x & 63;
    const uint32_t id_lo = part ? (uint32_t)cell : ~0u, id_hi = part ? (uint32_t)((uint64_t)cell >> 32) : ~0u;   // cells stay below 2^48
    const uint32_t before_lo = (uint32_t)__shfl_up((int)id_lo, 1), before_hi = (uint32_t)__shfl_up((int)id_hi, 1);
    const bool head = lane == 0 || !part || before_lo != id_lo || before_hi != id_hi;
    const unsigned long long heads = __ballot(head);
    const unsigned long long above = (heads >> lane) >> 1;   // heads of the lanes after this one
    *left = above ? __ffsll((long long)above) : 64 - lane;
    return head;
}

// The cell's eight words as they stand (two 16-byte loads; the cell's words start at a multiple of 32 bytes).
__device__ __forceinline__ void reject_load_slots(const uint32_t *so, uint32_t (&x)[kRejectSlots]) {
    const uint4 a = reinterpret_cast<const uint4 *>(so)[0], b = reinterpret_cast<const uint4 *>(so)[1];
    x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w;
    x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
}

// The chain of reject.h from slot `s` on with the value `v`; true when a value was carried past the last slot.
__device__ __forceinline__ bool reject_chain(uint32_t *so, uint32_t v, int s) {
    for (; s < kRejectSlots; ++s) {
        const uint32_t old = atomicMin(so + s, v);
        if (old == v) return false;
        if (old > v) {
            if (old == kRejectSlotFree) return false;
            v = old;
        }
    }
    return true;
}

template <bool kPlain>
__global__ __launch_bounds__(256) void mosaic_reject_claim_kernel(const MosaicImage *__restrict__ table, int n_images, const MosaicGrid g,
                                                                  uint32_t *slot_ord, uint32_t *slot_over) {
    const MosaicImage *__restrict__ im;
    uint32_t p;
    MosaicPixel m;
    const bool in = mosaic_walk(table, n_images, g, &im, &p, &m);
    size_t cell = 0;
    const bool part = in && mosaic_cell(g, m, &cell);
    const uint32_t mine = (uint32_t)im->ordinal;
    if constexpr (kPlain) {
        if (!part) return;
        if (reject_chain(slot_ord + cell * kRejectSlots, mine, 0)) atomicOr(slot_over + cell, 1u);
    } else {
        // (no lane leaves before the shuffles)  Lanes hold consecutive pixels of ONE image: a run's lanes carry one value.
        int left;
        const bool head = reject_run_head(part, cell, &left);
        if (!head || !part) return;
        uint32_t *so = slot_ord + cell * kRejectSlots;
        uint32_t x[kRejectSlots];
        reject_load_slots(so, x);   // each word: a value it held at some moment, so not below what it holds now
        bool present = false;
        int enter = kRejectSlots;
#pragma unroll
        for (int i = kRejectSlots - 1; i >= 0; --i) {
            present = present || x[i] == mine;
            if (x[i] > mine) enter = i;
        }
        if (present) return;
        // all eight smaller: eight other ordinals below this one reach the cell, this is a ninth
        if (enter == kRejectSlots || reject_chain(so, mine, enter)) {
            if (slot_over[cell] == 0) atomicOr(slot_over + cell, 1u);
        }
    }
}

template <bool kPlain>
__global__ __launch_bounds__(256) void mosaic_reject_sums_kernel(const MosaicImage *__restrict__ table, int n_images, const MosaicGrid g,
                                                                 const uint32_t *__restrict__ slot_ord,
                                                                 unsigned long long *__restrict__ slot_sum) {
    const MosaicImage *__restrict__ im;
    uint32_t p;
    MosaicPixel m;
    const bool in = mosaic_walk(table, n_images, g, &im, &p, &m);
    size_t cell = 0;
    const bool part = in && mosaic_cell(g, m, &cell);
    uint32_t count = part ? 1u : 0u;
    int xq[3] = {0, 0, 0};
    if (part) {
#pragma unroll
        for (int c = 0; c < 3; ++c) xq[c] = (int)gain_quantise(m.J[c]);   // |Xq| <= 2^17: a wave's run stays below 2^23
    }
    bool issue = part;
    if constexpr (!kPlain) {
        int left;
        const bool head = reject_run_head(part, cell, &left);
#pragma unroll
        for (int c = 0; c < 3; ++c) xq[c] = run_sum(xq[c], left);
        count = run_sum(count, left);
        issue = head && part;
    }
    if (!issue) return;
    uint32_t x[kRejectSlots];
    reject_load_slots(slot_ord + cell * kRejectSlots, x);   // final: the claim has seen every image
    const uint32_t mine = (uint32_t)im->ordinal;
    int k = -1;
#pragma unroll
    for (int i = 0; i < kRejectSlots; ++i)
        if (x[i] == mine) k = i;
    if (k < 0) return;   // not one of the cell's eight: the image does not vote
    unsigned long long *w = slot_sum + (cell * kRejectSlots + (size_t)k) * kRejectSlotWords;
    __hip_atomic_fetch_add(w, (unsigned long long)count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
    for (int c = 0; c < 3; ++c)
        __hip_atomic_fetch_add(w + 1 + c, (unsigned long long)(long long)xq[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One lane per cell.  The eight slots' counts and brightness sums sit in registers (every index a constant after unrolling: no
// scratch); the reference's three colour sums are read again where they lie.
__global__ __launch_bounds__(256) void mosaic_reject_consensus_kernel(size_t n_cells, const uint32_t *__restrict__ slot_ord,
                                                                      const long long *__restrict__ slot_sum, float *__restrict__ ref,
                                                                      int32_t *__restrict__ source, int32_t *__restrict__ views,
                                                                      unsigned long long *__restrict__ big) {
    const size_t cell = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (cell >= n_cells) return;
    uint32_t ord[kRejectSlots];
    reject_load_slots(slot_ord + cell * kRejectSlots, ord);
    const long long *__restrict__ ss = slot_sum + cell * (kRejectSlots * kRejectSlotWords);
    long long N[kRejectSlots], Y[kRejectSlots];
    int k = 0;
    uint32_t n_big = 0;
#pragma unroll
    for (int a = 0; a < kRejectSlots; ++a) {
        const bool held = ord[a] != kRejectSlotFree;   // the occupied slots are a prefix
        N[a] = held ? ss[a * kRejectSlotWords] : 0;
        Y[a] = held ? (ss[a * kRejectSlotWords + 1] + ss[a * kRejectSlotWords + 2]) + ss[a * kRejectSlotWords + 3] : 0;
        k += held ? 1 : 0;
        n_big += held && N[a] >= kRejectMaxSamples ? 1u : 0u;
    }
    if (n_big) __hip_atomic_fetch_add(big, (unsigned long long)n_big, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    int pick = -1;
    uint32_t pick_ord = 0;
    long long pick_n = 0;
    if (k >= kRejectMinViews && n_big == 0) {
        const int mid = (k - 1) / 2;
#pragma unroll
        for (int a = 0; a < kRejectSlots; ++a) {
            int before = 0;   // slots that come before slot a
#pragma unroll
            for (int b = 0; b < kRejectSlots; ++b) {
                if (b == a) continue;
                const long long l = Y[b] * N[a], r = Y[a] * N[b];   // below 2^59 each
                before += b < k && (l < r || (l == r && ord[b] < ord[a])) ? 1 : 0;
            }
            if (a < k && before == mid) { pick = a; pick_ord = ord[a]; pick_n = N[a]; }
        }
    }
    const float none = __uint_as_float(0x7fc00000u);
    const bool has = pick >= 0 && pick_n > 0;
    const int at = has ? pick : 0;   // (slot 0 of the cell: a load that is always in bounds)
    float *__restrict__ o = ref + cell * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float mean = (float)(((double)ss[at * kRejectSlotWords + 1 + c] / (double)pick_n) * 0x1p-14);
        o[c] = has ? mean : none;
    }
    source[cell] = has ? (int32_t)pick_ord : -1;
    views[cell] = k;
}

// surface.hip's cull with the colour test (the same block loop, store and launches: mosaic_walk.h).  kCount: a workgroup walks kMosaicCountBlocks consecutive 256-pixel blocks and adds its
// two sums to its image's row when the image changes and at the end (gain_flush).
template <bool kCount>
__global__ __launch_bounds__(256) void mosaic_reject_cull_kernel(const MosaicImage *__restrict__ table, int n_images, const MosaicGrid g,
                                                                 const float *__restrict__ ref, const int32_t *__restrict__ source, float tol,
                                                                 float *__restrict__ J_out, const MosaicReject out, uint32_t n_blocks) {
    __shared__ long long part[4][kRejectCountWords];
    const uint32_t b0 = kCount ? blockIdx.x * kMosaicCountBlocks : blockIdx.x;
    const uint32_t b1 = kCount ? (n_blocks - b0 < kMosaicCountBlocks ? n_blocks : b0 + kMosaicCountBlocks) : b0 + 1;
    long long w[kRejectCountWords] = {0, 0};   // of this lane: samples in cells with a reference, samples rejected
    const MosaicImage *__restrict__ cur = mosaic_block_image_at(table, n_images, b0);
    for (uint32_t block = b0; block < b1; ++block) {
        const MosaicImage *__restrict__ im;
        uint32_t p;
        MosaicPixel m;
        const bool in = mosaic_walk_at(table, n_images, g, block, &im, &p, &m);
        if constexpr (kCount) {
            if (im != cur) {
                gain_flush(w, part, cur->ordinal, out.counts);
                cur = im;
            }
        }
        const bool inside = p < (uint32_t)im->H * (uint32_t)im->W;
        size_t cell = 0;
        const bool has_cell = in && mosaic_cell(g, m, &cell);
        bool has_ref = false, reject = false;
        if (has_cell) {
            const int32_t src = source[cell];
            has_ref = src >= 0;
            if (has_ref && src != im->ordinal) {
                const float *__restrict__ r = ref + cell * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c) reject = reject || fabsf(m.J[c] - r[c]) > tol;
            }
        }
        if (inside) mosaic_store_copy(J_out, block, in && !reject, m);
        if (reject && out.rejected) __hip_atomic_fetch_add(out.rejected + cell, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if constexpr (kCount) {
            w[0] += has_ref ? 1 : 0;
            w[1] += reject ? 1 : 0;
        }
    }
    if constexpr (kCount) gain_flush(w, part, cur->ordinal, out.counts);
}

hipError_t launch_mosaic_reject_claim(bool plain, void *table, int n_images, const sucre_mosaic_image_t *images, int first_ordinal,
                                      const MosaicGrid &grid, uint32_t *slot_ord, uint32_t *slot_over, hipStream_t s) {
    mosaic_for_each_launch(table, n_images, images, first_ordinal, s, [&](uint32_t nb, const MosaicImage *entries, int nl) {
        if (plain) hipLaunchKernelGGL((mosaic_reject_claim_kernel<true>), dim3(nb), dim3(256), 0, s, entries, nl, grid, slot_ord, slot_over);
        else hipLaunchKernelGGL((mosaic_reject_claim_kernel<false>), dim3(nb), dim3(256), 0, s, entries, nl, grid, slot_ord, slot_over);
    });
    return hipGetLastError();
}

hipError_t launch_mosaic_reject_sums(bool plain, void *table, int n_images, const sucre_mosaic_image_t *images, int first_ordinal,
                                     const MosaicGrid &grid, const uint32_t *slot_ord, unsigned long long *slot_sum, hipStream_t s) {
    mosaic_for_each_launch(table, n_images, images, first_ordinal, s, [&](uint32_t nb, const MosaicImage *entries, int nl) {
        if (plain) hipLaunchKernelGGL((mosaic_reject_sums_kernel<true>), dim3(nb), dim3(256), 0, s, entries, nl, grid, slot_ord, slot_sum);
        else hipLaunchKernelGGL((mosaic_reject_sums_kernel<false>), dim3(nb), dim3(256), 0, s, entries, nl, grid, slot_ord, slot_sum);
    });
    return hipGetLastError();
}

hipError_t launch_mosaic_reject_consensus(const MosaicGrid &grid, const uint32_t *slot_ord, const long long *slot_sum, float *ref,
                                          int32_t *source, int32_t *views, unsigned long long *big, hipStream_t s) {
    const size_t n_cells = (size_t)grid.Hm * (size_t)grid.Wm;   // the caller has checked that the workgroups fit a launch
    hipLaunchKernelGGL(mosaic_reject_consensus_kernel, dim3((uint32_t)((n_cells + 255) / 256)), dim3(256), 0, s, n_cells, slot_ord, slot_sum,
                       ref, source, views, big);
    return hipGetLastError();
}

hipError_t launch_mosaic_reject_cull(void *table, int n_images, const sucre_mosaic_image_t *images, int first_ordinal,
                                     const MosaicGrid &grid, const float *ref, const int32_t *source, float tol, float *J_out,
                                     const MosaicReject &out, hipStream_t s) {
    return mosaic_for_each_cull_launch(table, n_images, images, first_ordinal, s, out.counts != nullptr, J_out,
                                       [&](dim3 blocks, const MosaicImage *entries, int nl, float *J_launch, uint32_t nb) {
        if (out.counts)
            hipLaunchKernelGGL((mosaic_reject_cull_kernel<true>), blocks, dim3(256), 0, s, entries, nl, grid, ref, source, tol, J_launch, out, nb);
        else
            hipLaunchKernelGGL((mosaic_reject_cull_kernel<false>), blocks, dim3(256), 0, s, entries, nl, grid, ref, source, tol, J_launch, out, nb);
    });
}

}  // namespace sucre

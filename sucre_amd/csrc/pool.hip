// Pooled radix select for gfx950 (pool.h): the histogram pass over a chunk of images, the locate step, the image table.
//
// pool_pass_kernel: one launch walks all images of the chunk.  A workgroup takes kPoolBlockPx consecutive pixels of ONE image
// (found by bisecting the table's first-workgroup column), every lane four adjacent pixels at a time -- three 16-byte loads --
// and the image's last n_px % 4 pixels one by one; it counts into 32-bit LDS histograms and flushes them with one 64-bit global
// atomic per non-zero bin.
//
// Contention: a restored image lives in roughly [0.05, 2], so the top key byte takes two or three values and in pass 0 nearly
// all lanes of a wave add to the same few LDS words.  pool_count can let the wave vote first -- the byte of its first pending
// lane is broadcast, the lanes that hold the same byte are counted by a ballot and ONE lane adds the count -- for
// SUCRE_POOL_VOTE_ROUNDS rounds before whoever is still pending adds its own 1.  Measured on an MI355X (32 x 1080p,
// profiles/pool_select_time.txt) the vote gains nothing: pass 0 takes 0.40 ms with three rounds against 0.38 ms with plain LDS
// atomics, pass 1 with one round 0.59 against 0.39 ms.  The product therefore builds with 0 rounds; the vote stays behind
// the knob for the next measurement.
#include "launch.h"
#include "order_key.h"
#include "pool.h"

// Rounds of the wave's vote in pass 0 (later passes: one, or none when this is 0); tools/exp/pool_select_time.py measures
//   make VARIANT=vote3 EXTRA=-DSUCRE_POOL_VOTE_ROUNDS=3
// against the product.
#ifndef SUCRE_POOL_VOTE_ROUNDS
#define SUCRE_POOL_VOTE_ROUNDS 0
#endif

namespace sucre {

// The images' pointers come out of a table in memory; they are device-memory pointers by contract (as invert.h's
// invert_global): global loads, not flat ones.
template <class T>
__device__ __forceinline__ const __attribute__((address_space(1))) T *pool_global(const T *p) {
    return (const __attribute__((address_space(1))) T *)p;
}

// h[byte] += 1 for every lane that is `on`.
template <int kRounds>
__device__ __forceinline__ void pool_count(uint32_t *h, bool on, uint32_t byte, uint32_t lane) {
    bool pend = on;
#pragma unroll
    for (int i = 0; i < kRounds; ++i) {
        if (pend) {
            const uint32_t b0 = __builtin_amdgcn_readfirstlane(byte);   // of the first pending lane
            const unsigned long long same = __ballot(byte == b0);        // pending lanes only
            if (byte == b0) {
                if (lane == (uint32_t)(__ffsll((long long)same) - 1)) atomicAdd(&h[b0], (uint32_t)__popcll(same));
                pend = false;
            }
        }
    }
    if (pend) atomicAdd(&h[byte], 1u);
}

template <int kPass>
__global__ __launch_bounds__(256) void pool_pass_kernel(const PoolImage *__restrict__ table, int n_images, int n_ranks,
                                                        PoolState *__restrict__ st) {
    typedef float f4 __attribute__((ext_vector_type(4)));
    constexpr int kRounds = kPass == 0 ? SUCRE_POOL_VOTE_ROUNDS : (SUCRE_POOL_VOTE_ROUNDS ? 1 : 0);
    constexpr int shift = 24 - 8 * kPass;
    __shared__ uint32_t h[3][kPoolMaxRanks][256];
    __shared__ uint32_t pre[3][kPoolMaxRanks];
    const int nr = kPass == 0 ? 1 : n_ranks;   // pass 0 does not depend on the ranks: [c][0]
    for (int c = 0; c < 3; ++c)
        for (int r = 0; r < nr; ++r) h[c][r][threadIdx.x] = 0u;
    if (threadIdx.x < 3 * kPoolMaxRanks) (&pre[0][0])[threadIdx.x] = (&st->prefix[0][0])[threadIdx.x];
    __syncthreads();
    // the image of this workgroup: the last one whose first workgroup is not behind blockIdx.x (an image without pixels
    // shares its first workgroup with its successor and is never found)
    int lo = 0, hi = n_images - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].block0 <= blockIdx.x) lo = mid;
        else hi = mid - 1;
    }
    const PoolImage *__restrict__ im = table + lo;
    const uint64_t n_px = (uint64_t)im->n_px;
    const auto *J = pool_global(im->J);
    const uint64_t base = (uint64_t)(blockIdx.x - im->block0) * kPoolBlockPx;
    const uint32_t lane = threadIdx.x & 63u;

    auto count = [&](float x0, float x1, float x2) {
        if (x0 != x0 || x1 != x1 || x2 != x2) return;   // np.all(~np.isnan(J), axis=2), sucre.py:87: the whole pixel drops out
        const uint32_t key[3] = {order_key(x0), order_key(x1), order_key(x2)};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const uint32_t byte = (key[c] >> shift) & 255u;
            if constexpr (kPass == 0) {
                pool_count<kRounds>(h[c][0], true, byte, lane);
            } else {
                const uint32_t top = key[c] >> (shift + 8);
                for (int r = 0; r < nr; ++r) pool_count<kRounds>(h[c][r], top == pre[c][r], byte, lane);
            }
        }
    };

    for (int g = 0; g < kPoolGroupsPerLane; ++g) {
        const uint64_t first = base + ((uint64_t)g * 256u + threadIdx.x) * 4u;
        if (first >= n_px) break;
        if (first + 4u <= n_px) {
            typedef const __attribute__((address_space(1))) f4 *f4_in;
            const f4_in p = (f4_in)(J + first * 3u);   // 48 bytes per group: 16-byte aligned with J
            const f4 a = p[0], b = p[1], d = p[2];
            count(a.x, a.y, a.z);
            count(a.w, b.x, b.y);
            count(b.z, b.w, d.x);
            count(d.y, d.z, d.w);
        } else {   // the image's last n_px % 4 pixels, one by one
            for (uint64_t i = first; i < n_px; ++i) count(J[i * 3u], J[i * 3u + 1u], J[i * 3u + 2u]);
        }
    }
    __syncthreads();
    for (int c = 0; c < 3; ++c)
        for (int r = 0; r < nr; ++r) {
            const uint32_t v = h[c][r][threadIdx.x];
            if (v) atomicAdd(reinterpret_cast<unsigned long long *>(&st->hist[c][r][threadIdx.x]), (unsigned long long)v);
        }
}

struct PoolRanks { uint64_t v[kPoolMaxRanks]; };

// After a pass (and the host's all-reduce of the histograms): the byte under which every rank falls; the histograms are
// cleared for the next pass.  One block.  `ranks` is read at pass 0 only.
template <int kPass>
__global__ __launch_bounds__(256) void pool_locate_kernel(PoolState *__restrict__ st, int n_ranks, const PoolRanks ranks,
                                                          float *__restrict__ out) {
    const int t = threadIdx.x;
    if (t < 3 * n_ranks) {
        const int c = t / n_ranks, r = t % n_ranks;
        const uint64_t *h = st->hist[c][kPass == 0 ? 0 : r];
        uint64_t rem = kPass == 0 ? ranks.v[r] : st->remaining[c][r];
        uint32_t b = 0;
        for (; b < 255u; ++b) {
            if (rem < h[b]) break;
            rem -= h[b];
        }
        const uint32_t prefix = (kPass == 0 ? 0u : st->prefix[c][r] << 8) | b;
        st->prefix[c][r] = prefix;
        st->remaining[c][r] = rem;
        if (kPass == 3) out[c * n_ranks + r] = key_value(prefix);
    }
    __syncthreads();
    for (int i = t; i < 3 * kPoolMaxRanks * 256; i += 256) (&st->hist[0][0][0])[i] = 0ull;
}

constexpr int kPoolSet = 32;   // table entries per set launch (by value: 32 x 24 bytes of kernel arguments)
struct PoolEntries { PoolImage e[kPoolSet]; };

// Entries i0 .. i0 + n - 1 of the table, handed over by value: the library performs no host-to-device copy.
__global__ void pool_set_kernel(PoolImage *dst, const PoolEntries src, int n) {
    if ((int)threadIdx.x < n) dst[threadIdx.x] = src.e[threadIdx.x];
}

size_t pool_state_bytes() { return sizeof(PoolState); }

size_t pool_table_bytes(int n_images) { return align_up((size_t)(n_images > 0 ? n_images : 1) * sizeof(PoolImage), 256); }

hipError_t launch_pool_begin(void *state, hipStream_t s) { return hipMemsetAsync(state, 0, sizeof(PoolState), s); }

hipError_t launch_pool_pass(void *state, int pass, void *table, int n_images, const sucre_pool_image_t *images, int n_ranks,
                            hipStream_t s) {
    auto *st = static_cast<PoolState *>(state);
    auto *entries = static_cast<PoolImage *>(table);
    uint64_t block0 = 0;
    for (int i0 = 0; i0 < n_images; i0 += kPoolSet) {
        PoolEntries src = {};
        const int n = n_images - i0 < kPoolSet ? n_images - i0 : kPoolSet;
        for (int j = 0; j < n; ++j) {
            PoolImage &e = src.e[j];
            e.J = images[i0 + j].J;
            e.n_px = images[i0 + j].n_px;
            e.block0 = (uint32_t)block0;
            block0 += pool_blocks(e.n_px);
        }
        hipLaunchKernelGGL(pool_set_kernel, dim3(1), dim3(64), 0, s, entries + i0, src, n);
    }
    const uint32_t n_blocks = (uint32_t)block0;   // the caller has checked that the grid fits
    if (n_blocks == 0) return hipGetLastError();  // no pixel in the chunk: nothing to add
    switch (pass) {
        case 0: hipLaunchKernelGGL(pool_pass_kernel<0>, dim3(n_blocks), dim3(256), 0, s, entries, n_images, n_ranks, st); break;
        case 1: hipLaunchKernelGGL(pool_pass_kernel<1>, dim3(n_blocks), dim3(256), 0, s, entries, n_images, n_ranks, st); break;
        case 2: hipLaunchKernelGGL(pool_pass_kernel<2>, dim3(n_blocks), dim3(256), 0, s, entries, n_images, n_ranks, st); break;
        default: hipLaunchKernelGGL(pool_pass_kernel<3>, dim3(n_blocks), dim3(256), 0, s, entries, n_images, n_ranks, st); break;
    }
    return hipGetLastError();
}

hipError_t launch_pool_locate(void *state, int pass, int n_ranks, const uint64_t *ranks, float *out, hipStream_t s) {
    auto *st = static_cast<PoolState *>(state);
    PoolRanks r = {};
    if (pass == 0)
        for (int i = 0; i < n_ranks; ++i) r.v[i] = ranks[i];
    switch (pass) {
        case 0: hipLaunchKernelGGL(pool_locate_kernel<0>, dim3(1), dim3(256), 0, s, st, n_ranks, r, out); break;
        case 1: hipLaunchKernelGGL(pool_locate_kernel<1>, dim3(1), dim3(256), 0, s, st, n_ranks, r, out); break;
        case 2: hipLaunchKernelGGL(pool_locate_kernel<2>, dim3(1), dim3(256), 0, s, st, n_ranks, r, out); break;
        default: hipLaunchKernelGGL(pool_locate_kernel<3>, dim3(1), dim3(256), 0, s, st, n_ranks, r, out); break;
    }
    return hipGetLastError();
}

}  // namespace sucre

// Outlier-trimmed refit, the device side (sucre_trim_outliers*): sigma-clips single observations out of the DENSE store of a
// matched (or imported), finalised and fitted workspace; the caller then finalises again and fits anew.
//
//   outlier  <=>  r_c^2 > tau^2_c for any channel c,   tau^2_c = float32(k^2 S_c / N)      r: residual.h, sucre.py:144
//
// with N, S_c the observation count and the sums of r^2 of the residual pass's view_stats over the kept views (float64, in view
// order; trim_threshold_kernel forms tau^2 on the device, so the host never reads the table).  A NaN compares false: that
// observation stays.  A pixel whose observations would ALL go keeps all of them (nothing there is more trustworthy than anything
// else, and a pixel must not lose its last observation).
//
// The residual pass's walk (residual.h): one wave per tile, lane l owns slots 4 l .. 4 l + 3, 16-byte loads, the per-pixel state
// stays in the lane across the loop over the views, and the residual of an observation is residual_obs -- the one function the
// residual pass evaluates, so the decision cannot drift from the number it is defined by.  Two sweeps over the tile's views:
//   1  counts every pixel's would-be survivors;
//   2  zeroes the dropped observations' ranges (colours and extension planes stay, behind z > 0: the store's rule) and leaves
//      every (tile, kept view) pair's match count, pixel bits (word w, bit b = slot 64 w + b) and range pair as
//      count_view_kernel (match.hip) would leave them on the chunk as it now is -- the neutral pair, no bits and count 0 where
//      nothing is left or nothing ever was -- so that the existing finalise pass (view totals, min_cover, n_obs, range span, store
//      format, compaction, plans) runs on it as on a freshly imported store.  Views that are not kept keep everything they hold
//      (their range pairs are restated as their chunks' own, see there).
// The wave owns the whole (tile, view) chunk, so count, range pair and bits are wave reductions; the drops per (tile, view) go to
// caller-owned scratch, view-major, and trim_view_sum_kernel adds every view's tiles.  No atomics: two calls give the same bits.
#pragma once
#include "residual.h"

namespace sucre {

struct TrimArgs {
    ResidualArgs R;              // what the walk reads (count, ssr, tile_view, view_stats: unused)
    uint8_t *obs;                // the dense store again, to write
    uint16_t *cnt;
    uint64_t *vbits;             // [n_tiles][n_views][4]
    uint2 *zrange;               // [n_tiles][n_views]
    const float *tau2;           // [3], on the device
    int32_t *dropped;            // (H, W)
    int32_t *tile_view_drop;     // scratch [n_views][n_tiles]: written for every tile of every kept view
    int64_t *view_dropped;       // [n_views]
};

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += (uint32_t)__shfl_xor((int)x, off, 64);
    return x;
}

template <bool kU16, int kExt, class Light>
__global__ __launch_bounds__(256) void trim_kernel(const TrimArgs T) {
    static_assert(kExt >= 0 && kExt <= 3 && !(kU16 && kExt), "extension planes ride with the f32 store only");
    const ResidualArgs &A = T.R;
    const int lane = threadIdx.x & 63;
    const int tile = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (tile >= A.n_tiles) return;   // (no barrier below: the wave is on its own)
    const int n_views = A.n_views;
    const ResidualWater water(A.params);
    const Light light(A.geom);
    const float tau2[3] = {T.tau2[0], T.tau2[1], T.tau2[2]};

    float J[4][3];
    residual_load_J(A, tile, lane, J);

    const uint16_t *tcnt = A.cnt + (size_t)tile * n_views;
    // the kept views that reach the tile (wave-uniform).  Sweep 2 rewrites tcnt[k] only after it has looked at view k and found
    // the view after it, so both sweeps walk the same views
    auto next_view = [&](int k) { while (k < n_views && !(tcnt[k] > 0 && A.view_keep[k] != 0u)) ++k; return k; };
    // bit j: the lane's slot j holds an observation (valid) / one that is an outlier (the return value)
    auto outliers = [&](const ResidualChunk &q, uint32_t &valid) {
        uint32_t out = 0u;
        valid = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float r[3];
            const bool v = residual_obs<kU16, kExt>(q, j, light, water, J[j], r);
            const bool o = (r[0] * r[0] > tau2[0]) | (r[1] * r[1] > tau2[1]) | (r[2] * r[2] > tau2[2]);   // (r = 0 in an empty slot)
            valid |= (v ? 1u : 0u) << j;
            out |= ((v && o) ? 1u : 0u) << j;
        }
        return out;
    };

    // sweep 1: bit j of `some` = pixel j keeps at least one observation
    uint32_t some = 0u;
    {
        int k = next_view(0);
        ResidualChunk cur = {};
        if (k < n_views) cur = residual_load_chunk<kExt>(A, tile, k, lane);
        while (k < n_views) {
            const int kn = next_view(k + 1);
            ResidualChunk nx = {};
            if (kn < n_views) nx = residual_load_chunk<kExt>(A, tile, kn, lane);
            uint32_t valid;
            const uint32_t out = outliers(cur, valid);
            some |= valid & ~out;
            cur = nx;
            k = kn;
        }
    }

    // sweep 2: the drops, and every kept view's pair as a recount of the chunk would leave it
    uint32_t nd[4] = {0u, 0u, 0u, 0u};
    {
        int k = next_view(0), done = 0;   // the kept views below `done` have their pair
        ResidualChunk cur = {};
        if (k < n_views) cur = residual_load_chunk<kExt>(A, tile, k, lane);
        for (;;) {
            // the views up to the next kept one that reaches the tile (all tests wave-uniform).  A kept view that never reached
            // the tile: nothing stored, nothing left.  A view that is NOT kept keeps its observations, count and bits; only its
            // range pair is restated as its chunk's own -- a matched store keeps a match wave's ranges over several views in the
            // pair of one of them (match.hip), and a dropped range must not stay in the image's span through it
            const int stop = k < n_views ? k : n_views;
            for (int e = done; e < stop; ++e) {
                const size_t pair = (size_t)tile * n_views + e;
                if (A.view_keep[e] != 0u) {
                    if (lane < 4) T.vbits[pair * 4 + lane] = 0ull;
                    if (lane == 0) {
                        T.zrange[pair] = make_uint2(0xffffffffu, 0u);
                        T.tile_view_drop[(size_t)e * A.n_tiles + tile] = 0;
                    }
                } else {
                    uint32_t zlo = 0xffffffffu, zhi = 0u;
                    if (tcnt[e] > 0) {
                        const float4 z4 = *reinterpret_cast<const float4 *>(A.obs + (size_t)tile * A.tile_stride + (size_t)e * A.view_stride + lane * 16);
                        const float zz[4] = {z4.x, z4.y, z4.z, z4.w};
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (zz[j] > 0.0f) { zlo = min(zlo, __float_as_uint(zz[j])); zhi = max(zhi, __float_as_uint(zz[j])); }
#pragma unroll
                        for (int off = 32; off > 0; off >>= 1) { zlo = min(zlo, (uint32_t)__shfl_xor((int)zlo, off, 64)); zhi = max(zhi, (uint32_t)__shfl_xor((int)zhi, off, 64)); }
                    }
                    if (lane == 0) T.zrange[pair] = make_uint2(zlo, zhi);
                }
            }
            if (k >= n_views) break;
            const int kn = next_view(k + 1);
            ResidualChunk nx = {};
            if (kn < n_views) nx = residual_load_chunk<kExt>(A, tile, kn, lane);
            uint32_t valid;
            const uint32_t drop = outliers(cur, valid) & some;   // the guard: a pixel without a survivor keeps everything
            const uint32_t keep = valid & ~drop;
            uint32_t zlo = 0xffffffffu, zhi = 0u;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                nd[j] += (drop >> j) & 1u;
                if ((drop >> j) & 1u) cur.zz[j] = 0.0f;
                if ((keep >> j) & 1u) { zlo = min(zlo, __float_as_uint(cur.zz[j])); zhi = max(zhi, __float_as_uint(cur.zz[j])); }
            }
            if (drop) {
                uint8_t *ch = T.obs + (size_t)tile * A.tile_stride + (size_t)k * A.view_stride;
                *reinterpret_cast<float4 *>(ch + lane * 16) = make_float4(cur.zz[0], cur.zz[1], cur.zz[2], cur.zz[3]);
            }
            const uint32_t left = wave_sum_u32((uint32_t)__builtin_popcount(keep));
            const uint32_t gone = wave_sum_u32((uint32_t)__builtin_popcount(drop));
            // slot 4 lane + j = bit 4 (lane % 16) + j of word lane / 16: the sixteen lanes of a word OR their nibbles together
            uint64_t word = (uint64_t)keep << (4 * (lane & 15));
#pragma unroll
            for (int off = 8; off > 0; off >>= 1) {
                word |= (uint64_t)__shfl_xor((unsigned long long)word, off, 64);
                zlo = min(zlo, (uint32_t)__shfl_xor((int)zlo, off, 64)); zhi = max(zhi, (uint32_t)__shfl_xor((int)zhi, off, 64));
            }
#pragma unroll
            for (int off = 32; off > 8; off >>= 1) { zlo = min(zlo, (uint32_t)__shfl_xor((int)zlo, off, 64)); zhi = max(zhi, (uint32_t)__shfl_xor((int)zhi, off, 64)); }
            const size_t pair = (size_t)tile * n_views + k;
            if ((lane & 15) == 0) T.vbits[pair * 4 + (lane >> 4)] = word;
            if (lane == 0) {
                T.cnt[pair] = (uint16_t)left;
                T.zrange[pair] = make_uint2(zlo, zhi);
                T.tile_view_drop[(size_t)k * A.n_tiles + tile] = (int32_t)gone;
            }
            done = k + 1;
            cur = nx;
            k = kn;
        }
    }

    const int ty = tile / A.tiles_x, tx = tile - ty * A.tiles_x;
    const int v = ty * kTile + (lane >> 2), u0 = tx * kTile + (lane & 3) * 4;
    if (v < A.H) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (u0 + j >= A.W) continue;
            T.dropped[(size_t)v * A.W + (u0 + j)] = (int32_t)nd[j];
        }
    }
}

// trim.hip: what every variant's launcher shares
size_t trim_scratch_bytes(const Layout &L);
TrimArgs trim_args(const Layout &L, uint8_t *ws, const float *tau2, int32_t *dropped, int64_t *view_dropped, void *scratch);
template <class K>
inline void launch_trim_kernel(K kernel, const TrimArgs &T, hipStream_t s) {
    hipLaunchKernelGGL(kernel, dim3((T.R.n_tiles + 3) / 4), dim3(256), 0, s, T);
}
void launch_trim_thresholds(const TrimArgs &T, const double *view_stats, double k2, float *tau2, hipStream_t s);   // before the sweeps
void launch_trim_colour(const TrimArgs &T, hipStream_t s);      // float32 colours, plain water model
void launch_trim_view_sums(const TrimArgs &T, hipStream_t s);   // behind them

}  // namespace sucre

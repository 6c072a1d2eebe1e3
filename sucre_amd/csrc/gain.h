// Per-view gain compensation, the device side (sucre_view_gains*, sucre_apply_view_gains*): one multiplicative gain per kept
// view and channel, estimated at the fit as it stands and divided out of the DENSE store; the caller then finalises again and
// fits anew.
//
//   g = sum I Ihat / sum Ihat^2   over the view's observations,   Ihat = l (J e^(-beta z) + B (1 - e^(-gamma z)))   sucre.py:79-82, 144
//
// -- the least-squares answer to I = g Ihat at fixed J and parameters.
//
// Estimate.  The residual pass's walk (residual.h): one wave per tile, lane l owns slots 4 l .. 4 l + 3, 16-byte loads, the
// lane's J stays in registers across the loop over the views, the next kept view's chunk is loaded before this one is evaluated,
// and I and Ihat of an observation are residual_model's -- the two numbers the residual pass subtracts, so the estimate cannot
// drift from the residual it minimises.  Per (tile, kept view that reaches the tile) a fixed-order tree (handoff.h) reduces
// seven numbers -- n, sum I Ihat R, G, B, sum Ihat^2 R, G, B, float32 FMAs -- and lane 0 writes them (and a zero) to caller-owned
// scratch, view-major; a term whose Ihat is not finite is selected out of both sums.  gain_view_kernel then adds every view's
// tiles in a fixed order in float64 and forms g, clamped to [1 / limit, limit], and float32(1 / g); g = 1 exactly where there is
// nothing to estimate from.  No atomics: two calls give the same bits.
//
// Apply.  The same wave-per-tile walk over the kept views with a match count, without model, J or range format: a slot with
// z > 0 has its three colours multiplied by the view's inv_c -- uint8: min(255, rintf(float(k) inv_c)), the chunk's three colour
// dwords stored back only where they changed; float32 planes: I inv_c, no clamp.  Ranges, counts, pixel bits, range pairs, empty
// slots and views that are not kept are not touched, so the existing finalise pass runs on the store as on a freshly imported
// one.  The uint8 values that met the clamp go per (tile, view) to scratch and through gain_clip_sum_kernel to a per-view count.
#pragma once
#include "trim.h"

namespace sucre {

constexpr int kGainSums = 7;         // n, sum I Ihat [3], sum Ihat^2 [3]
constexpr int kGainPairFloats = 8;   // a (tile, view) pair's seven numbers in scratch: two 16-byte stores

struct GainArgs {
    ResidualArgs R;              // what the walk reads (count, ssr, view_stats: unused; tile_view: two float4 per pair, view-major)
    double limit;
    double *sums;                // (n_views, 7)
    double *gains;               // (n_views, 3)
    float *inv;                  // (n_views, 3)
};

struct GainApplyArgs {
    uint8_t *obs;                // dense store: chunk(tile, k) at tile * tile_stride + k * view_stride
    size_t tile_stride, view_stride;
    const uint16_t *cnt;         // [n_tiles][n_views]
    const uint32_t *view_keep;   // [n_views]
    uint8_t *colour;             // float32 colours: their dense extension planes, float [chunk][3][256]
    const float *inv;            // (n_views, 3)
    int n_tiles, n_views;
    int32_t *tile_view_clip;     // scratch [n_views][n_tiles]: written for every (tile, kept view) pair with a match count
    int64_t *view_clipped;       // [n_views]
};

template <bool kU16, int kExt, class Light>
__global__ __launch_bounds__(256) void gain_sum_kernel(const GainArgs G) {
    static_assert(kExt >= 0 && kExt <= 3 && !(kU16 && kExt), "extension planes ride with the f32 store only");
    const ResidualArgs &A = G.R;
    const int lane = threadIdx.x & 63;
    const int tile = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (tile >= A.n_tiles) return;   // (no barrier below: the wave is on its own)
    const int n_views = A.n_views;
    const ResidualWater water(A.params);
    const Light light(A.geom);

    float J[4][3];
    residual_load_J(A, tile, lane, J);

    const uint16_t *tcnt = A.cnt + (size_t)tile * n_views;
    auto next_view = [&](int k) { while (k < n_views && !(tcnt[k] > 0 && A.view_keep[k] != 0u)) ++k; return k; };   // wave-uniform

    int k = next_view(0);
    ResidualChunk cur = {};
    if (k < n_views) cur = residual_load_chunk<kExt>(A, tile, k, lane);
    while (k < n_views) {
        const int kn = next_view(k + 1);
        ResidualChunk nx = {};
        if (kn < n_views) nx = residual_load_chunk<kExt>(A, tile, kn, lane);
        float vn = 0.0f, sih[3] = {0.0f, 0.0f, 0.0f}, shh[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float I[3], Ihat[3];
            const bool valid = residual_model<kU16, kExt>(cur, j, light, water, J[j], I, Ihat);
            vn += valid ? 1.0f : 0.0f;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const bool use = valid && __builtin_fabsf(Ihat[c]) < __builtin_inff();   // select, not multiply: J may be NaN
                const float h = use ? Ihat[c] : 0.0f, i = use ? I[c] : 0.0f;
                sih[c] = __builtin_fmaf(i, h, sih[c]);
                shh[c] = __builtin_fmaf(h, h, shh[c]);
            }
        }
        const float t0 = wave_sum_lane0(vn), t1 = wave_sum_lane0(sih[0]), t2 = wave_sum_lane0(sih[1]), t3 = wave_sum_lane0(sih[2]);
        const float t4 = wave_sum_lane0(shh[0]), t5 = wave_sum_lane0(shh[1]), t6 = wave_sum_lane0(shh[2]);
        if (lane == 0) {
            float4 *pair = A.tile_view + ((size_t)k * A.n_tiles + tile) * 2;
            pair[0] = make_float4(t0, t1, t2, t3);
            pair[1] = make_float4(t4, t5, t6, 0.0f);
        }
        cur = nx;
        k = kn;
    }
}

template <bool kFloatColour>
__global__ __launch_bounds__(256) void gain_apply_kernel(const GainApplyArgs P) {
    const int lane = threadIdx.x & 63;
    const int tile = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (tile >= P.n_tiles) return;   // (no barrier below: the wave is on its own)
    const int n_views = P.n_views;
    const uint16_t *tcnt = P.cnt + (size_t)tile * n_views;
    for (int k = 0; k < n_views; ++k) {
        if (!(tcnt[k] > 0 && P.view_keep[k] != 0u)) continue;   // (wave-uniform)
        const float inv[3] = {P.inv[k * 3 + 0], P.inv[k * 3 + 1], P.inv[k * 3 + 2]};
        uint8_t *ch = P.obs + (size_t)tile * P.tile_stride + (size_t)k * P.view_stride;
        const float4 z4 = *reinterpret_cast<const float4 *>(ch + lane * 16);
        const float zz[4] = {z4.x, z4.y, z4.z, z4.w};
        uint32_t clipped = 0u;
        if (kFloatColour) {
            uint8_t *planes = P.colour + ((size_t)tile * n_views + k) * kExtChunk;
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) {
                float4 *at = reinterpret_cast<float4 *>(planes + (size_t)(pl * kTilePx + lane * 4) * sizeof(float));
                const float4 v = *at;
                const float was[4] = {v.x, v.y, v.z, v.w};
                float now[4];
                bool changed = false;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    now[j] = zz[j] > 0.0f ? was[j] * inv[pl] : was[j];   // an empty slot keeps what it holds
                    changed |= __float_as_uint(now[j]) != __float_as_uint(was[j]);
                }
                if (changed) *at = make_float4(now[0], now[1], now[2], now[3]);
            }
        } else {
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) {
                uint32_t *at = reinterpret_cast<uint32_t *>(ch + kChunkZ + pl * kTilePx + lane * 4);
                const uint32_t was = *at;
                uint32_t now = was;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (!(zz[j] > 0.0f)) continue;
                    const float x = rintf((float)((was >> (8 * j)) & 255u) * inv[pl]);   // one rounded multiply, then half to even
                    clipped += x > 255.0f ? 1u : 0u;
                    const uint32_t b = (uint32_t)fminf(fmaxf(x, 0.0f), 255.0f);          // (a NaN or a negative inv: 0)
                    now = (now & ~(255u << (8 * j))) | (b << (8 * j));
                }
                if (now != was) *at = now;
            }
        }
        const uint32_t total = wave_sum_u32(clipped);
        if (lane == 0) P.tile_view_clip[(size_t)k * P.n_tiles + tile] = (int32_t)total;
    }
}

// gain.hip: what every variant's launcher shares
size_t gain_scratch_bytes(const Layout &L);
GainArgs gain_args(const Layout &L, const uint8_t *ws, double limit, double *gains, float *inv, double *sums, void *scratch);
GainApplyArgs gain_apply_args(const Layout &L, uint8_t *ws, uint8_t *colour, const float *inv, int64_t *view_clipped, void *scratch);
template <class K>
inline void launch_gain_kernel(K kernel, const GainArgs &G, hipStream_t s) {
    hipLaunchKernelGGL(kernel, dim3((G.R.n_tiles + 3) / 4), dim3(256), 0, s, G);
}
void launch_gain_colour(const GainArgs &G, hipStream_t s);      // float32 colours, plain water model
void launch_gain_view_sums(const GainArgs &G, hipStream_t s);   // the second kernel: tiles of every view, float64, then g
hipError_t launch_gain_apply(const GainApplyArgs &P, hipStream_t s);   // both kernels of the apply: P.colour decides the variant

}  // namespace sucre

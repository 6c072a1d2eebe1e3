// Fit residuals per pixel and per view (sucre_fit_residuals*): the one skeleton all variants are instantiated from.
//
//   r = I - l (J e^(-beta z) + B (1 - e^(-gamma z)))      sucre.py:79-82, 144 (l, z: sucre.py:52-64)
//
// One streaming pass over the DENSE store of a matched, finalised and fitted workspace, at the workspace's current parameters
// and current J (read through invperm from the strip state, as export_J_kernel does).  One wave per tile; lane l owns the four
// consecutive slots 4 l .. 4 l + 3 (one row of the tile: row l / 4, columns 4 (l % 4) ..), so a view costs it one 16-byte load
// of ranges and three colour dwords (float32 extension planes: one 16-byte load per plane).  The per-pixel sums stay in the
// owning lane across the loop over the views; the test "view kept and seen in this tile" is wave-uniform; the next view's chunk
// is loaded before this one is evaluated.  Per (tile, view) a fixed-order tree (handoff.h) reduces {n, sum r^2 R, G, B} and lane
// 0 writes them to caller-owned scratch, view-major; residual_view_sum_kernel then adds every view's tiles in a fixed order in
// float64.  No atomics: two calls give the same bits.  Plain loads, no LDS-DMA ring: the pass runs once per image, not per
// iteration.
//
// Variants (template arguments, chosen at launch):
//   kU16   the store was finalised with SUCRE_OBS_U16MM: the range is the one that store's fit reads,
//          0.001f * clamp(rintf(1000 z), 1, 65535) (compact.hip range_mm, fit.hip read_chunk);
//   kExt   0, or what the dense extension planes carry (SUCRE_EXT_*): float32 colours (bit 1) and / or camera points (bit 0);
//   Light  NoLight (l = 1, z = the stored range) or light.hip's model: l and z from cP through light_obs.
#pragma once
#include "fit_math.h"
#include "handoff.h"

namespace sucre {

// head of the scratch buffer: the light variants' geometry of the CURRENT parameters (float [16]: R, t, Sigma^-1) and, behind it,
// the twists light_geometry leaves with it (double [72]) -- derived into scratch so that neither workspace is written
constexpr size_t kResidualGeomBytes = 1024;

struct ResidualArgs {
    const uint8_t *obs;          // dense store: chunk(tile, k) at tile * tile_stride + k * view_stride
    size_t tile_stride, view_stride;
    const uint16_t *cnt;         // [n_tiles][n_views]
    const uint32_t *view_keep;   // [n_views]
    const uint32_t *invperm;     // dense slot -> sorted slot
    const float *state;          // J planes of the strips
    const float *params;         // B[3], beta[3], gamma[3]
    const float *geom;           // light variants: R[9], t[3], Sigma^-1[4]
    const uint8_t *ext, *ext2;   // dense extension planes: float [chunk][3][256]
    int H, W, tiles_x, n_tiles, n_views;
    int32_t *count;              // (H, W)
    float *ssr;                  // (H, W, 3)
    float4 *tile_view;           // scratch [n_views][n_tiles]: n, sum r^2 R, G, B of the tile's observations in the view
    double *view_stats;          // (n_views, 4)
};

struct NoLight {
    __device__ __forceinline__ explicit NoLight(const float *) {}
    __device__ __forceinline__ void lz(const float (&)[3], float zc, float &l, float &z) const { l = 1.0f; z = zc; }
};

struct ResidualChunk { float zz[4]; uint32_t cc[3]; float p[3][4], f[3][4]; };   // ranges, colour words, extension planes (sets 1, 2)

// The pieces of the walk that the outlier trim (trim.h) shares with the residual pass, so that its decisions are made from the
// very numbers the residuals are: the lane's J, the lane's share of a chunk, one observation's residual.

// the current J of the lane's four pixels, where the fit keeps it
__device__ __forceinline__ void residual_load_J(const ResidualArgs &A, int tile, int lane, float (&J)[4][3]) {
    const uint4 d4 = *reinterpret_cast<const uint4 *>(A.invperm + (size_t)tile * kTilePx + lane * 4);
    const uint32_t d[4] = {d4.x, d4.y, d4.z, d4.w};
    const uint32_t last = (uint32_t)A.n_tiles * kTilePx - 1u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t dst = min(d[j], last);   // (a workspace that was never finalised holds anything here)
        const float *st = A.state + (size_t)(dst / kStripPx) * kStateFloats + dst % kStripPx;
#pragma unroll
        for (int c = 0; c < 3; ++c) J[j][c] = st[c * kStripPx];
    }
}

// the lane's slots 4 lane .. 4 lane + 3 of chunk (tile, k)
template <int kExt>
__device__ __forceinline__ ResidualChunk residual_load_chunk(const ResidualArgs &A, int tile, int k, int lane) {
    constexpr bool kPoints = (kExt & 1) != 0, kFloatColour = (kExt & 2) != 0;
    ResidualChunk q;
    const uint8_t *ch = A.obs + (size_t)tile * A.tile_stride + (size_t)k * A.view_stride;
    const float4 z4 = *reinterpret_cast<const float4 *>(ch + lane * 16);
    q.zz[0] = z4.x; q.zz[1] = z4.y; q.zz[2] = z4.z; q.zz[3] = z4.w;
    if (!kFloatColour) {
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) q.cc[pl] = *reinterpret_cast<const uint32_t *>(ch + kChunkZ + pl * kTilePx + lane * 4);
    }
    if (kExt) {
        const size_t eo = ((size_t)tile * A.n_views + k) * kExtChunk;
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) {
            const float4 v = *reinterpret_cast<const float4 *>(A.ext + eo + (size_t)(pl * kTilePx + lane * 4) * sizeof(float));
            q.p[pl][0] = v.x; q.p[pl][1] = v.y; q.p[pl][2] = v.z; q.p[pl][3] = v.w;
        }
        if (kPoints && kFloatColour) {
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) {
                const float4 v = *reinterpret_cast<const float4 *>(A.ext2 + eo + (size_t)(pl * kTilePx + lane * 4) * sizeof(float));
                q.f[pl][0] = v.x; q.f[pl][1] = v.y; q.f[pl][2] = v.z; q.f[pl][3] = v.w;
            }
        }
    }
    return q;
}

// water parameters as the evaluation reads them: B, -beta log2 e, -gamma log2 e
struct ResidualWater {
    float B[3], nb[3], ng[3];
    __device__ __forceinline__ explicit ResidualWater(const float *params) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { B[c] = params[c]; nb[c] = -params[3 + c] * kLog2e; ng[c] = -params[6 + c] * kLog2e; }
    }
};

// The two numbers a residual is the difference of, for the lane's slot j of the chunk: the observed I[c] and the modelled
// Ihat[c] -- whatever the slot holds, also where it is empty (the callers select).  Returns whether the slot holds an
// observation.  residual_obs subtracts the two; the gain pass (gain.h) sums their products, from the very same numbers.
template <bool kU16, int kExt, class Light>
__device__ __forceinline__ bool residual_model(const ResidualChunk &cur, int j, const Light &light, const ResidualWater &w,
                                               const float (&J)[3], float (&I)[3], float (&Ihat)[3]) {
    constexpr bool kPoints = (kExt & 1) != 0, kFloatColour = (kExt & 2) != 0;
    const bool valid = cur.zz[j] > 0.0f;   // an empty slot holds range 0
    float zc = cur.zz[j];
    if (kU16) zc = kMPerMm * fminf(fmaxf(rintf(zc * kMmPerM), 1.0f), 65535.0f);
    const float cP[3] = {kPoints ? cur.p[0][j] : 0.0f, kPoints ? cur.p[1][j] : 0.0f, kPoints ? cur.p[2][j] : 0.0f};
    float l, z;
    light.lz(cP, zc, l, z);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float a = fast_exp2(z * w.nb[c]), g = fast_exp2(z * w.ng[c]);
        float m = __builtin_fmaf(J[c], a, w.B[c] * (1.0f - g));
        if (kPoints) m = l * m;
        Ihat[c] = m;
        I[c] = kFloatColour ? (kPoints ? cur.f[c][j] : cur.p[c][j]) : unit_from_u8((cur.cc[c] >> (8 * j)) & 255u);
    }
    return valid;
}

// r[c] of the lane's slot j of the chunk (0 for an empty slot); returns whether the slot holds an observation
template <bool kU16, int kExt, class Light>
__device__ __forceinline__ bool residual_obs(const ResidualChunk &cur, int j, const Light &light, const ResidualWater &w,
                                             const float (&J)[3], float (&r)[3]) {
    float I[3], Ihat[3];
    const bool valid = residual_model<kU16, kExt>(cur, j, light, w, J, I, Ihat);
#pragma unroll
    for (int c = 0; c < 3; ++c) r[c] = valid ? I[c] - Ihat[c] : 0.0f;   // select, not multiply: J may be NaN where nothing is observed
    return valid;
}

template <bool kU16, int kExt, class Light>
__global__ __launch_bounds__(256) void residual_kernel(const ResidualArgs A) {
    static_assert(kExt >= 0 && kExt <= 3 && !(kU16 && kExt), "extension planes ride with the f32 store only");
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

    float ssr[4][3], pn[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { pn[j] = 0.0f; ssr[j][0] = ssr[j][1] = ssr[j][2] = 0.0f; }

    int k = next_view(0);
    ResidualChunk cur = {};
    if (k < n_views) cur = residual_load_chunk<kExt>(A, tile, k, lane);
    while (k < n_views) {
        const int kn = next_view(k + 1);
        ResidualChunk nx = {};
        if (kn < n_views) nx = residual_load_chunk<kExt>(A, tile, kn, lane);
        float vn = 0.0f, vs[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float r[3];
            const bool valid = residual_obs<kU16, kExt>(cur, j, light, water, J[j], r);
            const float one = valid ? 1.0f : 0.0f;
            pn[j] += one;
            vn += one;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                ssr[j][c] = __builtin_fmaf(r[c], r[c], ssr[j][c]);
                vs[c] = __builtin_fmaf(r[c], r[c], vs[c]);
            }
        }
        const float t0 = wave_sum_lane0(vn), t1 = wave_sum_lane0(vs[0]), t2 = wave_sum_lane0(vs[1]), t3 = wave_sum_lane0(vs[2]);
        if (lane == 0) A.tile_view[(size_t)k * A.n_tiles + tile] = make_float4(t0, t1, t2, t3);
        cur = nx;
        k = kn;
    }

    const int ty = tile / A.tiles_x, tx = tile - ty * A.tiles_x;
    const int v = ty * kTile + (lane >> 2), u0 = tx * kTile + (lane & 3) * 4;
    if (v < A.H) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (u0 + j >= A.W) continue;
            const size_t o = (size_t)v * A.W + (u0 + j);
            A.count[o] = (int32_t)pn[j];
#pragma unroll
            for (int c = 0; c < 3; ++c) A.ssr[o * 3 + c] = ssr[j][c];
        }
    }
}

// residual.hip: what every variant's launcher shares
ResidualArgs residual_args(const Layout &L, const uint8_t *ws, int32_t *count, float *ssr, double *view_stats, void *scratch);
template <class K>
inline void launch_residual_kernel(K kernel, const ResidualArgs &A, hipStream_t s) {
    hipLaunchKernelGGL(kernel, dim3((A.n_tiles + 3) / 4), dim3(256), 0, s, A);
}
void launch_residual_colour(const ResidualArgs &A, hipStream_t s);      // float32 colours, plain water model
void launch_residual_view_sums(const ResidualArgs &A, hipStream_t s);   // the second kernel: tiles of every view, float64

}  // namespace sucre

// Per-view gain compensation for gfx950 (sucre_view_gains*, sucre_apply_view_gains*; the kernels and their description:
// gain.h).  This file holds the estimate's variants without a light model, the two small kernels behind the passes, the apply
// (which needs no model) and what the launchers share; the light-model variants of the estimate sit next to light_obs in
// light.hip, as the residual pass's do.
#include "gain.h"

namespace sucre {

// View k's seven sums: its tiles added in a fixed order in float64 (thread t takes tiles t, t + 256, ...; a fixed-shape tree; the
// four waves in order), then its gains.  A view that is not kept, or a tile the view does not reach, was never written to
// scratch: the same two tests as in the pass decide what is read.  g = 1 and inv = 1 exactly where there is nothing to estimate
// from -- the view is not kept (its sums are zeros), n = 0, sum Ihat^2 or the quotient not finite and positive; otherwise g is
// clamped to [1 / limit, limit] and inv = float32(1 / g).  One workgroup per view.
__global__ __launch_bounds__(256) void gain_view_kernel(const GainArgs G) {
    __shared__ double w4[kGainSums][4];
    __shared__ double total[kGainSums];
    const ResidualArgs &A = G.R;
    const int k = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    double x[kGainSums];
#pragma unroll
    for (int q = 0; q < kGainSums; ++q) x[q] = 0.0;
    if (A.view_keep[k] != 0u) {   // (workgroup-uniform)
        for (int tile = t; tile < A.n_tiles; tile += 256) {
            if (A.cnt[(size_t)tile * A.n_views + k] == 0) continue;
            const float4 *pair = A.tile_view + ((size_t)k * A.n_tiles + tile) * 2;
            const float4 a = pair[0], b = pair[1];
            x[0] += (double)a.x; x[1] += (double)a.y; x[2] += (double)a.z; x[3] += (double)a.w;
            x[4] += (double)b.x; x[5] += (double)b.y; x[6] += (double)b.z;
        }
    }
#pragma unroll
    for (int q = 0; q < kGainSums; ++q) {
        const double y = wave_sum_lane0(x[q]);
        if (lane == 0) w4[q][wave] = y;
    }
    __syncthreads();
    if (t < kGainSums) {
        const double y = ((w4[t][0] + w4[t][1]) + w4[t][2]) + w4[t][3];
        total[t] = y;
        G.sums[(size_t)k * kGainSums + t] = y;
    }
    __syncthreads();
    if (t < 3) {
        const double n = total[0], sih = total[1 + t], shh = total[4 + t];
        double g = 1.0;
        if (n > 0.0 && shh > 0.0 && shh < (double)__builtin_inff()) {
            const double q = sih / shh;
            if (q > 0.0 && q < (double)__builtin_inff()) g = fmin(fmax(q, 1.0 / G.limit), G.limit);
        }
        G.gains[(size_t)k * 3 + t] = g;
        G.inv[(size_t)k * 3 + t] = (float)(1.0 / g);
    }
}

// view k's clamped values: its tiles' counts added up (thread t takes tiles t, t + 256, ...); 0 for a view that is not kept and
// for a tile the view does not reach, which the apply never wrote.  One workgroup per view.
__global__ __launch_bounds__(256) void gain_clip_sum_kernel(const GainApplyArgs P) {
    __shared__ long long w4[4];
    const int k = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    long long x = 0;
    if (P.view_keep[k] != 0u)   // (workgroup-uniform)
        for (int tile = t; tile < P.n_tiles; tile += 256)
            if (P.cnt[(size_t)tile * P.n_views + k] != 0) x += P.tile_view_clip[(size_t)k * P.n_tiles + tile];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
    if (lane == 0) w4[wave] = x;
    __syncthreads();
    if (t == 0) P.view_clipped[k] = (int64_t)(w4[0] + w4[1] + w4[2] + w4[3]);
}

// one buffer serves both passes: the estimate's eight floats per (tile, view) pair; the apply's count per pair uses its head
size_t gain_scratch_bytes(const Layout &L) {
    return kResidualGeomBytes + (size_t)L.n_tiles * L.n_views * kGainPairFloats * sizeof(float);
}

GainArgs gain_args(const Layout &L, const uint8_t *ws, double limit, double *gains, float *inv, double *sums, void *scratch) {
    GainArgs G = {};
    G.R = residual_args(L, ws, nullptr, nullptr, nullptr, scratch);
    G.limit = limit;
    G.sums = sums; G.gains = gains; G.inv = inv;
    return G;
}

GainApplyArgs gain_apply_args(const Layout &L, uint8_t *ws, uint8_t *colour, const float *inv, int64_t *view_clipped, void *scratch) {
    GainApplyArgs P = {};
    P.obs = ws + L.off_obs;
    P.tile_stride = L.obs_tile_stride; P.view_stride = L.obs_view_stride;
    P.cnt = reinterpret_cast<const uint16_t *>(ws + L.off_cnt);
    P.view_keep = reinterpret_cast<const uint32_t *>(ws + L.off_view_keep);
    P.colour = colour;
    P.inv = inv;
    P.n_tiles = L.n_tiles; P.n_views = L.n_views;
    P.tile_view_clip = reinterpret_cast<int32_t *>(static_cast<uint8_t *>(scratch) + kResidualGeomBytes);
    P.view_clipped = view_clipped;
    return P;
}

void launch_gain_view_sums(const GainArgs &G, hipStream_t s) {
    hipLaunchKernelGGL(gain_view_kernel, dim3(G.R.n_views), dim3(256), 0, s, G);
}

void launch_gain_colour(const GainArgs &G, hipStream_t s) {
    launch_gain_kernel(gain_sum_kernel<false, SUCRE_EXT_COLOUR, NoLight>, G, s);
}

hipError_t launch_view_gains(const Layout &L, const uint8_t *ws, int fmt, double limit, double *gains, float *inv, double *sums,
                             void *scratch, hipStream_t s) {
    const GainArgs G = gain_args(L, ws, limit, gains, inv, sums, scratch);
    if (fmt == SUCRE_OBS_U16MM) launch_gain_kernel(gain_sum_kernel<true, 0, NoLight>, G, s);
    else launch_gain_kernel(gain_sum_kernel<false, 0, NoLight>, G, s);
    launch_gain_view_sums(G, s);
    return hipGetLastError();
}

hipError_t launch_gain_apply(const GainApplyArgs &P, hipStream_t s) {
    const dim3 grid((P.n_tiles + 3) / 4);
    if (P.colour) hipLaunchKernelGGL(gain_apply_kernel<true>, grid, dim3(256), 0, s, P);
    else hipLaunchKernelGGL(gain_apply_kernel<false>, grid, dim3(256), 0, s, P);
    hipLaunchKernelGGL(gain_clip_sum_kernel, dim3(P.n_views), dim3(256), 0, s, P);
    return hipGetLastError();
}

hipError_t launch_apply_view_gains(const Layout &L, uint8_t *ws, const float *inv, int64_t *view_clipped, void *scratch, hipStream_t s) {
    return launch_gain_apply(gain_apply_args(L, ws, nullptr, inv, view_clipped, scratch), s);
}

}  // namespace sucre

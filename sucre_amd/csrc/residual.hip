// Per-pixel and per-view fit residuals for gfx950 (sucre_fit_residuals*; the skeleton and its description: residual.h).
// This file holds the variants without a light model -- uint8 colours with float32 or millimetre ranges, float32 colours -- the
// second kernel and what the launchers share; the light-model variants sit next to light_obs in light.hip.
#include "residual.h"

namespace sucre {

// view k's row of the table: its tiles added in a fixed order in float64 (thread t takes tiles t, t + 256, ...; a fixed-shape
// tree; the four waves in order).  A view that is not kept, or a tile the view does not reach, was never written to scratch:
// the same two tests as in the pass decide what is read.  One workgroup per view.
__global__ __launch_bounds__(256) void residual_view_sum_kernel(const ResidualArgs A) {
    __shared__ double w4[4][4];
    const int k = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    double x[4] = {0.0, 0.0, 0.0, 0.0};
    if (A.view_keep[k] != 0u) {   // (workgroup-uniform)
        for (int tile = t; tile < A.n_tiles; tile += 256) {
            if (A.cnt[(size_t)tile * A.n_views + k] == 0) continue;
            const float4 q = A.tile_view[(size_t)k * A.n_tiles + tile];
            x[0] += (double)q.x; x[1] += (double)q.y; x[2] += (double)q.z; x[3] += (double)q.w;
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const double y = wave_sum_lane0(x[q]);
        if (lane == 0) w4[q][wave] = y;
    }
    __syncthreads();
    if (t < 4) A.view_stats[(size_t)k * 4 + t] = ((w4[t][0] + w4[t][1]) + w4[t][2]) + w4[t][3];
}

size_t residual_scratch_bytes(const Layout &L) {
    return kResidualGeomBytes + (size_t)L.n_tiles * L.n_views * sizeof(float4);
}

ResidualArgs residual_args(const Layout &L, const uint8_t *ws, int32_t *count, float *ssr, double *view_stats, void *scratch) {
    ResidualArgs A = {};
    A.obs = ws + L.off_obs;
    A.tile_stride = L.obs_tile_stride; A.view_stride = L.obs_view_stride;
    A.cnt = reinterpret_cast<const uint16_t *>(ws + L.off_cnt);
    A.view_keep = reinterpret_cast<const uint32_t *>(ws + L.off_view_keep);
    A.invperm = reinterpret_cast<const uint32_t *>(ws + L.off_invperm);
    A.state = reinterpret_cast<const float *>(ws + L.off_state);
    A.params = reinterpret_cast<const float *>(ws + L.off_params);
    A.H = L.H; A.W = L.W; A.tiles_x = L.tiles_x; A.n_tiles = L.n_tiles; A.n_views = L.n_views;
    A.count = count; A.ssr = ssr; A.view_stats = view_stats;
    A.tile_view = reinterpret_cast<float4 *>(static_cast<uint8_t *>(scratch) + kResidualGeomBytes);
    return A;
}

void launch_residual_view_sums(const ResidualArgs &A, hipStream_t s) {
    hipLaunchKernelGGL(residual_view_sum_kernel, dim3(A.n_views), dim3(256), 0, s, A);
}

void launch_residual_colour(const ResidualArgs &A, hipStream_t s) {
    launch_residual_kernel(residual_kernel<false, SUCRE_EXT_COLOUR, NoLight>, A, s);
}

hipError_t launch_residuals(const Layout &L, const uint8_t *ws, int fmt, int32_t *count, float *ssr, double *view_stats,
                            void *scratch, hipStream_t s) {
    const ResidualArgs A = residual_args(L, ws, count, ssr, view_stats, scratch);
    if (fmt == SUCRE_OBS_U16MM) launch_residual_kernel(residual_kernel<true, 0, NoLight>, A, s);
    else launch_residual_kernel(residual_kernel<false, 0, NoLight>, A, s);
    launch_residual_view_sums(A, s);
    return hipGetLastError();
}

}  // namespace sucre

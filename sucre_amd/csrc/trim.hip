// Outlier-trimmed refit for gfx950 (sucre_trim_outliers*; the sweeps and their description: trim.h).  This file holds the
// variants without a light model, the two small kernels around the sweeps and what the launchers share; the light-model
// variants sit next to light_obs in light.hip, as the residual pass's do.
#include "trim.h"

namespace sucre {

// tau^2_c = float32(k^2 S_c / N) over the kept views' rows of the residual pass's table, added in view order in float64 (thread
// q walks column q; views that are not kept hold zeros there, and are skipped all the same).  N = 0: nothing can be dropped --
// +inf, which no r^2 exceeds.  One workgroup.
__global__ __launch_bounds__(64) void trim_threshold_kernel(const double *__restrict__ view_stats, const uint32_t *__restrict__ view_keep,
                                                            int n_views, double k2, float *__restrict__ tau2) {
    __shared__ double sum[4];
    const int q = threadIdx.x;
    if (q < 4) {
        double x = 0.0;
        for (int k = 0; k < n_views; ++k)
            if (view_keep[k] != 0u) x += view_stats[(size_t)k * 4 + q];
        sum[q] = x;
    }
    __syncthreads();
    if (q < 3) tau2[q] = sum[0] > 0.0 ? (float)(k2 * sum[1 + q] / sum[0]) : __builtin_inff();
}

// view k's drops: its tiles' counts added up (thread t takes tiles t, t + 256, ...); 0 for a view that is not kept, whose
// tiles the sweeps never wrote.  One workgroup per view.
__global__ __launch_bounds__(256) void trim_view_sum_kernel(const TrimArgs T) {
    __shared__ long long w4[4];
    const int k = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    long long x = 0;
    if (T.R.view_keep[k] != 0u)   // (workgroup-uniform)
        for (int tile = t; tile < T.R.n_tiles; tile += 256) x += T.tile_view_drop[(size_t)k * T.R.n_tiles + tile];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
    if (lane == 0) w4[wave] = x;
    __syncthreads();
    if (t == 0) T.view_dropped[k] = (int64_t)(w4[0] + w4[1] + w4[2] + w4[3]);
}

size_t trim_scratch_bytes(const Layout &L) {
    return kResidualGeomBytes + align_up((size_t)L.n_tiles * L.n_views * sizeof(int32_t), 256);
}

TrimArgs trim_args(const Layout &L, uint8_t *ws, const float *tau2, int32_t *dropped, int64_t *view_dropped, void *scratch) {
    TrimArgs T = {};
    T.R = residual_args(L, ws, nullptr, nullptr, nullptr, scratch);
    T.R.tile_view = nullptr;
    T.obs = ws + L.off_obs;
    T.cnt = reinterpret_cast<uint16_t *>(ws + L.off_cnt);
    T.vbits = reinterpret_cast<uint64_t *>(ws + L.off_vbits);
    T.zrange = reinterpret_cast<uint2 *>(ws + L.off_zrange);
    T.tau2 = tau2;
    T.dropped = dropped;
    T.view_dropped = view_dropped;
    T.tile_view_drop = reinterpret_cast<int32_t *>(static_cast<uint8_t *>(scratch) + kResidualGeomBytes);
    return T;
}

void launch_trim_thresholds(const TrimArgs &T, const double *view_stats, double k2, float *tau2, hipStream_t s) {
    hipLaunchKernelGGL(trim_threshold_kernel, dim3(1), dim3(64), 0, s, view_stats, T.R.view_keep, T.R.n_views, k2, tau2);
}

void launch_trim_view_sums(const TrimArgs &T, hipStream_t s) {
    hipLaunchKernelGGL(trim_view_sum_kernel, dim3(T.R.n_views), dim3(256), 0, s, T);
}

void launch_trim_colour(const TrimArgs &T, hipStream_t s) {
    launch_trim_kernel(trim_kernel<false, SUCRE_EXT_COLOUR, NoLight>, T, s);
}

hipError_t launch_trim(const Layout &L, uint8_t *ws, int fmt, double k_sigma, const double *view_stats, int32_t *dropped,
                       int64_t *view_dropped, float *tau2, void *scratch, hipStream_t s) {
    const TrimArgs T = trim_args(L, ws, tau2, dropped, view_dropped, scratch);
    launch_trim_thresholds(T, view_stats, k_sigma * k_sigma, tau2, s);
    if (fmt == SUCRE_OBS_U16MM) launch_trim_kernel(trim_kernel<true, 0, NoLight>, T, s);
    else launch_trim_kernel(trim_kernel<false, 0, NoLight>, T, s);
    launch_trim_view_sums(T, s);
    return hipGetLastError();
}

}  // namespace sucre

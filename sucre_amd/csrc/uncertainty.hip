// Standard errors of the water parameters and of J for gfx950 (sucre_fit_uncertainty*; the kernel and its description:
// uncertainty.h).  This file holds the second kernel and the launchers: uint8 colours with float32 or millimetre ranges, and
// float32 colours from the dense extension planes.
#include "uncertainty.h"

namespace sucre {

// word q of the sums: the tiles added in a fixed order in float64 (thread t takes tiles t, t + 256, ...; a fixed-shape tree; the
// four waves in order).  Every tile wrote its 24 words, a tile without a kept view zeros.  One workgroup per word.
__global__ __launch_bounds__(256) void uncertainty_sum_kernel(const UncertaintyArgs U) {
    __shared__ double w4[4];
    const int q = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int n_tiles = U.R.n_tiles;
    const double *row = U.tile_sums + (size_t)q * n_tiles;
    double x = 0.0;
    for (int tile = t; tile < n_tiles; tile += 256) x += row[tile];
    const double y = wave_sum_lane0(x);
    if (lane == 0) w4[wave] = y;
    __syncthreads();
    if (t == 0) U.sums[q] = ((w4[0] + w4[1]) + w4[2]) + w4[3];
}

size_t uncertainty_scratch_bytes(const Layout &L) {
    return (size_t)kUncertaintyWords * L.n_tiles * sizeof(double);
}

static UncertaintyArgs uncertainty_args(const Layout &L, const uint8_t *ws, int32_t *count, float *jterms, double *sums, void *scratch) {
    UncertaintyArgs U = {};
    U.R = residual_args(L, ws, count, nullptr, nullptr, scratch);
    U.R.tile_view = nullptr;
    U.jterms = reinterpret_cast<float4 *>(jterms);
    U.tile_sums = static_cast<double *>(scratch);
    U.sums = sums;
    return U;
}

template <class K>
static void launch_uncertainty_kernels(K kernel, const UncertaintyArgs &U, hipStream_t s) {
    hipLaunchKernelGGL(kernel, dim3((U.R.n_tiles + 3) / 4), dim3(256), 0, s, U);
    hipLaunchKernelGGL(uncertainty_sum_kernel, dim3(kUncertaintyWords), dim3(256), 0, s, U);
}

hipError_t launch_uncertainty(const Layout &L, const uint8_t *ws, int fmt, int32_t *count, float *jterms, double *sums, void *scratch,
                              hipStream_t s) {
    const UncertaintyArgs U = uncertainty_args(L, ws, count, jterms, sums, scratch);
    if (fmt == SUCRE_OBS_U16MM) launch_uncertainty_kernels(uncertainty_kernel<true, 0>, U, s);
    else launch_uncertainty_kernels(uncertainty_kernel<false, 0>, U, s);
    return hipGetLastError();
}

// float32 colours, plain water model: its nine parameters are the first nine of `lws`, the colours its dense extension planes
hipError_t launch_uncertainty_colour(const Layout &L, const uint8_t *ws, const uint8_t *lws, int32_t *count, float *jterms, double *sums,
                                     void *scratch, hipStream_t s) {
    UncertaintyArgs U = uncertainty_args(L, ws, count, jterms, sums, scratch);
    U.R.params = reinterpret_cast<const float *>(lws + light_params_offset(L));
    U.R.ext = light_ext_dense(L, const_cast<uint8_t *>(lws));
    launch_uncertainty_kernels(uncertainty_kernel<false, SUCRE_EXT_COLOUR>, U, s);
    return hipGetLastError();
}

}  // namespace sucre

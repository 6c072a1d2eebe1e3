// Multi-band blend of the seabed mosaic for gfx950 (sucre_mosaic_band_*; the description: bands.h).
#include "bands.h"
#include "match_pixel.h"

namespace sucre {

// One tap of the filter: a (three channels) and m of bands.h.  A tap outside the image is not read.
struct BandTap {
    float a[3];
    int m;
};

// kFirst: the tap forms S_0 from the image's depth and J; otherwise it reads S (the image's block of S_in), a NaN marking a non-member.
template <bool kFirst>
__device__ __forceinline__ BandTap band_tap(const MosaicImage *__restrict__ im, const float *__restrict__ S, int u, int v, int W, int H) {
    BandTap t = {{0.0f, 0.0f, 0.0f}, 0};
    if (u < 0 || u >= W || v < 0 || v >= H) return t;
    const size_t q = (size_t)v * (size_t)W + (size_t)u;
    float x0, x1, x2;
    bool in;
    if constexpr (kFirst) {
        const float d = global_ptr(im->depth)[q];
        const auto *pj = global_ptr(im->J) + q * 3;
        x0 = pj[0]; x1 = pj[1]; x2 = pj[2];
        in = mosaic_member(d, x0, x1, x2);
        x0 = fminf(fmaxf(x0, -1024.0f), 1024.0f);
        x1 = fminf(fmaxf(x1, -1024.0f), 1024.0f);
        x2 = fminf(fmaxf(x2, -1024.0f), 1024.0f);
    } else {
        const auto *ps = global_ptr(S) + q * 3;
        x0 = ps[0]; x1 = ps[1]; x2 = ps[2];
        in = x0 == x0 && x1 == x1 && x2 == x2;
    }
    if (in) { t.a[0] = x0; t.a[1] = x1; t.a[2] = x2; t.m = 1; }
    return t;
}

// One lane per pixel on the walk's row segments; S_in, S_out and D_out point at the launch's first pixel.
template <bool kFirst>
__global__ __launch_bounds__(256) void band_split_kernel(const MosaicImage *__restrict__ table, int n_images, int s,
                                                         const float *__restrict__ S_in, float *__restrict__ S_out,
                                                         float *__restrict__ D_out) {
    const MosaicImage *__restrict__ im = mosaic_block_image(table, n_images);
    const int W = im->W, H = im->H;
    const uint32_t n_px = (uint32_t)H * (uint32_t)W;   // H, W <= 32767: below 2^30
    const uint32_t p = (blockIdx.x - im->block0) * kMosaicBlockPx + threadIdx.x;
    if (p >= n_px) return;
    const int v = (int)(p / (uint32_t)W), u = (int)(p - (uint32_t)v * (uint32_t)W);
    const size_t image0 = (size_t)im->block0 * kMosaicBlockPx * 3;
    const float *__restrict__ Si = kFirst ? nullptr : S_in + image0;

    float nh[3][3];
    int ah[3];
    BandTap centre = {};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const int vv = v + (r - 1) * s;
        const BandTap l = band_tap<kFirst>(im, Si, u - s, vv, W, H), c = band_tap<kFirst>(im, Si, u, vv, W, H),
                      g = band_tap<kFirst>(im, Si, u + s, vv, W, H);
#pragma unroll
        for (int k = 0; k < 3; ++k) nh[r][k] = (l.a[k] + 2.0f * c.a[k]) + g.a[k];
        ah[r] = (l.m + 2 * c.m) + g.m;
        if (r == 1) centre = c;
    }
    const int A = (ah[0] + 2 * ah[1]) + ah[2];
    const size_t o = image0 + (size_t)p * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float next = __uint_as_float(0x7fc00000u), detail = next;
        if (centre.m) {
            const float N = (nh[0][k] + 2.0f * nh[1][k]) + nh[2][k];
            next = N / (float)A;   // a member has A >= 4
            detail = centre.a[k] - next;
        }
        S_out[o + k] = next;
        D_out[o + k] = detail;
    }
}

// One lane per cell: the blended bands of a filled cell, coarse to fine; an empty cell's output is not touched.
__global__ __launch_bounds__(256) void band_combine_kernel(size_t n_cells, int n_bands, const long long *__restrict__ acc,
                                                           float *__restrict__ J_out) {
    const size_t cell = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (cell >= n_cells) return;
    const long long *a = acc + ((size_t)(n_bands - 1) * n_cells + cell) * kMosaicAccWords;
    if (a[7] <= 0) return;
    float sum[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) sum[c] = mosaic_quotient(a[c], a[6]);
    for (int j = n_bands - 2; j >= 0; --j) {
        a = acc + ((size_t)j * n_cells + cell) * kMosaicAccWords;
        const long long wsum = a[6];
#pragma unroll
        for (int c = 0; c < 3; ++c) sum[c] = sum[c] + mosaic_quotient(a[c], wsum);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) J_out[cell * 3 + c] = sum[c];
}

hipError_t launch_band_split(void *table, int n_images, const sucre_mosaic_image_t *images, int level, const float *S_in, float *S_out,
                             float *D_out, hipStream_t s) {
    size_t base = 0;   // floats ahead of this launch's first pixel
    mosaic_for_each_launch(table, n_images, images, 0, s, [&](uint32_t nb, const MosaicImage *entries, int nl) {
        if (level == 0)
            hipLaunchKernelGGL((band_split_kernel<true>), dim3(nb), dim3(256), 0, s, entries, nl, 1, nullptr, S_out + base, D_out + base);
        else
            hipLaunchKernelGGL((band_split_kernel<false>), dim3(nb), dim3(256), 0, s, entries, nl, 1 << level, S_in + base, S_out + base,
                               D_out + base);
        base += (size_t)nb * kMosaicBlockPx * 3;
    });
    return hipGetLastError();
}

hipError_t launch_band_combine(const MosaicGrid &grid, int n_bands, const long long *acc_bands, float *J_out, hipStream_t s) {
    const size_t n_cells = (size_t)grid.Hm * (size_t)grid.Wm;   // the caller has checked that the workgroups fit a launch
    hipLaunchKernelGGL(band_combine_kernel, dim3((uint32_t)((n_cells + 255) / 256)), dim3(256), 0, s, n_cells, n_bands, acc_bands, J_out);
    return hipGetLastError();
}

}  // namespace sucre

// Single-view inversion for gfx950 (invert.h): the image table, and the variants without light.
//   invert_kernel<InvertNoLight, false>   uint8 colours, water model   (fit.hip's closed-form arithmetic)
//   invert_kernel<InvertNoLight, true>    float32 colours, water model (light.hip's, l = 1)
// The two light variants are instantiated in light.hip, next to light_obs.
#include "invert.h"

namespace sucre {

constexpr int kInvertSet = 32;   // table entries per set launch (by value: 32 x 72 bytes of kernel arguments)
struct InvertEntries { InvertImage e[kInvertSet]; };
struct InvertParams { float v[19]; };

// Entries i0 .. i0 + n - 1 of the table and (n_params > 0) the parameters, handed over by value: the library performs no
// host-to-device copy.
__global__ void invert_set_kernel(InvertImage *dst, const InvertEntries src, int n, float *pdst, const InvertParams p, int n_params) {
    if ((int)threadIdx.x < n) dst[threadIdx.x] = src.e[threadIdx.x];
    if ((int)threadIdx.x < n_params) pdst[threadIdx.x] = p.v[threadIdx.x];
}

size_t invert_bytes(int n_images) { return align_up(kInvertOffTable + (size_t)n_images * sizeof(InvertImage), 256); }

uint64_t invert_blocks(int H, int W) { return ((uint64_t)H * (uint64_t)W + kInvertBlockPx - 1) / kInvertBlockPx; }

hipError_t launch_invert(void *table, int n_images, const sucre_invert_image_t *images, const float *params, unsigned flags,
                         hipStream_t s) {
    auto *base = static_cast<uint8_t *>(table);
    auto *entries = reinterpret_cast<InvertImage *>(base + kInvertOffTable);
    float *pdev = reinterpret_cast<float *>(base + kInvertOffParams);
    const bool light = flags & SUCRE_INVERT_LIGHT, fcolour = flags & SUCRE_INVERT_FLOAT_COLOUR;
    InvertParams p = {};
    for (int i = 0; i < (light ? 19 : 9); ++i) p.v[i] = params[i];
    uint64_t block0 = 0;
    for (int i0 = 0; i0 < n_images; i0 += kInvertSet) {
        InvertEntries src = {};
        const int n = n_images - i0 < kInvertSet ? n_images - i0 : kInvertSet;
        for (int j = 0; j < n; ++j) {
            const sucre_invert_image_t &im = images[i0 + j];
            InvertImage &e = src.e[j];
            e.depth = im.depth; e.rgb = im.rgb; e.J = im.J; e.H = im.H; e.W = im.W;
            for (int q = 0; q < 9; ++q) e.Kinv[q] = im.Kinv[q];
            e.block0 = (uint32_t)block0;
            block0 += invert_blocks(im.H, im.W);
        }
        hipLaunchKernelGGL(invert_set_kernel, dim3(1), dim3(64), 0, s, entries + i0, src, n, pdev, p, i0 == 0 ? 19 : 0);
    }
    const uint32_t n_blocks = (uint32_t)block0;   // the caller has checked that the grid fits
    if (light) return launch_invert_light(table, n_images, n_blocks, fcolour, s);
    if (fcolour) hipLaunchKernelGGL((invert_kernel<InvertNoLight, true>), dim3(n_blocks), dim3(256), 0, s, entries, n_images, pdev, nullptr);
    else hipLaunchKernelGGL((invert_kernel<InvertNoLight, false>), dim3(n_blocks), dim3(256), 0, s, entries, n_images, pdev, nullptr);
    return hipGetLastError();
}

}  // namespace sucre

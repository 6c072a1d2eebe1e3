// The walk of the seabed mosaic's phases (mosaic.h, "Walk") and what it says of a pixel: one copy for every translation unit whose
// lanes must agree on who takes part and where (mosaic.hip: the phases and the blend; surface.hip: the surface test).
#pragma once
#include "mosaic.h"
#include "match_pixel.h"

namespace sucre {

// What every phase needs to know about one pixel, formed by every phase with these very operations.
struct MosaicPixel {
    bool in;          // takes part (d > 0, no NaN in J)
    float z;          // its range
    float a_s, a_t;   // its plane coordinates
    float a_n;        // its coordinate along e3, the mosaic's viewing direction (surface.h: the only reader; dead code elsewhere)
    float J[3];
};

__device__ __forceinline__ MosaicPixel mosaic_pixel(const MosaicImage *__restrict__ im, const float *Kinv, bool pin, const float *R,
                                                    const float *t, const float *axes, uint32_t p, uint32_t W) {
    MosaicPixel m;
    const uint32_t v = p / W, u = p - v * W;
    const float d = global_ptr(im->depth)[p];
    const auto *pj = global_ptr(im->J) + (size_t)p * 3;
    m.J[0] = pj[0]; m.J[1] = pj[1]; m.J[2] = pj[2];
    m.in = mosaic_member(d, m.J[0], m.J[1], m.J[2]);
    float cP[3], wP[3];
    unproject(Kinv, pin, (float)u, (float)v, d, cP);
    m.z = sqrtf(cP[0] * cP[0] + cP[1] * cP[1] + cP[2] * cP[2]);
    rigid(R, t, cP, wP);
    m.a_s = dot3(axes + 0, wP[0], wP[1], wP[2]);
    m.a_t = dot3(axes + 3, wP[0], wP[1], wP[2]);
    m.a_n = dot3(axes + 6, wP[0], wP[1], wP[2]);
    return m;
}

// The pixel's cell, or false when it falls outside the grid (caller-given bounds) or its coordinates are not numbers.
__device__ __forceinline__ bool mosaic_cell(const MosaicGrid &g, const MosaicPixel &m, size_t *cell) {
    const float qs = (m.a_s - g.lo_s) / g.gsd, qt = (m.a_t - g.lo_t) / g.gsd;
    if (!(qs >= 0.0f && qs < (float)g.Wm && qt >= 0.0f && qt < (float)g.Hm)) return false;
    const int col = (int)qs, row = (int)qt;
    if (col >= g.Wm || row >= g.Hm) return false;   // (float)Wm may round up above 2^24: never index past the grid
    *cell = (size_t)row * (size_t)g.Wm + (size_t)col;
    return true;
}

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t y = (uint32_t)__shfl_xor((int)x, o);
        x = y < x ? y : x;
    }
    return x;
}

// Suffix sum over the lane's run: after the step with offset o, x holds the sum over lanes lane .. min(lane + 2 o, end of run) - 1.
// `left`: lanes from this one to the end of its run, this one included.  (The blend's accumulate and the direct gain solve's slots.)
template <typename T>
__device__ __forceinline__ T run_sum(T x, int left) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T y = __shfl_down(x, o);
        if (o < left) x += y;
    }
    return x;
}

// What a walk says of the lane's pixel once the workgroup's image is found: pixel threadIdx.x of 256-pixel block `block` of the launch
// in `im`.  False for a lane past the image's last pixel and for a pixel that does not take part.
__device__ __forceinline__ bool mosaic_walk_image(const MosaicImage *__restrict__ im, uint32_t block, const MosaicGrid &g,
                                                  const MosaicImage *__restrict__ *image, uint32_t *pixel, MosaicPixel *m) {
    const uint32_t W = (uint32_t)im->W, n_px = (uint32_t)im->H * W;   // H, W <= 32767: below 2^30
    const uint32_t p = (block - im->block0) * kMosaicBlockPx + threadIdx.x;
    const bool inside = p < n_px;
    float Kinv[9], R[9], t[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) { Kinv[i] = im->Kinv[i]; R[i] = im->R[i]; }
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = im->t[i];
    const bool pin = pinhole_form(Kinv);
    *m = MosaicPixel{};
    if (inside) *m = mosaic_pixel(im, Kinv, pin, R, t, g.axes, p, W);
    *image = im;
    *pixel = p;
    return inside && m->in;
}

// The walk of every phase: the workgroup's image, the lane's pixel and what mosaic_pixel says of it.
__device__ __forceinline__ bool mosaic_walk(const MosaicImage *__restrict__ table, int n_images, const MosaicGrid &g,
                                            const MosaicImage *__restrict__ *image, uint32_t *pixel, MosaicPixel *m) {
    return mosaic_walk_image(mosaic_block_image(table, n_images), blockIdx.x, g, image, pixel, m);
}

// The walk of 256-pixel block `block` of the launch's grid, for a kernel whose workgroups each walk several (mosaic_block_image_at:
// a second copy of the search alone, mosaic.h says why); the pixel's numbers come from the one mosaic_pixel.
__device__ __forceinline__ bool mosaic_walk_at(const MosaicImage *__restrict__ table, int n_images, const MosaicGrid &g, uint32_t block,
                                               const MosaicImage *__restrict__ *image, uint32_t *pixel, MosaicPixel *m) {
    return mosaic_walk_image(mosaic_block_image_at(table, n_images, block), block, g, image, pixel, m);
}

// ---- what the kernels that write a copy of J share (surface.hip's cull, one- and two-sided; reject.hip's) ----

constexpr uint32_t kMosaicCountBlocks = 32;   // 256-pixel blocks a workgroup of a cull's counting form walks, one after the other

// The lane's pixel of the copy: it sits where the lane sits in the launch, pixel block 256 + threadIdx.x behind `J_out`; J bit for
// bit where the pixel is kept, the NaN 0x7fc00000 in all three channels where it is not.
__device__ __forceinline__ void mosaic_store_copy(float *__restrict__ J_out, uint32_t block, bool keep, const MosaicPixel &m) {
    const float none = __uint_as_float(0x7fc00000u);
    float *__restrict__ o = J_out + ((size_t)block * kMosaicBlockPx + threadIdx.x) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = keep ? m.J[c] : none;
}

// The launches of a cull over images[0 .. n): those of a phase (mosaic_for_each_launch, 32 images each), every one told its grid --
// one workgroup per kMosaicCountBlocks blocks in the counting form, one per block otherwise --, its part of J_out and its blocks.
template <typename Launch>
static hipError_t mosaic_for_each_cull_launch(void *table, int n_images, const sucre_mosaic_image_t *images, int first_ordinal,
                                              hipStream_t s, bool counting, float *J_out, Launch launch) {
    size_t base = 0;   // floats ahead of this launch's first pixel
    mosaic_for_each_launch(table, n_images, images, first_ordinal, s, [&](uint32_t nb, const MosaicImage *entries, int nl) {
        launch(dim3(counting ? (nb + kMosaicCountBlocks - 1) / kMosaicCountBlocks : nb), entries, nl, J_out + base, nb);
        base += (size_t)nb * kMosaicBlockPx * 3;
    });
    return hipGetLastError();
}

}  // namespace sucre

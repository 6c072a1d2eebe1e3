// Single-view inversion: the fitted water (and light) model applied to an image through its OWN depth map.
//
// With one observation per pixel -- the image matched against itself -- SUCRe.update_J (sucre.py:66-77) is
//   J = (I - l B (1 - e^(-gamma z))) a / a^2,   a = l e^(-beta z),   cP = K^-1 d [u+.5, v+.5, 1],   z = ||cP|| (+ ||lP|| with light)
// per pixel: no matching, no workspace, no neighbour.  invert_kernel is elementwise and bound by its 19 (uint8 colours) or 28
// bytes per pixel; one launch walks several images of any sizes.
//
// The results are the BITS the engine's closed-form kernels leave for a store that holds only the self-match, so every
// operation below restates one of theirs, in their order (the library is built with -ffp-contract=off; every FMA is explicit):
//   geometry      match.hip: unproject / mul3 (the pinhole form drops the zero terms of the chain and changes no finite result),
//                 then z = sqrtf(x x + y y + z z), IEEE
//   uint8, water  fit.hip: closed_terms / closed_pass<.., kJOnly = true> on one level -- the colour folded into y = fma(k, 1/255,
//                 -(B (1 - g))), the sums started from 0 and from Jp = 0, J = 0 + N / D, v_exp_f32 as it is
//   the others    light.hip: light_grad_kernel<true, true, ..>'s solve -- y = I - b with I = unit_from_u8(k) or the float32 colour,
//                 num = fma(y, a, 0), den = fma(a, a, 0), J = num / den, and a pixel with a zero denominator solved again with
//                 gradual underflow (fit_math.h) -- with l = 1, z = the range when there is no light (its kColour form)
// Walk: a flat pixel index, four adjacent pixels per lane (one 16-byte depth load, three colour dwords or three 16-byte colour
// loads, three 16-byte stores of J); a group may straddle rows, so (u, v) is formed per pixel; the last H W % 4 pixels of an
// image go one by one.  Workgroup b of the grid finds its image by bisecting the table's first-workgroup column.
#pragma once
#include <type_traits>

#include "fit_math.h"

namespace sucre {

constexpr int kInvertMaxImages = 4096;     // images per sucre_invert_images call (the table's bisection: 12 steps)
constexpr uint32_t kInvertBlockPx = 1024;  // 256 lanes x 4 pixels
// head of the table buffer: the parameters as the kernel reads them, and the light geometry derived from them
constexpr size_t kInvertOffParams = 0;     // float [19]
constexpr size_t kInvertOffGeom = 128;     // float [16]: R, t, Sigma^-1 (light_geometry)
constexpr size_t kInvertOffDexp = 256;     // double [72]: light_geometry's twists (unused here; it writes them)
constexpr size_t kInvertOffTable = 1024;   // InvertImage [n_images]

struct InvertImage {   // sucre_invert_image_t with its reserved word put to use
    const float *depth;
    const void *rgb;
    float *J;
    int32_t H, W;
    float Kinv[9];
    uint32_t block0;   // the image's first workgroup in the launch grid
};
static_assert(sizeof(InvertImage) == sizeof(sucre_invert_image_t), "the device table entry is the public struct");

// No light: l = 1 and z is the range itself (what light_grad_kernel's kColour branch sets).
struct InvertNoLight {
    static constexpr bool kLight = false;
    __device__ __forceinline__ explicit InvertNoLight(const float *) {}
    template <bool kGradual>
    __device__ __forceinline__ void lz(const float (&)[3], float zc, float &l, float &z) const { l = 1.0f; z = zc; }
};

// The images' pointers come out of a table in memory: the compiler cannot know their address space and would use flat
// loads and stores; they are device-memory pointers by contract (as match.hip's global_ptr).
template <class T>
__device__ __forceinline__ const __attribute__((address_space(1))) T *invert_global(const T *p) {
    return (const __attribute__((address_space(1))) T *)p;
}
template <class T>
__device__ __forceinline__ __attribute__((address_space(1))) T *invert_global(T *p) {
    return (__attribute__((address_space(1))) T *)p;
}

struct InvertWater { float B[3], nb[3], ng[3]; };   // B, -beta log2(e), -gamma log2(e): fit.hip's Water, light.hip's nb / ng

__device__ __forceinline__ InvertWater invert_water(const float *__restrict__ params) {
    InvertWater w;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        w.B[c] = params[c];
        w.nb[c] = -params[3 + c] * kLog2e;
        w.ng[c] = -params[6 + c] * kLog2e;
    }
    return w;
}

__device__ __forceinline__ bool invert_pinhole_form(const float *M) {
    return M[1] == 0.f && M[3] == 0.f && M[6] == 0.f && M[7] == 0.f && M[8] == 1.f;
}

// cP = Kinv (d [u+.5, v+.5, 1]) as match.hip forms the camera point of a matched pixel
__device__ __forceinline__ void invert_unproject(const float *Kinv, bool pin, float u, float v, float d, float (&out)[3]) {
    const float x = d * (u + 0.5f), y = d * (v + 0.5f), z = d * 1.0f;
    if (pin) {
        out[0] = __builtin_fmaf(Kinv[2], z, Kinv[0] * x);
        out[1] = __builtin_fmaf(Kinv[5], z, Kinv[4] * y);
        out[2] = z;
    } else {
#pragma unroll
        for (int r = 0; r < 3; ++r)
            out[r] = __builtin_fmaf(Kinv[3 * r + 2], z, __builtin_fmaf(Kinv[3 * r + 1], y, Kinv[3 * r] * x));
    }
}

// One pixel.  k: its uint8 colour, f: its float32 colour (the one kFloatColour selects is read).
template <class Model, bool kFloatColour>
__device__ __forceinline__ void invert_pixel(const Model &m, const InvertWater &w, const float *Kinv, bool pin, uint32_t u, uint32_t v,
                                             float d, const uint32_t (&k)[3], const float (&f)[3], float (&J)[3]) {
    if (!(d > 0.0f)) {   // fit_init's rule, and what update_J leaves where nothing is observed
        J[0] = J[1] = J[2] = __builtin_nanf("");
        return;
    }
    float cP[3];
    invert_unproject(Kinv, pin, (float)u, (float)v, d, cP);
    const float zc = sqrtf(cP[0] * cP[0] + cP[1] * cP[1] + cP[2] * cP[2]);
    if constexpr (!Model::kLight && !kFloatColour) {
        constexpr float kInv255 = (float)(1.0 / 255.0);
        const bool valid = zc > 0.0f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float a = fast_exp2(zc * w.nb[c]), g = fast_exp2(zc * w.ng[c]);
            const float omg = 1.0f - g;
            const float y = __builtin_fmaf((float)k[c], kInv255, -(w.B[c] * omg));
            float p = __builtin_fmaf(-0.0f, a, y);   // measured from Jp = 0
            p = valid ? p : 0.0f;
            const float N = __builtin_fmaf(p, a, 0.0f);
            const float D = __builtin_fmaf(a, valid ? a : 0.0f, 0.0f);
            J[c] = 0.0f + N / D;
        }
    } else {
        float num[3], den[3];
        auto solve = [&](auto gradual) {
            constexpr bool kGradual = decltype(gradual)::value;
#pragma unroll
            for (int c = 0; c < 3; ++c) num[c] = den[c] = 0.f;
            if (!(zc > 0.0f)) return;
            float l, z;
            m.template lz<kGradual>(cP, zc, l, z);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float a = l * exp2_as<kGradual>(z * w.nb[c]);
                const float b = l * w.B[c] * (1.0f - exp2_as<kGradual>(z * w.ng[c]));
                const float y = kFloatColour ? f[c] - b : unit_from_u8(k[c]) - b;
                num[c] = __builtin_fmaf(y, a, num[c]);
                den[c] = __builtin_fmaf(a, a, den[c]);
            }
        };
        solve(std::false_type{});
        if (zc > 0.0f && (den[0] == 0.f || den[1] == 0.f || den[2] == 0.f)) solve(std::true_type{});
#pragma unroll
        for (int c = 0; c < 3; ++c) J[c] = num[c] / den[c];
    }
}

template <class Model, bool kFloatColour>
__global__ __launch_bounds__(256) void invert_kernel(const InvertImage *__restrict__ table, int n_images, const float *__restrict__ params,
                                                     const float *__restrict__ geom) {
    typedef float f4 __attribute__((ext_vector_type(4)));
    // the image of this workgroup: the last one whose first workgroup is not behind blockIdx.x (wave-uniform: scalar loads)
    int lo = 0, hi = n_images - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].block0 <= blockIdx.x) lo = mid;
        else hi = mid - 1;
    }
    const InvertImage *__restrict__ im = table + lo;
    const uint32_t W = (uint32_t)im->W, n_px = (uint32_t)im->H * W;   // H, W <= 32767: below 2^30
    const uint32_t first = ((blockIdx.x - im->block0) * 256u + threadIdx.x) * 4u;
    if (first >= n_px) return;
    float Kinv[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) Kinv[i] = im->Kinv[i];
    const bool pin = invert_pinhole_form(Kinv);
    const InvertWater w = invert_water(params);
    const Model m(geom);
    const auto *depth = invert_global(im->depth);
    auto *J = invert_global(im->J);
    const auto *rgb_f = invert_global(static_cast<const float *>(im->rgb));
    const auto *rgb_k = invert_global(static_cast<const uint8_t *>(im->rgb));
    uint32_t v = first / W, u = first - v * W;
    if (first + 4u <= n_px) {
        typedef const __attribute__((address_space(1))) f4 *f4_in;
        typedef const __attribute__((address_space(1))) uint32_t *u32_in;
        const f4 d4 = *(f4_in)(depth + first);
        const float d[4] = {d4.x, d4.y, d4.z, d4.w};
        uint32_t cw[3] = {0u, 0u, 0u};
        float fc[12];
        if constexpr (kFloatColour) {
            const f4_in p = (f4_in)(rgb_f + (size_t)first * 3);
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const f4 x = p[q];
                fc[4 * q] = x.x; fc[4 * q + 1] = x.y; fc[4 * q + 2] = x.z; fc[4 * q + 3] = x.w;
            }
        } else {
            const u32_in p = (u32_in)(rgb_k + (size_t)first * 3);
            cw[0] = p[0]; cw[1] = p[1]; cw[2] = p[2];
        }
        float out[12];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            while (u >= W) { u -= W; ++v; }   // the group may straddle rows (several, when W < 4)
            uint32_t k[3] = {0u, 0u, 0u};
            float f[3] = {0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if constexpr (kFloatColour) f[c] = fc[3 * j + c];
                else k[c] = (cw[(3 * j + c) >> 2] >> (8 * ((3 * j + c) & 3))) & 255u;
            }
            float Jp[3];
            invert_pixel<Model, kFloatColour>(m, w, Kinv, pin, u, v, d[j], k, f, Jp);
            out[3 * j] = Jp[0]; out[3 * j + 1] = Jp[1]; out[3 * j + 2] = Jp[2];
            ++u;
        }
        auto *o = (__attribute__((address_space(1))) f4 *)(J + (size_t)first * 3);
#pragma unroll
        for (int q = 0; q < 3; ++q) o[q] = f4{out[4 * q], out[4 * q + 1], out[4 * q + 2], out[4 * q + 3]};
    } else {   // the image's last H W % 4 pixels, one by one
        for (uint32_t i = first; i < n_px; ++i) {
            while (u >= W) { u -= W; ++v; }
            uint32_t k[3] = {0u, 0u, 0u};
            float f[3] = {0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if constexpr (kFloatColour) f[c] = rgb_f[(size_t)i * 3 + c];
                else k[c] = rgb_k[(size_t)i * 3 + c];
            }
            float Jp[3];
            invert_pixel<Model, kFloatColour>(m, w, Kinv, pin, u, v, depth[i], k, f, Jp);
            J[(size_t)i * 3] = Jp[0]; J[(size_t)i * 3 + 1] = Jp[1]; J[(size_t)i * 3 + 2] = Jp[2];
            ++u;
        }
    }
}

}  // namespace sucre

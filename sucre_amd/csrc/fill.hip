// Push-pull hole filling of the mosaic for gfx950 (sucre_mosaic_fill_*; the rules: fill.h).
#include "fill.h"
#include "match_pixel.h"

namespace sucre {

typedef float fill_f4 __attribute__((ext_vector_type(4)));   // a native vector: one 16-byte global access

// The lane's cell of an H x W level: workgroup b holds the 64 x 4 tile (b / tiles_x, b % tiles_x), a wave one row of it.
__device__ __forceinline__ bool fill_cell(int H, int W, int *y, int *x) {
    const uint32_t tiles_x = ((uint32_t)W + kFillTileW - 1) / kFillTileW;
    const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    *x = (int)(tx * kFillTileW + (threadIdx.x & (kFillTileW - 1)));
    *y = (int)(ty * kFillTileH + threadIdx.x / kFillTileW);
    return *x < W && *y < H;
}

__device__ __forceinline__ FillRecord fill_load(const FillRecord *level, size_t i) {
    const auto *p = global_ptr(reinterpret_cast<const fill_f4 *>(level + i));
    const fill_f4 a = p[0], b = p[1];
    return FillRecord{{a.x, a.y, a.z, a.w, b.x, b.y}, b.z, b.w};
}

__device__ __forceinline__ void fill_store(FillRecord *level, size_t i, const FillRecord &r) {
    auto *p = (__attribute__((address_space(1))) fill_f4 *)reinterpret_cast<fill_f4 *>(level + i);
    p[0] = fill_f4{r.c[0], r.c[1], r.c[2], r.c[3]};
    p[1] = fill_f4{r.c[4], r.c[5], r.w, r.g};
}

// What level 0 holds of a cell, as stored.
struct FillCell {
    uint32_t j[3], r[3];
    int32_t source;
};

__device__ __forceinline__ FillCell fill_base_cell(const FillBase &b, size_t i) {
    FillCell k;
    const auto *pj = global_ptr(b.J) + i * 3;
    const auto *pr = global_ptr(b.raw) + i * 3;
    k.j[0] = pj[0]; k.j[1] = pj[1]; k.j[2] = pj[2];
    k.r[0] = pr[0]; k.r[1] = pr[1]; k.r[2] = pr[2];
    k.source = global_ptr(b.source)[i];
    return k;
}

__device__ __forceinline__ bool fill_finite(uint32_t bits) { return (bits & 0x7f800000u) != 0x7f800000u; }

// The record a level-0 cell stands for: its values with w = 1 when it is valid, zeros otherwise.
__device__ __forceinline__ FillRecord fill_base_record(const FillCell &k) {
    const bool valid = k.source >= 0 && fill_finite(k.j[0]) && fill_finite(k.j[1]) && fill_finite(k.j[2]);
    FillRecord r = {};
    if (valid) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { r.c[c] = __uint_as_float(k.j[c]); r.c[3 + c] = (float)k.r[c]; }
        r.w = 1.0f;
    }
    return r;
}

// Level l+1 (dst, Hd x Wd, g = l+1) from level l (Hs x Ws: src, or level 0 read in place).
template <bool kBase>
__global__ __launch_bounds__(256) void fill_pull_kernel(const FillBase base, const FillRecord *__restrict__ src, int Hs, int Ws,
                                                        FillRecord *__restrict__ dst, int Hd, int Wd, float g) {
    int y, x;
    if (!fill_cell(Hd, Wd, &y, &x)) return;
    FillRecord k[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int sy = 2 * y + (i >> 1), sx = 2 * x + (i & 1);
        k[i] = FillRecord{};
        if (sy < Hs && sx < Ws) {
            const size_t cell = (size_t)sy * (size_t)Ws + (size_t)sx;
            if constexpr (kBase) k[i] = fill_base_record(fill_base_cell(base, cell));
            else k[i] = fill_load(src, cell);
        }
    }
    const float Wt = ((k[0].w + k[1].w) + k[2].w) + k[3].w;
    FillRecord r = {};
    if (Wt > 0.0f) {
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            const float p0 = k[0].w * k[0].c[c], p1 = k[1].w * k[1].c[c], p2 = k[2].w * k[2].c[c], p3 = k[3].w * k[3].c[c];
            const float S = ((p0 + p1) + p2) + p3;
            r.c[c] = S / Wt;
        }
        r.w = Wt * 0.25f;
        r.g = g;
    }
    fill_store(dst, (size_t)y * (size_t)Wd + (size_t)x, r);
}

// The empty cells of level l (H x W: `level`, in place; or level 0, whose three outputs are written for every cell) from level
// l+1 (up, Hu x Wu, complete).
template <bool kBase>
__global__ __launch_bounds__(256) void fill_push_kernel(const FillBase base, FillRecord *__restrict__ level, int H, int W,
                                                        const FillRecord *__restrict__ up, int Hu, int Wu, const FillOut out) {
    int y, x;
    if (!fill_cell(H, W, &y, &x)) return;
    const size_t cell = (size_t)y * (size_t)W + (size_t)x;
    if constexpr (kBase) {
        const FillCell k = fill_base_cell(base, cell);
        if (k.source >= 0) {   // measured: copied as it is, finite or not
#pragma unroll
            for (int c = 0; c < 3; ++c) { out.J[cell * 3 + c] = k.j[c]; out.raw[cell * 3 + c] = (uint8_t)k.r[c]; }
            out.level[cell] = 0;
            return;
        }
    } else {
        const auto *own = global_ptr(reinterpret_cast<const float *>(level + cell));
        if (own[6] > 0.0f) return;
    }
    const int py = y >> 1, px = x >> 1;
    int ny = py + ((y & 1) ? 1 : -1), nx = px + ((x & 1) ? 1 : -1);
    ny = ny < 0 ? 0 : (ny > Hu - 1 ? Hu - 1 : ny);
    nx = nx < 0 ? 0 : (nx > Wu - 1 ? Wu - 1 : nx);
    const FillRecord t[4] = {fill_load(up, (size_t)py * (size_t)Wu + (size_t)px), fill_load(up, (size_t)py * (size_t)Wu + (size_t)nx),
                             fill_load(up, (size_t)ny * (size_t)Wu + (size_t)px), fill_load(up, (size_t)ny * (size_t)Wu + (size_t)nx)};
    const float a0 = t[0].w > 0.0f ? 0.5625f : 0.0f, a1 = t[1].w > 0.0f ? 0.1875f : 0.0f, a2 = t[2].w > 0.0f ? 0.1875f : 0.0f,
                a3 = t[3].w > 0.0f ? 0.0625f : 0.0f;
    const float A = ((a0 + a1) + a2) + a3;
    FillRecord r = {};
    if (A > 0.0f) {
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            const float p0 = a0 * t[0].c[c], p1 = a1 * t[1].c[c], p2 = a2 * t[2].c[c], p3 = a3 * t[3].c[c];
            const float S = ((p0 + p1) + p2) + p3;
            r.c[c] = S / A;
        }
        r.w = 1.0f;
        if (a0 > 0.0f) r.g = fmaxf(r.g, t[0].g);
        if (a1 > 0.0f) r.g = fmaxf(r.g, t[1].g);
        if (a2 > 0.0f) r.g = fmaxf(r.g, t[2].g);
        if (a3 > 0.0f) r.g = fmaxf(r.g, t[3].g);
    }
    if constexpr (kBase) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            out.J[cell * 3 + c] = A > 0.0f ? __float_as_uint(r.c[c]) : 0x7fc00000u;
            out.raw[cell * 3 + c] = A > 0.0f ? (uint8_t)rintf(fminf(fmaxf(r.c[3 + c], 0.0f), 255.0f)) : (uint8_t)0;
        }
        out.level[cell] = A > 0.0f ? (int32_t)r.g : -1;
    } else {
        if (A > 0.0f) fill_store(level, cell, r);
    }
}

struct FillLevels {
    int H[kFillMaxLevels + 1], W[kFillMaxLevels + 1];
    FillRecord *at[kFillMaxLevels + 1];   // at[0]: none, level 0 is the mosaic itself
};

static FillLevels fill_levels(int Hm, int Wm, int levels, void *pyramid) {
    FillLevels v = {};
    v.H[0] = Hm; v.W[0] = Wm;
    auto *p = static_cast<uint8_t *>(pyramid);
    for (int l = 1; l <= levels; ++l) {
        v.H[l] = fill_next(v.H[l - 1]); v.W[l] = fill_next(v.W[l - 1]);
        v.at[l] = reinterpret_cast<FillRecord *>(p);
        p += fill_level_bytes(v.H[l], v.W[l]);
    }
    return v;
}

hipError_t launch_fill_pull(int Hm, int Wm, int levels, const FillBase &base, void *pyramid, hipStream_t s) {
    const FillLevels v = fill_levels(Hm, Wm, levels, pyramid);
    for (int l = 0; l < levels; ++l) {
        const dim3 grid((uint32_t)fill_blocks(v.H[l + 1], v.W[l + 1]));
        if (l == 0)
            hipLaunchKernelGGL((fill_pull_kernel<true>), grid, dim3(256), 0, s, base, (const FillRecord *)nullptr, v.H[0], v.W[0], v.at[1],
                               v.H[1], v.W[1], 1.0f);
        else
            hipLaunchKernelGGL((fill_pull_kernel<false>), grid, dim3(256), 0, s, base, (const FillRecord *)v.at[l], v.H[l], v.W[l],
                               v.at[l + 1], v.H[l + 1], v.W[l + 1], (float)(l + 1));
    }
    return hipGetLastError();
}

hipError_t launch_fill_push(int Hm, int Wm, int levels, const FillBase &base, void *pyramid, const FillOut &out, hipStream_t s) {
    const FillLevels v = fill_levels(Hm, Wm, levels, pyramid);
    for (int l = levels - 1; l >= 0; --l) {
        const dim3 grid((uint32_t)fill_blocks(v.H[l], v.W[l]));
        if (l == 0)
            hipLaunchKernelGGL((fill_push_kernel<true>), grid, dim3(256), 0, s, base, (FillRecord *)nullptr, v.H[0], v.W[0],
                               (const FillRecord *)v.at[1], v.H[1], v.W[1], out);
        else
            hipLaunchKernelGGL((fill_push_kernel<false>), grid, dim3(256), 0, s, base, v.at[l], v.H[l], v.W[l],
                               (const FillRecord *)v.at[l + 1], v.H[l + 1], v.W[l + 1], out);
    }
    return hipGetLastError();
}

}  // namespace sucre

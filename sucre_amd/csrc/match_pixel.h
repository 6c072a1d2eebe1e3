// The fused two-way match of one target pixel against one view (the file header of match.hip describes the test), and the
// float32 chains it is made of.  Every kernel that needs a match calls match_pixel(), so their match sets are the same
// by construction: match_kernel and match_map_kernel (match.hip), consistency_kernel (consist.hip).  The including file
// is built with -ffp-contract=off and IEEE divide / sqrt (csrc/Makefile).
#pragma once
#include "experiment.h"
#include "launch.h"

namespace sucre {

__device__ __forceinline__ float dot3(const float *a, float x, float y, float z) {
    float acc = a[0] * x;
    acc = __builtin_fmaf(a[1], y, acc);
    acc = __builtin_fmaf(a[2], z, acc);
    return acc;
}

// A pinhole camera matrix and its inverse have the form [[a, 0, b], [0, c, d], [0, 0, 1]] (sfm.py:62-78; torch's LU
// inverse of an upper-triangular matrix keeps the zeros exact).  For such a matrix the FMA chain of dot3() loses its
// terms with a zero coefficient without changing a bit of any finite result: fma(0, y, acc) = acc and 0 * x = 0 exactly
// (only the sign of a zero can differ, which no comparison, truncation or product downstream sees), and a non-finite
// x, y or z still makes c0 or c1 non-finite, so the bound test rejects the point in both forms.  9 -> 4 operations per
// product; the flag is wave-uniform (one scalar branch).
__host__ __device__ __forceinline__ bool pinhole_form(const float *M) {
    return M[1] == 0.f && M[3] == 0.f && M[6] == 0.f && M[7] == 0.f && M[8] == 1.f;
}

__device__ __forceinline__ void mul3(const float *M, bool pin, float x, float y, float z, float out[3]) {
    if (pin) {
        out[0] = __builtin_fmaf(M[2], z, M[0] * x);
        out[1] = __builtin_fmaf(M[5], z, M[4] * y);
        out[2] = z;
    } else {
        out[0] = dot3(M + 0, x, y, z);
        out[1] = dot3(M + 3, x, y, z);
        out[2] = dot3(M + 6, x, y, z);
    }
}

// sfm.py:90-93
__device__ __forceinline__ void unproject(const float *Kinv, bool pin, float u, float v, float d, float out[3]) {
    const float x = d * (u + 0.5f), y = d * (v + 0.5f), z = d * 1.0f;
    mul3(Kinv, pin, x, y, z, out);
}

// sfm.py:49-55
__device__ __forceinline__ void rigid(const float *R, const float *t, const float p[3], float out[3]) {
    out[0] = dot3(R + 0, p[0], p[1], p[2]) + t[0];
    out[1] = dot3(R + 3, p[0], p[1], p[2]) + t[1];
    out[2] = dot3(R + 6, p[0], p[1], p[2]) + t[2];
}

// x / z and y / z as far as their users can tell.  Everything downstream of the two IEEE quotients of sfm.py:106 is a
// comparison with an integer (-1 < d, d < W) or Tensor.long() (truncation), so a quotient may be replaced by any value
// that lies strictly between the same two consecutive integers.  a = x * rcp(z) is within 1.5 * 2^-23 |a| of the real
// quotient (v_rcp_f32: 1 ulp; the product: half an ulp), and the correctly rounded quotient is monotone and reaches an
// integer n only from within half an ulp of n (<= 2^-24 (|a| + 1)): if a is farther than 2^-21 |a| + 2^-23 from every
// integer -- more than twice those bounds together -- truncation and bound tests of a ARE those of the IEEE quotient.
// Otherwise (a within that margin of an integer: ~0.1 % of the lanes at a = 1000; or a NaN / infinite / zero, which
// covers a denormal or zero z) the whole wave takes the two IEEE divisions.  12 instructions instead of 22 per pair of
// quotients, four pairs per matching pixel pair; the match sets keep equal to the reference's bit for bit
// (experiment.h: SUCRE_EXACT_DIV=1 builds the plain form; test_pixel_quotients_on_the_integer_boundaries).
__device__ __forceinline__ void pixel_quotients(float x, float y, float z, float *px, float *py) {
    if (kExactDiv) {
        *px = x / z;
        *py = y / z;
        return;
    }
    const float rc = __builtin_amdgcn_rcpf(z);
    float ax = x * rc, ay = y * rc;
    const float sx = __builtin_fmaf(-__builtin_fabsf(ax), 0x1p-21f, __builtin_fabsf(ax - __builtin_rintf(ax)));
    const float sy = __builtin_fmaf(-__builtin_fabsf(ay), 0x1p-21f, __builtin_fabsf(ay - __builtin_rintf(ay)));
    const bool unsure = !(sx > 0x1p-23f) || !(sy > 0x1p-23f);   // NaN lands here too
    if (__builtin_amdgcn_ballot_w64(unsure) != 0ull) {
        ax = x / z;
        ay = y / z;
    }
    *px = ax;
    *py = ay;
}

// sfm.py:103-107,116-117: world point -> continuous pixel; true when Tensor.long() of it lies inside WxH.
// trunc(x) in [0, W-1]  <=>  -1 < x < W ; NaN and +-inf fail both comparisons like INT64_MIN fails the bound test.
__device__ __forceinline__ bool project(const float *Rinv, const float *tinv, const float *K, bool pin, float Wf, float Hf,
                                        const float wP[3], float *px, float *py) {
    float cP[3], c[3];
    rigid(Rinv, tinv, wP, cP);
    mul3(K, pin, cP[0], cP[1], cP[2], c);
    pixel_quotients(c[0], c[1], c[2], px, py);
    return (*px > -1.0f) && (*px < Wf) && (*py > -1.0f) && (*py < Hf);
}

// The views' pixel pointers come out of a table in memory, so the compiler cannot know their address space and would
// gather through flat loads (which also count against the LDS counter); they are device-memory pointers by contract.
template <class T>
__device__ __forceinline__ const __attribute__((address_space(1))) T *global_ptr(const T *p) {
    return (const __attribute__((address_space(1))) T *)p;
}

// The fused two-way test for one target pixel whose world point is wP: returns true and the matched pixel of
// view 2 (linear index q, camera-frame point c2) iff p1 -> p2 -> p1 closes (see the file header).
// `packed`: the view's `depth` pointer holds sucre_pack_view's 8-byte records {float32 depth, r, g, b, 0} (its `rgb`
// pointer is NULL): depth and colour of the landing pixel arrive with ONE gather -- *rgbw gets the colour word.
__device__ __forceinline__ bool match_pixel(const CamDev &c1, float W1f, float H1f, const sucre_view_t *vw, bool packed,
                                            float W2f, float H2f, bool pin, const float wP[3], int u1, int v1,
                                            size_t *q_out, float c2[3], uint32_t *rgbw) {
    float px, py;
    if (!project(vw->Rinv, vw->tinv, vw->K, pin, W2f, H2f, wP, &px, &py)) return false;
    const int u2 = (int)px, v2 = (int)py;
    const size_t q = (size_t)v2 * vw->W + u2;
    float d2;
    if (packed) {
        const unsigned long long rec = global_ptr(reinterpret_cast<const unsigned long long *>(vw->depth))[q];
        d2 = __uint_as_float((uint32_t)rec);
        *rgbw = (uint32_t)(rec >> 32);
    } else {
        d2 = global_ptr(vw->depth)[q];
    }
    if (!(d2 > 0.0f)) return false;
    float w2[3], qx, qy;
    unproject(vw->Kinv, pin, (float)u2, (float)v2, d2, c2);
    rigid(vw->R, vw->t, c2, w2);
    if (!project(c1.Rinv, c1.tinv, c1.K, pin, W1f, H1f, w2, &qx, &qy)) return false;
    if ((int)qx != u1 || (int)qy != v1) return false;
    *q_out = q;
    return true;
}

// the target's camera as the kernels take it (by value: SGPR-resident)
inline CamDev to_cam(const sucre_view_t &v) {
    CamDev c;
    for (int i = 0; i < 9; ++i) { c.K[i] = v.K[i]; c.Kinv[i] = v.Kinv[i]; c.R[i] = v.R[i]; c.Rinv[i] = v.Rinv[i]; }
    for (int i = 0; i < 3; ++i) { c.t[i] = v.t[i]; c.tinv[i] = v.tinv[i]; }
    c.H = v.H; c.W = v.W;
    return c;
}

}  // namespace sucre

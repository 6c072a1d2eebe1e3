// Standard errors of the water parameters and of J (sucre_fit_uncertainty*): the float64 statistics of the Gauss-Newton normal
// equations of sucre.adam's objective at the fit as it stands.
//
//   I = J a + B (1 - g),  a = e^(-beta z),  g = e^(-gamma z)                    sucre.py:79-82, 144 (z: sucre.py:52-53)
//   dJ = a,  dB = 1 - g,  dbeta = -J z a,  dgamma = B z g,  r = I - (J a + B dB)       per observation and channel
//   per pixel p:     A_p = sum dJ^2,  b_p = sum dJ (dB, dbeta, dgamma),  k_p = b_p / A_p
//   over the image:  H = sum_obs d d^T - sum_p b_p b_p^T / A_p   (d = (dB, dbeta, dgamma): the 3x3 normal matrix of
//                    (B, beta, gamma) with every pixel's own J eliminated),  SSR = sum r^2,  N observations,  P pixels seen
// The host (engine.water_uncertainty) turns them into s^2 = SSR / (N - P - 3), cov = s^2 H^-1 and, per pixel,
// sigma_J^2 = s^2 (1 / A_p + k_p^T H^-1 k_p).  Channels do not couple.
//
// Why float64.  What the observations say about B, beta, gamma is what is left of d once each pixel's J has been eliminated: a
// 30-65x cancellation on the project's synthetic scenes, in a matrix whose scaled condition number is 1e3 - 3e4.  Float32 sums
// leave H wrong by 5e-4 - 9e-4 relative, which that condition number turns into garbage; the same one-pass sums in float64
// agree with the cancellation-free form (tests/uncertainty_ref.py) to 4e-13 - 2.6e-12.  Everything below the loads is double,
// one IEEE operation per step (the build has -ffp-contract=off); z, J, B, beta, gamma and I are the float32 numbers the
// residual pass reads -- the SUCRE_OBS_U16MM range rule, unit_from_u8 or the float32 colour plane -- promoted.
//
// The skeleton is residual_kernel's (residual.h: residual_load_J, residual_load_chunk, ResidualArgs' geometry), so the numbers
// come from the very slots the residuals come from.  One wave per tile; lane l owns the slots 4 l .. 4 l + 3; the loop over
// the kept views with a count in the tile is wave-uniform; the next view's chunk is loaded before this one is evaluated.  A
// lane keeps in doubles: A and the three b per pixel and channel (48), the six sums d d' and sum r^2 per channel over its four
// pixels (21), and n per pixel.  Behind the loop it subtracts its four pixels' b b^T / A from its own sums, writes count and
// jterms, and the wave's fixed-order trees (handoff.h) reduce the 24 words, which lane 0 writes to the tile's place in
// caller-owned scratch, word-major.  uncertainty_sum_kernel then adds the tiles of every word in a fixed order.  No atomics:
// two calls give the same bits.  No scratch memory (the Makefile's rule): every register array is indexed by unrolled loops.
//
// A pixel that has observations but no finite positive A in some channel (every e^(-beta z) underflowed, or a parameter is not
// finite) has no J to eliminate: nothing is subtracted for it, its jterms are 0 in every channel and word 2 counts it; its
// observations still stand in N, SSR and the sums d d^T, so engine.water_uncertainty declares an image with such pixels not
// well posed instead of trusting the sums.  The test is per pixel, not per channel: ONE channel without an A zeroes the pixel's
// jterms (hence sigma_J is NaN) in all three, and word 2 has no channel, so well_posed is False for all three channels of the
// image, not only for the one affected.
//
// Variants (template arguments, chosen at launch): kU16 as in residual.h; kExt 0 or SUCRE_EXT_COLOUR (float32 colours).  No
// light variant: the lamp's ten parameters would have to join (B, beta, gamma); errors conditional on a fixed lamp would
// understate.
//
// Limits: Gauss-Newton at the current point, not necessarily at the minimum; observations are taken as independent with one
// variance per channel, so errors shared by views (depth maps, poses) are not in it.
//
// Measured on an MI355X (tests/test_gpu_uncertainty.py against the restatement, worst over its cases as a fraction of the bar):
// H, scaled Frobenius distance, bar 1e-9: 3.8e-5 (i.e. 3.8e-14);  SSR, bar 1e-9: 2.4e-6;  jterms, bar 2^-23: 0.50 (the one float32
// rounding);  J_se, bar 1e-6: 0.81 (closed form; 0.51-0.63 elsewhere, 0.08 on the deep scene: the float32 jterms through a
// quadratic form whose B and gamma directions nearly cancel);  se, bar 1e-6: 6.5e-5.  226 VGPRs (246 with float32 colours), two
// waves per SIMD, no scratch.  1920x1080 x 65 views, 79.0 M observations: 0.93 ms per pass -- 3.6 x the residual pass, 4 % of a
// 200-iteration fit; not byte-bound (1.0 TB/s of the store against the residual pass's 3.7); whether FP64 throughput or latency
// at two waves per SIMD limits it was not separated, no counters were collected (tools/uncertainty_time.py,
// profiles/uncertainty_time.txt).
#pragma once
#include "residual.h"

namespace sucre {

constexpr int kUncertaintyWords = SUCRE_UNCERTAINTY_WORDS;   // N, P, pixels without A, then 7 per channel
static_assert(kUncertaintyWords == 3 + 3 * 7, "the layout of sums_dev");

struct UncertaintyArgs {
    ResidualArgs R;      // geometry, store, J, parameters and count (H, W) as the residual pass takes them; ssr, tile_view unused
    float4 *jterms;      // (H, W, 3): {1 / A, k_B, k_beta, k_gamma}
    double *tile_sums;   // scratch [kUncertaintyWords][n_tiles]
    double *sums;        // [kUncertaintyWords]
};

template <bool kU16, int kExt>
__global__ __launch_bounds__(256) void uncertainty_kernel(const UncertaintyArgs U) {
    static_assert((kExt == 0 || kExt == 2) && !(kU16 && kExt), "uint8 or float32 colours; extension planes ride with the f32 store only");
    constexpr bool kFloatColour = kExt == 2;
    const ResidualArgs &A = U.R;
    const int lane = threadIdx.x & 63;
    const int tile = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (tile >= A.n_tiles) return;   // (no barrier below: the wave is on its own)
    const int n_views = A.n_views;

    double B[3], beta[3], gamma[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) { B[c] = (double)A.params[c]; beta[c] = (double)A.params[3 + c]; gamma[c] = (double)A.params[6 + c]; }

    float J[4][3];
    residual_load_J(A, tile, lane, J);

    const uint16_t *tcnt = A.cnt + (size_t)tile * n_views;
    auto next_view = [&](int k) { while (k < n_views && !(tcnt[k] > 0 && A.view_keep[k] != 0u)) ++k; return k; };   // wave-uniform

    double pa[4][3], pb[4][3][3], S[3][7];
    float pn[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        pn[j] = 0.0f;
#pragma unroll
        for (int c = 0; c < 3; ++c) { pa[j][c] = 0.0; pb[j][c][0] = pb[j][c][1] = pb[j][c][2] = 0.0; }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int i = 0; i < 7; ++i) S[c][i] = 0.0;

    int k = next_view(0);
    ResidualChunk cur = {};
    if (k < n_views) cur = residual_load_chunk<kExt>(A, tile, k, lane);
    while (k < n_views) {
        const int kn = next_view(k + 1);
        ResidualChunk nx = {};
        if (kn < n_views) nx = residual_load_chunk<kExt>(A, tile, kn, lane);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool valid = cur.zz[j] > 0.0f;   // an empty slot holds range 0
            float zc = cur.zz[j];
            if (kU16) zc = kMPerMm * fminf(fmaxf(rintf(zc * kMmPerM), 1.0f), 65535.0f);
            const double z = (double)zc;
            pn[j] += valid ? 1.0f : 0.0f;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double Jd = (double)J[j][c];
                const double I = (double)(kFloatColour ? cur.p[c][j] : unit_from_u8((cur.cc[c] >> (8 * j)) & 255u));
                const double a = exp(-(beta[c] * z)), g = exp(-(gamma[c] * z));
                const double omg = 1.0 - g;
                // select, not multiply: J may be NaN where nothing is observed
                const double dJ = valid ? a : 0.0;
                const double dB = valid ? omg : 0.0;
                const double db = valid ? -((Jd * z) * a) : 0.0;
                const double dg = valid ? (B[c] * z) * g : 0.0;
                const double r = valid ? I - (Jd * a + B[c] * omg) : 0.0;
                pa[j][c] += dJ * dJ;
                pb[j][c][0] += dJ * dB; pb[j][c][1] += dJ * db; pb[j][c][2] += dJ * dg;
                S[c][0] += dB * dB; S[c][1] += dB * db; S[c][2] += dB * dg;
                S[c][3] += db * db; S[c][4] += db * dg; S[c][5] += dg * dg;
                S[c][6] += r * r;
            }
        }
        cur = nx;
        k = kn;
    }

    // the lane's four pixels: eliminate J, write count and jterms
    const int ty = tile / A.tiles_x, tx = tile - ty * A.tiles_x;
    const int v = ty * kTile + (lane >> 2), u0 = tx * kTile + (lane & 3) * 4;
    double w_n = 0.0, w_p = 0.0, w_bad = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool seen = pn[j] > 0.0f;
        bool ok = seen;
#pragma unroll
        for (int c = 0; c < 3; ++c) ok = ok && pa[j][c] > 0.0 && pa[j][c] < __builtin_inf();   // (false for a NaN)
        w_n += (double)pn[j];
        w_p += seen ? 1.0 : 0.0;
        w_bad += (seen && !ok) ? 1.0 : 0.0;
        float4 jt[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double Ap = ok ? pa[j][c] : 1.0;
            const double kB = ok ? pb[j][c][0] / Ap : 0.0, kb = ok ? pb[j][c][1] / Ap : 0.0, kg = ok ? pb[j][c][2] / Ap : 0.0;
            const double bB = ok ? pb[j][c][0] : 0.0, bb = ok ? pb[j][c][1] : 0.0, bg = ok ? pb[j][c][2] : 0.0;
            S[c][0] -= kB * bB; S[c][1] -= kB * bb; S[c][2] -= kB * bg;
            S[c][3] -= kb * bb; S[c][4] -= kb * bg; S[c][5] -= kg * bg;
            jt[c] = make_float4(ok ? (float)(1.0 / Ap) : 0.0f, (float)kB, (float)kb, (float)kg);
        }
        if (v < A.H && u0 + j < A.W) {
            const size_t o = (size_t)v * A.W + (u0 + j);
            A.count[o] = (int32_t)pn[j];
#pragma unroll
            for (int c = 0; c < 3; ++c) U.jterms[o * 3 + c] = jt[c];
        }
    }

    // the tile's 24 words: fixed-order trees, lane 0 writes
    double *row = U.tile_sums + tile;
    const size_t nt = (size_t)A.n_tiles;
    const double t_n = wave_sum_lane0(w_n), t_p = wave_sum_lane0(w_p), t_bad = wave_sum_lane0(w_bad);
    if (lane == 0) { row[0] = t_n; row[nt] = t_p; row[2 * nt] = t_bad; }
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int i = 0; i < 7; ++i) {
            const double t = wave_sum_lane0(S[c][i]);
            if (lane == 0) row[(size_t)(3 + 7 * c + i) * nt] = t;
        }
}

}  // namespace sucre

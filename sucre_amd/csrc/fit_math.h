// Small device helpers shared by fit.hip and light.hip.
#pragma once
#include "experiment.h"
#include "launch.h"

namespace sucre {

constexpr float kLog2e = 1.44269504088896340736f;
// float32(float64(k)/255) for every uint8 k (loader.py:157,163) as fma(k, hi, k*lo); checked for all 256 values
// in tests/test_host_logic.py and on the GPU by tests/test_gpu_parity.py.
constexpr float kInv255Hi = (float)(1.0 / 255.0);
constexpr float kInv255Lo = (float)(1.0 / 255.0 - (double)kInv255Hi);

__device__ __forceinline__ float unit_from_u8(uint32_t k) {
    const float kf = (float)k;
    return __builtin_fmaf(kf, kInv255Hi, kf * kInv255Lo);
}

__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

// v_exp_f32 flushes results below 2^-126 to zero; torch.exp underflows gradually.  Nothing in a gradient can tell the
// two apart, but the closed-form J = sum(y a) / sum(a^2) of a pixel whose every a^2 underflows is +-inf with a denormal
// a and 0/0 = NaN with a flushed one: the solves redo such a pixel with this form (3 more instructions, never on the
// hot path).
__device__ __forceinline__ float gradual_exp2(float x) {
    const bool tiny = x < -126.0f;
    return fast_exp2(tiny ? x + 64.0f : x) * (tiny ? 0x1p-64f : 1.0f);
}
template <bool kGradual>
__device__ __forceinline__ float exp2_as(float x) { return kGradual ? gradual_exp2(x) : fast_exp2(x); }

// torch/optim/adam.py::_single_tensor_adam (non-capturable, no amsgrad, no weight decay), float32
__device__ __forceinline__ void adam_update(float &p, float &m, float &v, float g, const AdamCoef &co) {
    m = __builtin_fmaf(co.w1, g - m, m);
    v = (v * co.beta2) + (co.w2 * g) * g;
    const float denom = sqrtf(v) / co.bc2_sqrt + co.eps;
    p = p + (co.step_size_neg * m) / denom;
}

// dL/dB, dL/dbeta, dL/dgamma of channel q % 3 (q = 0..2, 3..5, 6..8: the parameter's place among the nine) from the ten reduced
// sums -- sB[3], sGZ[3], sBeta[3], cost -- with scale = (1/3) / n_obs (fit.hip's header).  sum_at(i) and B_at(c) are callables,
// called inside the branch that needs them: a caller's loads stay conditional.  B is the one BEFORE its own step.
template <class SumAt, class BAt>
__device__ __forceinline__ double water_grad(int q, float scale, SumAt sum_at, BAt B_at) {
    const int c = q % 3;
    if (q < 3) return -2.0 * (double)scale * sum_at(c);              // dL/dB
    if (q < 6) return 2.0 * (double)scale * sum_at(6 + c);           // dL/dbeta
    return -2.0 * (double)scale * (double)B_at(c) * sum_at(3 + c);   // dL/dgamma
}

// May a fit launch run the B-scaled form of its chunk arithmetic (fit.hip, grad_terms / closed_terms: bo = fma(-B, g, B) in
// one instruction, the sums of r (1 - g) accumulated as sum r bo = B sum r (1 - g) and divided by B, in float64, where the
// launch's sums become final)?  Only when all three |B_c| are finite and inside [kScaledBMin, kScaledBMax]: with B_c = 0 the
// scaled sum is identically 0 and dL/dB would be lost, and a NaN or infinite B must keep poisoning what it poisons today.
// Below 2^-24 nothing is claimed for the scaled sums (B (1 - g) of a short range nears the denormals); above 8 the model
// itself leaves the range the fit is held in -- the colours are in [0, 1], the fixtures' B in 0.001 .. 0.53, while the
// absolute bars on the parameters (1e-5) and on a closed-form J, which is of B's size (1e-4), are a few float32 roundings
// wide from |B| = 16 on in either form (tests/test_gpu_scaled_b.py) -- so such a launch keeps the arithmetic it has always
// had.  One channel outside: the WHOLE launch -- all three -- runs the unscaled form.  The waves of a launch evaluate it on
// the parameters they load, and the workgroup that finishes the sums on the same words again (nothing writes them in
// between): the two cannot disagree.
// SUCRE_SCALED_B=0 (experiment.h) builds the unscaled form everywhere.
constexpr float kScaledBMin = 0x1p-24f, kScaledBMax = 0x1p+3f;
__host__ __device__ inline bool scaled_b_ok(float B0, float B1, float B2) {
    if (!kScaledBBuilt) return false;
    const float a0 = __builtin_fabsf(B0), a1 = __builtin_fabsf(B1), a2 = __builtin_fabsf(B2);
    // (comparisons with a NaN are false; infinity is above the window)
    return a0 >= kScaledBMin && a0 <= kScaledBMax && a1 >= kScaledBMin && a1 <= kScaledBMax && a2 >= kScaledBMin && a2 <= kScaledBMax;
}

// The same step for a pixel's J (three per pixel and iteration: 158 of the J-parameter kernel's ~2000 instructions per
// pixel were the two IEEE divisions and the IEEE square root of these three steps): hardware square root and reciprocals
// (1 ulp each) instead of the IEEE sequences, 11 instead of ~42 instructions per channel.  The fit is held to a tolerance,
// not to bit parity -- its sums already run in another order than torch's -- and the difference sits below that noise:
// RMS(J) against the reference's own 200-step runs 5.8e-8 / 5.3e-8 with this form, 5.3e-8 / 5.5e-8 with the IEEE one, and
// the oracle itself is 5.7e-8 / 5.5e-8 from the reference (tools/exp/adam_accuracy.py).  +2.9 % on the headline, same box
// (tools/exp/ab_bench.sh exactadam).  Special values behave as in adam_update: v = 0 -> denom = eps; v = inf -> no step;
// a NaN J stays NaN.  SUCRE_EXACT_J_ADAM=1 (experiment.h) builds the IEEE form.
__device__ __forceinline__ void adam_update_J(float &p, float &m, float &v, float g, const AdamCoef &co) {
    if (kExactJAdam) {
        adam_update(p, m, v, g, co);
        return;
    }
    m = __builtin_fmaf(co.w1, g - m, m);
    v = (v * co.beta2) + (co.w2 * g) * g;
    const float denom = __builtin_fmaf(__builtin_amdgcn_sqrtf(v), __builtin_amdgcn_rcpf(co.bc2_sqrt), co.eps);
    p = __builtin_fmaf(co.step_size_neg * m, __builtin_amdgcn_rcpf(denom), p);
}

}  // namespace sucre

// Probe: the J-parameter chunk arithmetic of csrc/fit.hip (accumulate_chunk<false>: 4 levels x 3 channels, 24 exponentials
// back to back) on REGISTER data -- no LDS reads, no DMA, no plan -- at 1..6 waves per SIMD: how many shader cycles does a
// chunk cost a SIMD when nothing but the arithmetic runs?  (round 5; build: hipcc -O3 --offload-arch=gfx950 -ffp-contract=off -fno-slp-vectorize,
// as csrc/Makefile builds fit.hip)
// Round 13: the scaled-B form of the chunk (fit.hip grad_terms<true>) in the compiler's depth-first order and in STAGED orders
// -- one kind of instruction for a group of chains at a time, held with sched_barrier -- on the same register data: all 12
// chains at once, 6 + 6 (two levels x three channels), 3 + 3 + 3 + 3 (level by level).  Every accumulator takes the same
// products in the same sequence in all of them.  Do five resident waves already hide the dependency bubbles of the
// depth-first order?  And the control that explained the answer: the depth-first order with s_nop at chosen places of a chain.
// (profiles/r13_staged_terms_probe.txt; VGPRs: add -Rpass-analysis=kernel-resource-usage)
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>

struct Water { float B[3], nb[3], ng[3]; };
struct Acc { float pa[3], pb[3], sB[3], sGZ[3], cost; };
constexpr float kInv255 = (float)(1.0 / 255.0);

template <int kVariant>
__device__ __forceinline__ void chunk(const float (&zz)[4], const uint32_t (&cc)[3], const Water &w, const float (&J)[3], Acc &acc) {
    float ea[4][3], eg[4][3];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) { ea[j][c] = zz[j] * w.nb[c]; eg[j][c] = zz[j] * w.ng[c]; }
    if (kVariant != 2) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (kVariant == 1) { ea[j][c] = ea[j][c] * 0.5f + 1.0f; eg[j][c] = eg[j][c] * 0.5f + 1.0f; }   // exponentials replaced by FMAs
            else { ea[j][c] = __builtin_amdgcn_exp2f(ea[j][c]); eg[j][c] = __builtin_amdgcn_exp2f(eg[j][c]); }
        }
    if (kVariant != 2) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float z = zz[j];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const uint32_t k = (cc[c] >> (8 * j)) & 255u;
            const float a = ea[j][c], g = eg[j][c];
            const float omg = 1.0f - g;
            const float Ihat = __builtin_fmaf(J[c], a, w.B[c] * omg);
            float r = __builtin_fmaf((float)k, kInv255, -Ihat);
            const float rz = r * z;
            acc.cost = __builtin_fmaf(r, r, acc.cost);
            acc.pa[c] = __builtin_fmaf(r, a, acc.pa[c]);
            acc.pb[c] = __builtin_fmaf(rz, a, acc.pb[c]);
            acc.sB[c] = __builtin_fmaf(r, omg, acc.sB[c]);
            acc.sGZ[c] = __builtin_fmaf(rz, g, acc.sGZ[c]);
        }
    }
}

// A stage ends here: the values named are complete before this point and read only after it.  sched_barrier alone holds the
// machine scheduler but not instruction selection, which places arithmetic that no barrier depends on where it likes -- seen:
// half of a stage's products emitted behind the last barrier.  The empty asm makes the dependence real and costs nothing.
__device__ __forceinline__ void pin3(float (&x)[3]) { asm volatile("" : "+v"(x[0]), "+v"(x[1]), "+v"(x[2])); }
template <int kN>
__device__ __forceinline__ void stage_end(float (&x)[kN][3]) {
#pragma unroll
    for (int j = 0; j < kN; ++j) pin3(x[j]);
    __builtin_amdgcn_sched_barrier(0);
}
__device__ __forceinline__ void stage_end(Acc &acc) {
    pin3(acc.pa); pin3(acc.pb); pin3(acc.sB); pin3(acc.sGZ);
    asm volatile("" : "+v"(acc.cost));
    __builtin_amdgcn_sched_barrier(0);
}

// Scaled-B chunk (fit.hip grad_terms<true>), exponentials as in variant 0.
// kGroup = 0: fit.hip's source, the order left to the compiler -- which, with this kernel's registers to spare, interleaves the
//             chains itself; the fit kernels are short of registers and get them depth first (profiles/r13_staged_terms_probe.txt).
// kGroup = 5: depth first, one observation-channel after the other, as the fit kernels are emitted today: the reference.
// kGroup = 6: depth first with an s_nop behind every chain (the staged forms carry one behind most stages: the compiler puts it
//             between a VOP3 result and the empty asm that names it).
// kGroup = 4, 2, 1: that many levels' chains (x 3 channels) staged together.
template <int kGroup>
__device__ __forceinline__ void chunk_scaled(const float (&zz)[4], const uint32_t (&cc)[3], const Water &w, const float (&J)[3], Acc &acc) {
    float ea[4][3], eg[4][3];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) { ea[j][c] = zz[j] * w.nb[c]; eg[j][c] = zz[j] * w.ng[c]; }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) { ea[j][c] = __builtin_amdgcn_exp2f(ea[j][c]); eg[j][c] = __builtin_amdgcn_exp2f(eg[j][c]); }
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (kGroup == 0 || kGroup == 5 || kGroup == 6 || kGroup >= 16) {
        constexpr int kNops = kGroup >= 16 ? kGroup - 16 : 0;   // where a chain carries an s_nop: 1 behind bo, 2 Ihat, 4 r, 8 rz, 16 its end
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float z = zz[j];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const uint32_t k = (cc[c] >> (8 * j)) & 255u;
                const float a = ea[j][c], g = eg[j][c];
                float bo = __builtin_fmaf(-w.B[c], g, w.B[c]);
                if constexpr ((kNops & 1) != 0) asm volatile("s_nop 0" : "+v"(bo));
                float Ihat = __builtin_fmaf(J[c], a, bo);
                if constexpr ((kNops & 2) != 0) asm volatile("s_nop 0" : "+v"(Ihat));
                float r = __builtin_fmaf((float)k, kInv255, -Ihat);
                if constexpr ((kNops & 4) != 0) asm volatile("s_nop 0" : "+v"(r));
                float rz = r * z;
                if constexpr ((kNops & 8) != 0) asm volatile("s_nop 0" : "+v"(rz));
                acc.cost = __builtin_fmaf(r, r, acc.cost);
                acc.pa[c] = __builtin_fmaf(r, a, acc.pa[c]);
                acc.pb[c] = __builtin_fmaf(rz, a, acc.pb[c]);
                acc.sB[c] = __builtin_fmaf(r, bo, acc.sB[c]);
                acc.sGZ[c] = __builtin_fmaf(rz, g, acc.sGZ[c]);
                if constexpr (kGroup == 6 || (kNops & 16) != 0) asm volatile("s_nop 0");
                if constexpr (kGroup == 5 || kGroup == 6 || kGroup >= 16) {
                    asm volatile("" : "+v"(acc.cost), "+v"(acc.pa[c]), "+v"(acc.pb[c]), "+v"(acc.sB[c]), "+v"(acc.sGZ[c]));
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
    } else {
#pragma unroll
        for (int j0 = 0; j0 < 4; j0 += kGroup) {
            float bo[kGroup][3], t[kGroup][3], kf[kGroup][3], rz[kGroup][3];
#pragma unroll
            for (int j = 0; j < kGroup; ++j)
#pragma unroll
                for (int c = 0; c < 3; ++c) bo[j][c] = __builtin_fmaf(-w.B[c], eg[j0 + j][c], w.B[c]);
            stage_end(bo);
#pragma unroll
            for (int j = 0; j < kGroup; ++j)
#pragma unroll
                for (int c = 0; c < 3; ++c) t[j][c] = __builtin_fmaf(J[c], ea[j0 + j][c], bo[j][c]);   // Ihat
            stage_end(t);
#pragma unroll
            for (int j = 0; j < kGroup; ++j)
#pragma unroll
                for (int c = 0; c < 3; ++c) kf[j][c] = (float)((cc[c] >> (8 * (j0 + j))) & 255u);
            stage_end(kf);
#pragma unroll
            for (int j = 0; j < kGroup; ++j)
#pragma unroll
                for (int c = 0; c < 3; ++c) t[j][c] = __builtin_fmaf(kf[j][c], kInv255, -t[j][c]);     // r
            stage_end(t);
#pragma unroll
            for (int j = 0; j < kGroup; ++j)
#pragma unroll
                for (int c = 0; c < 3; ++c) rz[j][c] = t[j][c] * zz[j0 + j];
            stage_end(rz);
#pragma unroll
            for (int j = 0; j < kGroup; ++j)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float r = t[j][c];
                    acc.cost = __builtin_fmaf(r, r, acc.cost);
                    acc.pa[c] = __builtin_fmaf(r, ea[j0 + j][c], acc.pa[c]);
                    acc.pb[c] = __builtin_fmaf(rz[j][c], ea[j0 + j][c], acc.pb[c]);
                    acc.sB[c] = __builtin_fmaf(r, bo[j][c], acc.sB[c]);
                    acc.sGZ[c] = __builtin_fmaf(rz[j][c], eg[j0 + j][c], acc.sGZ[c]);
                }
            stage_end(acc);
        }
    }
}

// kVariant 0..2: the unscaled chunk above; 10 + kGroup: chunk_scaled<kGroup>.
template <int kVariant, int kWaves>
__global__ __launch_bounds__(256, kWaves) void k(float *out, int iters, const float *params) {
    Water w;
    for (int c = 0; c < 3; ++c) { w.B[c] = params[c]; w.nb[c] = params[3 + c]; w.ng[c] = params[6 + c]; }
    float J[3] = {0.3f + threadIdx.x * 1e-4f, 0.4f + threadIdx.x * 1e-4f, 0.5f + threadIdx.x * 1e-4f};
    Acc acc = {};
    float zz[4] = {3.0f + threadIdx.x * 1e-3f, 3.1f, 3.2f, 3.3f};
    uint32_t cc[3] = {0x10203040u + threadIdx.x, 0x50607080u + threadIdx.x, 0x11223344u + threadIdx.x};
    for (int it = 0; it < iters; ++it) {
        if constexpr (kVariant >= 10) chunk_scaled<kVariant - 10>(zz, cc, w, J, acc);
        else chunk<kVariant>(zz, cc, w, J, acc);
#pragma unroll
        for (int j = 0; j < 4; ++j) zz[j] += 1e-4f;   // (seven more instructions per chunk; keeps the work in the loop)
#pragma unroll
        for (int c = 0; c < 3; ++c) cc[c] += 0x01010101u;   // (round 13: all three words, so that no conversion leaves the loop)
    }
    float s = acc.cost;
    for (int c = 0; c < 3; ++c) s += acc.pa[c] + acc.pb[c] + acc.sB[c] + acc.sGZ[c];
    out[blockIdx.x * 256 + threadIdx.x] = s;
}

template <int kVariant, int kWaves>
double run(const char *name, const float *params, float *out, double ref_ns = 0.0) {
    const int iters = 4000, blocks = 256 * kWaves;
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    hipLaunchKernelGGL((k<kVariant, kWaves>), dim3(blocks), dim3(256), 0, 0, out, iters, params); hipDeviceSynchronize();
    hipEventRecord(e0);
    hipLaunchKernelGGL((k<kVariant, kWaves>), dim3(blocks), dim3(256), 0, 0, out, iters, params);
    hipEventRecord(e1); hipDeviceSynchronize();
    float ms; hipEventElapsedTime(&ms, e0, e1);
    const double chunks_per_simd = (double)kWaves * iters;
    const double ns = ms * 1e6 / chunks_per_simd;
    printf("%-34s %d waves/SIMD: %7.3f ms -> %6.1f ns per chunk per SIMD (= %5.0f cycles at 2.2 GHz)", name, kWaves, ms, ns, ns * 2.2);
    if (ref_ns > 0.0) printf("  %+5.1f %% against depth first", (ns / ref_ns - 1.0) * 100.0);
    printf("\n");
    return ns;
}

// The scaled-B chunk at kWaves waves per SIMD: depth first (the reference), then the staged groupings and the compiler's own
// order against it; twice, so that the run's own spread is seen.  (At six waves -- 80 registers -- the 12-chain grouping spills:
// not run.)
template <int kWaves>
void run_staged(const float *params, float *out) {
    for (int rep = 0; rep < 2; ++rep) {
        const double ref = run<15, kWaves>("scaled-B chunk, depth first", params, out);
        if constexpr (kWaves < 6) run<14, kWaves>("  staged, all 12 chains", params, out, ref);
        run<12, kWaves>("  staged, 6 + 6", params, out, ref);
        run<11, kWaves>("  staged, 3 + 3 + 3 + 3", params, out, ref);
        run<10, kWaves>("  order left to the compiler", params, out, ref);
        if constexpr (kWaves == 5) {
            run<16, kWaves>("  depth first + s_nop: end", params, out, ref);
            run<10 + 16 + 4, kWaves>("  depth first + s_nop: r", params, out, ref);
            run<10 + 16 + 4 + 16, kWaves>("  depth first + s_nop: r, end", params, out, ref);
            run<10 + 16 + 2 + 4 + 16, kWaves>("  depth first + s_nop: Ihat, r, end", params, out, ref);
            run<10 + 16 + 31, kWaves>("  depth first + s_nop: all five", params, out, ref);
        }
    }
}

int main() {
    float hp[9] = {0.1f, 0.1f, 0.1f, -0.144f, -0.144f, -0.144f, -0.2f, -0.2f, -0.2f}, *params, *out;
    hipMalloc(&params, sizeof(hp)); hipMemcpy(params, hp, sizeof(hp), hipMemcpyHostToDevice);
    hipMalloc(&out, 256 * 8 * 256 * 4);
    run<0, 1>("chunk (24 exp back to back)", params, out); run<0, 2>("chunk (24 exp back to back)", params, out);
    run<0, 4>("chunk (24 exp back to back)", params, out); run<0, 5>("chunk (24 exp back to back)", params, out);
    run<0, 6>("chunk (24 exp back to back)", params, out);
    run<2, 5>("chunk, compiler's own schedule", params, out);
    run<1, 5>("chunk, exponentials -> FMAs", params, out);
    run_staged<1>(params, out); run_staged<2>(params, out); run_staged<3>(params, out);
    run_staged<4>(params, out); run_staged<5>(params, out); run_staged<6>(params, out);
    return 0;
}

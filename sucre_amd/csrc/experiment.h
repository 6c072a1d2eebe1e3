// Build-time knobs of the experiments recorded in DESIGN.md section 4.2 (tools/exp/*.sh build them as
//   make VARIANT=<name> EXTRA="-D..."  ->  sucre_amd/libsucre_hip_<name>.so,   selected at run time with SUCRE_HIP_LIB).
// The product build defines none of them; tests/test_host_logic.py compiles every one so that they cannot rot.
// They are variants of ONE code path (same kernels, same ABI), never alternative back ends.
#pragma once

// Ablations of the fit kernels: the arithmetic of a chunk compiled out (the data are still touched), the LDS-DMA copies
// compiled out (the ring keeps whatever LDS holds).  Results are meaningless; only the launch time is read.
#ifdef SUCRE_EXP_NOCOMPUTE
constexpr bool kExpNoCompute = true;
#else
constexpr bool kExpNoCompute = false;
#endif
#ifdef SUCRE_EXP_NOLOAD
constexpr bool kExpNoLoad = true;
#else
constexpr bool kExpNoLoad = false;
#endif
// J-parameter kernels: the stepped J and moments are computed and not written (how much of a launch is the write stream).
#ifdef SUCRE_EXP_NOSTORE
constexpr bool kExpNoStore = true;
#else
constexpr bool kExpNoStore = false;
#endif
// The stepped J (and moments) written with the streaming policy (nt): 0 never, 1 always, 2 in batch launches only (the product).
// Same box, round 5.  1080p x 65 views: 1 = 126.3-126.5 us alone against 127.2-127.4, 84.5-84.8 Mpix/s with two images in
// flight against 85.1-85.2 (nothing to gain: 8 % of a launch's bytes).  Config 1 in launches of 32 (35 % of the bytes are these
// stores): a launch alone 244.6-245.2 against 245.2-248.0 us, but 221.7-223.0 against 208.8-210.1 Mpix/s with two slots in
// flight (the other slot's match kernels find their views in L2); closed form 248.5-249.7 against 241.9-245.0.
#ifndef SUCRE_STORE_NT
#define SUCRE_STORE_NT 2
#endif
constexpr int kStoreNt = SUCRE_STORE_NT;

// Waves per SIMD the fit kernels are compiled for (= workgroups per CU of their persistent grids).  J-parameter kernel, same
// box, two rounds (round 5): 5 waves 126.6-127.1 us alone / 85.7 Mpix/s; 6 waves (77 registers; deal 64,52,42,32,24,16)
// 126.1-126.4 / 85.8-85.9; 6 waves with equal shares 130.4-130.7 / 85.4-85.6; round 4: 4 waves = 5 waves.  Not occupancy.
#ifndef SUCRE_FIT_WAVES
#define SUCRE_FIT_WAVES 5
#endif
#ifndef SUCRE_CLOSED_WAVES
#define SUCRE_CLOSED_WAVES 4
#endif

// Strips per fit wave of a small image (layout.h make_layout: the image's own grid is ceil(tiles / this), at most the persistent
// grid; 1 = the rule until round 5).
#ifndef SUCRE_MIN_STRIPS
#define SUCRE_MIN_STRIPS 4
#endif

// Slots of a wave's LDS-DMA ring (prefetch depth + 1) and the cache policy of its copies (" nt": items are read once per
// launch -- measured 20 % faster than the default policy; next to it " sc0", " sc1", " sc0 sc1": equal).
#ifndef SUCRE_RING
#define SUCRE_RING 3
#endif
#ifndef SUCRE_DMA_POLICY
#define SUCRE_DMA_POLICY " nt"
#endif

// match.hip: the pixel quotients x/z, y/z as two IEEE divisions everywhere (1) instead of x * rcp(z) with the divisions
// as the fallback near integers (0, the product; same match sets by construction -- DESIGN.md section 4.1; the A/B of
// tools/exp/ab_lib.sh exactdiv).
#ifndef SUCRE_EXACT_DIV
#define SUCRE_EXACT_DIV 0
#endif
constexpr bool kExactDiv = SUCRE_EXACT_DIV != 0;

// fit.hip / light.hip: Adam's step on a pixel's J with the IEEE divisions and square root of torch's formula (1) instead of
// the hardware reciprocal / square root (0, the product: fit_math.h adam_update_J; tools/exp/ab_bench.sh exactadam).
#ifndef SUCRE_EXACT_J_ADAM
#define SUCRE_EXACT_J_ADAM 0
#endif
constexpr bool kExactJAdam = SUCRE_EXACT_J_ADAM != 0;

// fit.hip: the backscatter term of a chunk as bo = fma(-B, g, B) with the sums of r (1 - g) accumulated B-scaled and divided by
// B once per launch (1, the product: one instruction per observation-channel fewer; fit_math.h scaled_b_ok says for which B) or
// as B * (1 - g) everywhere, the form until round 10 (0; tools/exp/ab_vs.sh / ab_bench.sh unscaledb).
// (tests/test_scaled_b_host.py builds the 0 form, so that it cannot rot.)
#if !defined(SUCRE_SCALED_B)
#define SUCRE_SCALED_B 1
#endif
constexpr bool kScaledBBuilt = SUCRE_SCALED_B != 0;

// fit.hip / abi.hip: sucre_fit_run takes its J-parameter iterations in PAIRS of launches that read and write a pixel's Adam moments
// once per pair instead of once per launch (1; fit.hip, 'Paired iterations': same operations in the same order, same bits) or one
// by one as until round 11 (0: no paired kernel is built, the plan kernel writes no paired streams, and fit_grad_kernel's text is
// the parent's).  At run time SUCRE_FIT_UNPAIRED (sucre_hip.h) picks the launches one by one in a build that has both; whether
// the engine pairs by default follows the measurement in profiles/r12_paired_j_ab.txt (engine.py, PAIRED_FIT).
// (tests/test_paired_host.py builds the 0 form, so that it cannot rot.)
#if !defined(SUCRE_PAIRED_J)
#define SUCRE_PAIRED_J 1
#endif
constexpr bool kPairedBuilt = SUCRE_PAIRED_J != 0;

// fit.hip: the terms behind a full chunk's exponentials in the J-parameter kernels carry three s_nop per observation-channel --
// behind Ihat, behind r, behind the last accumulation (1, the product: grad_terms' kYield; same operations in the same order on
// every value, so the same bits) -- or none, the form until round 12 (0: make VARIANT=unstaged EXTRA=-DSUCRE_STAGED_TERMS=0 gives
// the parent's instruction sequences, tools/isa_digest.py).  The knob is named after the design it was opened for, the chains of a
// chunk issued stage by stage: built and measured in the probe and in the kernels, that form gains exactly what the s_nops gain
// which the compiler places behind its stages (profiles/r13_staged_terms_probe.txt, r13_staged_terms_ab.txt), at 50 more lines
// and 6 more registers; the s_nops alone were kept.
// (tests/test_staged_host.py builds the 0 form, so that it cannot rot.)
#if !defined(SUCRE_STAGED_TERMS)
#define SUCRE_STAGED_TERMS 1
#endif
constexpr bool kStagedTerms = SUCRE_STAGED_TERMS != 0;

// fit.hip: in fit_grad_kernel (L, F and the one-launch kernel) a pass over a 24-bit range-code store is compiled on its own, its
// format tests folded away, and a strip's run of unmasked full chunks is straight-line code unrolled by the ring -- the slot a
// compile-time constant (the ds_read offset behind ONE lane address), the wait the one immediate, level j's red converted from
// byte 3 of code word j where it lies (1, the product: stream_strips' kLaneBytes, accumulate_chunk_z24; the producer side -- which
// item goes to which slot, the DMAs, the stores, the waits' immediates -- and every value's operations are untouched, so the same
// bits) -- or the per-chunk step for every chunk, the form until round 13 (0: make VARIANT=generic EXTRA=-DSUCRE_STRAIGHT_CHUNKS=0
// gives the parent's instruction sequences, tools/isa_digest.py).  The straight run stands on the yields of SUCRE_STAGED_TERMS: a
// build without them keeps the text it had before either knob (tests/test_staged_host.py pins it).
// (tests/test_straight_chunks_host.py builds the 0 form, so that it cannot rot.)
#if !defined(SUCRE_STRAIGHT_CHUNKS)
#define SUCRE_STRAIGHT_CHUNKS 1
#endif
constexpr bool kStraightChunks = SUCRE_STRAIGHT_CHUNKS != 0 && kStagedTerms;

// fit.hip, timing only: every wave of a J-parameter launch records when it entered and left its strips (100 MHz wall clock) --
// how much of a launch is its ragged end (tools/exp/wave_times.py).
#ifdef SUCRE_EXP_WAVE_TIMES
constexpr bool kExpWaveTimes = true;
#define SUCRE_EXP_EXPORT extern "C" __attribute__((visibility("default")))
#else
constexpr bool kExpWaveTimes = false;
#define SUCRE_EXP_EXPORT [[maybe_unused]] static
#endif

// layout.h: the work a wave of each workgroup generation is dealt, in 64ths of what a wave of generation 0 (the oldest) gets;
// the first must be 64.  64 everywhere = equal shares.  Measured (tools/exp/wave_times.py, ab_solo.sh, round 4): with
// 64,44,24,14,5 a J-parameter launch ALONE on the GPU takes 126 instead of 134 us (its waves then end within 20 us of each
// other instead of 75), but with two images in flight -- the default -- the second launch's workgroups arrive as the first one's
// leave, no longer one generation per CU, and an image takes 25.1 instead of 24.4 ms.  Round 5 (tools/exp/ab_vs.sh, one box,
// two rounds each; launch alone / Mpix/s with two images in flight): equal shares 131.9-132.1 us / 84.91-84.95;
// **64,50,38,28,20: 127.3-128.0 / 84.89-85.06** (the product: nothing lost in flight, 3.3 % gained alone);
// 64,56,48,40,32: 131.3 / 84.3; 64,48,36,28,22: 128.1-128.7 / 84.5-84.7; 64,52,40,28,16: 125.7-125.9 / 84.54-84.57;
// 64,48,34,22,12: 125.2-125.6 / 84.2-84.6; 64,46,30,20,10: 125.2-125.5 / 84.3; 64,44,24,14,5: 126.2-126.6 / 81.4-81.5.
#ifndef SUCRE_DEAL_FIT
#define SUCRE_DEAL_FIT 64, 50, 38, 28, 20
#endif
// The closed-form kernel (four generations, instruction-bound) takes the unequal deal as its product default (round 5): alone a
// launch takes 140.8-142.3 instead of 148.4 us (same box, tools/exp/ab_vs.sh; 0.51 instead of 0.49 of the HBM peak by SURVEY
// 8(d)'s bytes) and an image restored alone 29.4 instead of 30.9 ms; with two images in flight 75.6-75.9 against 75.9 Mpix/s --
// unlike the J-parameter kernel it loses nothing there.  (64,54,44,34: 143.5 us; 64,44,28,12: 139-140 us alone but 75.0 Mpix/s
// in flight; 64,56,40,24: 140.9.)
#ifndef SUCRE_DEAL_CLOSED
#define SUCRE_DEAL_CLOSED 64, 48, 32, 20
#endif

// Knobs whose question is closed are listed, with their measurements and the commit that last held their code, under
// 'Retired knobs' in tools/exp/README.md.

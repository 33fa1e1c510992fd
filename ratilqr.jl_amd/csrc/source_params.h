// source_params.h -- model parameters drawn per rollout (rat_user_params, include/ratilqr.h "Source models"), as the Monte-Carlo kernels of
// source models apply them: rat_src_user_noisy_rollout (source_user_noise.h), both variants of rat_src_rare_rollout (source_rare.h) and
// rat_src_user_events (source_events.h) include this header and call rat_src_params once per rollout, in front of step 0, then hand q to
// the user's functions wherever they handed a.p.  rat_src_params_sample at the end is the kernel of rat_policy_params_sample (SRC_PARAMS):
// the hook alone.  The solver's kernels (source_kernels.h), rat_src_noisy_rollout (source_noisy.h: no counted rng) and PETS (source_pets.h)
// do not include it: they run on the nominal p.  Without RAT_USER_PARAMS_ON -- the state of every handle until
// rat_policy_params_sampling switches sampling on -- the header is empty, whether or not the source defines the hook: the kernels
// compile to what they compiled to before.  RAT_N_PARAMS, RAT_PARAM_NORMALS, RAT_PARAM_UNIFORMS come from the command line with
// RAT_USER_PARAMS_ON.  src_rollout_params at the end is what those kernels hold: the rollout's own q, or nothing with sampling off.
//
// The i-th parameter normal / uniform of the rollout with GLOBAL index g (independent of K and of how a call is cut into launches):
//   injected   zpn[g RAT_PARAM_NORMALS + i],  zpu[g RAT_PARAM_UNIFORMS + i]   (the handle's copy of the caller's streams, whole)
//   generator  Philox4x32-10 (rat_philox.h), key (seed lo, seed hi):
//                normals   counter (g lo, g hi, 0xFFFFFFFF, i / 2): u01(r0, r1), u01(r2, r3), Box-Muller -> normal 2q, normal 2q + 1
//                uniforms  counter (g lo, g hi, 0xFFFFFFFF, 0x80000000 | i / 2): uniform 2q is u01(r0, r1), uniform 2q + 1 is u01(r2, r3)
// rat_rng's pairing (rat_rng.h) under a step word no step uses, so the per-step draws keep their counters.  Under RAT_RNG_SHIFT alone the
// parameter normals come from N(0, 1) and add nothing to logw (rat_policy_rare_event_noise / _user).
//
// RAT_PARAM_SHIFT (the rat_policy_rare_event_params variant of source_rare.h's modules alone; it comes from the command line with
// RAT_USER_PARAMS_ON): the i-th parameter normal is drawn from the shifted proposal, z = pshift[i] + xi with xi the draw above, and
// -s z + s^2 / 2 is added to the rollout's logw at the draw, in draw order, in rat_rng.h's form; a hook that draws fewer normals than it
// declared adds fewer terms.  The shift row [RAT_PARAM_NORMALS] is one address for the whole wavefront.  Uniforms are not shifted.
// Without the macro RAT_PARAM_NORMAL is the identity, the struct has no further member and the functions no further argument.
//
// RAT_RNG_PICK (source_sobol.h's module alone, rat_policy_sobol; rat_rng.h has the rule): the generator's parameter draws come from two
// streams, `seed` and a second seed, chosen per draw index by two masks (bit i: parameter normal / uniform i is the second stream's), each
// draw bit for bit the plain generator's under its stream's seed, the spare of a block reused only between neighbours of one key.  The
// functions take the second seed and the masks behind `over`.  Without the macro the header preprocesses to what it was.
#pragma once
#include "source_step.h"

#ifdef RAT_RNG_PICK               // (with sampling off too: the rollout's draw() keeps one signature)
#define RAT_PARAM_PICK_ARGS , unsigned long long seed_b, unsigned long long pick_pn, unsigned long long pick_pu
#define RAT_PARAM_PICK_PASS , seed_b, pick_pn, pick_pu
#else
#define RAT_PARAM_PICK_ARGS
#define RAT_PARAM_PICK_PASS
#endif

#ifdef RAT_USER_PARAMS_ON
#include "rat_normal.h"
#include "rat_philox.h"
#include "source_args.h"

#ifndef RAT_USER_PARAMS
#error "the source does not define RAT_USER_PARAMS: parameter sampling is on (rat_policy_params_sampling) and needs '#define RAT_USER_PARAMS' and rat_user_params(rng, p, q)"
#endif
#if !defined(RAT_N_PARAMS) || RAT_N_PARAMS < 1 || RAT_N_PARAMS > 32
#error "rat_user_params is compiled for 1 .. 32 parameters (RAT_N_PARAMS)"
#endif
#if !defined(RAT_PARAM_NORMALS) || !defined(RAT_PARAM_UNIFORMS)
#error "RAT_PARAM_NORMALS and RAT_PARAM_UNIFORMS must be defined"
#endif
#if defined(RAT_PARAM_SHIFT) && (RAT_PARAM_NORMALS < 1 || RAT_PARAM_NORMALS > 12)
#error "rat_policy_rare_event_params shifts 1 .. 12 parameter normals"
#endif
#if defined(RAT_PARAM_SHIFT) && defined(RAT_PARAMS_SAMPLE_KERNEL)
#error "rat_policy_params_sample draws from N(0, 1): it is not compiled with RAT_PARAM_SHIFT"
#endif

#if defined(RAT_RNG_PICK) && (defined(RAT_PARAM_SHIFT) || defined(RAT_PARAMS_SAMPLE_KERNEL))
#error "RAT_RNG_PICK is source_sobol.h's: not combined with RAT_PARAM_SHIFT or the kernel of rat_policy_params_sample"
#endif
#if defined(RAT_RNG_PICK) && (RAT_PARAM_NORMALS > 64 || RAT_PARAM_UNIFORMS > 64)
#error "rat_policy_sobol masks at most 64 parameter normals and 64 parameter uniforms"
#endif

#ifdef RAT_PARAM_SHIFT
#define RAT_PARAM_NORMAL(i, xi) proposal(i, xi)
#define RAT_PARAM_SHIFT_ARGS , const double *pshift, double &logw
#define RAT_PARAM_SHIFT_PASS , pshift, logw
#else
#define RAT_PARAM_NORMAL(i, xi) xi
#define RAT_PARAM_SHIFT_ARGS
#define RAT_PARAM_SHIFT_PASS
#endif

// rat_rng's interface (normal(), uniform()) with bounds of its own; a draw beyond them returns NaN and records the overdraw (bit 0
// normals, bit 1 uniforms: the caller moves them to bits 2 and 3 of the kernel's flag)
struct rat_param_rng {
    const double *zn, *zu;        // injected: this rollout's slots; generator: null
    bool gen;
    unsigned g0, g1, k0, k1;      // generator: the rollout's counter words, key
    int in, iu, over;
    double spare_n, spare_u;      // the second output of the last generator block
#ifdef RAT_RNG_PICK
    unsigned kb0, kb1;            // the second stream's key
    unsigned long long pick_n, pick_u;   // bit i: parameter normal / uniform i is the second stream's
#endif
#ifdef RAT_PARAM_SHIFT
    const double *shift;          // the parameter shift row [RAT_PARAM_NORMALS]: one address for the whole wavefront
    double logw;
    __device__ __forceinline__ double proposal(int i, double xi) {
        const double sv = shift[i];
        const double z = sv + xi;
        logw += __builtin_fma(-sv, z, 0.5 * sv * sv);
        return z;
    }
#endif

    __device__ __forceinline__ double normal() {
        const int i = in++;
        if (i >= RAT_PARAM_NORMALS) { over |= 1; return __builtin_nan(""); }
        if (!gen) return RAT_PARAM_NORMAL(i, zn[i]);
#ifdef RAT_RNG_PICK
        const bool b = (pick_n >> i) & 1;
        if ((i & 1) && b == (bool)((pick_n >> (i - 1)) & 1)) return spare_n;
        unsigned r[4];
        philox4x32_10(g0, g1, 0xFFFFFFFFu, (unsigned)(i >> 1), b ? kb0 : k0, b ? kb1 : k1, r);
        double z0, z1;
        ratn_box_muller(u01(r[0], r[1]), u01(r[2], r[3]), &z0, &z1);
        if (i & 1) return z1;                                         // (its neighbour came from the other stream)
        spare_n = z1;
        return z0;
#else
        if (i & 1) return RAT_PARAM_NORMAL(i, spare_n);
        unsigned r[4];
        philox4x32_10(g0, g1, 0xFFFFFFFFu, (unsigned)(i >> 1), k0, k1, r);
        double z0;
        ratn_box_muller(u01(r[0], r[1]), u01(r[2], r[3]), &z0, &spare_n);
        return RAT_PARAM_NORMAL(i, z0);
#endif
    }
    __device__ __forceinline__ double uniform() {
        const int i = iu++;
        if (i >= RAT_PARAM_UNIFORMS) { over |= 2; return __builtin_nan(""); }
        if (!gen) return zu[i];
#ifdef RAT_RNG_PICK
        const bool b = (pick_u >> i) & 1;
        if ((i & 1) && b == (bool)((pick_u >> (i - 1)) & 1)) return spare_u;
        unsigned r[4];
        philox4x32_10(g0, g1, 0xFFFFFFFFu, 0x80000000u | (unsigned)(i >> 1), b ? kb0 : k0, b ? kb1 : k1, r);
        if (i & 1) return u01(r[2], r[3]);
        spare_u = u01(r[2], r[3]);
        return u01(r[0], r[1]);
#else
        if (i & 1) return spare_u;
        unsigned r[4];
        philox4x32_10(g0, g1, 0xFFFFFFFFu, 0x80000000u | (unsigned)(i >> 1), k0, k1, r);
        spare_u = u01(r[2], r[3]);
        return u01(r[0], r[1]);
#endif
    }
};

// The rollout's parameters.  q arrives as anything and leaves holding what rat_user_params made of a copy of p[0 .. RAT_N_PARAMS) for the
// rollout with global index g; zpn, zpu: the handle's injected streams (whole, indexed by g) or both null: the generator under `seed`.
// over: the hook's overdraw bits are OR-ed in at bits 2 (normals) and 3 (uniforms).  Returns true where q holds a NaN although p had
// none: the rollout's DomainError (the caller sets dom).  A hook that leaves q alone changes no bit.
// Under RAT_PARAM_SHIFT: pshift is the shift row of the parameter normals, logw leaves holding the parameter part of the likelihood ratio.
__device__ __forceinline__ bool rat_src_params(long g, unsigned long long seed, const double *zpn, const double *zpu, const double *p,
                                               double (&q)[RAT_N_PARAMS], int &over RAT_PARAM_SHIFT_ARGS RAT_PARAM_PICK_ARGS) {
    rat_param_rng rng;
    rng.gen = (zpn == nullptr && zpu == nullptr);
    rng.zn = (rng.gen || RAT_PARAM_NORMALS == 0) ? nullptr : zpn + g * (long)RAT_PARAM_NORMALS;
    rng.zu = (rng.gen || RAT_PARAM_UNIFORMS == 0) ? nullptr : zpu + g * (long)RAT_PARAM_UNIFORMS;
    rng.g0 = (unsigned)g; rng.g1 = (unsigned)(g >> 32);
    rng.k0 = (unsigned)seed; rng.k1 = (unsigned)(seed >> 32);
    rng.in = 0; rng.iu = 0; rng.over = 0; rng.spare_n = 0.0; rng.spare_u = 0.0;
#ifdef RAT_PARAM_SHIFT
    rng.shift = pshift; rng.logw = 0.0;
#endif
#ifdef RAT_RNG_PICK
    rng.kb0 = (unsigned)seed_b; rng.kb1 = (unsigned)(seed_b >> 32); rng.pick_n = pick_pn; rng.pick_u = pick_pu;
#endif
    bool inok = true;
#pragma unroll
    for (int i = 0; i < RAT_N_PARAMS; ++i) { q[i] = p[i]; inok = inok && !src_nan(q[i]); }
    rat_user_params(rng, p, q);
    bool outnan = false;
#pragma unroll
    for (int i = 0; i < RAT_N_PARAMS; ++i) outnan = outnan || src_nan(q[i]);
    over |= rng.over << 2;
#ifdef RAT_PARAM_SHIFT
    logw = rng.logw;
#endif
    return inok && outnan;
}

#ifdef RAT_PARAMS_SAMPLE_KERNEL
// rat_policy_params_sample: the hook alone for rollouts j0 .. j0 + K - 1, one lane each; q_out [K][RAT_N_PARAMS], rollout slowest
extern "C" __global__ __launch_bounds__(64) void rat_src_params_sample(SrcParamsArgs a) {
    const long j = (long)blockIdx.x * 64 + threadIdx.x;
    if (j >= a.K) return;
    double q[RAT_N_PARAMS];
    int over = 0;
    (void)rat_src_params(j + a.j0, a.seed, a.zpn, a.zpu, a.p, q, over);
#pragma unroll
    for (int i = 0; i < RAT_N_PARAMS; ++i) a.q_out[j * (long)RAT_N_PARAMS + i] = q[i];
    if (over) *a.overdraw = over;
}
#endif
#elif defined(RAT_PARAMS_SAMPLE_KERNEL)
#error "rat_policy_params_sample is compiled with parameter sampling on"
#elif defined(RAT_PARAM_SHIFT)
#error "RAT_PARAM_SHIFT needs parameter sampling on (rat_policy_params_sampling)"
#endif

// What a rollout hands the user's functions as p: the problem's, or with parameter sampling on its own, drawn once in front of step 0.
// Without RAT_USER_PARAMS_ON the type is empty, draw() does nothing and of() is its argument: no q[] exists.
struct src_rollout_params {
#ifdef RAT_USER_PARAMS_ON
    double q[RAT_N_PARAMS];
    // rat_src_params: true for the DomainError of a NaN parameter; the hook's overdraw bits go to `over` (and under RAT_PARAM_SHIFT the
    // parameter part of the rollout's likelihood ratio to `logw`)
    __device__ __forceinline__ bool draw(long g, unsigned long long seed, const double *zpn, const double *zpu, const double *p,
                                         int &over RAT_PARAM_SHIFT_ARGS RAT_PARAM_PICK_ARGS) {
        return rat_src_params(g, seed, zpn, zpu, p, q, over RAT_PARAM_SHIFT_PASS RAT_PARAM_PICK_PASS);
    }
    __device__ __forceinline__ const double *of(const double *) const { return q; }
#else
    __device__ __forceinline__ bool draw(long, unsigned long long, const double *, const double *, const double *, int & RAT_PARAM_PICK_ARGS) { return false; }
    __device__ __forceinline__ const double *of(const double *p) const { return p; }
#endif
};

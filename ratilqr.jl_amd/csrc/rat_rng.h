// rat_rng.h -- the random-number source a generative source model draws from (rat_user_f_stochastic, include/ratilqr.h "Generative source
// models"): rng.normal() is N(0, 1), rng.uniform() is U[0, 1).  Compiled by hiprtc in front of the user's source; RAT_PETS_NORMALS and
// RAT_PETS_UNIFORMS (the declared draws per step) come from the command line.  The library embeds this header (Makefile: source_embed.inc).
//
// The i-th normal / uniform of trajectory j at step t:
//   injected   zn[(j N + t) RAT_PETS_NORMALS + i],  zu[(j N + t) RAT_PETS_UNIFORMS + i]   (j counted from the launch's first trajectory)
//   generator  Philox4x32-10 (rat_philox.h), key (seed lo, seed hi), with g = j + traj0 the global trajectory index:
//                normals   counter (g lo, g hi, t, i / 2): two 53-bit uniforms (u01(r0, r1), u01(r2, r3)), Box-Muller (rat_normal.h)
//                          -> (z0, z1); normal 2q is z0, normal 2q + 1 is z1
//                uniforms  counter (g lo, g hi, t, 0x80000000 | i / 2): uniform 2q is u01(r0, r1), uniform 2q + 1 is u01(r2, r3)
// A draw beyond the declared count returns NaN and records the overdraw (bit 0 normals, bit 1 uniforms).
//
// RAT_RNG_SHIFT (defined by source_rare.h alone, rat_policy_rare_event_noise): the i-th normal of a step is drawn from the shifted
// proposal, z = shift[i] + xi with xi the draw above, and the log-likelihood ratio of the draw, -s z + s^2 / 2, is added to logw at the
// draw, in draw order -- a sequential likelihood ratio, valid when the number of draws depends on earlier draws.  Uniforms are not
// shifted.  Without the macro RAT_RNG_NORMAL is the identity and the struct has no further member.
//
// RAT_RNG_PICK (the command line of source_sobol.h's module alone, rat_policy_sobol): every generator draw comes from one of two streams,
// the one above under key (k0, k1) or the same counters under a second key (kb0, kb1).  Bit i of pick_n / pick_u says that normal /
// uniform i of every step is the second stream's; the draw is bit for bit what the plain generator yields under that stream's seed for
// (g, t, i), the pairing included: normal 2q is z0 and normal 2q + 1 is z1 of block q of its OWN stream.  The spare of a block serves
// draw 2q + 1 only where draws 2q and 2q + 1 have the same key; otherwise draw 2q + 1 runs block q of its own stream and takes the second
// output.  Keys and masks are the same for a whole wavefront and a draw's index is a constant once the user's loops are unrolled, so the
// choice is a scalar select.  Without the macro the header preprocesses to what it was.  Not combined with RAT_RNG_SHIFT.
#pragma once
#include "rat_normal.h"
#include "rat_philox.h"

#if !defined(RAT_PETS_NORMALS) || !defined(RAT_PETS_UNIFORMS)
#error "RAT_PETS_NORMALS and RAT_PETS_UNIFORMS must be defined"
#endif

#if defined(RAT_RNG_PICK) && defined(RAT_RNG_SHIFT)
#error "RAT_RNG_PICK is not combined with RAT_RNG_SHIFT"
#endif
#if defined(RAT_RNG_PICK) && (RAT_PETS_NORMALS > 64 || RAT_PETS_UNIFORMS > 64)
#error "rat_policy_sobol masks at most 64 normals and 64 uniforms per step"
#endif

#ifdef RAT_RNG_SHIFT
#define RAT_RNG_NORMAL(i, xi) proposal(i, xi)
#else
#define RAT_RNG_NORMAL(i, xi) xi
#endif

struct rat_rng {
    const double *zn, *zu;        // injected: this (trajectory, step)'s slots; generator: null
    bool gen;
    unsigned g0, g1, t, k0, k1;   // generator: counter words of this (trajectory, step), key
    int in, iu, over;
    double spare_n, spare_u;      // the second output of the last generator block
#ifdef RAT_RNG_PICK
    unsigned kb0, kb1;            // the second stream's key
    unsigned long long pick_n, pick_u;   // bit i: normal / uniform i of a step is the second stream's
#endif
#ifdef RAT_RNG_SHIFT
    const double *shift;          // the step's shift row [RAT_PETS_NORMALS]: one address for the whole wavefront
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
        if (i >= RAT_PETS_NORMALS) { over |= 1; return __builtin_nan(""); }
        if (!gen) return zn[i];
#ifdef RAT_RNG_PICK
        const bool b = (pick_n >> i) & 1;
        if ((i & 1) && b == (bool)((pick_n >> (i - 1)) & 1)) return spare_n;
        unsigned r[4];
        philox4x32_10(g0, g1, t, (unsigned)(i >> 1), b ? kb0 : k0, b ? kb1 : k1, r);
        double z0, z1;
        ratn_box_muller(u01(r[0], r[1]), u01(r[2], r[3]), &z0, &z1);
        if (i & 1) return z1;                                         // (its neighbour came from the other stream)
        spare_n = z1;
        return z0;
#else
        if (i & 1) return RAT_RNG_NORMAL(i, spare_n);
        unsigned r[4];
        philox4x32_10(g0, g1, t, (unsigned)(i >> 1), k0, k1, r);
        double z0;
        ratn_box_muller(u01(r[0], r[1]), u01(r[2], r[3]), &z0, &spare_n);
        return RAT_RNG_NORMAL(i, z0);
#endif
    }
    __device__ __forceinline__ double uniform() {
        const int i = iu++;
        if (i >= RAT_PETS_UNIFORMS) { over |= 2; return __builtin_nan(""); }
        if (!gen) return zu[i];
#ifdef RAT_RNG_PICK
        const bool b = (pick_u >> i) & 1;
        if ((i & 1) && b == (bool)((pick_u >> (i - 1)) & 1)) return spare_u;
        unsigned r[4];
        philox4x32_10(g0, g1, t, 0x80000000u | (unsigned)(i >> 1), b ? kb0 : k0, b ? kb1 : k1, r);
        if (i & 1) return u01(r[2], r[3]);
        spare_u = u01(r[2], r[3]);
        return u01(r[0], r[1]);
#else
        if (i & 1) return spare_u;
        unsigned r[4];
        philox4x32_10(g0, g1, t, 0x80000000u | (unsigned)(i >> 1), k0, k1, r);
        spare_u = u01(r[2], r[3]);
        return u01(r[0], r[1]);
#endif
    }
};

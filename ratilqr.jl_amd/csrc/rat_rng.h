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
#pragma once
#include "rat_normal.h"
#include "rat_philox.h"

#if !defined(RAT_PETS_NORMALS) || !defined(RAT_PETS_UNIFORMS)
#error "RAT_PETS_NORMALS and RAT_PETS_UNIFORMS must be defined"
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
        if (i & 1) return RAT_RNG_NORMAL(i, spare_n);
        unsigned r[4];
        philox4x32_10(g0, g1, t, (unsigned)(i >> 1), k0, k1, r);
        double z0;
        ratn_box_muller(u01(r[0], r[1]), u01(r[2], r[3]), &z0, &spare_n);
        return RAT_RNG_NORMAL(i, z0);
    }
    __device__ __forceinline__ double uniform() {
        const int i = iu++;
        if (i >= RAT_PETS_UNIFORMS) { over |= 2; return __builtin_nan(""); }
        if (!gen) return zu[i];
        if (i & 1) return spare_u;
        unsigned r[4];
        philox4x32_10(g0, g1, t, 0x80000000u | (unsigned)(i >> 1), k0, k1, r);
        spare_u = u01(r[2], r[3]);
        return u01(r[0], r[1]);
    }
};

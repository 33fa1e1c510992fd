// source_policy.h -- the controller the user writes (rat_user_policy, include/ratilqr.h "Source models"), as the Monte-Carlo rollout
// kernels of source models apply it: rat_src_noisy_rollout (source_noisy.h), rat_src_user_noisy_rollout (source_user_noise.h) and both
// variants of rat_src_rare_rollout (source_rare.h) include this header and call the one function below, once per step, behind the affine
// law and in front of everything that reads u -- the trajectory outputs, the cost, the sampler, f, the events.  The solver's own kernels
// (source_kernels.h), PETS (source_pets.h) and rat_src_user_events (source_events.h, which reads the u a rollout kernel wrote) do not
// include it: iLEQG stays the reference's algorithm.  Without RAT_USER_POLICY the header is empty and the kernels hold no u_prev: a
// source without the hook compiles to what it compiled to before.  The NaN tests below stay spelt out, not src_nan (source_step.h): with
// the predicate one row of the kernels' resource table moves (profiles/source_step.md).
#pragma once

#ifdef RAT_USER_POLICY
// The step's hook.  u arrives holding the affine law's control (l_k open loop) and leaves holding the applied one; u_prev arrives holding
// the control applied at step k - 1 (the caller zeroes it in front of step 0) and leaves holding u.  x: 12 entries, RAT_N live; u, u_prev:
// 4 entries, RAT_M live.  Returns true where the hook put a NaN into u[0 .. RAT_M) although x and the affine u had none: the rollout's
// DomainError, as a NaN from f is (the caller sets dom; c then sees the NaN as well).  A hook that leaves u alone changes no bit.
__device__ __forceinline__ bool rat_src_policy(int k, const double (&x)[12], double (&u)[4], double (&u_prev)[4], const double *p) {
    bool inok = true;
#pragma unroll
    for (int q = 0; q < RAT_N; ++q) inok = inok && !(x[q] != x[q]);
#pragma unroll
    for (int q = 0; q < RAT_M; ++q) inok = inok && !(u[q] != u[q]);
    rat_user_policy(k, x, u_prev, u, p);
    bool outnan = false;
#pragma unroll
    for (int q = 0; q < RAT_M; ++q) outnan = outnan || (u[q] != u[q]);
#pragma unroll
    for (int q = 0; q < 4; ++q) u_prev[q] = u[q];
    return inok && outnan;
}
#endif

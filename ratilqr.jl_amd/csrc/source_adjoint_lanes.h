// source_adjoint_lanes.h -- what the adjoint sweeps (source_adjoint.h, source_adjoint_params.h) share: the exchange within a team of
// lanes and the finiteness test of a sensitivity.
#pragma once

// the value lane `src` of the wavefront holds (no <hip/hip_runtime.h> under hiprtc): both halves through ds_bpermute
__device__ __forceinline__ double adj_from(double v, int src) {
    int w[2];
    __builtin_memcpy(w, &v, 8);
    w[0] = __builtin_amdgcn_ds_bpermute(src << 2, w[0]);
    w[1] = __builtin_amdgcn_ds_bpermute(src << 2, w[1]);
    double r;
    __builtin_memcpy(&r, w, 8);
    return r;
}
__device__ __forceinline__ bool adj_finite(double v) { return __builtin_fabs(v) < __builtin_inf(); }

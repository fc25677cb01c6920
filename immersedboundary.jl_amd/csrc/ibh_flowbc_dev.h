// libibhip: device bodies of the FlowBC call (cfd.jl:243-300) and of Sutherland's law (cfd.jl:71-77) -- shared by the
// pointwise kernels of ibh_cfd.hip and the fused boundary-condition kernel of ibh_bcflow.hip.  Float32, the reference's
// evaluation order (-ffp-contract=off).
#pragma once
#include "ibh_common.h"

namespace flowbc_dev {

__device__ __forceinline__ float sutherland(const ibh_fluid& f, float T) {
    T = ibh_max(T, 10.0f);
    // mu_ref * ((T/Tref)^(2/3)) * (Tref + S) / (T + S)     (cfd.jl:75, exponent as in the reference)
    // x^(2/3) = exp2(2/3 log2 x) on the transcendental unit (v_log_f32 / v_exp_f32, 1 ulp each) instead of the ~100
    // instructions of the library's powf -- a third of a viscous face flux.  The whole viscosity stays within 10 ulps of
    // the float64 evaluation for T in [10, 1e5] K (x in [0.037, 366]; tests/test_gpu_percell_closures.py::test_pointwise_edges)
    return f.mu_ref * __builtin_amdgcn_exp2f((2.0f / 3.0f) * __builtin_amdgcn_logf(T / f.Tref)) * (f.Tref + f.S) / (T + f.S);
}

// Julia's `b * y` for a Bool b: `false` is a strong zero (false * NaN == 0, with the sign of y); `b ? y : 0` otherwise
__device__ __forceinline__ float jl_bool_times(bool b, float y) { return b ? y : copysignf(0.0f, y); }

// The FlowBC call at one point: boundary state (pb, Tb, ub) from the image-point primitives (p, T, u) and the unit normal.
// normal_flow: uinf[0] is the normal velocity and `transp` is added to it; with_dudn: the wall-function slip scaling
// (:287-292) with du!dn and the image distance.
template <int ND>
__device__ __forceinline__ void flow_bc_point(const ibh_fluid& f, float p, float T, const float* u, const float* nn,
                                              float pinf, float Tinf, const float* uinf, int normal_flow, bool with_dudn,
                                              float dudn, float imd, float transp, float& pb, float& Tb, float* ub) {
    float un, cur = u[0] * nn[0];
#pragma unroll
    for (int j = 1; j < ND; ++j) cur = cur + u[j] * nn[j];
    if (normal_flow) {
        un = uinf[0];
    } else {
        un = nn[0] * uinf[0];
#pragma unroll
        for (int j = 1; j < ND; ++j) un = un + nn[j] * uinf[j];
    }
    const float a = sqrtf(f.gamma * f.R * ibh_max(T, 10.0f));
    const float M = fabsf(un) / a;
    // (un >= 0) * ((M > 1) * p_inf + (M <= 1) * p) + (un < 0) * ((M > 1) * p + (M <= 1) * p_inf) with Julia's Bool
    // weights: a NaN Mach number (NaN temperature) makes every weight false and pb = 0, a NaN under a false weight is 0
    pb = jl_bool_times(un >= 0.0f, jl_bool_times(M > 1.0f, pinf) + jl_bool_times(M <= 1.0f, p)) +
         jl_bool_times(un < 0.0f, jl_bool_times(M > 1.0f, p) + jl_bool_times(M <= 1.0f, pinf));
    Tb = jl_bool_times(un > 0.0f, Tinf) + jl_bool_times(un <= 0.0f, T);
    if (normal_flow) {
        const float d = un - cur + transp;
#pragma unroll
        for (int j = 0; j < ND; ++j) ub[j] = u[j] + nn[j] * d;
    } else {
#pragma unroll
        for (int j = 0; j < ND; ++j) ub[j] = (un < 0.0f) ? u[j] : uinf[j];
    }
    if (with_dudn) {
        float V = ub[0] * ub[0];
#pragma unroll
        for (int j = 1; j < ND; ++j) V = V + ub[j] * ub[j];
        V = sqrtf(V) + 1.1920929e-07f;
        const float sc = (V - dudn * imd) / V;
#pragma unroll
        for (int j = 0; j < ND; ++j) ub[j] = ub[j] * sc;
    }
}

}  // namespace flowbc_dev

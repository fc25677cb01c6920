// libibhip: the conservative update of an explicit Euler step for ONE row, in its three forms
//     P_out = state2primitive([primitive2state(P0) * a + b *] primitive2state(base) + (c * dt) * R)
//                                                                     (cfd.jl:106-123, :137-151 around advection.jl:87)
// and the pseudo-time stage of a dual time step (not in the reference), with h = c * dt,
//     P_out = state2primitive((primitive2state(P0) + (R + S) * h) / (1 + h * g))
// as device functions: the bodies of the ibh_update_euler* kernels (ibh_march.hip) and the store epilogue of the 2-D
// single-kernel Euler sweeps (ibh_quad2d_euler.h, ibh_sweep2d.h: ibh_step_euler, ibh_stage_euler, ibh_stage_euler_ssp in one
// launch).  The formulas and their order are those of k_p2s, k_update_dev and k_s2p (ibh_cfd.hip, ibh_march.hip) -- both
// max(T, 10) clamps, k / 2 -- so the result is bit for bit the separate launches'.  The tuned sweep bodies are compiled with
// contraction on; these functions must not be: their expressions carry contract(off) wherever they are inlined.
#pragma once
#include "ibh_common.h"

// What a sweep or an update kernel stores.  Each form takes everything the previous one takes:
//   FORM_RESIDUAL  R(P)                                                                              (the sweeps alone)
//   FORM_STEP      s2p(p2s(P) + dt R)                                       ibh_update_euler, ibh_step_euler
//   FORM_STAGE     s2p(p2s(P0) + (c dt) R): a low-storage Runge-Kutta stage  ibh_update_euler_stage, ibh_stage_euler
//   FORM_SSP       s2p((p2s(P0) a + p2s(P) b) + (c dt) R): a Shu-Osher stage  ibh_update_euler_ssp, ibh_stage_euler_ssp
//   FORM_DUAL      s2p((p2s(P0) + (R + S) (c dt)) / (1 + (c dt) g)): a pseudo-time stage of a dual time step, the physical
//                  time derivative g Q - S taken point-implicitly.  It reads what FORM_STAGE reads (not the swept state, as
//                  FORM_SSP does) and the source S         ibh_update_euler_dual, ibh_stage_euler_dual
enum EulerForm : int { FORM_RESIDUAL = 0, FORM_STEP, FORM_STAGE, FORM_SSP, FORM_DUAL };

namespace euler_step {

// what a form takes beside the swept state, its residual and dt.  FORM_STEP reads nothing of it; FORM_STAGE reads the base
// state P0 (leading dimension ld0; it may be the output), the coefficient c of dt and, for a per-cell time step, the nc
// values dtc (dt is then unused); FORM_SSP also reads a and b, the weights of the base state and of the swept state;
// FORM_DUAL reads, instead of a and b, the source S of the physical step (conserved variables, leading dimension lds) and g,
// the coefficient of Q^{n+1} in its backward difference
struct FormArgs {
    const float* P0 = nullptr; uint32_t ld0 = 0; float c = 1.0f; const float* dtc = nullptr;
    float a = 0.0f, b = 1.0f;
    const float* S = nullptr; uint32_t lds = 0; float g = 0.0f;
};

// the time step of a stage: one IEEE multiply, the broadcast dt .* c
__device__ __forceinline__ float stage_dt(float c, float dt) {
#pragma clang fp contract(off)
    return c * dt;
}

// primitive2state of one row (k_p2s): P = [p T u v (w)], Q = [rho E rho*u rho*v (rho*w)]
template <int ND>
__device__ __forceinline__ void p2s_row(float Rgas, float gamma, const float (&P)[ND + 2], float (&Q)[ND + 2]) {
#pragma clang fp contract(off)  // (scoped to this body: the including header's own setting is left alone)
    const float p0 = P[0], T = ibh_max(P[1], 10.0f);
    float k = P[2] * P[2];
#pragma unroll
    for (int j = 1; j < ND; ++j) k = k + P[2 + j] * P[2 + j];
    k = k / 2.0f;
    const float rho0 = p0 / (Rgas * T);
    Q[0] = rho0;
    Q[1] = rho0 * (Rgas / (gamma - 1.0f) * T + k);
#pragma unroll
    for (int j = 0; j < ND; ++j) Q[2 + j] = rho0 * P[2 + j];
}

// state2primitive of one row (k_s2p)
template <int ND>
__device__ __forceinline__ void s2p_row(float Rgas, float gamma, const float (&Q)[ND + 2], float (&out)[ND + 2]) {
#pragma clang fp contract(off)
    const float rho = Q[0], E = Q[1];
    float u[ND];
    float k2 = 0.f;
#pragma unroll
    for (int j = 0; j < ND; ++j) {
        u[j] = Q[2 + j] / rho;
        k2 = (j == 0) ? u[j] * u[j] : k2 + u[j] * u[j];
    }
    k2 = k2 / 2.0f;
    const float p = (gamma - 1.0f) * (E - rho * k2);
    out[0] = p;
    out[1] = ibh_max(p / (rho * Rgas), 10.0f);
#pragma unroll
    for (int j = 0; j < ND; ++j) out[2 + j] = u[j];
}

// FORM_STEP and, on the row of the base state with h = stage_dt(c, dt), FORM_STAGE: Q = primitive2state(P) + r * h per
// component (k_update_dev).  r = residuals of [rho E rho*u rho*v (rho*w)], out may be P
template <int ND>
__device__ __forceinline__ void update_row(float Rgas, float gamma, const float (&P)[ND + 2], const float (&r)[ND + 2],
                                           float h, float (&out)[ND + 2]) {
#pragma clang fp contract(off)
    float Q[ND + 2];
    p2s_row<ND>(Rgas, gamma, P, Q);
#pragma unroll
    for (int v = 0; v < ND + 2; ++v) Q[v] = Q[v] + r[v] * h;
    s2p_row<ND>(Rgas, gamma, Q, out);
}

// FORM_SSP: Q = (primitive2state(P0) * a + primitive2state(P) * b) + r * h per component, in this order and without
// contraction -- the broadcasts Q0 .* a .+ Q .* b, then k_update_dev.  No term is dropped for a == 0 or b == 0: that would
// change the sign of zeros.  out may be P0 or P
template <int ND>
__device__ __forceinline__ void blend_row(float Rgas, float gamma, const float (&P0)[ND + 2], const float (&P)[ND + 2],
                                          const float (&r)[ND + 2], float a, float b, float h, float (&out)[ND + 2]) {
#pragma clang fp contract(off)
    float Q0[ND + 2], Q[ND + 2];
    p2s_row<ND>(Rgas, gamma, P0, Q0);
    p2s_row<ND>(Rgas, gamma, P, Q);
#pragma unroll
    for (int v = 0; v < ND + 2; ++v) Q[v] = (Q0[v] * a + Q[v] * b) + r[v] * h;
    s2p_row<ND>(Rgas, gamma, Q, out);
}

// FORM_DUAL on the row of the base state, h = stage_dt(c, dt): Q = (primitive2state(P0) + (r + s) * h) / (1 + h * g) per
// component -- the broadcasts R .+ S and h .* g .+ 1, k_update_dev, the broadcast ./ -- every sum, product and the (IEEE)
// divide rounded on its own, in this order.  s = the row of the source S, g >= 0.  With g == 0 and s == 0 this is update_row
// up to the sign of a zero (r + 0 and Q / 1).  out may be P0
template <int ND>
__device__ __forceinline__ void dual_row(float Rgas, float gamma, const float (&P0)[ND + 2], const float (&r)[ND + 2],
                                         const float (&s)[ND + 2], float h, float g, float (&out)[ND + 2]) {
#pragma clang fp contract(off)
    float Q[ND + 2];
    p2s_row<ND>(Rgas, gamma, P0, Q);
    const float den = h * g + 1.0f;
#pragma unroll
    for (int v = 0; v < ND + 2; ++v) Q[v] = (Q[v] + (r[v] + s[v]) * h) / den;
    s2p_row<ND>(Rgas, gamma, Q, out);
}

// The source of a physical step for one row, S = primitive2state(Pn) * cn [+ primitive2state(Pm) * cm] (BDF2: both terms;
// BDF1: the first alone): the broadcasts Qn .* cn .+ Qm .* cm, each product and the sum rounded on its own
template <int ND, bool BDF2>
__device__ __forceinline__ void dual_source_row(float Rgas, float gamma, const float (&Pn)[ND + 2], const float (&Pm)[ND + 2],
                                                float cn, float cm, float (&S)[ND + 2]) {
#pragma clang fp contract(off)
    float Qn[ND + 2], Qm[ND + 2];
    p2s_row<ND>(Rgas, gamma, Pn, Qn);
    if constexpr (BDF2) p2s_row<ND>(Rgas, gamma, Pm, Qm);
#pragma unroll
    for (int v = 0; v < ND + 2; ++v) {
        if constexpr (BDF2) S[v] = Qn[v] * cn + Qm[v] * cm;
        else S[v] = Qn[v] * cn;
    }
}

}  // namespace euler_step

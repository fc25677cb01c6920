// libibhip: the conservative update of an explicit Euler step for ONE row,
//     P_out = state2primitive(primitive2state(P) + dt * R)           (cfd.jl:106-123, :137-151 around advection.jl:87)
// as one device function: the body of ibh_update_euler (ibh_march.hip) and the store epilogue of the 2-D single-kernel Euler
// sweeps in their STEP form (ibh_quad2d_euler.h, ibh_sweep2d.h: ibh_step_euler in one launch).  The formulas and their order
// are those of k_p2s, k_update_dev and k_s2p (ibh_cfd.hip, ibh_march.hip) -- both max(T, 10) clamps, k / 2 -- so the result
// is bit for bit the three launches'.  The tuned sweep bodies are compiled with contraction on; this function must not be:
// its expressions carry contract(off) wherever they are inlined.
// A Runge-Kutta stage of the low-storage family (ibh_update_euler_stage, ibh_stage_euler; the STAGE form of the sweeps) is
// the same row function on a base state P0 that need not be the state the residual was swept from, with the time step
// stage_dt(alpha, dt): P_out = state2primitive(primitive2state(P0) + (alpha * dt) R).
// A Shu-Osher stage of a strong-stability-preserving scheme (ibh_update_euler_ssp, ibh_stage_euler_ssp; the SSP form of the
// sweeps) blends two states before the update: blend_row, P_out = state2primitive((primitive2state(P0) * a +
// primitive2state(P) * b) + R * stage_dt(c, dt)), every product and sum rounded on its own.
#pragma once
#include "ibh_common.h"

namespace euler_step {

// P = [p T u v (w)], r = residuals of [rho E rho*u rho*v (rho*w)], out may be P
template <int ND>
__device__ __forceinline__ void update_row(float Rgas, float gamma, const float (&P)[ND + 2], const float (&r)[ND + 2],
                                           float dt, float (&out)[ND + 2]) {
#pragma clang fp contract(off)  // (scoped to this body: the including header's own setting is left alone)
    // primitive2state (k_p2s)
    const float p0 = P[0], T = ibh_max(P[1], 10.0f);
    float k = P[2] * P[2];
#pragma unroll
    for (int j = 1; j < ND; ++j) k = k + P[2 + j] * P[2 + j];
    k = k / 2.0f;
    const float rho0 = p0 / (Rgas * T);
    float Q[ND + 2];
    Q[0] = rho0;
    Q[1] = rho0 * (Rgas / (gamma - 1.0f) * T + k);
#pragma unroll
    for (int j = 0; j < ND; ++j) Q[2 + j] = rho0 * P[2 + j];
    // Q += dt * R (k_update_dev)
#pragma unroll
    for (int v = 0; v < ND + 2; ++v) Q[v] = Q[v] + r[v] * dt;
    // state2primitive (k_s2p)
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

// what the STAGE form of a sweep takes beside dt: the base state (it may be the output), the stage coefficient and, for a
// per-cell time step, the nc values (dt is then unused)
// SSP form: a and b are the weights of the base state and of the swept state in the blend, alpha is the coefficient c of dt
struct StageArgs {
    const float* P0 = nullptr; uint32_t ld0 = 0; float alpha = 1.0f; const float* dtc = nullptr;
    float a = 0.0f, b = 1.0f;
};

// the time step of a stage: one IEEE multiply, the broadcast dt .* alpha
__device__ __forceinline__ float stage_dt(float alpha, float dt) {
#pragma clang fp contract(off)
    return alpha * dt;
}

// primitive2state of one row (k_p2s): the lines update_row opens with
template <int ND>
__device__ __forceinline__ void p2s_row(float Rgas, float gamma, const float (&P)[ND + 2], float (&Q)[ND + 2]) {
#pragma clang fp contract(off)
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

// A Shu-Osher stage for one row: Q_new = (primitive2state(P0) * a + primitive2state(P) * b) + r * h per component, in this
// order and without contraction -- the broadcasts Q0 .* a .+ Q .* b, then k_update_dev -- and out = state2primitive(Q_new)
// (k_s2p).  No term is dropped for a == 0 or b == 0: that would change the sign of zeros.  out may be P0 or P
template <int ND>
__device__ __forceinline__ void blend_row(float Rgas, float gamma, const float (&P0)[ND + 2], const float (&P)[ND + 2],
                                          const float (&r)[ND + 2], float a, float b, float h, float (&out)[ND + 2]) {
#pragma clang fp contract(off)
    float Q0[ND + 2], Q[ND + 2];
    p2s_row<ND>(Rgas, gamma, P0, Q0);
    p2s_row<ND>(Rgas, gamma, P, Q);
#pragma unroll
    for (int v = 0; v < ND + 2; ++v) Q[v] = (Q0[v] * a + Q[v] * b) + r[v] * h;
    // state2primitive (k_s2p)
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

}  // namespace euler_step

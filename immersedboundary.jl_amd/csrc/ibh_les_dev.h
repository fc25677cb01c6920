// libibhip: device bodies of the pointwise LES closures and shock sensors over a register table g[ND][ND],
// g[i][j] = d u_i / d x_j -- shear_rate (turbulence.jl:110-124), Smagorinsky_νSGS (:134-137), Ducros_sensor (:253-283),
// WALE_νSGS (:292-337) and CFD.shock_sensor (cfd.jl:589-617) -- and of Wray_Agarwal (:222-241) at one cell, shared by the
// pointwise kernels of ibh_turb.hip / ibh_cfd.hip and the fused closures that consume cell_gradient where it is made:
// ibh_les_of (k_les_of3 and k_les_of_cells in ibh_turb.hip), ibh_shear_rate_of_velocity[_grad]
// (k_shear_of_velocity3, k_shear_of_velocity_cells), ibh_k_epsilon_rhs (k_k_epsilon_rhs3, k_k_epsilon_rhs_cells: shear_rate)
// and ibh_wray_agarwal_of (k_wray_agarwal_of3, k_wray_agarwal_of_cells).  Float32, the reference's operation order
// (-ffp-contract=off).
#pragma once
#include "ibh_common.h"

namespace les_dev {

constexpr float EPS32 = 1.1920929e-07f;   // eps(Float32): Ducros_sensor, WALE_νSGS
constexpr float EPS_SHOCK = 1e-14f;       // 1f-14: CFD.shock_sensor

enum : int { MODEL_NONE = 0, MODEL_SMAGORINSKY = 1, MODEL_WALE = 2 };

// what ibh_les_of writes (each pointer may be null; the choice is uniform over a launch)
struct Outputs {
    float *nusgs, *ducros, *shock, *S, *G;
    int64_t ldg;
};

// shear_rate: sqrt(2 Sij Sij)
template <int ND>
__device__ __forceinline__ float shear_rate(const float (&g)[ND][ND]) {
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < ND; ++i)
#pragma unroll
        for (int j = 0; j < ND; ++j) {
            const float t = (g[i][j] + g[j][i]) / 2.0f;
            s = s + t * t;
        }
    return sqrtf(2.0f * s);
}

// Smagorinsky_νSGS: (Cs Δ)^2 S
__device__ __forceinline__ float smagorinsky(float Delta, float S, float Cs) {
    const float t = Cs * Delta;
    return t * t * S;
}

// Ducros_sensor: (div^2 + eps) / (div^2 + |curl|^2 + eps)
template <int ND>
__device__ __forceinline__ float ducros(const float (&g)[ND][ND]) {
    float div = 0.0f;
#pragma unroll
    for (int i = 0; i < ND; ++i) div = div + g[i][i];
    const float div2 = div * div;
    float curl2;
    if constexpr (ND == 2) {
        const float w = g[1][0] - g[0][1];
        curl2 = w * w;
    } else {
        const float a = g[2][1] - g[1][2];
        const float b = g[0][2] - g[2][0];
        const float d = g[1][0] - g[0][1];
        curl2 = a * a + b * b + d * d;
    }
    return (div2 + EPS32) / (div2 + curl2 + EPS32);
}

// WALE_νSGS, the invariants: SS = Sij Sij, SdSd = Sdij Sdij of the traceless symmetric part of g^2
__device__ __forceinline__ void wale_invariants(const float (&g)[3][3], float& SS, float& SdSd) {
    float g2[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            float s = 0.0f;
#pragma unroll
            for (int k = 0; k < 3; ++k) s = s + g[i][k] * g[k][j];
            g2[i][j] = s;
        }
    SS = 0.0f;
    SdSd = 0.0f;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float t = (g[i][j] + g[j][i]) / 2.0f;
            SS = SS + t * t;
            const float dlt = (i == j) ? (1.0f / 3.0f) : 0.0f;
            const float q = (g2[i][j] + g2[j][i]) / 2.0f - g2[i][j] * dlt;
            SdSd = SdSd + q * q;
        }
}
// ... and the model from them: Cw Δ^2 SdSd^(3/2) / (SS^(5/2) + SdSd^(5/4) + eps)
__device__ __forceinline__ float wale_of_invariants(float Delta, float SS, float SdSd, float Cw) {
    return Cw * (Delta * Delta) * powf(SdSd, 1.5f) / (powf(SS, 2.5f) + powf(SdSd, 1.25f) + EPS32);
}
__device__ __forceinline__ float wale(const float (&g)[3][3], float Delta, float Cw) {
    float SS, SdSd;
    wale_invariants(g, SS, SdSd);
    return wale_of_invariants(Delta, SS, SdSd, Cw);
}

// CFD.shock_sensor: as Ducros with eps = 1f-14; in 2-D both trips of the loop visit the one vorticity component (2 w^2),
// as the reference
template <int ND>
__device__ __forceinline__ float shock(const float (&g)[ND][ND]) {
    float divu = 0.0f, vort2 = 0.0f;
#pragma unroll
    for (int i = 0; i < ND; ++i) {
        const int in = (i + 1) % ND, inn = (in + 1) % ND;
        divu = divu + g[i][i];
        const float w = g[inn][in] - g[in][inn];
        vort2 = vort2 + w * w;
    }
    divu = divu * divu;
    return (divu + EPS_SHOCK) / (divu + vort2 + EPS_SHOCK);
}

// Wray_Agarwal (turbulence.jl:222-241) at one cell, dot = grad R . grad S and C2 = sigmaR + C1 / kappa^2:
// nut = R, nuR = sigmaR R, S = min(C1 R S + C2 dot R / (S + eps), 10 R)
struct WrayAgarwal {
    float nut, nuR, S;
};
__device__ __forceinline__ WrayAgarwal wray_agarwal(float r, float s, float dot, float sigmaR, float C1, float C2) {
    const float src = C1 * r * s + C2 * dot * (r / (s + EPS32));
    return {r, r * sigmaR, ibh_min(src, 10.0f * r)};
}

// the register table of cell c from an nd x nd table of device pointers, G[i * ND + j] = d u_i / d x_j
template <int ND>
__device__ __forceinline__ void load_table(const float* const (&G)[9], int64_t c, float (&g)[ND][ND]) {
#pragma unroll
    for (int i = 0; i < ND; ++i)
#pragma unroll
        for (int j = 0; j < ND; ++j) g[i][j] = G[i * ND + j][c];
}

}  // namespace les_dev

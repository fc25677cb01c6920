// libibhip: device body of wall_function (turbulence.jl:11-100) -- shared by the pointwise kernels of ibh_turb.hip and the
// fused boundary-condition kernel of ibh_bcflow.hip.  Float32, the reference's operation order (-ffp-contract=off).
#pragma once
#include "ibh_common.h"

namespace wall_dev {

constexpr float EPS32 = 1.1920929e-07f;

struct WallParams {
    float kappa, C, A, beta, betastar, D, Aplus, omega;
    int n_iter;
};
inline WallParams wall_params(const float* p, int n_iter) {
    return WallParams{p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], n_iter};
}

__device__ __forceinline__ float von_karman(float yp, float kappa, float C) {
    return ibh_min(logf(ibh_max(yp, 1.0f)) / kappa + C, yp);  // :11-16
}

// wall_function(Rey) :27-70
__device__ __forceinline__ void wall_point(float Rey, const WallParams& w, float& yp, float& up, float& mup, float& kp,
                                           float& dudy) {
    Rey = ibh_clamp(fabsf(Rey), EPS32, INFINITY);  // clamp(abs(Rey), eps, Inf32)
    yp = sqrtf(Rey);
    up = 0.0f;
    for (int it = 0; it < w.n_iter; ++it) {
        up = von_karman(yp, w.kappa, w.C);
        yp = w.omega * (Rey / up) + (1.0f - w.omega) * yp;
    }
    up = Rey / yp;
    const float e = 1.0f - expf(-yp / w.A);
    mup = w.kappa * yp * (e * e);
    dudy = 1.0f / (1.0f + mup);
    kp = ibh_min(yp * yp / (6.0f * w.betastar / w.beta - 2.0f), w.D * expf(-yp / w.Aplus));
}

// wall_function(y, u, nu) :72-100 at one point
struct WallOut {
    float utau, nut, k, omega, eps, dudn;
};
__device__ __forceinline__ WallOut wall_eval(float y, float u, float nu, const WallParams& w) {
    float yp, up, mup, kp, dudy;
    wall_point(u * y / nu, w, yp, up, mup, kp, dudy);
    const float ut = u / up;
    const float nt = mup * nu;
    const float kk = kp * (ut * ut);
    const float om = kk / nt;
    WallOut o;
    o.utau = ut;
    o.nut = nt;
    o.k = kk;
    o.omega = om;
    o.eps = w.betastar * om * kk;
    o.dudn = dudy * (ut * ut) / nu;
    return o;
}

}  // namespace wall_dev

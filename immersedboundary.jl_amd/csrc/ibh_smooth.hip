// libibhip: implicit residual smoothing of an explicit march, device resident -- the third classic acceleration of a
// pseudo-time march beside the local time step and the multi-stage step.  Between the sweep and the update the residual R is
// replaced by n_iter Jacobi iterations on (I + eps L) S = R, L the unweighted Laplacian of the face graph (ibh_smooth_dev.h
// has the formula and its order):
//   * ibh_smooth_residual: n_iter iterations, one launch each, ping-pong between S and tmp so that the last one lands in S;
//   * ibh_update_euler_smoothed: ONE more iteration from (R, Sprev) inside the conservative update -- the smoothed row goes
//     from registers into euler_step::update_row (a low-storage stage) or blend_row (a Shu-Osher stage) and is never written.
// A smoothed stage with n_iter iterations is therefore the sweep, n_iter - 1 Jacobi launches and this update.
// Arithmetic: contract(off), IEEE divide; bit for bit tests/smooth_model.py and the composition of the two entries.
#include <cmath>

#include "ibh_common.h"
#include "ibh_euler_step_dev.h"
#include "ibh_smooth_dev.h"

#define SMOOTH_BLOCK 256
#define SMOOTH_MAX_NV 8

namespace {

using smooth::Faces;

// S = one Jacobi iteration from (R, Sprev): thread per cell, all NV variables of the cell in that thread (the side-table
// entries and the CSR walks are paid once per cell).  S aliases neither R nor Sprev: other threads gather Sprev
template <int ND, int NV>
__global__ __launch_bounds__(SMOOTH_BLOCK) void k_smooth_residual(int32_t nc, Faces G, const float* __restrict__ R, int64_t ldr,
                                                                  const float* __restrict__ Sprev, int64_t ldp, float eps,
                                                                  float* __restrict__ S, int64_t lds) {
    for (int64_t c = IBH_WG_X() * (int64_t)blockDim.x + threadIdx.x; c < nc; c += (int64_t)gridDim.x * blockDim.x) {
        float r[NV], o[NV];
#pragma unroll
        for (int v = 0; v < NV; ++v) r[v] = R[c + v * ldr];
        smooth::smooth_row<ND, NV>(G, nc, (int32_t)c, r, Sprev, ldp, eps, o);
#pragma unroll
        for (int v = 0; v < NV; ++v) S[c + v * lds] = o[v];
    }
}

// The last Jacobi iteration fused with the update of the form: FORM_STAGE  P_out = s2p(p2s(P0) + (c dt) S),
// FORM_SSP  P_out = s2p((p2s(P0) a + p2s(P) b) + (c dt) S), S = smooth_row(R, Sprev) of the cell.  The rows of P0 and P are
// read whole before the row of P_out is written (P_out may be either); R and Sprev are gathered by other threads, so P_out
// is neither (no __restrict__ on the states)
template <int ND, int FORM, bool PER_CELL>
__global__ __launch_bounds__(SMOOTH_BLOCK) void k_update_euler_smoothed(float Rgas, float gamma, int32_t nc, Faces G,
                                                                        const float* P0, int64_t ld0, const float* P,
                                                                        int64_t ldp, const float* __restrict__ R, int64_t ldr,
                                                                        const float* __restrict__ Sprev, int64_t lds, float eps,
                                                                        const float* __restrict__ dt, float a, float b, float cf,
                                                                        float* P_out, int64_t ldo) {
    static_assert(FORM == FORM_STAGE || FORM == FORM_SSP, "a smoothed update is a stage or a Shu-Osher stage");
    constexpr int NV = ND + 2;
    float h = 0.0f;
    if constexpr (!PER_CELL) h = euler_step::stage_dt(cf, *dt);
    for (int64_t c = IBH_WG_X() * (int64_t)blockDim.x + threadIdx.x; c < nc; c += (int64_t)gridDim.x * blockDim.x) {
        float r[NV], s[NV], Br[NV], o[NV];
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            r[v] = R[c + v * ldr];
            Br[v] = P0[c + v * ld0];
        }
        smooth::smooth_row<ND, NV>(G, nc, (int32_t)c, r, Sprev, lds, eps, s);
        if constexpr (PER_CELL) h = euler_step::stage_dt(cf, dt[c]);
        if constexpr (FORM == FORM_SSP) {
            float Pr[NV];
#pragma unroll
            for (int v = 0; v < NV; ++v) Pr[v] = P[c + v * ldp];
            euler_step::blend_row<ND>(Rgas, gamma, Br, Pr, s, a, b, h, o);
        } else {
            euler_step::update_row<ND>(Rgas, gamma, Br, s, h, o);
        }
#pragma unroll
        for (int v = 0; v < NV; ++v) P_out[c + v * ldo] = o[v];
    }
}

inline dim3 cells_grid(int32_t nc) { return dim3(ibh_grid_cap(nc, SMOOTH_BLOCK, 4096)); }

using SmoothKernel = decltype(&k_smooth_residual<2, 1>);
#define SMOOTH_ROW(ND)                                                                                                   \
    {k_smooth_residual<ND, 1>, k_smooth_residual<ND, 2>, k_smooth_residual<ND, 3>, k_smooth_residual<ND, 4>,             \
     k_smooth_residual<ND, 5>, k_smooth_residual<ND, 6>, k_smooth_residual<ND, 7>, k_smooth_residual<ND, 8>}
constexpr SmoothKernel smooth_kernels[2][SMOOTH_MAX_NV] = {SMOOTH_ROW(2), SMOOTH_ROW(3)};

using UpdateKernel = decltype(&k_update_euler_smoothed<2, FORM_STAGE, false>);
#define UPDATE_ROW(ND)                                                                                                   \
    {{k_update_euler_smoothed<ND, FORM_STAGE, false>, k_update_euler_smoothed<ND, FORM_STAGE, true>},                    \
     {k_update_euler_smoothed<ND, FORM_SSP, false>, k_update_euler_smoothed<ND, FORM_SSP, true>}}
constexpr UpdateKernel update_kernels[2][2][2] = {UPDATE_ROW(2), UPDATE_ROW(3)};   // [nd - 2][blend][per-cell dt]

inline bool eps_ok(float eps) { return eps >= 0.0f && std::isfinite(eps); }

}  // namespace

extern "C" {

int ibh_smooth_residual(const ibh_part* p, const float* R, int nv, int64_t ldr, float eps, int n_iter, float* S, int64_t lds,
                        float* tmp, int64_t ldt) {
    IBH_REQUIRE(p && R && S, "ibh_smooth_residual: null argument");
    IBH_REQUIRE(p->nd == 2 || p->nd == 3, "ibh_smooth_residual: nd must be 2 or 3");
    IBH_REQUIRE(nv >= 1 && nv <= SMOOTH_MAX_NV, "ibh_smooth_residual: nv must be 1 .. 8");
    IBH_REQUIRE(p->nc >= 0 && ldr >= p->nc && lds >= p->nc, "ibh_smooth_residual: a leading dimension is smaller than nc");
    IBH_REQUIRE(eps_ok(eps), "ibh_smooth_residual: eps must be finite and >= 0");
    IBH_REQUIRE(n_iter >= 1, "ibh_smooth_residual: n_iter must be >= 1");
    IBH_REQUIRE(n_iter == 1 || tmp, "ibh_smooth_residual: tmp must be given from n_iter = 2 (the ping-pong partner of S)");
    IBH_REQUIRE(n_iter == 1 || ldt >= p->nc, "ibh_smooth_residual: a leading dimension is smaller than nc");
    IBH_REQUIRE(S != R && (n_iter == 1 || (tmp != R && tmp != S)),
                "ibh_smooth_residual: S and tmp may alias neither each other nor R");
    if (p->nc == 0) return 0;
    IBH_REQUIRE(p->side, "ibh_smooth_residual: the partition has no side table");
    const Faces G = smooth::faces(p);
    const SmoothKernel k = smooth_kernels[p->nd - 2][nv - 1];
    const float* src = R;
    int64_t lsrc = ldr;
    for (int m = 1; m <= n_iter; ++m) {   // iteration m writes S when an even number of iterations follows it
        const bool toS = ((n_iter - m) & 1) == 0;
        float* dst = toS ? S : tmp;
        const int64_t ldst = toS ? lds : ldt;
        hipLaunchKernelGGL(k, cells_grid(p->nc), dim3(SMOOTH_BLOCK), 0, ibh_stream, p->nc, G, R, ldr, src, lsrc, eps, dst, ldst);
        src = dst;
        lsrc = ldst;
    }
    IBH_LAUNCH_CHECK();
    return 0;
}

int ibh_update_euler_smoothed(const ibh_part* p, const ibh_fluid* f, int blend, const float* P0, int64_t ld0, const float* P,
                              int64_t ldp, const float* R, int64_t ldr, const float* Sprev, int64_t lds, float eps,
                              const float* dt, int dt_per_cell, float a, float b, float c, float* P_out, int64_t ldo) {
    IBH_REQUIRE(p && f && P0 && R && Sprev && dt && P_out, "ibh_update_euler_smoothed: null argument");
    IBH_REQUIRE(blend == 0 || blend == 1, "ibh_update_euler_smoothed: blend must be 0 (stage) or 1 (Shu-Osher)");
    IBH_REQUIRE(!blend || P, "ibh_update_euler_smoothed: null argument (the Shu-Osher form reads P)");
    IBH_REQUIRE(p->nd == 2 || p->nd == 3, "ibh_update_euler_smoothed: nd must be 2 or 3");
    IBH_REQUIRE(p->nc >= 0 && ld0 >= p->nc && ldr >= p->nc && lds >= p->nc && ldo >= p->nc && (!blend || ldp >= p->nc),
                "ibh_update_euler_smoothed: a leading dimension is smaller than nc");
    IBH_REQUIRE(eps_ok(eps), "ibh_update_euler_smoothed: eps must be finite and >= 0");
    IBH_REQUIRE(P_out != R && P_out != Sprev,
                "ibh_update_euler_smoothed: P_out may not alias R or Sprev: other cells gather them (P_out may be P0 or P, "
                "Sprev may be R)");
    if (p->nc == 0) return 0;
    IBH_REQUIRE(p->side, "ibh_update_euler_smoothed: the partition has no side table");
    hipLaunchKernelGGL(update_kernels[p->nd - 2][blend][dt_per_cell != 0], cells_grid(p->nc), dim3(SMOOTH_BLOCK), 0, ibh_stream,
                       f->R, f->gamma, p->nc, smooth::faces(p), P0, ld0, P, ldp, R, ldr, Sprev, lds, eps, dt, a, b, c, P_out, ldo);
    IBH_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"

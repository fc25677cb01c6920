// libibhip: the pieces of an explicit solver step around the residual sweep, device resident (test/advection.jl:30-89):
//   * ibh_bcset_*: an ordered list of ghost-cell boundary conditions whose closures the library knows (a constant value,
//     copy(u): advection.jl:30-46) applied to a field with the semantics of the sequential impose_bc! calls
//     (ImmersedBoundary.jl:1197-1247: every ghost cell of a boundary is interpolated BEFORE any of them is written; a later
//     boundary sees the earlier ones): boundaries that do not read each other's ghost cells form a level, a level is two
//     launches (interpolate + closure + blend into a side buffer, scatter) whatever the number of boundaries;
//   * ibh_timestep_advection (ibh_timestep.hip): dt = scale * 0.5 / max over cells and dimensions of
//     unsigned_green_gauss(at_faces(C_d, d), d) (advection.jl:52-59) left in device memory -- no host read-back in the loop.
// The step itself (sweep + u += dt ud in one launch) is ibh_step_advection in ibh_fused.hip.
//   * ibh_update_euler: P_out = state2primitive(primitive2state(P) + dt R) in one launch (euler_step::update_row); the Euler
//     step around it is ibh_step_euler in ibh_fused.hip, its time step ibh_timestep_euler in ibh_timestep.hip.
//   * ibh_update_euler_stage: the same row function on a base state P0 with the time step alpha * dt, a Runge-Kutta stage of
//     the low-storage family; the stage around it is ibh_stage_euler in ibh_fused.hip.
//   * ibh_update_euler_ssp: a Shu-Osher stage, the update of the blend a primitive2state(P0) + b primitive2state(P) with the
//     time step c * dt (euler_step::blend_row); the stage around it is ibh_stage_euler_ssp in ibh_fused.hip.
//   * ibh_update_euler_dual, ibh_dual_source: a pseudo-time stage of a dual time step with the physical time derivative taken
//     point-implicitly (euler_step::dual_row), and the constant part of that derivative; the stage around the first is
//     ibh_stage_euler_dual in ibh_fused.hip.
// Arithmetic: the operator kernels' (ibh_ops.hip): -ffp-contract=off, the reference's evaluation order.
#include <algorithm>
#include <cfloat>
#include <memory>
#include <vector>

#include "ibh_bcset_dev.h"
#include "ibh_common.h"
#include "ibh_euler_step_dev.h"

#define MARCH_BLOCK 256

namespace {

// ghosts g0 .. g1 of the set: interpolate from the field, closure, blend (k_bc_blend) -- into `gval`, NOT into the field:
// every ghost cell of these boundaries is interpolated from the field as it was before any of them is written
__global__ void k_bcset_interp(int32_t g0, int32_t g1, const float* __restrict__ eta, const int32_t* __restrict__ off,
                               const int32_t* __restrict__ donor, const float* __restrict__ w,
                               const int32_t* __restrict__ bidx, const int32_t* __restrict__ mode,
                               const float* __restrict__ value, const float* __restrict__ a, float* __restrict__ gval,
                               const int32_t* __restrict__ ghost, float* a_out) {
    bcset_dev::interp_wg(blockIdx.x, gridDim.x, g0, g1, eta, off, donor, w, bidx, mode, value, a, gval, ghost, a_out);
}
__global__ void k_bcset_scatter(int32_t g0, int32_t g1, const int32_t* __restrict__ ghost, const float* __restrict__ gval,
                                float* __restrict__ a) {
    bcset_dev::scatter_wg(blockIdx.x, gridDim.x, g0, g1, ghost, gval, a);
}

// out = u + dt * r with dt in device memory (the update of advection.jl:87 for partitions without the fused step kernel)
__global__ void k_update_dev(int64_t n, const float* __restrict__ dt, const float* __restrict__ u,
                             const float* __restrict__ r, float* __restrict__ out) {
    const float h = *dt;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = u[i] + r[i] * h;
}

// The update kernels of an Euler step, one per form (EulerForm, ibh_euler_step_dev.h) and each with its entry's own argument
// list.  The grid-stride loops are written out, k_update_euler_dual's too: moved into one device function template over the
// form, the same loop compiles to other instruction orders in all twelve instantiations of the first three
// (scripts/kernel_bodies.py), and these kernels are held
// instruction for instruction.  What differs between them is which rows are loaded and the one call of a row function.
// P_out = state2primitive(primitive2state(P) + dt R), one thread per row: the row is read whole before it is written, so
// P_out may be P (no __restrict__ on the two).  dt: one value, or one per row (PER_CELL)
template <int ND, bool PER_CELL>
__global__ __launch_bounds__(MARCH_BLOCK) void k_update_euler(float Rgas, float gamma, int64_t n, const float* P, int64_t ldp,
                                                              const float* __restrict__ R, int64_t ldr,
                                                              const float* __restrict__ dt, float* P_out, int64_t ldo) {
    constexpr int NV = ND + 2;
    float h = 0.0f;
    if constexpr (!PER_CELL) h = *dt;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float Pr[NV], r[NV], o[NV];
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            Pr[v] = P[i + v * ldp];
            r[v] = R[i + v * ldr];
        }
        if constexpr (PER_CELL) h = dt[i];
        euler_step::update_row<ND>(Rgas, gamma, Pr, r, h, o);
#pragma unroll
        for (int v = 0; v < NV; ++v) P_out[i + v * ldo] = o[v];
    }
}

// A stage: P_out = state2primitive(primitive2state(P0) + (alpha dt) R).  k_update_euler with one more IEEE multiply
// (euler_step::stage_dt); P_out may be P0
template <int ND, bool PER_CELL>
__global__ __launch_bounds__(MARCH_BLOCK) void k_update_euler_stage(float Rgas, float gamma, int64_t n, const float* P0,
                                                                    int64_t ld0, const float* __restrict__ R, int64_t ldr,
                                                                    const float* __restrict__ dt, float alpha, float* P_out,
                                                                    int64_t ldo) {
    constexpr int NV = ND + 2;
    float h = 0.0f;
    if constexpr (!PER_CELL) h = euler_step::stage_dt(alpha, *dt);
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float Pr[NV], r[NV], o[NV];
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            Pr[v] = P0[i + v * ld0];
            r[v] = R[i + v * ldr];
        }
        if constexpr (PER_CELL) h = euler_step::stage_dt(alpha, dt[i]);
        euler_step::update_row<ND>(Rgas, gamma, Pr, r, h, o);
#pragma unroll
        for (int v = 0; v < NV; ++v) P_out[i + v * ldo] = o[v];
    }
}

// A Shu-Osher stage: P_out = state2primitive((primitive2state(P0) a + primitive2state(P) b) + (c dt) R)
// (euler_step::blend_row).  The rows of P0 and of P are read whole before the row of P_out is written: P_out may be either
template <int ND, bool PER_CELL>
__global__ __launch_bounds__(MARCH_BLOCK) void k_update_euler_ssp(float Rgas, float gamma, int64_t n, const float* P0,
                                                                  int64_t ld0, const float* P, int64_t ldp,
                                                                  const float* __restrict__ R, int64_t ldr,
                                                                  const float* __restrict__ dt, float a, float b, float c,
                                                                  float* P_out, int64_t ldo) {
    constexpr int NV = ND + 2;
    float h = 0.0f;
    if constexpr (!PER_CELL) h = euler_step::stage_dt(c, *dt);
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float Br[NV], Pr[NV], r[NV], o[NV];
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            Br[v] = P0[i + v * ld0];
            Pr[v] = P[i + v * ldp];
            r[v] = R[i + v * ldr];
        }
        if constexpr (PER_CELL) h = euler_step::stage_dt(c, dt[i]);
        euler_step::blend_row<ND>(Rgas, gamma, Br, Pr, r, a, b, h, o);
#pragma unroll
        for (int v = 0; v < NV; ++v) P_out[i + v * ldo] = o[v];
    }
}

// A pseudo-time stage of a dual time step: P_out = state2primitive((primitive2state(P0) + (R + S) (alpha dt)) / (1 + (alpha dt)
// g)) (euler_step::dual_row).  The rows of P0, R and S are read whole before the row of P_out is written: P_out may be P0
template <int ND, bool PER_CELL>
__global__ __launch_bounds__(MARCH_BLOCK) void k_update_euler_dual(float Rgas, float gamma, int64_t n, const float* P0,
                                                                   int64_t ld0, const float* __restrict__ R, int64_t ldr,
                                                                   const float* __restrict__ S, int64_t lds,
                                                                   const float* __restrict__ dt, float alpha, float g,
                                                                   float* P_out, int64_t ldo) {
    constexpr int NV = ND + 2;
    float h = 0.0f;
    if constexpr (!PER_CELL) h = euler_step::stage_dt(alpha, *dt);
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float Pr[NV], r[NV], s[NV], o[NV];
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            Pr[v] = P0[i + v * ld0];
            r[v] = R[i + v * ldr];
            s[v] = S[i + v * lds];
        }
        if constexpr (PER_CELL) h = euler_step::stage_dt(alpha, dt[i]);
        euler_step::dual_row<ND>(Rgas, gamma, Pr, r, s, h, g, o);
#pragma unroll
        for (int v = 0; v < NV; ++v) P_out[i + v * ldo] = o[v];
    }
}

// The source of a physical step, S = primitive2state(Pn) cn [+ primitive2state(Pm) cm] (euler_step::dual_source_row), one
// thread per row.  S aliases neither state (ibh_dual_source checks it)
template <int ND, bool BDF2>
__global__ __launch_bounds__(MARCH_BLOCK) void k_dual_source(float Rgas, float gamma, int64_t n, const float* __restrict__ Pn,
                                                             int64_t ldn, const float* __restrict__ Pm, int64_t ldm, float cn,
                                                             float cm, float* __restrict__ S, int64_t lds) {
    constexpr int NV = ND + 2;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float a[NV], b[NV] = {}, s[NV];
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            a[v] = Pn[i + v * ldn];
            if constexpr (BDF2) b[v] = Pm[i + v * ldm];
        }
        euler_step::dual_source_row<ND, BDF2>(Rgas, gamma, a, b, cn, cm, s);
#pragma unroll
        for (int v = 0; v < NV; ++v) S[i + v * lds] = s[v];
    }
}

// the four instantiations of an update kernel K as k[nd - 2][per-cell dt], and the launch of the one that (nd, dt_per_cell)
// picks over n rows
#define UPDATE_KERNELS(K) {{K<2, false>, K<2, true>}, {K<3, false>, K<3, true>}}
template <class K, class... A>
int launch_update(K const (&k)[2][2], int nd, int dt_per_cell, int64_t n, A... args) {
    hipLaunchKernelGGL(k[nd - 2][dt_per_cell != 0], dim3(ibh_grid_cap(n, MARCH_BLOCK, 2048)), dim3(MARCH_BLOCK), 0, ibh_stream,
                       args...);
    IBH_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" {

int ibh_bcset_create(ibh_bcset** out, int nbc, const ibh_bc* const* bcs, const int32_t* modes, const float* values) {
    IBH_REQUIRE(out && nbc >= 1 && nbc <= IBH_MAX_BC && bcs && modes && values, "ibh_bcset_create: bad argument");
    *out = nullptr;
    for (int k = 0; k < nbc; ++k) {
        IBH_REQUIRE(bcs[k] && (modes[k] == 0 || modes[k] == 1), "ibh_bcset_create: null boundary or bad mode");
        IBH_REQUIRE(bcs[k]->ng == 0 || (int32_t)bcs[k]->h_off.size() == bcs[k]->ng + 1,
                    "ibh_bcset_create: boundary without host stencils");
    }
    // Levels.  Sequential impose_bc! calls: boundary k is interpolated from the field as boundaries 1..k-1 left it and
    // before any of its own ghost cells is written.  Interpolating a whole LEVEL of boundaries into a side buffer and
    // scattering afterwards is the same thing iff no boundary of the level has a donor cell that is a ghost cell of an
    // earlier boundary of the same level (its own ghost cells and those of later boundaries are read as they were: right)
    // and no ghost cell belongs to two boundaries of the level.  level(k) = 1 + max level of the earlier boundaries it
    // depends on that way.
    std::vector<std::vector<int32_t>> gs(nbc);
    for (int k = 0; k < nbc; ++k) {
        gs[k] = bcs[k]->h_ghost;
        std::sort(gs[k].begin(), gs[k].end());
    }
    int level[IBH_MAX_BC] = {0}, nlev = 0;
    for (int k = 0; k < nbc; ++k) {
        int lv = 0;
        for (int j = 0; j < k; ++j) {
            bool dep = false;
            for (int32_t c : bcs[k]->h_donor)
                if (std::binary_search(gs[j].begin(), gs[j].end(), c)) { dep = true; break; }
            for (int32_t c : gs[k])
                if (!dep && std::binary_search(gs[j].begin(), gs[j].end(), c)) { dep = true; break; }
            if (dep) lv = std::max(lv, level[j] + 1);
        }
        level[k] = lv;
        nlev = std::max(nlev, lv + 1);
    }
    std::unique_ptr<ibh_bcset> s(new ibh_bcset());
    s->nbc = nbc;
    s->nlev = nlev;
    std::vector<int32_t> ghost, off{0}, donor, bidx, mode(modes, modes + nbc);
    std::vector<float> eta, w, value(values, values + nbc);
    for (int lv = 0; lv < nlev; ++lv) {  // ghosts ordered by level, boundaries of a level in their order
        s->seg[lv] = (int32_t)ghost.size();
        for (int k = 0; k < nbc; ++k) {
            if (level[k] != lv) continue;
            const ibh_bc* b = bcs[k];
            for (int32_t g = 0; g < b->ng; ++g) {
                ghost.push_back(b->h_ghost[g]);
                eta.push_back(b->h_eta[g]);
                bidx.push_back(k);
                for (int32_t j = b->h_off[g]; j < b->h_off[g + 1]; ++j) {
                    donor.push_back(b->h_donor[j]);
                    w.push_back(b->h_w[j]);
                }
                off.push_back((int32_t)donor.size());
            }
        }
    }
    s->seg[nlev] = s->ng = (int32_t)ghost.size();
    for (int lv = 0; lv < nlev; ++lv) {  // a level none of whose ghost cells is one of its donors needs no side buffer
        std::vector<int32_t> gl(ghost.begin() + s->seg[lv], ghost.begin() + s->seg[lv + 1]);
        std::sort(gl.begin(), gl.end());
        bool hazard = false;
        for (int32_t j = off[s->seg[lv]]; j < off[s->seg[lv + 1]] && !hazard; ++j)
            hazard = std::binary_search(gl.begin(), gl.end(), donor[j]);
        s->direct[lv] = !hazard;
    }
    IBH_TRY(s->own.upload(&s->ghost, ghost));
    IBH_TRY(s->own.upload(&s->eta, eta));
    IBH_TRY(s->own.upload(&s->off, off));
    IBH_TRY(s->own.upload(&s->donor, donor));
    IBH_TRY(s->own.upload(&s->w, w));
    IBH_TRY(s->own.upload(&s->bidx, bidx));
    IBH_TRY(s->own.upload(&s->mode, mode));
    IBH_TRY(s->own.upload(&s->value, value));
    IBH_TRY(s->own.alloc(&s->gval, std::max<size_t>(ghost.size(), 1)));
    *out = s.release();
    return 0;
}

int ibh_bcset_destroy(ibh_bcset* s) {
    delete s;
    return 0;
}

int ibh_bcset_info(const ibh_bcset* s, int32_t* n_ghost, int32_t* n_levels) {
    IBH_REQUIRE(s, "ibh_bcset_info: null set");
    if (n_ghost) *n_ghost = s->ng;
    if (n_levels) {
        int nd = 0;
        for (int lv = 0; lv < s->nlev; ++lv) nd += s->direct[lv];
        *n_levels = s->nlev | (nd << 16);  // low half: levels; high half: how many of them are blended in one launch
    }
    return 0;
}

int ibh_bcset_apply(const ibh_bcset* s, float* a) {
    IBH_REQUIRE(s && a, "ibh_bcset_apply: null argument");
    if (s->ng == 0) return 0;
    for (int lv = 0; lv < s->nlev; ++lv) {
        const int32_t g0 = s->seg[lv], g1 = s->seg[lv + 1];
        if (g1 == g0) continue;
        const int nwg = std::min(ibh_grid(g1 - g0, MARCH_BLOCK), 2048);
        if (s->direct[lv]) {
            hipLaunchKernelGGL(k_bcset_interp, dim3(nwg), dim3(MARCH_BLOCK), 0, ibh_stream, g0, g1, s->eta, s->off, s->donor,
                               s->w, s->bidx, s->mode, s->value, a, s->gval, s->ghost, a);
            continue;
        }
        hipLaunchKernelGGL(k_bcset_interp, dim3(nwg), dim3(MARCH_BLOCK), 0, ibh_stream, g0, g1, s->eta, s->off, s->donor,
                           s->w, s->bidx, s->mode, s->value, a, s->gval, (const int32_t*)nullptr, (float*)nullptr);
        hipLaunchKernelGGL(k_bcset_scatter, dim3(nwg), dim3(MARCH_BLOCK), 0, ibh_stream, g0, g1, s->ghost, s->gval, a);
    }
    IBH_LAUNCH_CHECK();
    return 0;
}

int ibh_update_dev(int64_t n, const float* dt_dev, const float* u, const float* r, float* out) {
    IBH_REQUIRE(dt_dev && u && r && out, "ibh_update_dev: null argument");
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_update_dev, dim3(std::min(ibh_grid(n, MARCH_BLOCK), 2048)), dim3(MARCH_BLOCK), 0, ibh_stream, n,
                       dt_dev, u, r, out);
    IBH_LAUNCH_CHECK();
    return 0;
}

// P_out = state2primitive(primitive2state(P) + dt * R): the three launches and three passes over nd + 2 columns of the
// composition in one.  dt: one device value, or n of them (dt_per_cell: the local time step of a pseudo-time march)
int ibh_update_euler(const ibh_fluid* f, int nd, int64_t n, const float* P, int64_t ldp, const float* R, int64_t ldr,
                     const float* dt, int dt_per_cell, float* P_out, int64_t ldo) {
    IBH_REQUIRE(f && P && R && dt && P_out, "ibh_update_euler: null argument");
    IBH_REQUIRE(nd == 2 || nd == 3, "ibh_update_euler: nd must be 2 or 3");
    IBH_REQUIRE(n >= 0 && ldp >= n && ldr >= n && ldo >= n, "ibh_update_euler: a leading dimension is smaller than n");
    IBH_REQUIRE(P_out != R && P != R, "ibh_update_euler: R may not alias P or P_out (P_out may be P)");
    if (n == 0) return 0;
    static constexpr decltype(&k_update_euler<2, false>) k[2][2] = UPDATE_KERNELS(k_update_euler);
    return launch_update(k, nd, dt_per_cell, n, f->R, f->gamma, n, P, ldp, R, ldr, dt, P_out, ldo);
}

// A Runge-Kutta stage of the low-storage family, P_out = state2primitive(primitive2state(P0) + (alpha * dt) * R) in one
// launch: bit for bit ibh_update_euler(P0, R, dt .* alpha) with the product taken by the broadcast layer
int ibh_update_euler_stage(const ibh_fluid* f, int nd, int64_t n, const float* P0, int64_t ld0, const float* R, int64_t ldr,
                           const float* dt, int dt_per_cell, float alpha, float* P_out, int64_t ldo) {
    IBH_REQUIRE(f && P0 && R && dt && P_out, "ibh_update_euler_stage: null argument");
    IBH_REQUIRE(nd == 2 || nd == 3, "ibh_update_euler_stage: nd must be 2 or 3");
    IBH_REQUIRE(n >= 0 && ld0 >= n && ldr >= n && ldo >= n, "ibh_update_euler_stage: a leading dimension is smaller than n");
    IBH_REQUIRE(P_out != R && P0 != R, "ibh_update_euler_stage: R may not alias P0 or P_out (P_out may be P0)");
    if (n == 0) return 0;
    static constexpr decltype(&k_update_euler_stage<2, false>) k[2][2] = UPDATE_KERNELS(k_update_euler_stage);
    return launch_update(k, nd, dt_per_cell, n, f->R, f->gamma, n, P0, ld0, R, ldr, dt, alpha, P_out, ldo);
}

// A Shu-Osher stage of a strong-stability-preserving Runge-Kutta scheme in one launch,
//     P_out = state2primitive((primitive2state(P0) * a + primitive2state(P) * b) + (c * dt) * R):
// bit for bit primitive2state twice, the broadcasts dt .* c and Q0 .* a .+ Q .* b, the column updates and state2primitive
int ibh_update_euler_ssp(const ibh_fluid* f, int nd, int64_t n, const float* P0, int64_t ld0, const float* P, int64_t ldp,
                         const float* R, int64_t ldr, const float* dt, int dt_per_cell, float a, float b, float c,
                         float* P_out, int64_t ldo) {
    IBH_REQUIRE(f && P0 && P && R && dt && P_out, "ibh_update_euler_ssp: null argument");
    IBH_REQUIRE(nd == 2 || nd == 3, "ibh_update_euler_ssp: nd must be 2 or 3");
    IBH_REQUIRE(n >= 0 && ld0 >= n && ldp >= n && ldr >= n && ldo >= n,
                "ibh_update_euler_ssp: a leading dimension is smaller than n");
    IBH_REQUIRE(P_out != R && P0 != R && P != R,
                "ibh_update_euler_ssp: R may not alias P0, P or P_out (P_out may be P0 or P, P0 may be P)");
    if (n == 0) return 0;
    static constexpr decltype(&k_update_euler_ssp<2, false>) k[2][2] = UPDATE_KERNELS(k_update_euler_ssp);
    return launch_update(k, nd, dt_per_cell, n, f->R, f->gamma, n, P0, ld0, P, ldp, R, ldr, dt, a, b, c, P_out, ldo);
}

// A pseudo-time stage of a dual time step in one launch,
//     P_out = state2primitive((primitive2state(P0) + (R + S) * (alpha * dt)) / (1 + (alpha * dt) * g)):
// bit for bit primitive2state, the broadcasts R .+ S, dt .* alpha and h .* g .+ 1, the column updates, the broadcast ./ and
// state2primitive.  S (conserved variables) and g come from the physical step's backward difference (ibh_dual_source)
int ibh_update_euler_dual(const ibh_fluid* f, int nd, int64_t n, const float* P0, int64_t ld0, const float* R, int64_t ldr,
                          const float* S, int64_t lds, const float* dt, int dt_per_cell, float alpha, float g, float* P_out,
                          int64_t ldo) {
    IBH_REQUIRE(f && P0 && R && S && dt && P_out, "ibh_update_euler_dual: null argument");
    IBH_REQUIRE(nd == 2 || nd == 3, "ibh_update_euler_dual: nd must be 2 or 3");
    IBH_REQUIRE(n >= 0 && ld0 >= n && ldr >= n && lds >= n && ldo >= n,
                "ibh_update_euler_dual: a leading dimension is smaller than n");
    IBH_REQUIRE(g >= 0.0f && g <= FLT_MAX, "ibh_update_euler_dual: g must be finite and >= 0");
    IBH_REQUIRE(P_out != R && P0 != R && P_out != S && R != S,
                "ibh_update_euler_dual: R and S may alias neither each other nor P_out, R not P0 (P_out may be P0)");
    if (n == 0) return 0;
    static constexpr decltype(&k_update_euler_dual<2, false>) k[2][2] = UPDATE_KERNELS(k_update_euler_dual);
    return launch_update(k, nd, dt_per_cell, n, f->R, f->gamma, n, P0, ld0, R, ldr, S, lds, dt, alpha, g, P_out, ldo);
}

// The source of a physical step of a dual time march, S = primitive2state(Pn) * cn + primitive2state(Pm) * cm -- the terms of
// the backward difference that the inner iterations do not change -- or, with Pm null (BDF1, the first step),
// primitive2state(Pn) * cn: bit for bit primitive2state and the broadcasts Qn .* cn .+ Qm .* cm
int ibh_dual_source(const ibh_fluid* f, int nd, int64_t n, const float* Pn, int64_t ldn, const float* Pm, int64_t ldm, float cn,
                    float cm, float* S, int64_t lds) {
    IBH_REQUIRE(f && Pn && S, "ibh_dual_source: null argument");
    IBH_REQUIRE(nd == 2 || nd == 3, "ibh_dual_source: nd must be 2 or 3");
    IBH_REQUIRE(n >= 0 && ldn >= n && lds >= n && (!Pm || ldm >= n), "ibh_dual_source: a leading dimension is smaller than n");
    IBH_REQUIRE(S != Pn && S != Pm, "ibh_dual_source: S may not alias Pn or Pm");
    if (n == 0) return 0;
    const dim3 grid(ibh_grid_cap(n, MARCH_BLOCK, 2048)), block(MARCH_BLOCK);
    if (Pm) {
        auto k = nd == 2 ? k_dual_source<2, true> : k_dual_source<3, true>;
        hipLaunchKernelGGL(k, grid, block, 0, ibh_stream, f->R, f->gamma, n, Pn, ldn, Pm, ldm, cn, cm, S, lds);
    } else {
        auto k = nd == 2 ? k_dual_source<2, false> : k_dual_source<3, false>;
        hipLaunchKernelGGL(k, grid, block, 0, ibh_stream, f->R, f->gamma, n, Pn, ldn, Pn, ldn, cn, cm, S, lds);
    }
    IBH_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"

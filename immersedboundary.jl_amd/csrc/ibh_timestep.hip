// libibhip: the time step of an explicit step on face-list partitions (ibh_timestep_advection, ibh_timestep_euler) and the
// BC-set launches of a march step that carry the NEXT step's time step beside them (ibh_bcset_apply_with_dt).  The device
// bodies are ibh_dt_dev.h and ibh_bcset_dev.h; here are the kernels around them and the launches.
#include "ibh_bcset_dev.h"
#include "ibh_common.h"

#define OPS_BLOCK 256
#include "ibh_dt_dev.h"
using dt_dev::GradDims;
using dt_dev::grad_dims;
using dt_dev::dt_partial_wg;
using dt_dev::dt_final_wg;

namespace {

// dt of an explicit advection step (test/advection.jl:52-59, :65): max over cells and dimensions of
// unsigned_green_gauss(at_faces(C_d, d), d) -- the same expressions as k_at_faces + k_green_gauss(unsigned), a face value
// evaluated by both of its cells instead of being written and read back.  Two launches and NO atomics: workgroup maxima into
// an array, then one workgroup reduces them and writes dt = (0.5 / max) * scale.  (A single launch whose workgroups meet at
// one counter -- atomicMax + last-workgroup-out -- took 39 us for 1 024 workgroups: arrivals at one address serialise at
// ~35 ns each across the XCDs; this form takes ~8.)
// TILED: the partition is made of complete 8^ND blocks in order (cell c = block c / 8^ND, position c % 8^ND, x fastest): the
// cell across an in-block face is c -+ 8^d -- what the side table holds for it -- so the table is read by the cells on the
// block faces only (a quarter of the index traffic in 2-D; round 4: 18.6 -> us per evaluation at 0.87 M cells)
template <int ND, bool TILED>
__global__ __launch_bounds__(OPS_BLOCK) void k_timestep_advection(int32_t nc, GradDims G, const float* __restrict__ C,
                                                                  int64_t ldc, float* __restrict__ partial) {
    dt_partial_wg<ND, TILED>(blockIdx.x, gridDim.x, nc, G, dt_dev::ArrayLoad{C, ldc}, partial);
}
// the same for the acoustic wave speeds |u_d| + a of P = [p T u v (w)], computed on the fly (ibh_timestep_euler); CELLS: the
// local time step of every cell as well
template <int ND, bool TILED, bool CELLS>
__global__ __launch_bounds__(OPS_BLOCK) void k_timestep_euler(int32_t nc, GradDims G, const float* __restrict__ P, int64_t ldp,
                                                              float Rgas, float gamma, float* __restrict__ partial,
                                                              float scale, float* __restrict__ dt_cells) {
    dt_partial_wg<ND, TILED, dt_dev::AcousticLoad, CELLS>(blockIdx.x, gridDim.x, nc, G,
                                                          dt_dev::AcousticLoad{P, ldp, Rgas, gamma}, partial, scale, dt_cells);
}
__global__ __launch_bounds__(OPS_BLOCK) void k_dt_from_partials(int n, const float* __restrict__ partial, float scale,
                                                                float* __restrict__ dt) {
    dt_final_wg(n, partial, scale, dt);
}
// ---- a march step's BC-set launches with the time step of the NEXT step riding beside them (horizontal fusion: the time
// step depends on C alone, the boundary conditions on the field; both are short launches bound by dependent loads, and side
// by side they cost what the longer one costs): workgroups [0, nwg_bc) run the BC-set body, the rest the dt body.
struct BcLaunch {
    int32_t g0, g1;
    const float *eta, *w, *value;
    const int32_t *off, *donor, *bidx, *mode, *ghost_direct, *ghost;
    float* gval;
};
template <int ND, bool TILED>
__global__ __launch_bounds__(OPS_BLOCK) void k_bcinterp_dt(int nwg_bc, BcLaunch B, float* a, int32_t nc, GradDims G,
                                                           const float* __restrict__ C, int64_t ldc,
                                                           float* __restrict__ partial) {
    if ((int)blockIdx.x < nwg_bc)
        bcset_dev::interp_wg(blockIdx.x, nwg_bc, B.g0, B.g1, B.eta, B.off, B.donor, B.w, B.bidx, B.mode, B.value, a, B.gval,
                             B.ghost_direct, a);
    else dt_partial_wg<ND, TILED>(blockIdx.x - nwg_bc, gridDim.x - nwg_bc, nc, G, dt_dev::ArrayLoad{C, ldc}, partial);
}
__global__ __launch_bounds__(OPS_BLOCK) void k_bcscatter_dt(int nwg_bc, BcLaunch B, float* a, int npart,
                                                            const float* __restrict__ partial, float scale,
                                                            float* __restrict__ dt) {
    if ((int)blockIdx.x < nwg_bc) bcset_dev::scatter_wg(blockIdx.x, nwg_bc, B.g0, B.g1, B.ghost, B.gval, a);
    else dt_final_wg(npart, partial, scale, dt);
}
// a direct level (interpolation blended straight into the field) as the second launch of the set: interp body + dt final
__global__ __launch_bounds__(OPS_BLOCK) void k_bcinterp_dtfinal(int nwg_bc, BcLaunch B, float* a, int npart,
                                                                const float* __restrict__ partial, float scale,
                                                                float* __restrict__ dt) {
    if ((int)blockIdx.x < nwg_bc)
        bcset_dev::interp_wg(blockIdx.x, nwg_bc, B.g0, B.g1, B.eta, B.off, B.donor, B.w, B.bidx, B.mode, B.value, a, B.gval,
                             B.ghost_direct, a);
    else dt_final_wg(npart, partial, scale, dt);
}

// the four instantiations of a kernel K<ND, TILED> (K<ND, TILED, CELLS> for the second form) as k[nd - 2][tiled]; the kernel
// of partition p is dt_kernel(k, p) (tiled: complete blocks in order, ibh_tiled)
#define DT_KERNELS(K) {{K<2, false>, K<2, true>}, {K<3, false>, K<3, true>}}
#define DT_KERNELS_CELLS(K, CELLS) {{K<2, false, CELLS>, K<2, true, CELLS>}, {K<3, false, CELLS>, K<3, true, CELLS>}}
template <class K>
K dt_kernel(K const (&k)[2][2], const ibh_part* p) {
    return k[p->nd - 2][p->sum.tiled != 0];
}

// the workgroup maxima of the time step live with the partition, not in the per-thread scratch: a march step launches them
// in one call and reduces them in the next (partials_done below)
int ensure_march_tmp(ibh_part* p) {
    if (p->march_tmp) return 0;
    IBH_TRY(p->own.alloc(&p->march_tmp, 8192));
    p->march_tmp_n = 8192;
    return 0;
}

}  // namespace

extern "C" {

int ibh_timestep_advection(ibh_part* p, const float* C, int64_t ldc, float scale, float* dt_dev) {
    IBH_REQUIRE(p && C && dt_dev && (p->nd == 2 || p->nd == 3) && p->nc > 0, "ibh_timestep_advection: bad argument");
    IBH_TRY(ensure_march_tmp(p));
    const GradDims G = grad_dims(p);
    // one cell per thread up to 2 M cells (every load of a cell in flight at once: the kernel is two dependent round trips,
    // not bandwidth; with 1 024 workgroups and 3-4 cells per thread it took 18.6 us at 0.87 M cells)
    const int nwg = ibh_grid_cap(p->nc, OPS_BLOCK, 8192);
    static constexpr decltype(&k_timestep_advection<2, false>) k[2][2] = DT_KERNELS(k_timestep_advection);
    hipLaunchKernelGGL(dt_kernel(k, p), dim3(nwg), dim3(OPS_BLOCK), 0, ibh_stream, p->nc, G, C, ldc, p->march_tmp);
    hipLaunchKernelGGL(k_dt_from_partials, dim3(1), dim3(OPS_BLOCK), 0, ibh_stream, nwg, p->march_tmp, scale, dt_dev);
    IBH_LAUNCH_CHECK();
    return 0;
}

// The CFL time step of an explicit Euler step: the advection script's formula above with the acoustic speed C_d = |u_d| + a in
// place of C, evaluated from P by the loader (no wave-speed array); bit for bit ibh_timestep_advection on the materialised
// C.  dt_device: the global time step; dt_cells: (0.5 / max_d(...)[c]) * scale per cell; either may be null, not both.  Two
// launches like ibh_timestep_advection, one when only dt_cells is asked for.
int ibh_timestep_euler(ibh_part* p, const ibh_fluid* f, const float* P, int64_t ldp, float scale, float* dt_device,
                       float* dt_cells) {
    IBH_REQUIRE(p && f && P, "ibh_timestep_euler: null argument");
    IBH_REQUIRE(dt_device || dt_cells, "ibh_timestep_euler: null dt_device and dt_cells (one of them must be given)");
    IBH_REQUIRE(p->nd == 2 || p->nd == 3, "ibh_timestep_euler: nd must be 2 or 3");
    IBH_REQUIRE(p->nc > 0, "ibh_timestep_euler: empty partition");
    IBH_REQUIRE(ldp >= p->nc, "ibh_timestep_euler: ldp is smaller than the number of cells");
    IBH_TRY(ensure_march_tmp(p));
    const GradDims G = grad_dims(p);
    const int nwg = ibh_grid_cap(p->nc, OPS_BLOCK, 8192);
    static constexpr decltype(&k_timestep_euler<2, false, false>) k[2][2][2] = {
        DT_KERNELS_CELLS(k_timestep_euler, false), DT_KERNELS_CELLS(k_timestep_euler, true)};   // k[cells][nd - 2][tiled]
    hipLaunchKernelGGL(dt_kernel(k[dt_cells != nullptr], p), dim3(nwg), dim3(OPS_BLOCK), 0, ibh_stream, p->nc, G, P, ldp, f->R,
                       f->gamma, p->march_tmp, scale, dt_cells);
    if (dt_device)
        hipLaunchKernelGGL(k_dt_from_partials, dim3(1), dim3(OPS_BLOCK), 0, ibh_stream, nwg, p->march_tmp, scale, dt_device);
    IBH_LAUNCH_CHECK();
    return 0;
}

// ibh_bcset_apply(s, a) with ibh_timestep_advection(p, C, ldc, scale, dt_next) riding in its launches: the partial maxima
// beside the first launch of the set, the final reduction beside the second.  Same kernels' bodies, same results; sets with
// fewer than two launches take the separate launches for what is left.
// partials_done: the partial maxima are in p->march_tmp already (a caller that launched them elsewhere); the final reduction
// then rides in the FIRST launch of the set
int ibh_bcset_apply_with_dt(const ibh_bcset* s, float* a, ibh_part* p, const float* C, int64_t ldc, float scale,
                            float* dt_next, int partials_done) {
    IBH_REQUIRE(s && a && p && C && dt_next && (p->nd == 2 || p->nd == 3) && p->nc > 0, "ibh_bcset_apply_with_dt: bad argument");
    IBH_TRY(ensure_march_tmp(p));
    const GradDims G = grad_dims(p);
    const int nwg_dt = ibh_grid_cap(p->nc, OPS_BLOCK, 8192);
    static constexpr decltype(&k_bcinterp_dt<2, false>) k_interp_dt[2][2] = DT_KERNELS(k_bcinterp_dt);
    int stage = partials_done ? 1 : 0;   // 0: partial maxima not launched yet, 1: final reduction not launched yet, 2: done
    for (int lv = 0; lv < s->nlev; ++lv) {
        const int32_t g0 = s->seg[lv], g1 = s->seg[lv + 1];
        if (g1 == g0) continue;
        const int nwg = ibh_grid_cap(g1 - g0, OPS_BLOCK, 2048);
        BcLaunch B{g0, g1, s->eta, s->w, s->value, s->off, s->donor, s->bidx, s->mode, s->direct[lv] ? s->ghost : nullptr,
                   s->ghost, s->gval};
        // the interpolation launch of the level
        if (stage == 0) {
            hipLaunchKernelGGL(dt_kernel(k_interp_dt, p), dim3(nwg + nwg_dt), dim3(OPS_BLOCK), 0, ibh_stream, nwg, B, a, p->nc,
                               G, C, ldc, p->march_tmp);
            stage = 1;
        } else if (stage == 1) {
            hipLaunchKernelGGL(k_bcinterp_dtfinal, dim3(nwg + 1), dim3(OPS_BLOCK), 0, ibh_stream, nwg, B, a, nwg_dt,
                               p->march_tmp, scale, dt_next);
            stage = 2;
        } else {
            hipLaunchKernelGGL(k_bcinterp_dtfinal, dim3(nwg), dim3(OPS_BLOCK), 0, ibh_stream, nwg, B, a, 0, p->march_tmp, scale,
                               dt_next);
        }
        if (s->direct[lv]) continue;
        // the scatter launch of the level
        if (stage == 1) {
            hipLaunchKernelGGL(k_bcscatter_dt, dim3(nwg + 1), dim3(OPS_BLOCK), 0, ibh_stream, nwg, B, a, nwg_dt, p->march_tmp,
                               scale, dt_next);
            stage = 2;
        } else {
            hipLaunchKernelGGL(k_bcscatter_dt, dim3(nwg), dim3(OPS_BLOCK), 0, ibh_stream, nwg, B, a, 0, p->march_tmp, scale,
                               dt_next);
        }
    }
    IBH_LAUNCH_CHECK();
    if (stage == 0) return ibh_timestep_advection(p, C, ldc, scale, dt_next);
    if (stage == 1) {
        hipLaunchKernelGGL(k_dt_from_partials, dim3(1), dim3(OPS_BLOCK), 0, ibh_stream, nwg_dt, p->march_tmp, scale, dt_next);
        IBH_LAUNCH_CHECK();
    }
    return 0;
}

}  // extern "C"

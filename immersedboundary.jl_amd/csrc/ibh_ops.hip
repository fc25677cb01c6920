// libibhip: face-list ("general") grid-operator kernels -- one entry point per reference
// operator (ImmersedBoundary.jl:873-1157), accumulators, ghost-cell BC, row gather/scatter
// and the small vector ops of the FAS loop.  HBM-bound gathers: threads run over the
// contiguous row index (cell or face) so loads/stores of the row-major side are coalesced;
// the variable index is the slow grid dimension.  Also here, beside cell_gradient_at: the thread-per-cell forms of the fused
// closures of ibh_turb.hip (k_shear_of_velocity_cells, k_les_of_cells, k_k_epsilon_rhs_cells, k_wray_agarwal_of_cells).
//
// Arithmetic follows the reference's broadcast order operation by operation (compiled
// with -ffp-contract=off, IEEE divide/sqrt) so results are bit-comparable with the oracle.
#include "ibh_bcset_dev.h"
#include "ibh_common.h"
#include "ibh_les_dev.h"
#include "ibh_transport_dev.h"

#define OPS_BLOCK 256
#include "ibh_dt_dev.h"
using dt_dev::GradDims;
using dt_dev::grad_dims;
using dt_dev::dt_partial_wg;
using dt_dev::dt_final_wg;

namespace {

__device__ __forceinline__ float face_avg(float uo, float un, float ho, float hn) {
    // at_faces (:907-909): (u_o*h_n + u_n*h_o)/(h_n + h_o)
    return (uo * hn + un * ho) / (hn + ho);
}

__global__ void k_gather(const int32_t* __restrict__ rows, int32_t n, const float* __restrict__ src, int64_t lds,
                         float* __restrict__ dst, int64_t ldd) {
    int64_t v = blockIdx.y;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        dst[i + v * ldd] = src[rows[i] + v * lds];
}

__global__ void k_scatter(const int32_t* __restrict__ rows, int32_t n, const float* __restrict__ src, int64_t lds,
                          float* __restrict__ dst, int64_t ldd) {
    int64_t v = blockIdx.y;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        dst[rows[i] + v * ldd] = src[i + v * lds];
}

__global__ void k_copy_rows(const int32_t* __restrict__ drows, const int32_t* __restrict__ srows, int32_t n,
                            const float* __restrict__ src, int64_t lds, float* __restrict__ dst, int64_t ldd) {
    int64_t v = blockIdx.y;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        dst[drows[i] + v * ldd] = src[srows[i] + v * lds];
}

__global__ void k_at_faces(int32_t nf, const int32_t* __restrict__ own, const int32_t* __restrict__ nei,
                           const float* __restrict__ h, const float* __restrict__ u, int64_t ldu,
                           float* __restrict__ out, int64_t ldo) {
    int64_t v = blockIdx.y;
    for (int64_t f = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; f < nf; f += (int64_t)gridDim.x * blockDim.x) {
        int32_t o = own[f], n = nei[f];
        out[f + v * ldo] = face_avg(u[o + v * ldu], u[n + v * ldu], h[o], h[n]);
    }
}

// mode 0: face_distance, 1: owner_distance, 2: neighbor_distance
__global__ void k_distances(int32_t nf, const int32_t* __restrict__ own, const int32_t* __restrict__ nei,
                            const float* __restrict__ h, int mode, float* __restrict__ out) {
    for (int64_t f = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; f < nf; f += (int64_t)gridDim.x * blockDim.x) {
        float ho = h[own[f]], hn = h[nei[f]];
        out[f] = mode == 0 ? (ho + hn) / 2.0f : (mode == 1 ? ho / 2.0f : hn / 2.0f);
    }
}

__global__ void k_face_gradient(int32_t nf, const int32_t* __restrict__ own, const int32_t* __restrict__ nei,
                                const float* __restrict__ h, const float* __restrict__ u, int64_t ldu,
                                float* __restrict__ out, int64_t ldo) {
    int64_t v = blockIdx.y;
    for (int64_t f = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; f < nf; f += (int64_t)gridDim.x * blockDim.x) {
        int32_t o = own[f], n = nei[f];
        float fd = (h[o] + h[n]) / 2.0f;                       // face_distance (:1001)
        out[f + v * ldo] = (u[n + v * ldu] - u[o + v * ldu]) / fd;  // :1041-1043
    }
}

// mean over a CSR row of a face field (face accumulator with weights 1/len, :501-506)
__device__ __forceinline__ float csr_mean(const int32_t* __restrict__ off, const int32_t* __restrict__ idx, int32_t c,
                                          const float* __restrict__ uf) {
    int32_t b = off[c], e = off[c + 1];
    if (e == b) return 0.0f;
    float w = 1.0f / (float)(e - b);
    float s = uf[idx[b]] * w;
    for (int32_t k = b + 1; k < e; ++k) s = s + uf[idx[k]] * w;
    return s;
}

__global__ void k_green_gauss(int32_t nc, const int32_t* __restrict__ loff, const int32_t* __restrict__ lidx,
                              const int32_t* __restrict__ roff, const int32_t* __restrict__ ridx,
                              const float* __restrict__ h, const float* __restrict__ uf, int64_t ldf,
                              float* __restrict__ out, int64_t ldo, int uns) {
    int64_t v = blockIdx.y;
    const float* ufv = uf + v * ldf;
    for (int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; c < nc; c += (int64_t)gridDim.x * blockDim.x) {
        float ar = csr_mean(roff, ridx, (int32_t)c, ufv);
        float al = csr_mean(loff, lidx, (int32_t)c, ufv);
        out[c + v * ldo] = (uns ? (ar + al) : (ar - al)) / h[c];  // :925 / :941
    }
}

// cell_gradient = green_gauss(at_faces(u)) without materialising the face field (:965-972)
__device__ __forceinline__ float csr_mean_face_avg(const int32_t* __restrict__ off, const int32_t* __restrict__ idx,
                                                   int32_t c, const int32_t* __restrict__ own,
                                                   const int32_t* __restrict__ nei, const float* __restrict__ h,
                                                   const float* __restrict__ u) {
    int32_t b = off[c], e = off[c + 1];
    if (e == b) return 0.0f;
    float w = 1.0f / (float)(e - b);
    float s = 0.0f;
    for (int32_t k = b; k < e; ++k) {
        int32_t f = idx[k];
        int32_t o = own[f], n = nei[f];
        float t = face_avg(u[o], u[n], h[o], h[n]) * w;
        s = (k == b) ? t : s + t;
    }
    return s;
}

// cell_gradient(part, u), the tuple form, on partitions without the block structure: all dimensions in one launch
// (thread per cell and field; out[(d * nv + v) * ldo + c], the layout of ibh_cell_gradient_nd)
// Sides with ONE face (side table of the partition, ibh_common.h) are evaluated directly from the cell across -- the same
// expression the CSR walk evaluates for its single entry (weight 1.0f) -- the others walk the lists.
template <int ND>
__global__ void k_cell_gradient_all(int32_t nc, GradDims G, const float* __restrict__ u, int64_t ldu, int nv,
                                    float* __restrict__ out, int64_t ldo) {
    const int64_t v = blockIdx.y;
    const float* uv = u + v * ldu;
    for (int64_t c = IBH_WG_X() * (int64_t)blockDim.x + threadIdx.x; c < nc; c += (int64_t)gridDim.x * blockDim.x) {
        int32_t sd[2 * ND];
#pragma unroll
        for (int s = 0; s < 2 * ND; ++s) sd[s] = G.side[(int64_t)s * nc + c];
        const float uc = uv[c];
#pragma unroll
        for (int d = 0; d < ND; ++d) {
            const float hc = G.h[d][c];
            const int32_t l = sd[2 * d], r = sd[2 * d + 1];
            float ar, al;
            if (r >= 0) ar = face_avg(uc, uv[r], hc, G.h[d][r]) * 1.0f;
            else if (r == -2) ar = 0.0f;
            else ar = csr_mean_face_avg(G.d[d].roff, G.d[d].ridx, (int32_t)c, G.d[d].owners, G.d[d].neighbors, G.h[d], uv);
            if (l >= 0) al = face_avg(uv[l], uc, G.h[d][l], hc) * 1.0f;
            else if (l == -2) al = 0.0f;
            else al = csr_mean_face_avg(G.d[d].loff, G.d[d].lidx, (int32_t)c, G.d[d].owners, G.d[d].neighbors, G.h[d], uv);
            out[c + ((int64_t)d * nv + v) * ldo] = (ar - al) / hc;
        }
    }
}

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

// gradient of one field at cell c in every dimension: the expressions of k_cell_gradient_all
template <int ND>
__device__ __forceinline__ void cell_gradient_at(const GradDims& G, const int32_t (&sd)[2 * ND], int32_t nc, int32_t c,
                                                 const float* __restrict__ uv, float (&g)[ND]) {
    const float uc = uv[c];
#pragma unroll
    for (int d = 0; d < ND; ++d) {
        const float hc = G.h[d][c];
        const int32_t l = sd[2 * d], r = sd[2 * d + 1];
        float ar, al;
        if (r >= 0) ar = face_avg(uc, uv[r], hc, G.h[d][r]) * 1.0f;
        else if (r == -2) ar = 0.0f;
        else ar = csr_mean_face_avg(G.d[d].roff, G.d[d].ridx, c, G.d[d].owners, G.d[d].neighbors, G.h[d], uv);
        if (l >= 0) al = face_avg(uv[l], uc, G.h[d][l], hc) * 1.0f;
        else if (l == -2) al = 0.0f;
        else al = csr_mean_face_avg(G.d[d].loff, G.d[d].lidx, c, G.d[d].owners, G.d[d].neighbors, G.h[d], uv);
        g[d] = (ar - al) / hc;
    }
}
// ---- the fused closures on face-list partitions (ibh_turb.hip dispatches here): thread per cell, the gradients never
// leave the registers -- the expressions of k_cell_gradient_all and the pointwise formulas of ibh_les_dev.h /
// ibh_transport_dev.h, bit-identical to the composition.  What the kernels share: the 2 ND entries of cell c in the side
// table, and the way out of the table g[i][j] = d u_i / d x_j when the gradients are asked for (column ND j + i: the tuple
// cell_gradient's layout).  The loop of cell_gradient_at over the velocity components stays written in the kernels: inside
// a function it reorders a third of their instructions, and the 3-D kernels measured 1 % slower.
template <int ND>
__device__ __forceinline__ void cell_sides(const GradDims& G, int32_t nc, int64_t c, int32_t (&sd)[2 * ND]) {
#pragma unroll
    for (int s = 0; s < 2 * ND; ++s) sd[s] = G.side[(int64_t)s * nc + c];
}
template <int ND>
__device__ __forceinline__ void store_gradients(const float (&g)[ND][ND], float* __restrict__ Gout, int64_t ldg, int64_t c) {
#pragma unroll
    for (int i = 0; i < ND; ++i)
#pragma unroll
        for (int j = 0; j < ND; ++j) Gout[(int64_t)(ND * j + i) * ldg + c] = g[i][j];
}
// ibh_shear_rate_of_velocity[_grad]: k_les_of_cells without a model, asked for S (and G) -- kept as a kernel of its own for
// its registers (71 against 78 VGPRs in 3-D: seven waves per SIMD against six)
template <int ND>
__global__ void k_shear_of_velocity_cells(int32_t nc, GradDims G, const float* __restrict__ vel, int64_t ldv,
                                          float* __restrict__ S, float* __restrict__ Gout, int64_t ldg) {
    for (int64_t c = IBH_WG_X() * (int64_t)blockDim.x + threadIdx.x; c < nc; c += (int64_t)gridDim.x * blockDim.x) {
        int32_t sd[2 * ND];
        cell_sides<ND>(G, nc, c, sd);
        float g[ND][ND];   // g[i][j] = d u_i / d x_j
#pragma unroll
        for (int i = 0; i < ND; ++i) cell_gradient_at<ND>(G, sd, nc, (int32_t)c, vel + (int64_t)i * ldv, g[i]);
        S[c] = les_dev::shear_rate<ND>(g);
        if (Gout) store_gradients<ND>(g, Gout, ldg, c);
    }
}
// the LES closure of a velocity field (ibh_les_of): the requested outputs from registers
template <int ND>
__global__ void k_les_of_cells(int32_t nc, GradDims G, const float* __restrict__ vel, int64_t ldv,
                               const float* __restrict__ Delta, int model, float Cmodel, les_dev::Outputs O) {
    for (int64_t c = IBH_WG_X() * (int64_t)blockDim.x + threadIdx.x; c < nc; c += (int64_t)gridDim.x * blockDim.x) {
        int32_t sd[2 * ND];
        cell_sides<ND>(G, nc, c, sd);
        float g[ND][ND];   // g[i][j] = d u_i / d x_j
#pragma unroll
        for (int i = 0; i < ND; ++i) cell_gradient_at<ND>(G, sd, nc, (int32_t)c, vel + (int64_t)i * ldv, g[i]);
        if (O.S || model == les_dev::MODEL_SMAGORINSKY) {  // (uniform, as every branch below)
            const float s = les_dev::shear_rate<ND>(g);
            if (O.S) O.S[c] = s;
            if (model == les_dev::MODEL_SMAGORINSKY) O.nusgs[c] = les_dev::smagorinsky(Delta[c], s, Cmodel);
        }
        if constexpr (ND == 3) {
            if (model == les_dev::MODEL_WALE) O.nusgs[c] = les_dev::wale(g, Delta[c], Cmodel);
        }
        if (O.ducros) O.ducros[c] = les_dev::ducros<ND>(g);
        if (O.shock) O.shock[c] = les_dev::shock<ND>(g);
        if (O.G) store_gradients<ND>(g, O.G, O.ldg, c);
    }
}
// the right-hand sides of the standard k-epsilon model (ibh_k_epsilon_rhs): standard_kϵ with the expressions of
// ibh_turb.hip's k_keps, then both transport sums in one walk over the cell's faces (tr_dev::cell_sum: the walk and the flux
// of k_scalar_transport).  The diffusivity nu + nut / sigma of the cell across a face is made from that cell's own k and eps
// -- the bits the composition reads back from nuk / nue.
template <int ND>
__global__ void k_k_epsilon_rhs_cells(int32_t nc, GradDims G, const float* __restrict__ vel, int64_t ldv,
                                      const float* __restrict__ kf, const float* __restrict__ ef, float nu, tr_dev::KEps P,
                                      float* __restrict__ rk, float* __restrict__ reps, float* __restrict__ nut,
                                      float* __restrict__ Sout, float* __restrict__ Gout, int64_t ldg) {
    for (int64_t c = IBH_WG_X() * (int64_t)blockDim.x + threadIdx.x; c < nc; c += (int64_t)gridDim.x * blockDim.x) {
        int32_t sd[2 * ND];
        cell_sides<ND>(G, nc, c, sd);
        float g[ND][ND];   // g[i][j] = d u_i / d x_j
#pragma unroll
        for (int i = 0; i < ND; ++i) cell_gradient_at<ND>(G, sd, nc, (int32_t)c, vel + (int64_t)i * ldv, g[i]);
        const float S = les_dev::shear_rate<ND>(g);
        if (Sout) Sout[c] = S;   // (uniform, as every branch on an output pointer)
        if (Gout) store_gradients<ND>(g, Gout, ldg, c);
        const float kk = kf[c], ee = ef[c];
        const float nt = tr_dev::keps_nut(P, kk, ee);
        const float Pk = nt * (S * S);
        if (nut) nut[c] = nt;
        float rt[2] = {tr_dev::keps_Sk(Pk, ee), tr_dev::keps_Se(P, Pk, kk, ee)};
        tr_dev::cell_sum<ND, 2>(G.d, G.h, sd, (int32_t)c, [&](int d, int32_t o, int32_t n, float (&f)[2]) {
            const float ho = G.h[d][o], hn = G.h[d][n];
            const float ko = kf[o], kn = kf[n], eo = ef[o], en = ef[n];
            const float vo = vel[(int64_t)d * ldv + o], vn = vel[(int64_t)d * ldv + n];
            const float nto = tr_dev::keps_nut(P, ko, eo), ntn = tr_dev::keps_nut(P, kn, en);
            f[0] = tr_dev::flux(ko, kn, nu + nto / P.sk, nu + ntn / P.sk, vo * ko, vn * kn, ho, hn);
            f[1] = tr_dev::flux(eo, en, nu + nto / P.se, nu + ntn / P.se, vo * eo, vn * en, ho, hn);
        }, rt);
        rk[c] = rt[0];
        reps[c] = rt[1];
    }
}
// Wray_Agarwal of the gradients of (R, S) (ibh_wray_agarwal_of)
template <int ND>
__global__ void k_wray_agarwal_of_cells(int32_t nc, GradDims G, const float* __restrict__ R, const float* __restrict__ S,
                                        float sigmaR, float C1, float kappa, float* __restrict__ nut,
                                        float* __restrict__ nuR, float* __restrict__ Sout) {
    const float C2 = sigmaR + C1 / (kappa * kappa);
    for (int64_t c = IBH_WG_X() * (int64_t)blockDim.x + threadIdx.x; c < nc; c += (int64_t)gridDim.x * blockDim.x) {
        int32_t sd[2 * ND];
        cell_sides<ND>(G, nc, c, sd);
        float gR[ND], gS[ND];
        cell_gradient_at<ND>(G, sd, nc, (int32_t)c, R, gR);
        cell_gradient_at<ND>(G, sd, nc, (int32_t)c, S, gS);
        float dot = gR[0] * gS[0];
#pragma unroll
        for (int d = 1; d < ND; ++d) dot = dot + gR[d] * gS[d];
        const les_dev::WrayAgarwal w = les_dev::wray_agarwal(R[c], S[c], dot, sigmaR, C1, C2);
        nut[c] = w.nut;
        nuR[c] = w.nuR;
        Sout[c] = w.S;
    }
}

__global__ void k_cell_gradient(int32_t nc, DimData D, const float* __restrict__ h, const float* __restrict__ u,
                                int64_t ldu, float* __restrict__ out, int64_t ldo) {
    int64_t v = blockIdx.y;
    const float* uv = u + v * ldu;
    for (int64_t c = IBH_WG_X() * (int64_t)blockDim.x + threadIdx.x; c < nc; c += (int64_t)gridDim.x * blockDim.x) {
        float ar = csr_mean_face_avg(D.roff, D.ridx, (int32_t)c, D.owners, D.neighbors, h, uv);
        float al = csr_mean_face_avg(D.loff, D.lidx, (int32_t)c, D.owners, D.neighbors, h, uv);
        out[c + v * ldo] = (ar - al) / h[c];
    }
}

// JST_sensor for one dim (:1091-1096): nu = (1e-7 + |gg(dp)|)/(1e-7 + ugg(|dp|)), dp = p_n - p_o
__device__ __forceinline__ void csr_mean_diff(const int32_t* __restrict__ off, const int32_t* __restrict__ idx, int32_t c,
                                              const int32_t* __restrict__ own, const int32_t* __restrict__ nei,
                                              const float* __restrict__ p, float& sd, float& sa) {
    int32_t b = off[c], e = off[c + 1];
    sd = 0.0f;
    sa = 0.0f;
    if (e == b) return;
    float w = 1.0f / (float)(e - b);
    for (int32_t k = b; k < e; ++k) {
        int32_t f = idx[k];
        float d = p[nei[f]] - p[own[f]];
        float td = d * w, ta = fabsf(d) * w;
        sd = (k == b) ? td : sd + td;
        sa = (k == b) ? ta : sa + ta;
    }
}

__device__ __forceinline__ float jst_dim(const DimData& D, const float* __restrict__ h, const float* __restrict__ p,
                                         int32_t c) {
    float dr, ar, dl, al;
    csr_mean_diff(D.roff, D.ridx, c, D.owners, D.neighbors, p, dr, ar);
    csr_mean_diff(D.loff, D.lidx, c, D.owners, D.neighbors, p, dl, al);
    float hc = h[c];
    float gg = (dr - dl) / hc;
    float ugg = (ar + al) / hc;
    return (1e-7f + fabsf(gg)) / (1e-7f + ugg);
}

__global__ void k_jst(int32_t nc, int nd, int dim, DimData D0, DimData D1, DimData D2,
                      const float* __restrict__ spacing, const float* __restrict__ p, int64_t ldp,
                      float* __restrict__ out, int64_t ldo) {
    int64_t v = blockIdx.y;
    const float* pv = p + v * ldp;
    for (int64_t c = IBH_WG_X() * (int64_t)blockDim.x + threadIdx.x; c < nc; c += (int64_t)gridDim.x * blockDim.x) {
        float nu;
        if (dim > 0) {
            const DimData& D = dim == 1 ? D0 : (dim == 2 ? D1 : D2);
            nu = jst_dim(D, spacing + (int64_t)(dim - 1) * nc, pv, (int32_t)c);
        } else {
            nu = 1e-7f;  // :1082-1086
            nu = ibh_max(nu, jst_dim(D0, spacing, pv, (int32_t)c));
            nu = ibh_max(nu, jst_dim(D1, spacing + (int64_t)nc, pv, (int32_t)c));
            if (nd == 3) nu = ibh_max(nu, jst_dim(D2, spacing + 2 * (int64_t)nc, pv, (int32_t)c));
        }
        out[c + v * ldo] = nu;
    }
}

__device__ __forceinline__ float sgn(float x) { return (float)((x > 0.0f) - (x < 0.0f)); }
__device__ __forceinline__ float minmod(float a, float b) {  // :1099
    return ibh_min(fabsf(a), fabsf(b)) * (sgn(a) + sgn(b)) / 2.0f;
}

__global__ void k_muscl(int32_t nf, const int32_t* __restrict__ own, const int32_t* __restrict__ nei,
                        const float* __restrict__ h, const float* __restrict__ u, const float* __restrict__ du,
                        int64_t ld, const float* __restrict__ Dsens, int high_order, float* __restrict__ uL,
                        float* __restrict__ uR, int64_t ldf) {
    int64_t v = blockIdx.y;
    for (int64_t f = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; f < nf; f += (int64_t)gridDim.x * blockDim.x) {
        int32_t o = own[f], n = nei[f];
        float dow = h[o] / 2.0f, dn = h[n] / 2.0f;  // owner/neighbor_distance
        float uo = u[o + v * ld], un = u[n + v * ld];
        float guf = (un - uo) / (dow + dn);
        float duo = du[o + v * ld], dun = du[n + v * ld];
        float gu = (2.0f * duo - guf) * dow;
        float Du = (2.0f * dun - guf) * dn;
        float s = minmod(Du, gu);
        float l = uo + s, r = un - s;
        if (Dsens) {
            float Df = ibh_max(ibh_max(Dsens[o], Dsens[n]), 1e-7f);
            float uf = (uo * dn + un * dow) / (dow + dn);
            if (high_order) uf = uf + (duo * dow - dun * dn) / 8.0f;
            l = l * Df + (1.0f - Df) * uf;
            r = r * Df + (1.0f - Df) * uf;
        }
        uL[f + v * ldf] = l;
        uR[f + v * ldf] = r;
    }
}

__global__ void k_accumulate(int32_t n_out, const int32_t* __restrict__ off, const int32_t* __restrict__ idx,
                             const float* __restrict__ w, const int32_t* __restrict__ remap,
                             const float* __restrict__ v, int64_t ldv, float* __restrict__ out, int64_t ldo) {
    int64_t var = blockIdx.y;
    const float* vv = v + var * ldv;
    for (int64_t r = IBH_WG_X() * (int64_t)blockDim.x + threadIdx.x; r < n_out; r += (int64_t)gridDim.x * blockDim.x) {
        int32_t b = off[r], e = off[r + 1];
        float s = 0.0f;
        for (int32_t k = b; k < e; ++k) {
            int32_t j = idx[k];
            if (remap) j = remap[j];
            float t = w ? vv[j] * w[k] : vv[j];
            s = (k == b) ? t : s + t;
        }
        out[r + var * ldo] = s;
    }
}

// The same for several fields at once: one thread per row, the row's indices and weights read once for up to NVB
// fields (the per-(row, field) form reads them once per field).  Same sum order per field.
// v2 (optional): the stencil is applied to v - v2 (elementwise difference first, like `acc(a .- b)`); ADD: out .+= result
template <int NVB, bool ADD = false>
__global__ void k_accumulate_rows(int32_t n_out, const int32_t* __restrict__ off, const int32_t* __restrict__ idx,
                                  const float* __restrict__ w, const int32_t* __restrict__ remap,
                                  const float* __restrict__ v, int64_t ldv, float* __restrict__ out, int64_t ldo, int nv,
                                  const float* __restrict__ v2 = nullptr) {
    const int v0 = blockIdx.y * NVB;
    const int nb = min(NVB, nv - v0);
    const float* vv = v + (int64_t)v0 * ldv;
    const float* vv2 = v2 ? v2 + (int64_t)v0 * ldv : nullptr;
    float* oo = out + (int64_t)v0 * ldo;
    for (int64_t r = IBH_WG_X() * (int64_t)blockDim.x + threadIdx.x; r < n_out; r += (int64_t)gridDim.x * blockDim.x) {
        const int32_t b = off[r], e = off[r + 1];
        float s[NVB];
#pragma unroll
        for (int q = 0; q < NVB; ++q) s[q] = 0.0f;
        int32_t k = b;
        // rows that start on a 16-byte boundary (the 2^nd-point transfer operators: every row) take their entries four
        // at a time: one dwordx4 of indices, one of weights, the gathers of the four entries in flight together; the
        // sum keeps the entry order
        if ((b & 3) == 0 && w)
            for (; k + 4 <= e; k += 4) {
                const int4 j4 = *reinterpret_cast<const int4*>(idx + k);
                const float4 w4 = *reinterpret_cast<const float4*>(w + k);
                int32_t jj[4] = {j4.x, j4.y, j4.z, j4.w};
                const float ww[4] = {w4.x, w4.y, w4.z, w4.w};
                if (remap) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) jj[i] = remap[jj[i]];
                }
                float x[4][NVB];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int q = 0; q < NVB; ++q)
                        if (q < nb) x[i][q] = vv[jj[i] + (int64_t)q * ldv];
                if (vv2) {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int q = 0; q < NVB; ++q)
                            if (q < nb) x[i][q] = x[i][q] - vv2[jj[i] + (int64_t)q * ldv];
                }
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int q = 0; q < NVB; ++q)
                        if (q < nb) {
                            const float t = x[i][q] * ww[i];
                            s[q] = (k + i == b) ? t : s[q] + t;
                        }
            }
        for (; k < e; ++k) {
            int32_t j = idx[k];
            if (remap) j = remap[j];
            const float wk = w ? w[k] : 1.0f;
#pragma unroll
            for (int q = 0; q < NVB; ++q) {
                if (q < nb) {
                    float x = vv[j + (int64_t)q * ldv];
                    if (vv2) x = x - vv2[j + (int64_t)q * ldv];
                    const float t = w ? x * wk : x;
                    s[q] = (k == b) ? t : s[q] + t;
                }
            }
        }
#pragma unroll
        for (int q = 0; q < NVB; ++q)
            if (q < nb) oo[r + (int64_t)q * ldo] = ADD ? oo[r + (int64_t)q * ldo] + s[q] : s[q];
    }
}

// out .+= acc(a .- b) for up to 8 fields with the donors' fields side by side: a pre-pass writes d[j][0..7] = a[j, :] - b[j, :]
// (32 bytes per donor), the row kernel then takes a donor with TWO 16-byte gathers instead of two 4-byte gathers per field
// (6 fields x 8 donors: 16 gather instructions per row instead of 96) -- same differences, same products, same order.
__global__ void k_pack_diff8(int32_t n_in, int nv, const float* __restrict__ a, const float* __restrict__ b, int64_t ld,
                             float* __restrict__ d) {
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < (int64_t)n_in * 8; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t j = t >> 3;
        const int q = (int)(t & 7);
        d[t] = q < nv ? a[j + (int64_t)q * ld] - b[j + (int64_t)q * ld] : 0.0f;
    }
}
template <int NV>
__global__ void k_accumulate_packed_add(int32_t n_out, const int32_t* __restrict__ off, const int32_t* __restrict__ idx,
                                        const float* __restrict__ w, const float4* __restrict__ d, float* __restrict__ out,
                                        int64_t ldo) {
    for (int64_t r = IBH_WG_X() * (int64_t)blockDim.x + threadIdx.x; r < n_out; r += (int64_t)gridDim.x * blockDim.x) {
        const int32_t b = off[r], e = off[r + 1];
        float s[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) s[q] = 0.0f;
        int32_t k = b;
        if ((b & 3) == 0)
            for (; k + 4 <= e; k += 4) {
                const int4 j4 = *reinterpret_cast<const int4*>(idx + k);
                const float4 w4 = *reinterpret_cast<const float4*>(w + k);
                const int32_t jj[4] = {j4.x, j4.y, j4.z, j4.w};
                const float ww[4] = {w4.x, w4.y, w4.z, w4.w};
                float4 lo[4], hi[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    lo[i] = d[2 * (int64_t)jj[i]];
                    if (NV > 4) hi[i] = d[2 * (int64_t)jj[i] + 1];
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float x[8] = {lo[i].x, lo[i].y, lo[i].z, lo[i].w, NV > 4 ? hi[i].x : 0.0f, NV > 4 ? hi[i].y : 0.0f,
                                        NV > 4 ? hi[i].z : 0.0f, NV > 4 ? hi[i].w : 0.0f};
#pragma unroll
                    for (int q = 0; q < NV; ++q) {
                        const float t = x[q] * ww[i];
                        s[q] = (k + i == b) ? t : s[q] + t;
                    }
                }
            }
        for (; k < e; ++k) {
            const int64_t j = idx[k];
            const float wk = w[k];
            const float4 lo = d[2 * j];
            float4 hi = float4{0.0f, 0.0f, 0.0f, 0.0f};
            if (NV > 4) hi = d[2 * j + 1];
            const float x[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
            for (int q = 0; q < NV; ++q) {
                const float t = x[q] * wk;
                s[q] = (k == b) ? t : s[q] + t;
            }
        }
#pragma unroll
        for (int q = 0; q < NV; ++q) out[r + (int64_t)q * ldo] = out[r + (int64_t)q * ldo] + s[q];
    }
}

// a[ghost] = eta*ia + (1-eta)*ba (:1242-1245); ba from array, constant, or ia (copy BC)
__global__ void k_bc_blend(int32_t ng, const int32_t* __restrict__ ghost, const float* __restrict__ eta,
                           float* __restrict__ a, int64_t lda, const float* __restrict__ ia, int64_t ldi,
                           const float* __restrict__ ba, int64_t ldb, const float* __restrict__ bconst) {
    int64_t v = blockIdx.y;
    for (int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; g < ng; g += (int64_t)gridDim.x * blockDim.x) {
        float e = eta[g];
        float i = ia[g + v * ldi];
        float b = ba ? ba[g + v * ldb] : bconst[v];
        a[ghost[g] + v * lda] = e * i + (1.0f - e) * b;
    }
}

__global__ void k_axpy_clamped(int64_t n, float omega, const float* __restrict__ r, float* __restrict__ q) {
    float w = ibh_clamp(omega, 0.0f, 1.0f);   // Julia's clamp: a NaN omega stays NaN
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        q[i] = q[i] + w * r[i];
}

__global__ void k_axpy(int64_t n, float a, const float* __restrict__ x, float* __restrict__ y) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        y[i] = a * x[i] + y[i];
}

// sum x^2 in double: workgroup sums (ibh_reduce_dev.h), added by k_sum_partials (ibh_reduce.hip)
__global__ void k_sumsq(int64_t n, const float* __restrict__ x, double* __restrict__ out) {
    double s = 0.0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        double t = (double)x[i];
        s += t * t;
    }
    s = ibh_red::wg_reduce<OPS_BLOCK, ibh_red::Sum<double>>(s);
    if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// One pass of `FAS!` over a residual array (solver.jl:80-84): rr = r [+ source]; [q += clamp(omega, 0, 1) * rr]; [sum rr^2]
// -- `r .+= source`, the fixed-point update and the norm on ONE read of r (round 3 had the sum as an ATen kernel).
// <false, true, true> is ibh_axpy_clamped_sumsq (solver.jl:82 and the norm of :84 on the same array).
template <bool SRC, bool UPD, bool NRM>
__global__ void k_fas_update(int64_t n, float omega, const float* __restrict__ r, const float* __restrict__ src,
                             float* __restrict__ q, double* __restrict__ out) {
    const float w = ibh_clamp(omega, 0.0f, 1.0f);   // Julia's clamp: a NaN omega stays NaN
    double s = 0.0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float ri = r[i];
        if (SRC) ri = ri + src[i];
        if (UPD) q[i] = q[i] + w * ri;
        if (NRM) s += (double)ri * (double)ri;
    }
    if (NRM) {
        s = ibh_red::wg_reduce<OPS_BLOCK, ibh_red::Sum<double>>(s);
        if (threadIdx.x == 0) out[blockIdx.x] = s;
    }
}

inline dim3 grid2(int64_t n, int nv) { return dim3(ibh_grid_cap(n, OPS_BLOCK, 4096), nv); }
// a thread-per-cell kernel template <int ND> over the cells of p (x nv fields): k2, k3 = its instantiations for nd = 2, 3
template <class... P, class... A>
void launch_cells(const ibh_part* p, int nv, void (*k2)(P...), void (*k3)(P...), A... args) {
    const auto k = p->nd == 2 ? k2 : k3;
    hipLaunchKernelGGL(k, grid2(p->nc, nv), dim3(OPS_BLOCK), 0, ibh_stream, args...);
}

// launch of the accumulation kernels: per (row, field) for one field, per row over blocks of up to 4 fields otherwise
static inline void launch_accumulate(int32_t n_out, const int32_t* off, const int32_t* idx, const float* w,
                                     const int32_t* remap, const float* v, int64_t ldv, float* out, int64_t ldo, int nv) {
    if (nv == 1) {
        hipLaunchKernelGGL(k_accumulate, grid2(n_out, 1), dim3(OPS_BLOCK), 0, ibh_stream, n_out, off, idx, w, remap, v, ldv,
                           out, ldo);
    } else if (nv > 4 && nv <= 8) {
        // 5..8 fields (a state vector): indices and weights read ONCE for all of them (2.0 -> 1.3 ms per application of the
        // transfer operators of a 33.6 M-cell level to 6 fields)
        hipLaunchKernelGGL(k_accumulate_rows<8>, grid2(n_out, 1), dim3(OPS_BLOCK), 0, ibh_stream, n_out, off, idx, w, remap, v,
                           ldv, out, ldo, nv, (const float*)nullptr);
    } else {
        dim3 g = grid2(n_out, (nv + 3) / 4);
        hipLaunchKernelGGL(k_accumulate_rows<4>, g, dim3(OPS_BLOCK), 0, ibh_stream, n_out, off, idx, w, remap, v, ldv, out,
                           ldo, nv, (const float*)nullptr);
    }
}


}  // namespace

#define CHECK_DIM(p, dim) IBH_REQUIRE((p) && (dim) >= 1 && (dim) <= (p)->nd, "dim out of range or null partition")
#define CHECK_NV(nv) IBH_REQUIRE((nv) >= 1 && (nv) <= 65535, "nv out of range")

extern "C" {

int ibh_gather_rows(const int32_t* rows, int32_t n, const float* src, int nv, int64_t lds, float* dst, int64_t ldd) {
    CHECK_NV(nv);
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_gather, grid2(n, nv), dim3(OPS_BLOCK), 0, ibh_stream, rows, n, src, lds, dst, ldd);
    IBH_LAUNCH_CHECK();
    return 0;
}
int ibh_scatter_rows(const int32_t* rows, int32_t n, const float* src, int nv, int64_t lds, float* dst, int64_t ldd) {
    CHECK_NV(nv);
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_scatter, grid2(n, nv), dim3(OPS_BLOCK), 0, ibh_stream, rows, n, src, lds, dst, ldd);
    IBH_LAUNCH_CHECK();
    return 0;
}
int ibh_copy_rows(const int32_t* drows, const int32_t* srows, int32_t n, const float* src, int nv, int64_t lds,
                  float* dst, int64_t ldd) {
    CHECK_NV(nv);
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_copy_rows, grid2(n, nv), dim3(OPS_BLOCK), 0, ibh_stream, drows, srows, n, src, lds, dst, ldd);
    IBH_LAUNCH_CHECK();
    return 0;
}

int ibh_at_owners(const ibh_part* p, int dim, const float* u, int nv, int64_t ldu, float* out, int64_t ldo) {
    CHECK_DIM(p, dim);
    return ibh_gather_rows(p->dim[dim - 1].owners, p->dim[dim - 1].nf, u, nv, ldu, out, ldo);
}
int ibh_at_neighbors(const ibh_part* p, int dim, const float* u, int nv, int64_t ldu, float* out, int64_t ldo) {
    CHECK_DIM(p, dim);
    return ibh_gather_rows(p->dim[dim - 1].neighbors, p->dim[dim - 1].nf, u, nv, ldu, out, ldo);
}

int ibh_at_faces(const ibh_part* p, int dim, const float* u, int nv, int64_t ldu, float* out, int64_t ldo) {
    CHECK_DIM(p, dim);
    CHECK_NV(nv);
    const DimData& D = p->dim[dim - 1];
    if (D.nf == 0) return 0;
    hipLaunchKernelGGL(k_at_faces, grid2(D.nf, nv), dim3(OPS_BLOCK), 0, ibh_stream, D.nf, D.owners, D.neighbors,
                       p->spacing + (int64_t)(dim - 1) * p->nc, u, ldu, out, ldo);
    IBH_LAUNCH_CHECK();
    return 0;
}

int ibh_green_gauss(const ibh_part* p, int dim, const float* uf, int nv, int64_t ldf, float* out, int64_t ldo,
                    int uns) {
    CHECK_DIM(p, dim);
    CHECK_NV(nv);
    const DimData& D = p->dim[dim - 1];
    if (p->nc == 0) return 0;
    hipLaunchKernelGGL(k_green_gauss, grid2(p->nc, nv), dim3(OPS_BLOCK), 0, ibh_stream, p->nc, D.loff, D.lidx, D.roff,
                       D.ridx, p->spacing + (int64_t)(dim - 1) * p->nc, uf, ldf, out, ldo, uns);
    IBH_LAUNCH_CHECK();
    return 0;
}

int ibh_cell_gradient_all(const ibh_part* p, const float* u, int nv, int64_t ldu, float* out, int64_t ldo) {
    IBH_REQUIRE(p && u && out && (p->nd == 2 || p->nd == 3), "ibh_cell_gradient_all: bad argument");
    CHECK_NV(nv);
    if (p->nc == 0) return 0;
    launch_cells(p, nv, k_cell_gradient_all<2>, k_cell_gradient_all<3>, p->nc, grad_dims(p), u, ldu, nv, out, ldo);
    IBH_LAUNCH_CHECK();
    return 0;
}

// face-list forms of the fused closures (ibh_turb.hip dispatches here on partitions without block structure, arguments
// checked)
int ibh_shear_rate_of_velocity_cells(const ibh_part* p, const float* vel, int64_t ldv, float* S, float* Gout, int64_t ldg) {
    launch_cells(p, 1, k_shear_of_velocity_cells<2>, k_shear_of_velocity_cells<3>, p->nc, grad_dims(p), vel, ldv, S, Gout, ldg);
    IBH_LAUNCH_CHECK();
    return 0;
}
int ibh_wray_agarwal_of_cells(const ibh_part* p, const float* R, const float* S, float sigmaR, float C1, float kappa,
                              float* nut, float* nuR, float* Sout) {
    launch_cells(p, 1, k_wray_agarwal_of_cells<2>, k_wray_agarwal_of_cells<3>, p->nc, grad_dims(p), R, S, sigmaR, C1, kappa,
                 nut, nuR, Sout);
    IBH_LAUNCH_CHECK();
    return 0;
}
int ibh_les_of_cells(const ibh_part* p, const float* vel, int64_t ldv, const float* Delta, int model, float Cmodel,
                     float* nusgs, float* ducros, float* shock, float* S, float* Gout, int64_t ldg) {
    launch_cells(p, 1, k_les_of_cells<2>, k_les_of_cells<3>, p->nc, grad_dims(p), vel, ldv, Delta, model, Cmodel,
                 les_dev::Outputs{nusgs, ducros, shock, S, Gout, ldg});
    IBH_LAUNCH_CHECK();
    return 0;
}
int ibh_k_epsilon_rhs_cells(const ibh_part* p, const float* vel, int64_t ldv, const float* k, const float* eps, float nu,
                            const float* params5, float* rk, float* reps, float* nut, float* S, float* Gout, int64_t ldg) {
    launch_cells(p, 1, k_k_epsilon_rhs_cells<2>, k_k_epsilon_rhs_cells<3>, p->nc, grad_dims(p), vel, ldv, k, eps, nu,
                 tr_dev::keps_params(params5), rk, reps, nut, S, Gout, ldg);
    IBH_LAUNCH_CHECK();
    return 0;
}

// the workgroup maxima of the time step live with the partition, not in the per-thread scratch: a march step launches them
// in one call and reduces them in the next (partials_done below)
static hipError_t ensure_march_tmp(ibh_part* p) {
    if (p->march_tmp) return hipSuccess;
    const hipError_t e = hipMalloc((void**)&p->march_tmp, 8192 * sizeof(float));
    if (e == hipSuccess) p->march_tmp_n = 8192;
    return e;
}

int ibh_timestep_advection(ibh_part* p, const float* C, int64_t ldc, float scale, float* dt_dev) {
    IBH_REQUIRE(p && C && dt_dev && (p->nd == 2 || p->nd == 3) && p->nc > 0, "ibh_timestep_advection: bad argument");
    IBH_HIP(ensure_march_tmp(p));
    const GradDims G = grad_dims(p);
    // one cell per thread up to 2 M cells (every load of a cell in flight at once: the kernel is two dependent round trips,
    // not bandwidth; with 1 024 workgroups and 3-4 cells per thread it took 18.6 us at 0.87 M cells)
    const int nwg = ibh_grid_cap(p->nc, OPS_BLOCK, 8192);
    const bool tiled = p->info[20] != 0;   // complete blocks in order (ibh_api.hip)
#define DT_LAUNCH(ND_, T_) \
    hipLaunchKernelGGL((k_timestep_advection<ND_, T_>), dim3(nwg), dim3(OPS_BLOCK), 0, ibh_stream, p->nc, G, C, ldc, p->march_tmp)
    if (p->nd == 2) {
        if (tiled) DT_LAUNCH(2, true);
        else DT_LAUNCH(2, false);
    } else {
        if (tiled) DT_LAUNCH(3, true);
        else DT_LAUNCH(3, false);
    }
#undef DT_LAUNCH
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
    IBH_HIP(ensure_march_tmp(p));
    const GradDims G = grad_dims(p);
    const int nwg = ibh_grid_cap(p->nc, OPS_BLOCK, 8192);
    const bool tiled = p->info[20] != 0;
#define DT_LAUNCH(ND_, T_, C_)                                                                                           \
    hipLaunchKernelGGL((k_timestep_euler<ND_, T_, C_>), dim3(nwg), dim3(OPS_BLOCK), 0, ibh_stream, p->nc, G, P, ldp, f->R, \
                       f->gamma, p->march_tmp, scale, dt_cells)
#define DT_LAUNCH_C(ND_, T_)            \
    do {                                \
        if (dt_cells) DT_LAUNCH(ND_, T_, true); \
        else DT_LAUNCH(ND_, T_, false); \
    } while (0)
    if (p->nd == 2) {
        if (tiled) DT_LAUNCH_C(2, true);
        else DT_LAUNCH_C(2, false);
    } else {
        if (tiled) DT_LAUNCH_C(3, true);
        else DT_LAUNCH_C(3, false);
    }
#undef DT_LAUNCH_C
#undef DT_LAUNCH
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
    IBH_HIP(ensure_march_tmp(p));
    const GradDims G = grad_dims(p);
    const int nwg_dt = ibh_grid_cap(p->nc, OPS_BLOCK, 8192);
    const bool tiled = p->info[20] != 0;
    int stage = partials_done ? 1 : 0;   // 0: partial maxima not launched yet, 1: final reduction not launched yet, 2: done
    for (int lv = 0; lv < s->nlev; ++lv) {
        const int32_t g0 = s->seg[lv], g1 = s->seg[lv + 1];
        if (g1 == g0) continue;
        const int nwg = ibh_grid_cap(g1 - g0, OPS_BLOCK, 2048);
        BcLaunch B{g0, g1, s->eta, s->w, s->value, s->off, s->donor, s->bidx, s->mode, s->direct[lv] ? s->ghost : nullptr,
                   s->ghost, s->gval};
        // the interpolation launch of the level
        if (stage == 0) {
#define BCDT_LAUNCH(ND_, T_)                                                                                              \
    hipLaunchKernelGGL((k_bcinterp_dt<ND_, T_>), dim3(nwg + nwg_dt), dim3(OPS_BLOCK), 0, ibh_stream, nwg, B, a, p->nc, G, C, \
                       ldc, p->march_tmp)
            if (p->nd == 2) {
                if (tiled) BCDT_LAUNCH(2, true);
                else BCDT_LAUNCH(2, false);
            } else {
                if (tiled) BCDT_LAUNCH(3, true);
                else BCDT_LAUNCH(3, false);
            }
#undef BCDT_LAUNCH
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

int ibh_cell_gradient(const ibh_part* p, int dim, const float* u, int nv, int64_t ldu, float* out, int64_t ldo) {
    CHECK_DIM(p, dim);
    CHECK_NV(nv);
    if (p->nc == 0) return 0;
    hipLaunchKernelGGL(k_cell_gradient, grid2(p->nc, nv), dim3(OPS_BLOCK), 0, ibh_stream, p->nc, p->dim[dim - 1],
                       p->spacing + (int64_t)(dim - 1) * p->nc, u, ldu, out, ldo);
    IBH_LAUNCH_CHECK();
    return 0;
}

static int distances(const ibh_part* p, int dim, int mode, float* out) {
    CHECK_DIM(p, dim);
    const DimData& D = p->dim[dim - 1];
    if (D.nf == 0) return 0;
    hipLaunchKernelGGL(k_distances, grid2(D.nf, 1), dim3(OPS_BLOCK), 0, ibh_stream, D.nf, D.owners, D.neighbors,
                       p->spacing + (int64_t)(dim - 1) * p->nc, mode, out);
    IBH_LAUNCH_CHECK();
    return 0;
}
int ibh_face_distance(const ibh_part* p, int dim, float* out) { return distances(p, dim, 0, out); }
int ibh_owner_distance(const ibh_part* p, int dim, float* out) { return distances(p, dim, 1, out); }
int ibh_neighbor_distance(const ibh_part* p, int dim, float* out) { return distances(p, dim, 2, out); }

int ibh_face_gradient(const ibh_part* p, int dim, const float* u, int nv, int64_t ldu, float* out, int64_t ldo) {
    CHECK_DIM(p, dim);
    CHECK_NV(nv);
    const DimData& D = p->dim[dim - 1];
    if (D.nf == 0) return 0;
    hipLaunchKernelGGL(k_face_gradient, grid2(D.nf, nv), dim3(OPS_BLOCK), 0, ibh_stream, D.nf, D.owners, D.neighbors,
                       p->spacing + (int64_t)(dim - 1) * p->nc, u, ldu, out, ldo);
    IBH_LAUNCH_CHECK();
    return 0;
}

int ibh_jst_sensor(const ibh_part* p, int dim, const float* q, int nv, int64_t ldp, float* out, int64_t ldo) {
    IBH_REQUIRE(p && dim >= 0 && dim <= p->nd, "ibh_jst_sensor: dim out of range");
    CHECK_NV(nv);
    if (p->nc == 0) return 0;
    hipLaunchKernelGGL(k_jst, grid2(p->nc, nv), dim3(OPS_BLOCK), 0, ibh_stream, p->nc, p->nd, dim, p->dim[0], p->dim[1],
                       p->dim[2], p->spacing, q, ldp, out, ldo);
    IBH_LAUNCH_CHECK();
    return 0;
}

int ibh_muscl(const ibh_part* p, int dim, const float* u, const float* du, int nv, int64_t ld, const float* D,
              int high_order, float* uL, float* uR, int64_t ldf) {
    CHECK_DIM(p, dim);
    CHECK_NV(nv);
    const DimData& DD = p->dim[dim - 1];
    if (DD.nf == 0) return 0;
    hipLaunchKernelGGL(k_muscl, grid2(DD.nf, nv), dim3(OPS_BLOCK), 0, ibh_stream, DD.nf, DD.owners, DD.neighbors,
                       p->spacing + (int64_t)(dim - 1) * p->nc, u, du, ld, D, high_order, uL, uR, ldf);
    IBH_LAUNCH_CHECK();
    return 0;
}

int ibh_accumulate(const ibh_acc* a, const float* v, int nv, int64_t ldv, float* out, int64_t ldo) {
    IBH_REQUIRE(a, "ibh_accumulate: null accumulator");
    CHECK_NV(nv);
    if (a->n_out == 0) return 0;
    launch_accumulate(a->n_out, a->off, a->idx, a->w, (const int32_t*)nullptr, v, ldv, out, ldo, nv);
    IBH_LAUNCH_CHECK();
    return 0;
}

int ibh_accumulate_diff_add(const ibh_acc* a, const float* v, const float* v2, int nv, int64_t ldv, float* out,
                            int64_t ldo) {
    IBH_REQUIRE(a && v && v2 && out, "ibh_accumulate_diff_add: null argument");
    CHECK_NV(nv);
    if (a->n_out == 0) return 0;
    if (a->w && nv >= 2 && nv <= 8 && (int64_t)a->n_out >= 4 * (int64_t)a->n_in) {
        // many rows per donor (a prolongation): pack the donors' differences once, gather them 16 bytes at a time
        ibh_acc* am = const_cast<ibh_acc*>(a);
        if (!am->packed) IBH_HIP(hipMalloc((void**)&am->packed, sizeof(float) * 8 * (size_t)a->n_in));
        hipLaunchKernelGGL(k_pack_diff8, grid2((int64_t)a->n_in * 8, 1), dim3(OPS_BLOCK), 0, ibh_stream, a->n_in, nv, v, v2,
                           ldv, am->packed);
        const float4* d4 = reinterpret_cast<const float4*>(am->packed);
#define PACKED_LAUNCH(N)                                                                                               \
    hipLaunchKernelGGL(k_accumulate_packed_add<N>, grid2(a->n_out, 1), dim3(OPS_BLOCK), 0, ibh_stream, a->n_out, a->off,  \
                       a->idx, a->w, d4, out, ldo)
        switch (nv) {
            case 2: PACKED_LAUNCH(2); break;
            case 3: PACKED_LAUNCH(3); break;
            case 4: PACKED_LAUNCH(4); break;
            case 5: PACKED_LAUNCH(5); break;
            case 6: PACKED_LAUNCH(6); break;
            case 7: PACKED_LAUNCH(7); break;
            default: PACKED_LAUNCH(8); break;
        }
#undef PACKED_LAUNCH
        IBH_LAUNCH_CHECK();
        return 0;
    }
    for (int v0 = 0; v0 < nv; v0 += 8) {
        const int nb = nv - v0 < 8 ? nv - v0 : 8;
        hipLaunchKernelGGL((k_accumulate_rows<8, true>), grid2(a->n_out, 1), dim3(OPS_BLOCK), 0, ibh_stream, a->n_out, a->off,
                           a->idx, a->w, (const int32_t*)nullptr, v + (int64_t)v0 * ldv, ldv, out + (int64_t)v0 * ldo, ldo,
                           nb, v2 + (int64_t)v0 * ldv);
    }
    IBH_LAUNCH_CHECK();
    return 0;
}

int ibh_bc_interp(const ibh_bc* b, const float* a, int nv, int64_t lda, float* ia, int64_t ldi) {
    IBH_REQUIRE(b, "ibh_bc_interp: null boundary");
    CHECK_NV(nv);
    if (b->ng == 0) return 0;
    launch_accumulate(b->ng, b->interp.off, b->interp.idx, b->interp.w, b->image_domain, a, lda, ia, ldi, nv);
    IBH_LAUNCH_CHECK();
    return 0;
}

int ibh_bc_blend(const ibh_bc* b, float* a, int nv, int64_t lda, const float* ia, int64_t ldi, const float* ba,
                 int64_t ldb, const float* ba_const) {
    IBH_REQUIRE(b && (ba || ba_const), "ibh_bc_blend: need ba or ba_const");
    CHECK_NV(nv);
    if (b->ng == 0) return 0;
    float* dconst = nullptr;
    if (!ba) {
        IBH_HIP(hipMallocAsync((void**)&dconst, sizeof(float) * nv, ibh_stream));
        IBH_HIP(hipMemcpyAsync(dconst, ba_const, sizeof(float) * nv, hipMemcpyHostToDevice, ibh_stream));
    }
    hipLaunchKernelGGL(k_bc_blend, grid2(b->ng, nv), dim3(OPS_BLOCK), 0, ibh_stream, b->ng, b->ghost, b->eta, a, lda,
                       ia, ldi, ba, ldb, dconst);
    IBH_LAUNCH_CHECK();
    if (dconst) IBH_HIP(hipFreeAsync(dconst, ibh_stream));
    return 0;
}

int ibh_bc_apply(const ibh_bc* b, float* a, int nv, int64_t lda, int mode, const float* ba_const) {
    IBH_REQUIRE(b && (mode == 0 || mode == 1), "ibh_bc_apply: bad mode");
    CHECK_NV(nv);
    if (b->ng == 0) return 0;
    float* ia = nullptr;
    IBH_HIP(hipMallocAsync((void**)&ia, sizeof(float) * (size_t)b->ng * nv, ibh_stream));
    int rc = ibh_bc_interp(b, a, nv, lda, ia, b->ng);
    if (!rc) rc = (mode == 0) ? ibh_bc_blend(b, a, nv, lda, ia, b->ng, nullptr, 0, ba_const)
                              : ibh_bc_blend(b, a, nv, lda, ia, b->ng, ia, b->ng, nullptr);
    hipError_t e = hipFreeAsync(ia, ibh_stream);
    if (rc) return rc;
    IBH_HIP(e);
    return 0;
}

int ibh_axpy_clamped(int64_t n, float omega, const float* r, float* q) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_axpy_clamped, dim3(ibh_grid_cap(n, OPS_BLOCK, 2048)), dim3(OPS_BLOCK), 0, ibh_stream, n, omega, r, q);
    IBH_LAUNCH_CHECK();
    return 0;
}
int ibh_axpy_clamped_sumsq(int64_t n, float omega, const float* r, float* q, double* out) {
    IBH_REQUIRE(out, "ibh_axpy_clamped_sumsq: null argument");
    return ibh_fas_update(n, omega, r, nullptr, q, out);   // k_fas_update<false, true, true>
}
int ibh_fas_update(int64_t n, float omega, const float* r, const float* source, float* q, double* out_sumsq) {
    IBH_REQUIRE(r || n <= 0, "ibh_fas_update: null residual");
    double* part = out_sumsq ? (double*)ibh_red_scratch(IBH_RED_FAS) : nullptr;
    IBH_REQUIRE(!out_sumsq || part, "ibh_fas_update: no scratch");
    if (n <= 0) {
        if (out_sumsq) IBH_HIP(hipMemsetAsync(out_sumsq, 0, sizeof(double), ibh_stream));
        return 0;
    }
    if (!q && !out_sumsq) return 0;
    const int nwg = ibh_grid_cap(n, OPS_BLOCK, 2048);
#define FAS_LAUNCH(S, U, N) \
    hipLaunchKernelGGL((k_fas_update<S, U, N>), dim3(nwg), dim3(OPS_BLOCK), 0, ibh_stream, n, omega, r, source, q, part)
    if (source) {
        if (q && out_sumsq) FAS_LAUNCH(true, true, true);
        else if (q) FAS_LAUNCH(true, true, false);
        else FAS_LAUNCH(true, false, true);
    } else {
        if (q && out_sumsq) FAS_LAUNCH(false, true, true);
        else if (q) FAS_LAUNCH(false, true, false);
        else FAS_LAUNCH(false, false, true);
    }
#undef FAS_LAUNCH
    if (out_sumsq) ibh_launch_sum_partials(nwg, part, out_sumsq);
    IBH_LAUNCH_CHECK();
    return 0;
}
int ibh_axpy(int64_t n, float a, const float* x, float* y) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_axpy, dim3(ibh_grid_cap(n, OPS_BLOCK, 2048)), dim3(OPS_BLOCK), 0, ibh_stream, n, a, x, y);
    IBH_LAUNCH_CHECK();
    return 0;
}
int ibh_sumsq(int64_t n, const float* x, double* out) {
    double* part = (double*)ibh_red_scratch(IBH_RED_SUMSQ);
    IBH_REQUIRE(out && part, "ibh_sumsq: null argument or no scratch");
    if (n <= 0) {
        IBH_HIP(hipMemsetAsync(out, 0, sizeof(double), ibh_stream));
        return 0;
    }
    const int nwg = ibh_grid_cap(n, OPS_BLOCK, 1024);
    hipLaunchKernelGGL(k_sumsq, dim3(nwg), dim3(OPS_BLOCK), 0, ibh_stream, n, x, part);
    ibh_launch_sum_partials(nwg, part, out);
    IBH_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"

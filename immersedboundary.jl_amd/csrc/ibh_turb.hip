// libibhip: turbulence closures of /root/reference/src/turbulence.jl as pointwise kernels (thread per cell / per
// ghost): wall_function :27-100, shear_rate :110-124, Smagorinsky_νSGS :135-138, standard_kϵ :176-196,
// Wray_Agarwal :222-241, Ducros_sensor :252-282, WALE_νSGS :291-337.  Float32, the reference's operation order
// (-ffp-contract=off); log/exp/pow come from the device math library (a few ulp from Julia's).
// Velocity gradients: an nd x nd table of device pointers, g[i*nd + j] = d u_i / d x_j (the reference's Matrix of vectors).
// After them: the closures on an all-block 3-D partition with the gradients made where they are consumed (block kernels
// k_shear_of_velocity3, k_wray_agarwal_of3, k_les_of3, k_scalar_transport_blocks3, k_k_epsilon_rhs3),
// and the C entries, which send the same closures on a partition without block structure to the thread-per-cell *_cells
// kernels (before the block kernels: k_shear_of_velocity_cells, k_les_of_cells, k_k_epsilon_rhs_cells,
// k_wray_agarwal_of_cells).
#include "ibh_common.h"
#include "ibh_fused_int.h"
#include "ibh_wall_dev.h"
#include "ibh_les_dev.h"
#include "ibh_transport_dev.h"
#include "ibh_grad_dev.h"

namespace {

using dt_dev::GradDims;
using dt_dev::grad_dims;
using grad_dev::cell_gradient_at;
using grad_dev::cell_sides;
using grad_dev::store_gradients;

constexpr int TB = 256;

struct GradPtrs {
    const float* g[9];
};

using wall_dev::wall_point;
using wall_dev::WallParams;
using wall_dev::wall_params;

__global__ void k_wall_rey(int64_t n, const float* __restrict__ Rey, WallParams w, float* __restrict__ yp,
                           float* __restrict__ up, float* __restrict__ mup, float* __restrict__ kp,
                           float* __restrict__ dudy) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float a, b, c, d, e;
        wall_point(Rey[i], w, a, b, c, d, e);
        yp[i] = a; up[i] = b; mup[i] = c; kp[i] = d; dudy[i] = e;
    }
}

__global__ void k_wall(int64_t n, const float* __restrict__ y, const float* __restrict__ u, const float* __restrict__ nu,
                       WallParams w, float* __restrict__ utau, float* __restrict__ nut, float* __restrict__ k,
                       float* __restrict__ omega, float* __restrict__ eps, float* __restrict__ dudn) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const wall_dev::WallOut o = wall_dev::wall_eval(y[i], u[i], nu[i], w);
        utau[i] = o.utau;
        nut[i] = o.nut;
        k[i] = o.k;
        omega[i] = o.omega;
        eps[i] = o.eps;
        dudn[i] = o.dudn;
    }
}

template <int ND>
__global__ void k_shear(int64_t n, GradPtrs G, float* __restrict__ S) {
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n; c += (int64_t)gridDim.x * blockDim.x) {
        float g[ND][ND];
        les_dev::load_table<ND>(G.g, c, g);
        S[c] = les_dev::shear_rate<ND>(g);
    }
}

__global__ void k_smagorinsky(int64_t n, const float* __restrict__ D, const float* __restrict__ S, float Cs,
                              float* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = les_dev::smagorinsky(D[i], S[i], Cs);
}

__global__ void k_keps(int64_t n, const float* __restrict__ k, const float* __restrict__ e, const float* __restrict__ S,
                       float Cmu, float sk, float se, float C1, float C2, float* __restrict__ nuk, float* __restrict__ nue,
                       float* __restrict__ Sk, float* __restrict__ Se, float* __restrict__ nut) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float kk = k[i], ee = e[i];
        const float nt = Cmu * (kk * kk) / ee;
        const float Pk = nt * (S[i] * S[i]);
        nut[i] = nt;
        nuk[i] = nt / sk;
        nue[i] = nt / se;
        Sk[i] = Pk - ee;
        Se[i] = C1 * Pk * ee / kk - C2 * (ee * ee) / kk;
    }
}

template <int ND>
__global__ void k_wray_agarwal(int64_t n, const float* __restrict__ R, const float* __restrict__ S,
                               const float* __restrict__ gR, int64_t ldr, const float* __restrict__ gS, int64_t lds,
                               float sigmaR, float C1, float kappa, float* __restrict__ nut, float* __restrict__ nuR,
                               float* __restrict__ Sout) {
    const float C2 = sigmaR + C1 / (kappa * kappa);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float dot = gR[i] * gS[i];
#pragma unroll
        for (int d = 1; d < ND; ++d) dot = dot + gR[i + d * ldr] * gS[i + d * lds];
        // (les_dev::wray_agarwal written out: this kernel is the composition the fused forms are tested against, so its body
        // is held instruction for instruction, and through the function it comes out in another order:
        // profiles/closure_forms/README.md)
        const float r = R[i], s = S[i];
        const float src = C1 * r * s + C2 * dot * (r / (s + les_dev::EPS32));
        nut[i] = r;
        nuR[i] = r * sigmaR;
        Sout[i] = ibh_min(src, 10.0f * r);
    }
}

template <int ND>
__global__ void k_ducros(int64_t n, GradPtrs G, float* __restrict__ out) {
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n; c += (int64_t)gridDim.x * blockDim.x) {
        float g[ND][ND];
        les_dev::load_table<ND>(G.g, c, g);
        out[c] = les_dev::ducros<ND>(g);
    }
}

__global__ void k_wale(int64_t n, const float* __restrict__ Delta, GradPtrs G, float Cw, float* __restrict__ out) {
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n; c += (int64_t)gridDim.x * blockDim.x) {
        float g[3][3];
        les_dev::load_table<3>(G.g, c, g);
        out[c] = les_dev::wale(g, Delta[c], Cw);
    }
}

// ---- transport of a scalar with variable diffusivity, all dimensions in one launch (thread per cell, face lists):
//   out = S + sum_d green_gauss(at_faces(nu + nuR, d) .* face_gradient(R, d) .- at_faces(vel_d .* R, d), d)
// the composition of closures.euler_wray_agarwal_residual (turbulence.jl:222-241 closes it) operation by operation -- same
// expressions, same order as the operator kernels of ibh_ops.hip (-ffp-contract=off), so the result is theirs bit for bit;
// a face's flux is evaluated by both of its cells instead of being written and read back.
struct TransportDims {
    DimData d[IBH_MAXD];
    const float* h[IBH_MAXD];
    const float* vel[IBH_MAXD];
    const int32_t* side;      // side table of the partition: sides with one face are evaluated from the cell across
};
__device__ __forceinline__ float tr_flux_on(int32_t o, int32_t n, const float* __restrict__ h, const float* __restrict__ R,
                                            const float* __restrict__ nuR, const float* __restrict__ vel, float nu) {
    const float Ro = R[o], Rn = R[n];
    return tr_dev::flux(Ro, Rn, nu + nuR[o], nu + nuR[n], vel[o] * Ro, vel[n] * Rn, h[o], h[n]);
}
template <int ND>
__global__ void k_scalar_transport(int32_t nc, TransportDims T, const float* __restrict__ R, const float* __restrict__ nuR,
                                   float nu, const float* __restrict__ S, float* __restrict__ out) {
    for (int64_t c = IBH_WG_X() * (int64_t)blockDim.x + threadIdx.x; c < nc; c += (int64_t)gridDim.x * blockDim.x) {
        float rt[1] = {S[c]};
        int32_t sd[2 * ND];
#pragma unroll
        for (int s = 0; s < 2 * ND; ++s) sd[s] = T.side[(int64_t)s * nc + c];
        tr_dev::cell_sum<ND, 1>(T.d, T.h, sd, (int32_t)c, [&](int d, int32_t o, int32_t n, float (&f)[1]) {
            f[0] = tr_flux_on(o, n, T.h[d], R, nuR, T.vel[d], nu);
        }, rt);
        out[c] = rt[0];
    }
}

// ---- the fused closures on face-list partitions (thread per cell, the gradients never leave the registers) -- the
// expressions of k_cell_gradient_all (ibh_grad_dev.h) and the pointwise formulas of ibh_les_dev.h / ibh_transport_dev.h,
// bit-identical to the composition.  The loop of cell_gradient_at over the velocity components stays written in the
// kernels: inside a function it reorders a third of their instructions, and the 3-D kernels measured 1 % slower.
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
// k_keps above, then both transport sums in one walk over the cell's faces (tr_dev::cell_sum: the walk and the flux
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

}  // namespace

#include "ibh_wave3d.h"  // (here, not at the top: the pointwise kernels above are compiled as before without it)

namespace {

// ---- closures of a turbulence model on an all-block 3-D partition, gradients consumed where they are made (one wavefront
// per 8^3 block, blk3::wave_gradients of ibh_wave3d.h: the arithmetic of the tuple cell_gradient's block sweep; the pointwise formulas are
// those of the kernels above, from ibh_les_dev.h, evaluated without contraction).  What the block kernels share:
template <int NV>
struct FieldPtrs {
    const float* f[NV];
};
// the wave's place in a launch of one wavefront per block, four per workgroup (launch_blocks3 below): blk >= nblk is idle
struct Wave3 {
    int wave, lane;
    int32_t blk;
};
__device__ __forceinline__ Wave3 wave3(int32_t nwg) {
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    return {wave, (int)(threadIdx.x & 63), __builtin_amdgcn_readfirstlane(xcd_remap(blockIdx.x, nwg) * 4 + wave)};
}
// the 3 x 3 table t[i][j] = d u_i / d x_j of the lane's cell in plane k
__device__ __forceinline__ void cell_table(const float (&g)[3][8][3], int k, float (&t)[3][3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) t[i][j] = g[i][k][j];
}
// ... and its way out when the gradients are asked for: d u_i / d x_j in column 3 j + i (the tuple cell_gradient's layout)
__device__ __forceinline__ void store_table_nt(const float (&t)[3][3], float* __restrict__ G, uint32_t ldg, uint32_t c) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) __builtin_nontemporal_store(t[i][j], G + (size_t)(3 * j + i) * ldg + c);
}

//   k_shear_of_velocity3: S = shear_rate(cell_gradient(u), cell_gradient(v), cell_gradient(w))      (turbulence.jl:110-124)
//   k_wray_agarwal_of3:   (nut, nuR, S) = Wray_Agarwal(R, S, cell_gradient(R), cell_gradient(S))    (turbulence.jl:222-241)
// 12 B in + 4 B out per cell instead of 3 x (4 in + 16 out) + 36 in + 4 out; 8 in + 12 out instead of 2 x 20 + 44.
// k_shear_of_velocity3 is k_les_of3<MODEL_NONE> below asked for S (and G), the same arithmetic in the same order; it stays a
// kernel of its own because S alone came out 4 % slower through the LES kernel (profiles/closure_forms/README.md).
// Gout (or null): the nine gradients on the way -- a Navier-Stokes closure needs them again for its viscous fluxes.
__global__ __launch_bounds__(256) void k_shear_of_velocity3(const BlockDesc3* __restrict__ blocks,
                                                            const int32_t* __restrict__ htab,
                                                            const int32_t* __restrict__ ftab, int32_t nblk, int32_t nwg,
                                                            FieldPtrs<3> V, float* __restrict__ S,
                                                            float* __restrict__ Gout, uint32_t ldg) {
    __shared__ float lds[4 * BLK3W_PASSA_LDS];
    const auto [wave, lane, blk] = wave3(nwg);
    if (blk >= nblk) return;
    const BlockDesc3 bb = blocks[blk];
    float g[3][8][3];
    blk3::wave_gradients<3>(bb, htab, ftab, blk, V.f, lds + wave * BLK3W_PASSA_LDS, lane, g);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint32_t c = (uint32_t)bb.base + lane + 64 * k;
        float t[3][3];
        cell_table(g, k, t);
        S[c] = les_dev::shear_rate<3>(t);
        if (Gout) store_table_nt(t, Gout, ldg, c);   // (uniform)
    }
}
__global__ __launch_bounds__(256) void k_wray_agarwal_of3(const BlockDesc3* __restrict__ blocks,
                                                          const int32_t* __restrict__ htab,
                                                          const int32_t* __restrict__ ftab, int32_t nblk, int32_t nwg,
                                                          FieldPtrs<2> RS, float sigmaR, float C1, float kappa,
                                                          float* __restrict__ nut, float* __restrict__ nuR,
                                                          float* __restrict__ Sout) {
    __shared__ float lds[4 * BLK3W_PASSA_LDS];
    const auto [wave, lane, blk] = wave3(nwg);
    if (blk >= nblk) return;
    const BlockDesc3 bb = blocks[blk];
    float g[2][8][3];
    // (the written-out form: over the shared body this kernel measured slower, profiles/wave3d_gradients/README.md)
    blk3::wave_gradients_written_out<2>(bb, htab, ftab, blk, RS.f, lds + wave * BLK3W_PASSA_LDS, lane, g);
    const float C2 = sigmaR + C1 / (kappa * kappa);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint32_t c = (uint32_t)bb.base + lane + 64 * k;
        float dot = g[0][k][0] * g[1][k][0];
        dot = dot + g[0][k][1] * g[1][k][1];
        dot = dot + g[0][k][2] * g[1][k][2];
        const les_dev::WrayAgarwal w = les_dev::wray_agarwal(RS.f[0][c], RS.f[1][c], dot, sigmaR, C1, C2);
        nut[c] = w.nut;
        nuR[c] = w.nuR;
        Sout[c] = w.S;
    }
}

// ---- the LES closure of a velocity field on an all-block 3-D partition, gradients consumed where they are made:
//   nusgs  = Smagorinsky_νSGS(Delta, shear_rate(g)) or WALE_νSGS(Delta, g)      (turbulence.jl:134-137, :292-337)
//   ducros = Ducros_sensor(g), shock = CFD.shock_sensor(g), S = shear_rate(g)    (:253-283, cfd.jl:589-617, :110-124)
// with g = the nine gradients of blk3::wave_gradients (the tuple cell_gradient's arithmetic) and the pointwise formulas of
// ibh_les_dev.h (those of k_shear / k_smagorinsky / k_ducros / k_wale / k_shock): bit-identical to the composition.  Which
// outputs are written is uniform over the launch: the model is a template parameter, the others branch on their pointers.
// 12 B in + 4 B per requested output (+ 4 B of Delta with a model, + 36 B with G) per cell, one launch; the composition
// writes the nine gradients (3 x (4 in + 12 out)) and reads them back once per closure (36 in + 4 out each).
// WALE: three powf per cell.  Unrolled over the lane's eight cells they are 24 copies of the expansion, so the invariants
// SS, SdSd of the eight cells go through the wave's LDS tile (free once the gradients are made) and ONE copy of the
// expansion runs in a loop over them -- g itself is never indexed dynamically.
template <int MODEL>
__global__ __launch_bounds__(256) void k_les_of3(const BlockDesc3* __restrict__ blocks, const int32_t* __restrict__ htab,
                                                 const int32_t* __restrict__ ftab, int32_t nblk, int32_t nwg,
                                                 FieldPtrs<3> V, const float* __restrict__ Delta, float Cmodel,
                                                 les_dev::Outputs O) {
    __shared__ float lds[4 * BLK3W_PASSA_LDS];
    const auto [wave, lane, blk] = wave3(nwg);
    if (blk >= nblk) return;
    const BlockDesc3 bb = blocks[blk];
    float* wl = lds + wave * BLK3W_PASSA_LDS;
    float g[3][8][3];
    blk3::wave_gradients<3>(bb, htab, ftab, blk, V.f, wl, lane, g);
    if (MODEL == les_dev::MODEL_WALE) blk2::wave_lds_sync();   // the gradients' LDS reads are done: the tile takes the invariants
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint32_t c = (uint32_t)bb.base + lane + 64 * k;
        float t[3][3];
        cell_table(g, k, t);
        if (O.S || MODEL == les_dev::MODEL_SMAGORINSKY) {  // (uniform, as every branch on O below)
            const float s = les_dev::shear_rate<3>(t);
            if (O.S) O.S[c] = s;
            if (MODEL == les_dev::MODEL_SMAGORINSKY) O.nusgs[c] = les_dev::smagorinsky(Delta[c], s, Cmodel);
        }
        if (O.ducros) O.ducros[c] = les_dev::ducros<3>(t);
        if (O.shock) O.shock[c] = les_dev::shock<3>(t);
        if (MODEL == les_dev::MODEL_WALE) {
            float SS, SdSd;
            les_dev::wale_invariants(t, SS, SdSd);
            wl[k * 64 + lane] = SS;
            wl[512 + k * 64 + lane] = SdSd;
        }
        if (O.G) store_table_nt(t, O.G, (uint32_t)O.ldg, c);
    }
    if (MODEL == les_dev::MODEL_WALE) {
        blk2::wave_lds_sync();
#pragma unroll 1
        for (int k = 0; k < 8; ++k) {
            const uint32_t c = (uint32_t)bb.base + lane + 64 * k;
            O.nusgs[c] = les_dev::wale_of_invariants(Delta[c], wl[k * 64 + lane], wl[512 + k * 64 + lane], Cmodel);
        }
    }
}

// ---- transport of a scalar with variable diffusivity on an all-block 3-D partition (k_scalar_transport above is
// the face-list form): out = S + sum_d green_gauss(at_faces(nu + nuR, d) .* face_gradient(R, d) .- at_faces(u_d .* R, d), d).
// One wavefront per 8^3 block, lane = (i, j) with its z-column of R, nu + nuR and u_d R in registers; x / y neighbours from
// four LDS tiles; lane t also owns slot t of the six sides: it gathers the cell(s) across, evaluates the side's face flux(es)
// -- one, or the mean of four behind a FINE side -- and leaves it for the boundary cell.  The expressions and their order
// are those of the face-list kernel (no contraction): equal bit for bit wherever a side has one face.
#define TR3_LDS (4 * 512 + 384)
// The transport sum of ONE scalar over one block, by one wavefront (the body of k_scalar_transport_blocks3; also run twice,
// for k and for eps, by k_k_epsilon_rhs3).  The caller holds what every scalar over the block shares -- the block's
// spacing h, the halo cells' spacing hh, the velocities of the own cells Vk and of the halo cells hV -- and the scalar's
// own values: R and T = nu + nuR at the lane's eight cells (Rk, Tk) and at its six halo slots (hR, hT).  t_at(x) gives T
// at any cell x (the three extra cells behind a FINE slot), src(k, c) the source term of cell c = plane k of this lane.
template <class TAt, class Src>
__device__ __forceinline__ void tr3_wave(const BlockDesc3& bb, const int32_t* __restrict__ ftab, uint32_t nc,
                                         const float* __restrict__ hsp, float* lds, int lane, const float (&h)[3],
                                         const float (&hh)[6], const float (&Vk)[3][8], const float (&hV)[6],
                                         const float (&Rk)[8], const float (&Tk)[8], const float (&hR)[6],
                                         const float (&hT)[6], const float* __restrict__ R, const float* __restrict__ vel,
                                         uint32_t ldv, TAt t_at, Src src, float* __restrict__ out) {
    using blk2::ldg;
    float *tR = lds, *tT = lds + 512, *tAx = lds + 1024, *tAy = lds + 1536, *Hf = lds + 2048;
    const uint32_t base = (uint32_t)bb.base;
    float Ak[3][8], hA[6];
#pragma unroll
    for (int k = 0; k < 8; ++k)
#pragma unroll
        for (int d = 0; d < 3; ++d) Ak[d][k] = Vk[d][k] * Rk[k];
#pragma unroll
    for (int s = 0; s < 6; ++s) hA[s] = hV[s] * hR[s];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        tR[k * 64 + lane] = Rk[k];
        tT[k * 64 + lane] = Tk[k];
        tAx[k * 64 + lane] = Ak[0][k];
        tAy[k * 64 + lane] = Ak[1][k];
    }
    blk2::wave_lds_sync();
    // side fluxes: slot t = lane of side s belongs to boundary cell pos(s, t) of the tile
#pragma unroll
    for (int s = 0; s < 6; ++s) {
        const int d = s >> 1;
        const bool low = (s & 1) == 0;
        const int sd = d == 0 ? 1 : d == 1 ? 8 : 64, sa = d == 0 ? 8 : 1, sb = d == 2 ? 8 : 64;
        const int pos = (low ? 0 : 7) * sd + (lane & 7) * sa + (lane >> 3) * sb;
        const float Rb = tR[pos], Tb = tT[pos];
        const float Ab = d == 0 ? tAx[pos] : d == 1 ? tAy[pos] : (low ? Ak[2][0] : Ak[2][7]);
        const float hb = h[d];
        // the halo cell is the owner on a low side, the neighbour on a high side
        float F = low ? tr_dev::flux(hR[s], Rb, hT[s], Tb, hA[s], Ab, hh[s], hb) : tr_dev::flux(Rb, hR[s], Tb, hT[s], Ab, hA[s], hb, hh[s]);
        if (bb.type[s] == SIDE_FINE) {  // wave-uniform: three more faces behind this slot, mean of the four fluxes
            const int32_t* ft = ftab + (((size_t)bb.fine * 6 + s) * 64 + lane) * 3;
            F = F * 0.25f;
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const uint32_t x = (uint32_t)ft[q];
                const float Rx = ldg(R, x), Tx = t_at(x), Ax = ldg(vel + (size_t)d * ldv, x) * Rx;
                const float hx = ldg(hsp + (size_t)d * nc, x);
                const float Fq = low ? tr_dev::flux(Rx, Rb, Tx, Tb, Ax, Ab, hx, hb) : tr_dev::flux(Rb, Rx, Tb, Tx, Ab, Ax, hb, hx);
                F = F + Fq * 0.25f;
            }
        } else {
            F = F * 1.0f;
        }
        Hf[s * 64 + lane] = F;
    }
    blk2::wave_lds_sync();
    const int i = lane & 7, j = lane >> 3;
    const bool e0 = i == 0, e1 = i == 7, e2 = j == 0, e3 = j == 7;
    const float fzl = Hf[4 * 64 + lane], fzh = Hf[5 * 64 + lane];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint32_t c = base + lane + 64 * k;
        const float *r = tR + k * 64, *t = tT + k * 64, *ax = tAx + k * 64, *ay = tAy + k * 64;
        const float Rc = Rk[k], Tc = Tk[k];
        float fl[3], fr[3];
        // x and y: inside the plane or the side's flux (x sides: slot j + 8 k, y sides: slot i + 8 k)
        const int xl = e0 ? lane : lane - 1, xr = e1 ? lane : lane + 1, yl = e2 ? lane : lane - 8, yr = e3 ? lane : lane + 8;
        const float fxl = tr_dev::flux(r[xl], Rc, t[xl], Tc, ax[xl], Ak[0][k], h[0], h[0]) * 1.0f;
        const float fxr = tr_dev::flux(Rc, r[xr], Tc, t[xr], Ak[0][k], ax[xr], h[0], h[0]) * 1.0f;
        const float fyl = tr_dev::flux(r[yl], Rc, t[yl], Tc, ay[yl], Ak[1][k], h[1], h[1]) * 1.0f;
        const float fyr = tr_dev::flux(Rc, r[yr], Tc, t[yr], Ak[1][k], ay[yr], h[1], h[1]) * 1.0f;
        fl[0] = e0 ? Hf[0 * 64 + j + 8 * k] : fxl;
        fr[0] = e1 ? Hf[1 * 64 + j + 8 * k] : fxr;
        fl[1] = e2 ? Hf[2 * 64 + i + 8 * k] : fyl;
        fr[1] = e3 ? Hf[3 * 64 + i + 8 * k] : fyr;
        // z: registers
        const int kl = k > 0 ? k - 1 : 0, kh = k < 7 ? k + 1 : 7;
        const float fzl_in = tr_dev::flux(Rk[kl], Rc, Tk[kl], Tc, Ak[2][kl], Ak[2][k], h[2], h[2]) * 1.0f;
        const float fzr_in = tr_dev::flux(Rc, Rk[kh], Tc, Tk[kh], Ak[2][k], Ak[2][kh], h[2], h[2]) * 1.0f;
        fl[2] = k == 0 ? fzl : fzl_in;
        fr[2] = k == 7 ? fzh : fzr_in;
        float rt = src(k, c);
#pragma unroll
        for (int d = 0; d < 3; ++d) rt = rt + (fr[d] - fl[d]) / h[d];
        out[c] = rt;
    }
}
// what every scalar transported over a block shares: halo ids, spacings, velocities -- loaded once
struct Tr3Shared {
    uint32_t hid[6];
    float h[3], hh[6], Vk[3][8], hV[6];
};
__device__ __forceinline__ void tr3_shared(const BlockDesc3& bb, const int32_t* __restrict__ htab, int32_t blk, int lane,
                                           uint32_t nc, const float* __restrict__ hsp, const float* __restrict__ vel,
                                           uint32_t ldv, Tr3Shared& W) {
    using blk2::ldg;
    const uint32_t base = (uint32_t)bb.base;
    W.h[0] = hsp[base];                      // the block's spacing as the cells hold it
    W.h[1] = hsp[nc + base];
    W.h[2] = hsp[2 * (size_t)nc + base];
#pragma unroll
    for (int k = 0; k < 8; ++k)
#pragma unroll
        for (int d = 0; d < 3; ++d) W.Vk[d][k] = ldg(vel + (size_t)d * ldv, base + lane + 64 * k);
    blk3::halo_ids(bb, htab, blk, lane, W.hid);
#pragma unroll
    for (int s = 0; s < 6; ++s) {
        const int d = s >> 1;
        W.hV[s] = ldg(vel + (size_t)d * ldv, W.hid[s]);
        W.hh[s] = ldg(hsp + (size_t)d * nc, W.hid[s]);
    }
}
__global__ __launch_bounds__(256) void k_scalar_transport_blocks3(const BlockDesc3* __restrict__ blocks,
                                                                  const int32_t* __restrict__ htab,
                                                                  const int32_t* __restrict__ ftab, int32_t nblk,
                                                                  int32_t nwg, uint32_t nc, const float* __restrict__ hsp,
                                                                  const float* __restrict__ R, const float* __restrict__ nuR,
                                                                  float nu, const float* __restrict__ vel, uint32_t ldv,
                                                                  const float* __restrict__ S, float* __restrict__ out) {
    using blk2::ldg;
    __shared__ float lds_all[4 * TR3_LDS];
    const auto [wave, lane, blk] = wave3(nwg);
    if (blk >= nblk) return;
    const BlockDesc3 bb = blocks[blk];
    Tr3Shared W;
    tr3_shared(bb, htab, blk, lane, nc, hsp, vel, ldv, W);
    float Rk[8], Tk[8], hR[6], hT[6];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint32_t c = (uint32_t)bb.base + lane + 64 * k;
        Rk[k] = ldg(R, c);
        Tk[k] = nu + ldg(nuR, c);
    }
#pragma unroll
    for (int s = 0; s < 6; ++s) {
        hR[s] = ldg(R, W.hid[s]);
        hT[s] = nu + ldg(nuR, W.hid[s]);
    }
    tr3_wave(bb, ftab, nc, hsp, lds_all + wave * TR3_LDS, lane, W.h, W.hh, W.Vk, W.hV, Rk, Tk, hR, hT, R, vel, ldv,
             [=](uint32_t x) { return nu + ldg(nuR, x); }, [=](int, uint32_t c) { return ldg(S, c); }, out);
}

// ---- the right-hand sides of the standard k-epsilon model on an all-block 3-D partition in one launch (ibh_k_epsilon_rhs):
//   S = shear_rate(g), (nuk, nue, Sk, Se, nut) = standard_kϵ(k, eps, S)                       (turbulence.jl:110-124, :175-194)
//   rk = Sk + transport(k; nu + nuk),  reps = Se + transport(eps; nu + nue)                   (tr3_wave above)
// One wavefront per 8^3 block.  Stage 1: blk3::wave_gradients on the velocities -> S of the lane's eight cells (G stored on
// the way when asked); only the production nut S^2 stays live.  Stage 2: tr3_wave for k, then for eps, in a loop that is
// not unrolled (one copy of the body, one scalar's registers).  nut = Cmu k^2 / eps is pointwise, so the diffusivity of a
// neighbour cell is made from that cell's own k and eps with the expressions of k_keps -- the bits the composition reads
// back from the nuk / nue arrays -- and nuk, nue, Sk, Se never exist in memory: 20 B in + 8 B (+ 4 B nut) out per cell.
// The LDS tile of the wave is reused between the stages (max(BLK3W_PASSA_LDS, TR3_LDS) floats).
#define KE3_LDS (TR3_LDS > BLK3W_PASSA_LDS ? TR3_LDS : BLK3W_PASSA_LDS)
__global__ __launch_bounds__(256) void k_k_epsilon_rhs3(const BlockDesc3* __restrict__ blocks, const int32_t* __restrict__ htab,
                                                        const int32_t* __restrict__ ftab, int32_t nblk, int32_t nwg,
                                                        uint32_t nc, const float* __restrict__ hsp,
                                                        const float* __restrict__ vel, uint32_t ldv,
                                                        const float* __restrict__ kf, const float* __restrict__ ef, float nu,
                                                        tr_dev::KEps P, float* __restrict__ rk, float* __restrict__ reps,
                                                        float* __restrict__ nut, float* __restrict__ Sout,
                                                        float* __restrict__ Gout, uint32_t ldg_) {
    using blk2::ldg;
    __shared__ float lds_all[4 * KE3_LDS];
    const auto [wave, lane, blk] = wave3(nwg);
    if (blk >= nblk) return;
    const BlockDesc3 bb = blocks[blk];
    float* wl = lds_all + wave * KE3_LDS;
    const uint32_t base = (uint32_t)bb.base;
    float Pk[8];   // S, then the production nut S^2
    {
        const FieldPtrs<3> V{{vel, vel + ldv, vel + 2 * (size_t)ldv}};
        float g[3][8][3];
        blk3::wave_gradients<3>(bb, htab, ftab, blk, V.f, wl, lane, g);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint32_t c = base + lane + 64 * k;
            float t[3][3];
            cell_table(g, k, t);
            Pk[k] = les_dev::shear_rate<3>(t);
            if (Sout) Sout[c] = Pk[k];   // (uniform, as every branch on an output pointer)
            if (Gout) store_table_nt(t, Gout, ldg_, c);
        }
    }
    Tr3Shared W;
    tr3_shared(bb, htab, blk, lane, nc, hsp, vel, ldv, W);
    float kk[8], ee[8], nt[8], hk[6], he[6], hnt[6];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint32_t c = base + lane + 64 * k;
        kk[k] = ldg(kf, c);
        ee[k] = ldg(ef, c);
        nt[k] = tr_dev::keps_nut(P, kk[k], ee[k]);
        Pk[k] = nt[k] * (Pk[k] * Pk[k]);
        if (nut) nut[c] = nt[k];
    }
#pragma unroll
    for (int s = 0; s < 6; ++s) {
        hk[s] = ldg(kf, W.hid[s]);
        he[s] = ldg(ef, W.hid[s]);
        hnt[s] = tr_dev::keps_nut(P, hk[s], he[s]);
    }
#pragma unroll 1
    for (int q = 0; q < 2; ++q) {
        blk2::wave_lds_sync();   // the LDS reads of the stage before are done: the tile takes this scalar
        const bool second = q != 0;   // (uniform)
        const float* __restrict__ R = second ? ef : kf;
        float* __restrict__ out = second ? reps : rk;
        const float sg = second ? P.se : P.sk;
        float Rk[8], Tk[8], hR[6], hT[6];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            Rk[k] = second ? ee[k] : kk[k];
            Tk[k] = nu + nt[k] / sg;
        }
#pragma unroll
        for (int s = 0; s < 6; ++s) {
            hR[s] = second ? he[s] : hk[s];
            hT[s] = nu + hnt[s] / sg;
        }
        tr3_wave(bb, ftab, nc, hsp, wl, lane, W.h, W.hh, W.Vk, W.hV, Rk, Tk, hR, hT, R, vel, ldv,
                 [=](uint32_t x) { return nu + tr_dev::keps_nut(P, ldg(kf, x), ldg(ef, x)) / sg; },
                 [&](int k, uint32_t) { return second ? tr_dev::keps_Se(P, Pk[k], kk[k], ee[k]) : tr_dev::keps_Sk(Pk[k], ee[k]); },
                 out);
    }
}

inline int tgrid(int64_t n) {
    int g = ibh_grid(n, TB);
    return g > 4096 ? 4096 : g;
}
// a pointwise kernel template <int ND> over n elements: k2, k3 = its instantiations for nd = 2, 3
template <class... P, class... A>
void launch_nd(int nd, int64_t n, void (*k2)(P...), void (*k3)(P...), A... args) {
    const auto k = nd == 2 ? k2 : k3;
    hipLaunchKernelGGL(k, dim3(tgrid(n)), dim3(TB), 0, ibh_stream, args...);
}
// a block kernel over an all-block 3-D partition: one wavefront per 8^3 block, four per workgroup (wave3), and the five
// arguments every block kernel starts with
template <class... P, class... A>
void launch_blocks3(void (*k)(const BlockDesc3*, const int32_t*, const int32_t*, int32_t, int32_t, P...), const ibh_part* p,
                    A... args) {
    const int32_t nwg = (p->nblk + 3) / 4;
    hipLaunchKernelGGL(k, dim3(nwg), dim3(256), 0, ibh_stream, p->blocks3, p->htab3, p->ftab3, p->nblk, nwg, args...);
}
// the dispatch of a fused closure: nothing on an empty partition, cells() on one without block structure (the *_cells
// kernels above through launch_nd; the tuple cell_gradient is the face-list kernel there), blocks() on one made of complete
// 3-D blocks, the caller's message anywhere else
template <class Cells, class Blocks>
int fused_closure(const ibh_part* p, const char* needs, Cells cells, Blocks blocks) {
    if (p->nc == 0) return 0;
    if (!fused::has_blocks(p)) cells();
    else {
        IBH_REQUIRE(fused::all_blocks3(p), needs);
        blocks();
    }
    IBH_LAUNCH_CHECK();
    return 0;
}
}  // namespace

extern "C" {

int ibh_turb_wall_function_rey(int64_t n, const float* Rey, const float* params8, int n_iter, float* yplus, float* uplus,
                               float* muplus, float* kplus, float* dudy) {
    if (n <= 0) return 0;
    IBH_REQUIRE(Rey && params8 && yplus && uplus && muplus && kplus && dudy, "ibh_turb_wall_function_rey: null argument");
    hipLaunchKernelGGL(k_wall_rey, dim3(tgrid(n)), dim3(TB), 0, ibh_stream, n, Rey, wall_params(params8, n_iter), yplus,
                       uplus, muplus, kplus, dudy);
    IBH_LAUNCH_CHECK();
    return 0;
}
int ibh_turb_wall_function(int64_t n, const float* y, const float* u, const float* nu, const float* params8, int n_iter,
                           float* utau, float* nut, float* k, float* omega, float* eps, float* dudn) {
    if (n <= 0) return 0;
    IBH_REQUIRE(y && u && nu && params8 && utau && nut && k && omega && eps && dudn, "ibh_turb_wall_function: null argument");
    hipLaunchKernelGGL(k_wall, dim3(tgrid(n)), dim3(TB), 0, ibh_stream, n, y, u, nu, wall_params(params8, n_iter), utau,
                       nut, k, omega, eps, dudn);
    IBH_LAUNCH_CHECK();
    return 0;
}
static int grad_ptrs(int nd, const float* const* g, GradPtrs* G) {
    IBH_REQUIRE(g && (nd == 2 || nd == 3), "velocity gradient: nd x nd table of device pointers, nd = 2 or 3");
    for (int k = 0; k < nd * nd; ++k) {
        IBH_REQUIRE(g[k], "velocity gradient: null component");
        G->g[k] = g[k];
    }
    return 0;
}
int ibh_turb_shear_rate(int nd, int64_t n, const float* const* g, float* S) {
    if (n <= 0) return 0;
    GradPtrs G;
    int rc = grad_ptrs(nd, g, &G);
    if (rc) return rc;
    IBH_REQUIRE(S, "ibh_turb_shear_rate: null argument");
    launch_nd(nd, n, k_shear<2>, k_shear<3>, n, G, S);
    IBH_LAUNCH_CHECK();
    return 0;
}
int ibh_turb_smagorinsky(int64_t n, const float* Delta, const float* S, float Cs, float* out) {
    if (n <= 0) return 0;
    IBH_REQUIRE(Delta && S && out, "ibh_turb_smagorinsky: null argument");
    hipLaunchKernelGGL(k_smagorinsky, dim3(tgrid(n)), dim3(TB), 0, ibh_stream, n, Delta, S, Cs, out);
    IBH_LAUNCH_CHECK();
    return 0;
}
int ibh_turb_k_epsilon(int64_t n, const float* k, const float* eps, const float* S, const float* params5, float* nuk,
                       float* nue, float* Sk, float* Se, float* nut) {
    if (n <= 0) return 0;
    IBH_REQUIRE(k && eps && S && params5 && nuk && nue && Sk && Se && nut, "ibh_turb_k_epsilon: null argument");
    hipLaunchKernelGGL(k_keps, dim3(tgrid(n)), dim3(TB), 0, ibh_stream, n, k, eps, S, params5[0], params5[1], params5[2],
                       params5[3], params5[4], nuk, nue, Sk, Se, nut);
    IBH_LAUNCH_CHECK();
    return 0;
}
int ibh_turb_wray_agarwal(int nd, int64_t n, const float* R, const float* S, const float* gradR, int64_t ldr,
                          const float* gradS, int64_t lds, float sigmaR, float C1, float kappa, float* nut, float* nuR,
                          float* Sout) {
    if (n <= 0) return 0;
    IBH_REQUIRE(R && S && gradR && gradS && nut && nuR && Sout && (nd == 2 || nd == 3), "ibh_turb_wray_agarwal: bad argument");
    launch_nd(nd, n, k_wray_agarwal<2>, k_wray_agarwal<3>, n, R, S, gradR, ldr, gradS, lds, sigmaR, C1, kappa, nut, nuR, Sout);
    IBH_LAUNCH_CHECK();
    return 0;
}
// ibh_scalar_transport on an all-block 3-D partition (*done = 0: not applicable here)
int ibh_scalar_transport_blocks(const ibh_part* p, const float* R, const float* nuR, float nu, const float* vel, int64_t ldv,
                                const float* S, float* out, int* done) {
    *done = 0;
    if (!fused::all_blocks3(p) || !fused::T.transport_blocks) return 0;
    launch_blocks3(k_scalar_transport_blocks3, p, (uint32_t)p->nc, p->spacing, R, nuR, nu, vel, (uint32_t)ldv, S, out);
    IBH_LAUNCH_CHECK();
    *done = 1;
    return 0;
}
int ibh_scalar_transport(const ibh_part* p, const float* R, const float* nuR, float nu, const float* vel, int64_t ldv,
                         const float* S, float* out) {
    IBH_REQUIRE(p && R && nuR && vel && S && out && (p->nd == 2 || p->nd == 3), "ibh_scalar_transport: bad argument");
    if (p->nc == 0) return 0;
    {
        int done = 0;   // all-block 3-D partitions: the block kernel
        const int rc = ibh_scalar_transport_blocks(p, R, nuR, nu, vel, ldv, S, out, &done);
        if (rc || done) return rc;
    }
    TransportDims T;
    for (int d = 0; d < p->nd; ++d) {
        T.d[d] = p->dim[d];
        T.h[d] = p->spacing + (int64_t)d * p->nc;
        T.vel[d] = vel + (int64_t)d * ldv;
    }
    T.side = p->side;
    launch_nd(p->nd, p->nc, k_scalar_transport<2>, k_scalar_transport<3>, p->nc, T, R, nuR, nu, S, out);
    IBH_LAUNCH_CHECK();
    return 0;
}
int ibh_turb_ducros(int nd, int64_t n, const float* const* g, float* out) {
    if (n <= 0) return 0;
    GradPtrs G;
    int rc = grad_ptrs(nd, g, &G);
    if (rc) return rc;
    IBH_REQUIRE(out, "ibh_turb_ducros: null argument");
    launch_nd(nd, n, k_ducros<2>, k_ducros<3>, n, G, out);
    IBH_LAUNCH_CHECK();
    return 0;
}
int ibh_turb_wale(int64_t n, const float* Delta, const float* const* g, float Cw, float* out) {
    if (n <= 0) return 0;
    GradPtrs G;
    int rc = grad_ptrs(3, g, &G);
    if (rc) return rc;
    IBH_REQUIRE(Delta && out, "ibh_turb_wale: null argument");
    hipLaunchKernelGGL(k_wale, dim3(tgrid(n)), dim3(TB), 0, ibh_stream, n, Delta, G, Cw, out);
    IBH_LAUNCH_CHECK();
    return 0;
}

// The fused closures (fused_closure above): face-list kernels on a partition without block structure, block kernels on one
// made of complete blocks
int ibh_shear_rate_of_velocity_grad(ibh_part* p, const float* vel, int64_t ldv, float* S, float* G, int64_t ldg) {
    IBH_REQUIRE(p && vel && S, "ibh_shear_rate_of_velocity: null argument");
    IBH_REQUIRE(!G || ldg >= p->nc, "ibh_shear_rate_of_velocity_grad: ldg < nc");
    return fused_closure(
        p, "ibh_shear_rate_of_velocity: needs a 3-D partition made of complete blocks or one without "
           "block structure (compose cell_gradient and shear_rate otherwise)",
        [&] {
            launch_nd(p->nd, p->nc, k_shear_of_velocity_cells<2>, k_shear_of_velocity_cells<3>, p->nc, grad_dims(p), vel, ldv, S,
                      G, ldg);
        },
        [&] { launch_blocks3(k_shear_of_velocity3, p, FieldPtrs<3>{{vel, vel + ldv, vel + 2 * ldv}}, S, G, (uint32_t)ldg); });
}
int ibh_shear_rate_of_velocity(ibh_part* p, const float* vel, int64_t ldv, float* S) {
    return ibh_shear_rate_of_velocity_grad(p, vel, ldv, S, nullptr, 0);
}
int ibh_wray_agarwal_of(ibh_part* p, const float* R, const float* S, float sigmaR, float C1, float kappa, float* nut,
                        float* nuR, float* Sout) {
    IBH_REQUIRE(p && R && S && nut && nuR && Sout, "ibh_wray_agarwal_of: null argument");
    return fused_closure(
        p, "ibh_wray_agarwal_of: needs a 3-D partition made of complete blocks or one without block "
           "structure (compose cell_gradient and Wray_Agarwal otherwise)",
        [&] {
            launch_nd(p->nd, p->nc, k_wray_agarwal_of_cells<2>, k_wray_agarwal_of_cells<3>, p->nc, grad_dims(p), R, S, sigmaR, C1,
                      kappa, nut, nuR, Sout);
        },
        [&] { launch_blocks3(k_wray_agarwal_of3, p, FieldPtrs<2>{{R, S}}, sigmaR, C1, kappa, nut, nuR, Sout); });
}

// The LES closure of a velocity field in one launch
int ibh_les_of(ibh_part* p, const float* vel, int64_t ldv, const float* Delta, int model, float Cmodel, float* nusgs,
               float* ducros, float* shock, float* S, float* G, int64_t ldg) {
    IBH_REQUIRE(p && vel, "ibh_les_of: null partition or velocity");
    IBH_REQUIRE(nusgs || ducros || shock || S || G, "ibh_les_of: no output requested");
    IBH_REQUIRE(model >= 0 && model <= 2, "ibh_les_of: model must be 0 (none), 1 (Smagorinsky) or 2 (WALE)");
    IBH_REQUIRE(model == 0 || Delta, "ibh_les_of: a model needs Delta");
    IBH_REQUIRE(model == 0 || nusgs, "ibh_les_of: a model needs nusgs to write to");
    IBH_REQUIRE(model != 0 || !nusgs, "ibh_les_of: nusgs requested without a model");
    IBH_REQUIRE(ldv >= p->nc, "ibh_les_of: ldv < nc");
    IBH_REQUIRE(!G || ldg >= p->nc, "ibh_les_of: ldg < nc");
    IBH_REQUIRE(model != 2 || p->nd == 3, "ibh_les_of: WALE model only implemented for 3D");
    return fused_closure(
        p, "ibh_les_of: needs a 3-D partition made of complete blocks or one without block "
           "structure (compose cell_gradient and the pointwise closures otherwise)",
        [&] {
            launch_nd(p->nd, p->nc, k_les_of_cells<2>, k_les_of_cells<3>, p->nc, grad_dims(p), vel, ldv, Delta, model, Cmodel,
                      les_dev::Outputs{nusgs, ducros, shock, S, G, ldg});
        },
        [&] {
            launch_blocks3(model == 0 ? k_les_of3<0> : model == 1 ? k_les_of3<1> : k_les_of3<2>, p,
                           FieldPtrs<3>{{vel, vel + ldv, vel + 2 * ldv}}, Delta, Cmodel,
                           les_dev::Outputs{nusgs, ducros, shock, S, G, ldg});
        });
}

// The right-hand sides of the standard k-epsilon model in one launch
int ibh_k_epsilon_rhs(ibh_part* p, const float* vel, int64_t ldv, const float* k, const float* eps, float nu,
                      const float* params5, float* rk, float* reps, float* nut, float* S, float* G, int64_t ldg) {
    IBH_REQUIRE(p && vel && k && eps && params5 && rk && reps, "ibh_k_epsilon_rhs: null argument");
    IBH_REQUIRE(ldv >= p->nc, "ibh_k_epsilon_rhs: ldv < nc");
    IBH_REQUIRE(!G || ldg >= p->nc, "ibh_k_epsilon_rhs: ldg < nc");
    IBH_REQUIRE(p->nc == 0 || p->nd == 2 || p->nd == 3, "ibh_k_epsilon_rhs: the partition is neither 2-D nor 3-D");
    return fused_closure(
        p, "ibh_k_epsilon_rhs: needs a 3-D partition made of complete blocks or one without block "
           "structure (compose shear_rate_of_velocity, standard_k_epsilon and scalar_transport otherwise)",
        [&] {
            launch_nd(p->nd, p->nc, k_k_epsilon_rhs_cells<2>, k_k_epsilon_rhs_cells<3>, p->nc, grad_dims(p), vel, ldv, k, eps, nu,
                      tr_dev::keps_params(params5), rk, reps, nut, S, G, ldg);
        },
        [&] {
            launch_blocks3(k_k_epsilon_rhs3, p, (uint32_t)p->nc, p->spacing, vel, (uint32_t)ldv, k, eps, nu,
                           tr_dev::keps_params(params5), rk, reps, nut, S, G, (uint32_t)ldg);
        });
}

}  // extern "C"

// libibhip: turbulence closures of /root/reference/src/turbulence.jl as pointwise kernels (thread per cell / per
// ghost): wall_function :27-100, shear_rate :110-124, Smagorinsky_νSGS :135-138, standard_kϵ :176-196,
// Wray_Agarwal :222-241, Ducros_sensor :252-282, WALE_νSGS :291-337.  Float32, the reference's operation order
// (-ffp-contract=off); log/exp/pow come from the device math library (a few ulp from Julia's).
// Velocity gradients: an nd x nd table of device pointers, g[i*nd + j] = d u_i / d x_j (the reference's Matrix of vectors).
// At the end: the closures on an all-block 3-D partition with the gradients made where they are consumed (block kernels).
#include "ibh_common.h"
#include "ibh_fused_int.h"
#include "ibh_wall_dev.h"
#include "ibh_les_dev.h"

namespace {

constexpr int TB = 256;
constexpr float EPS32 = wall_dev::EPS32;

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
        const float r = R[i], s = S[i];
        const float src = C1 * r * s + C2 * dot * (r / (s + EPS32));
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
__device__ __forceinline__ float tr_face_avg(float uo, float un, float ho, float hn) { return (uo * hn + un * ho) / (hn + ho); }
__device__ __forceinline__ float tr_flux_on(int32_t o, int32_t n, const float* __restrict__ h, const float* __restrict__ R,
                                            const float* __restrict__ nuR, const float* __restrict__ vel, float nu) {
    const float ho = h[o], hn = h[n];
    const float Ro = R[o], Rn = R[n];
    const float conv = tr_face_avg(vel[o] * Ro, vel[n] * Rn, ho, hn);       // at_faces(vel_d .* R)
    const float nuf = tr_face_avg(nu + nuR[o], nu + nuR[n], ho, hn);        // at_faces(nu .+ nuR)
    const float fd = (ho + hn) / 2.0f;                                      // face_distance
    const float fg = (Rn - Ro) / fd;                                        // face_gradient(R)
    return nuf * fg - conv;
}
__device__ __forceinline__ float tr_flux(const DimData& D, const float* __restrict__ h, const float* __restrict__ R,
                                         const float* __restrict__ nuR, const float* __restrict__ vel, float nu, int32_t f) {
    return tr_flux_on(D.owners[f], D.neighbors[f], h, R, nuR, vel, nu);
}
__device__ __forceinline__ float tr_mean(const int32_t* __restrict__ off, const int32_t* __restrict__ idx, int32_t c,
                                         const DimData& D, const float* __restrict__ h, const float* __restrict__ R,
                                         const float* __restrict__ nuR, const float* __restrict__ vel, float nu) {
    const int32_t b = off[c], e = off[c + 1];
    if (e == b) return 0.0f;
    const float w = 1.0f / (float)(e - b);
    float s = tr_flux(D, h, R, nuR, vel, nu, idx[b]) * w;
    for (int32_t k = b + 1; k < e; ++k) s = s + tr_flux(D, h, R, nuR, vel, nu, idx[k]) * w;
    return s;
}
template <int ND>
__global__ void k_scalar_transport(int32_t nc, TransportDims T, const float* __restrict__ R, const float* __restrict__ nuR,
                                   float nu, const float* __restrict__ S, float* __restrict__ out) {
    for (int64_t c = IBH_WG_X() * (int64_t)blockDim.x + threadIdx.x; c < nc; c += (int64_t)gridDim.x * blockDim.x) {
        float rt = S[c];
        int32_t sd[2 * ND];
#pragma unroll
        for (int s = 0; s < 2 * ND; ++s) sd[s] = T.side[(int64_t)s * nc + c];
#pragma unroll
        for (int d = 0; d < ND; ++d) {
            const int32_t l = sd[2 * d], r = sd[2 * d + 1];
            float ar, al;
            if (r >= 0) ar = tr_flux_on((int32_t)c, r, T.h[d], R, nuR, T.vel[d], nu) * 1.0f;
            else if (r == -2) ar = 0.0f;
            else ar = tr_mean(T.d[d].roff, T.d[d].ridx, (int32_t)c, T.d[d], T.h[d], R, nuR, T.vel[d], nu);
            if (l >= 0) al = tr_flux_on(l, (int32_t)c, T.h[d], R, nuR, T.vel[d], nu) * 1.0f;
            else if (l == -2) al = 0.0f;
            else al = tr_mean(T.d[d].loff, T.d[d].lidx, (int32_t)c, T.d[d], T.h[d], R, nuR, T.vel[d], nu);
            rt = rt + (ar - al) / T.h[d][c];
        }
        out[c] = rt;
    }
}

}  // namespace

#include "ibh_block3d.h"  // (here, not at the top: the pointwise kernels above are compiled as before without it)

namespace {

// ---- closures of a turbulence model on an all-block 3-D partition, gradients consumed where they are made (one wavefront
// per 8^3 block, blk3::wave_gradients: the arithmetic of the tuple cell_gradient's block sweep; the pointwise formulas are
// those of k_shear / k_wray_agarwal above, evaluated without contraction):
//   k_shear_of_velocity3: S = shear_rate(cell_gradient(u), cell_gradient(v), cell_gradient(w))      (turbulence.jl:110-124)
//   k_wray_agarwal_of3:   (nut, nuR, S) = Wray_Agarwal(R, S, cell_gradient(R), cell_gradient(S))    (turbulence.jl:222-241)
// 12 B in + 4 B out per cell instead of 3 x (4 in + 16 out) + 36 in + 4 out; 8 in + 12 out instead of 2 x 20 + 44.
template <int NV>
struct FieldPtrs {
    const float* f[NV];
};
__global__ __launch_bounds__(256) void k_shear_of_velocity3(const BlockDesc3* __restrict__ blocks,
                                                            const int32_t* __restrict__ htab,
                                                            const int32_t* __restrict__ ftab, int32_t nblk, int32_t nwg,
                                                            FieldPtrs<3> V, float* __restrict__ S,
                                                            float* __restrict__ Gout, uint32_t ldg) {
    // Gout (or null): the nine gradients on the way, d u_i / d x_j in column 3 j + i (the tuple cell_gradient's layout) --
    // a Navier-Stokes closure needs them again for its viscous fluxes (three pass-A sweeps otherwise)
    __shared__ float lds[4 * BLK3W_PASSA_LDS];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int32_t blk = __builtin_amdgcn_readfirstlane(xcd_remap(blockIdx.x, nwg) * 4 + wave);
    if (blk >= nblk) return;
    const BlockDesc3 bb = blocks[blk];
    float g[3][8][3];
    blk3::wave_gradients<3>(bb, htab, ftab, blk, V.f, lds + wave * BLK3W_PASSA_LDS, lane, g);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        float s = 0.0f;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const float t = (g[i][k][j] + g[j][k][i]) / 2.0f;
                s = s + t * t;
            }
        S[(uint32_t)bb.base + lane + 64 * k] = sqrtf(2.0f * s);
        if (Gout) {  // (uniform)
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j)
                    __builtin_nontemporal_store(g[i][k][j], Gout + (size_t)(3 * j + i) * ldg + (uint32_t)bb.base + lane + 64 * k);
        }
    }
}
__global__ __launch_bounds__(256) void k_wray_agarwal_of3(const BlockDesc3* __restrict__ blocks,
                                                          const int32_t* __restrict__ htab,
                                                          const int32_t* __restrict__ ftab, int32_t nblk, int32_t nwg,
                                                          FieldPtrs<2> RS, float sigmaR, float C1, float kappa,
                                                          float* __restrict__ nut, float* __restrict__ nuR,
                                                          float* __restrict__ Sout) {
    __shared__ float lds[4 * BLK3W_PASSA_LDS];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int32_t blk = __builtin_amdgcn_readfirstlane(xcd_remap(blockIdx.x, nwg) * 4 + wave);
    if (blk >= nblk) return;
    const BlockDesc3 bb = blocks[blk];
    float g[2][8][3];
    blk3::wave_gradients<2>(bb, htab, ftab, blk, RS.f, lds + wave * BLK3W_PASSA_LDS, lane, g);
    const float C2 = sigmaR + C1 / (kappa * kappa);
    constexpr float EPS32 = 1.1920929e-07f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint32_t c = (uint32_t)bb.base + lane + 64 * k;
        float dot = g[0][k][0] * g[1][k][0];
        dot = dot + g[0][k][1] * g[1][k][1];
        dot = dot + g[0][k][2] * g[1][k][2];
        const float r = RS.f[0][c], s = RS.f[1][c];
        const float src = C1 * r * s + C2 * dot * (r / (s + EPS32));
        nut[c] = r;
        nuR[c] = r * sigmaR;
        Sout[c] = ibh_min(src, 10.0f * r);
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
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int32_t blk = __builtin_amdgcn_readfirstlane(xcd_remap(blockIdx.x, nwg) * 4 + wave);
    if (blk >= nblk) return;
    const BlockDesc3 bb = blocks[blk];
    float* wl = lds + wave * BLK3W_PASSA_LDS;
    float g[3][8][3];
    blk3::wave_gradients<3>(bb, htab, ftab, blk, V.f, wl, lane, g);
    if (MODEL == les_dev::MODEL_WALE) blk2::wave_lds_sync();   // the gradients' LDS reads are done: the tile takes the invariants
    const uint32_t ldg = (uint32_t)O.ldg;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint32_t c = (uint32_t)bb.base + lane + 64 * k;
        float t[3][3];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) t[i][j] = g[i][k][j];
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
        if (O.G) {  // d u_i / d x_j in column 3 j + i (the tuple cell_gradient's layout)
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) __builtin_nontemporal_store(t[i][j], O.G + (size_t)(3 * j + i) * ldg + c);
        }
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
__device__ __forceinline__ float tr3_avg(float uo, float un, float ho, float hn) { return (uo * hn + un * ho) / (hn + ho); }
__device__ __forceinline__ float tr3_flux(float Ro, float Rn, float To, float Tn, float Ao, float An, float ho, float hn) {
    const float conv = tr3_avg(Ao, An, ho, hn);   // at_faces(u_d .* R)
    const float nuf = tr3_avg(To, Tn, ho, hn);    // at_faces(nu .+ nuR)
    const float fd = (ho + hn) / 2.0f;            // face_distance
    const float fg = (Rn - Ro) / fd;              // face_gradient(R)
    return nuf * fg - conv;
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
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int32_t blk = __builtin_amdgcn_readfirstlane(xcd_remap(blockIdx.x, nwg) * 4 + wave);
    if (blk >= nblk) return;
    float* lds = lds_all + wave * TR3_LDS;
    float *tR = lds, *tT = lds + 512, *tAx = lds + 1024, *tAy = lds + 1536, *Hf = lds + 2048;
    const BlockDesc3 bb = blocks[blk];
    const uint32_t base = (uint32_t)bb.base;
    const float h[3] = {hsp[base], hsp[nc + base], hsp[2 * (size_t)nc + base]};   // the block's spacing as the cells hold it
    float Rk[8], Tk[8], Ak[3][8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint32_t c = base + lane + 64 * k;
        Rk[k] = ldg(R, c);
        Tk[k] = nu + ldg(nuR, c);
#pragma unroll
        for (int d = 0; d < 3; ++d) Ak[d][k] = ldg(vel + (size_t)d * ldv, c) * Rk[k];
    }
    uint32_t hid[6];
    hid[0] = blk3::halo_cell3s<0>(bb, htab, blk, lane);
    hid[1] = blk3::halo_cell3s<1>(bb, htab, blk, lane);
    hid[2] = blk3::halo_cell3s<2>(bb, htab, blk, lane);
    hid[3] = blk3::halo_cell3s<3>(bb, htab, blk, lane);
    hid[4] = blk3::halo_cell3s<4>(bb, htab, blk, lane);
    hid[5] = blk3::halo_cell3s<5>(bb, htab, blk, lane);
    float hR[6], hT[6], hA[6], hh[6];
#pragma unroll
    for (int s = 0; s < 6; ++s) {
        const int d = s >> 1;
        hR[s] = ldg(R, hid[s]);
        hT[s] = nu + ldg(nuR, hid[s]);
        hA[s] = ldg(vel + (size_t)d * ldv, hid[s]) * hR[s];
        hh[s] = ldg(hsp + (size_t)d * nc, hid[s]);
    }
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
        float F = low ? tr3_flux(hR[s], Rb, hT[s], Tb, hA[s], Ab, hh[s], hb) : tr3_flux(Rb, hR[s], Tb, hT[s], Ab, hA[s], hb, hh[s]);
        if (bb.type[s] == SIDE_FINE) {  // wave-uniform: three more faces behind this slot, mean of the four fluxes
            const int32_t* ft = ftab + (((size_t)bb.fine * 6 + s) * 64 + lane) * 3;
            F = F * 0.25f;
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const uint32_t x = (uint32_t)ft[q];
                const float Rx = ldg(R, x), Tx = nu + ldg(nuR, x), Ax = ldg(vel + (size_t)d * ldv, x) * Rx;
                const float hx = ldg(hsp + (size_t)d * nc, x);
                const float Fq = low ? tr3_flux(Rx, Rb, Tx, Tb, Ax, Ab, hx, hb) : tr3_flux(Rb, Rx, Tb, Tx, Ab, Ax, hb, hx);
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
        const float fxl = tr3_flux(r[xl], Rc, t[xl], Tc, ax[xl], Ak[0][k], h[0], h[0]) * 1.0f;
        const float fxr = tr3_flux(Rc, r[xr], Tc, t[xr], Ak[0][k], ax[xr], h[0], h[0]) * 1.0f;
        const float fyl = tr3_flux(r[yl], Rc, t[yl], Tc, ay[yl], Ak[1][k], h[1], h[1]) * 1.0f;
        const float fyr = tr3_flux(Rc, r[yr], Tc, t[yr], Ak[1][k], ay[yr], h[1], h[1]) * 1.0f;
        fl[0] = e0 ? Hf[0 * 64 + j + 8 * k] : fxl;
        fr[0] = e1 ? Hf[1 * 64 + j + 8 * k] : fxr;
        fl[1] = e2 ? Hf[2 * 64 + i + 8 * k] : fyl;
        fr[1] = e3 ? Hf[3 * 64 + i + 8 * k] : fyr;
        // z: registers
        const int kl = k > 0 ? k - 1 : 0, kh = k < 7 ? k + 1 : 7;
        const float fzl_in = tr3_flux(Rk[kl], Rc, Tk[kl], Tc, Ak[2][kl], Ak[2][k], h[2], h[2]) * 1.0f;
        const float fzr_in = tr3_flux(Rc, Rk[kh], Tc, Tk[kh], Ak[2][k], Ak[2][kh], h[2], h[2]) * 1.0f;
        fl[2] = k == 0 ? fzl : fzl_in;
        fr[2] = k == 7 ? fzh : fzr_in;
        float rt = ldg(S, c);
#pragma unroll
        for (int d = 0; d < 3; ++d) rt = rt + (fr[d] - fl[d]) / h[d];
        out[c] = rt;
    }
}

inline int tgrid(int64_t n) {
    int g = ibh_grid(n, TB);
    return g > 4096 ? 4096 : g;
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
    if (nd == 2) hipLaunchKernelGGL(k_shear<2>, dim3(tgrid(n)), dim3(TB), 0, ibh_stream, n, G, S);
    else hipLaunchKernelGGL(k_shear<3>, dim3(tgrid(n)), dim3(TB), 0, ibh_stream, n, G, S);
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
    if (nd == 2)
        hipLaunchKernelGGL(k_wray_agarwal<2>, dim3(tgrid(n)), dim3(TB), 0, ibh_stream, n, R, S, gradR, ldr, gradS, lds, sigmaR,
                           C1, kappa, nut, nuR, Sout);
    else
        hipLaunchKernelGGL(k_wray_agarwal<3>, dim3(tgrid(n)), dim3(TB), 0, ibh_stream, n, R, S, gradR, ldr, gradS, lds, sigmaR,
                           C1, kappa, nut, nuR, Sout);
    IBH_LAUNCH_CHECK();
    return 0;
}
// ibh_scalar_transport on an all-block 3-D partition (*done = 0: not applicable here)
int ibh_scalar_transport_blocks(const ibh_part* p, const float* R, const float* nuR, float nu, const float* vel, int64_t ldv,
                                const float* S, float* out, int* done) {
    *done = 0;
    if (!fused::all_blocks3(p) || !fused::T.transport_blocks) return 0;
    const int32_t nwg = (p->nblk + 3) / 4;
    hipLaunchKernelGGL(k_scalar_transport_blocks3, dim3(nwg), dim3(256), 0, ibh_stream, p->blocks3, p->htab3, p->ftab3,
                       p->nblk, nwg, (uint32_t)p->nc, p->spacing, R, nuR, nu, vel, (uint32_t)ldv, S, out);
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
    if (p->nd == 2)
        hipLaunchKernelGGL(k_scalar_transport<2>, dim3(tgrid(p->nc)), dim3(TB), 0, ibh_stream, p->nc, T, R, nuR, nu, S, out);
    else
        hipLaunchKernelGGL(k_scalar_transport<3>, dim3(tgrid(p->nc)), dim3(TB), 0, ibh_stream, p->nc, T, R, nuR, nu, S, out);
    IBH_LAUNCH_CHECK();
    return 0;
}
int ibh_turb_ducros(int nd, int64_t n, const float* const* g, float* out) {
    if (n <= 0) return 0;
    GradPtrs G;
    int rc = grad_ptrs(nd, g, &G);
    if (rc) return rc;
    IBH_REQUIRE(out, "ibh_turb_ducros: null argument");
    if (nd == 2) hipLaunchKernelGGL(k_ducros<2>, dim3(tgrid(n)), dim3(TB), 0, ibh_stream, n, G, out);
    else hipLaunchKernelGGL(k_ducros<3>, dim3(tgrid(n)), dim3(TB), 0, ibh_stream, n, G, out);
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

// The fused closures: face-list kernels on a partition without block structure (the tuple cell_gradient is the face-list
// kernel there: ibh_cell_gradient_nd), block kernels on one made of complete blocks
int ibh_shear_rate_of_velocity_grad(ibh_part* p, const float* vel, int64_t ldv, float* S, float* G, int64_t ldg) {
    IBH_REQUIRE(p && vel && S, "ibh_shear_rate_of_velocity: null argument");
    IBH_REQUIRE(!G || ldg >= p->nc, "ibh_shear_rate_of_velocity_grad: ldg < nc");
    if (p->nc == 0) return 0;
    if (!fused::has_blocks(p)) return ibh_shear_rate_of_velocity_cells(p, vel, ldv, S, G, ldg);
    IBH_REQUIRE(fused::all_blocks3(p), "ibh_shear_rate_of_velocity: needs a 3-D partition made of complete blocks or one without "
                                "block structure (compose cell_gradient and shear_rate otherwise)");
    FieldPtrs<3> V{{vel, vel + ldv, vel + 2 * ldv}};
    const int32_t nwg = (p->nblk + 3) / 4;
    hipLaunchKernelGGL(k_shear_of_velocity3, dim3(nwg), dim3(256), 0, ibh_stream, p->blocks3, p->htab3, p->ftab3, p->nblk, nwg,
                       V, S, G, (uint32_t)ldg);
    IBH_LAUNCH_CHECK();
    return 0;
}
int ibh_shear_rate_of_velocity(ibh_part* p, const float* vel, int64_t ldv, float* S) {
    return ibh_shear_rate_of_velocity_grad(p, vel, ldv, S, nullptr, 0);
}
int ibh_wray_agarwal_of(ibh_part* p, const float* R, const float* S, float sigmaR, float C1, float kappa, float* nut,
                        float* nuR, float* Sout) {
    IBH_REQUIRE(p && R && S && nut && nuR && Sout, "ibh_wray_agarwal_of: null argument");
    if (p->nc == 0) return 0;
    if (!fused::has_blocks(p)) return ibh_wray_agarwal_of_cells(p, R, S, sigmaR, C1, kappa, nut, nuR, Sout);
    IBH_REQUIRE(fused::all_blocks3(p), "ibh_wray_agarwal_of: needs a 3-D partition made of complete blocks or one without block "
                                "structure (compose cell_gradient and Wray_Agarwal otherwise)");
    FieldPtrs<2> RS{{R, S}};
    const int32_t nwg = (p->nblk + 3) / 4;
    hipLaunchKernelGGL(k_wray_agarwal_of3, dim3(nwg), dim3(256), 0, ibh_stream, p->blocks3, p->htab3, p->ftab3, p->nblk, nwg,
                       RS, sigmaR, C1, kappa, nut, nuR, Sout);
    IBH_LAUNCH_CHECK();
    return 0;
}

// The LES closure of a velocity field in one launch (dispatch as ibh_shear_rate_of_velocity_grad)
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
    if (p->nc == 0) return 0;
    if (!fused::has_blocks(p)) return ibh_les_of_cells(p, vel, ldv, Delta, model, Cmodel, nusgs, ducros, shock, S, G, ldg);
    IBH_REQUIRE(fused::all_blocks3(p), "ibh_les_of: needs a 3-D partition made of complete blocks or one without block "
                                "structure (compose cell_gradient and the pointwise closures otherwise)");
    FieldPtrs<3> V{{vel, vel + ldv, vel + 2 * ldv}};
    const les_dev::Outputs O{nusgs, ducros, shock, S, G, ldg};
    const int32_t nwg = (p->nblk + 3) / 4;
#define LES3_LAUNCH(M_)                                                                                                  \
    hipLaunchKernelGGL(k_les_of3<M_>, dim3(nwg), dim3(256), 0, ibh_stream, p->blocks3, p->htab3, p->ftab3, p->nblk, nwg, V, \
                       Delta, Cmodel, O)
    if (model == 0) LES3_LAUNCH(0);
    else if (model == 1) LES3_LAUNCH(1);
    else LES3_LAUNCH(2);
#undef LES3_LAUNCH
    IBH_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"

// libibhip: device pieces of the transport terms of a turbulence scalar,
//   S + sum_d green_gauss(at_faces(nu + nuR, d) .* face_gradient(R, d) .- at_faces(vel_d .* R, d), d),
// shared by the transport kernels of ibh_turb.hip and the fused k-epsilon right-hand sides (k_k_epsilon_rhs3 and
// k_k_epsilon_rhs_cells in ibh_turb.hip).  Float32, the expressions and the order of the operator kernels of
// ibh_ops.hip (-ffp-contract=off): a sum made here is the operator-by-operator composition's bit for bit.
#pragma once
#include "ibh_common.h"

namespace tr_dev {

__device__ __forceinline__ float face_avg(float uo, float un, float ho, float hn) { return (uo * hn + un * ho) / (hn + ho); }
// flux of one face from the values of its owner (o) and neighbour (n): R, T = nu + nuR, A = vel_d R, h = spacing along d
__device__ __forceinline__ float flux(float Ro, float Rn, float To, float Tn, float Ao, float An, float ho, float hn) {
    const float conv = face_avg(Ao, An, ho, hn);   // at_faces(vel_d .* R)
    const float nuf = face_avg(To, Tn, ho, hn);    // at_faces(nu .+ nuR)
    const float fd = (ho + hn) / 2.0f;             // face_distance
    const float fg = (Rn - Ro) / fd;               // face_gradient(R)
    return nuf * fg - conv;
}

// standard_kϵ (turbulence.jl:175-194), the expressions of k_keps: the values a cell's own k and ϵ give
struct KEps {
    float Cmu, sk, se, C1, C2;
};
inline KEps keps_params(const float* params5) {   // (host) the C entries' (Cmu, sigma_k, sigma_eps, C1eps, C2eps)
    return {params5[0], params5[1], params5[2], params5[3], params5[4]};
}
__device__ __forceinline__ float keps_nut(const KEps& P, float kk, float ee) { return P.Cmu * (kk * kk) / ee; }
__device__ __forceinline__ float keps_Sk(float Pk, float ee) { return Pk - ee; }
__device__ __forceinline__ float keps_Se(const KEps& P, float Pk, float kk, float ee) {
    return P.C1 * Pk * ee / kk - P.C2 * (ee * ee) / kk;
}

// green_gauss of NS scalars at cell c over the side table (sd: the cell's 2 ND entries; >= 0: the cell across the one face
// of the side, -2: no face, else the CSR row of the side): rt[q] += sum_d (right - left) / h_d.  f(d, o, n, t) leaves the
// fluxes of the face between owner o and neighbour n along d in t[NS].
template <int NS, class F>
__device__ __forceinline__ void mean_flux(const int32_t* __restrict__ off, const int32_t* __restrict__ idx, int32_t c,
                                          const DimData& D, int d, F& f, float (&s)[NS]) {
    const int32_t b = off[c], e = off[c + 1];
    if (e == b) {
#pragma unroll
        for (int q = 0; q < NS; ++q) s[q] = 0.0f;
        return;
    }
    const float w = 1.0f / (float)(e - b);
    float t[NS];
    f(d, D.owners[idx[b]], D.neighbors[idx[b]], t);
#pragma unroll
    for (int q = 0; q < NS; ++q) s[q] = t[q] * w;
    for (int32_t k = b + 1; k < e; ++k) {
        f(d, D.owners[idx[k]], D.neighbors[idx[k]], t);
#pragma unroll
        for (int q = 0; q < NS; ++q) s[q] = s[q] + t[q] * w;
    }
}
template <int ND, int NS, class F>
__device__ __forceinline__ void cell_sum(const DimData* D, const float* const* h, const int32_t (&sd)[2 * ND], int32_t c,
                                         F f, float (&rt)[NS]) {
#pragma unroll
    for (int d = 0; d < ND; ++d) {
        const int32_t l = sd[2 * d], r = sd[2 * d + 1];
        float ar[NS], al[NS];
        if (r >= 0) {
            f(d, c, r, ar);
#pragma unroll
            for (int q = 0; q < NS; ++q) ar[q] = ar[q] * 1.0f;
        } else if (r == -2) {
#pragma unroll
            for (int q = 0; q < NS; ++q) ar[q] = 0.0f;
        } else {
            mean_flux<NS>(D[d].roff, D[d].ridx, c, D[d], d, f, ar);
        }
        if (l >= 0) {
            f(d, l, c, al);
#pragma unroll
            for (int q = 0; q < NS; ++q) al[q] = al[q] * 1.0f;
        } else if (l == -2) {
#pragma unroll
            for (int q = 0; q < NS; ++q) al[q] = 0.0f;
        } else {
            mean_flux<NS>(D[d].loff, D[d].lidx, c, D[d], d, f, al);
        }
        const float hc = h[d][c];
#pragma unroll
        for (int q = 0; q < NS; ++q) rt[q] = rt[q] + (ar[q] - al[q]) / hc;
    }
}

}  // namespace tr_dev

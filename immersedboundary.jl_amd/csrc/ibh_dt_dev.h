// libibhip: device bodies of the time-step evaluation of an explicit step (ibh_timestep_advection, ibh_timestep_euler: ibh_timestep.hip), with
// the workgroup's index and count as arguments: the same code runs as its own launches and beside the BC-set workgroups of a
// march step (ibh_timestep.hip: k_bcinterp_dt / k_bcscatter_dt).
#pragma once
#include "ibh_common.h"
#include "ibh_reduce_dev.h"

#define DT_BLOCK 256

namespace dt_dev {

// at_faces (:907-909): (u_o*h_n + u_n*h_o)/(h_n + h_o)
__device__ __forceinline__ float dt_face_avg(float uo, float un, float ho, float hn) { return (uo * hn + un * ho) / (hn + ho); }
template <class Load>
__device__ __forceinline__ float dt_csr_mean_face_avg(const int32_t* __restrict__ off, const int32_t* __restrict__ idx,
                                                      int32_t c, const int32_t* __restrict__ own,
                                                      const int32_t* __restrict__ nei, const float* __restrict__ h,
                                                      const Load& load, int d) {
    int32_t b = off[c], e = off[c + 1];
    if (e == b) return 0.0f;
    float w = 1.0f / (float)(e - b);
    float s = 0.0f;
    for (int32_t k = b; k < e; ++k) {
        int32_t f = idx[k];
        int32_t o = own[f], n = nei[f];
        float t = dt_face_avg(load(d, o), load(d, n), h[o], h[n]) * w;
        s = (k == b) ? t : s + t;
    }
    return s;
}

struct GradDims {
    DimData d[IBH_MAXD];
    const float* h[IBH_MAXD];
    const int32_t* side;
};

inline GradDims grad_dims(const ibh_part* p) {
    GradDims G;
    for (int d = 0; d < p->nd; ++d) {
        G.d[d] = p->dim[d];
        G.h[d] = p->spacing + (int64_t)d * p->nc;
    }
    G.side = p->side;
    return G;
}

// Loaders: load(d, c) = the field value of cell c in dimension d.  ArrayLoad reads an (nc, nd) array (the advection script's
// C); AcousticLoad computes |u_d| + a from the primitives P = [p T u v (w)] on the fly -- abs(u_d) + sqrt(gamma R max(T, 10)),
// the arithmetic of k_pointwise mode 0 (ibh_cfd.hip) and of the IEEE broadcasts abs and + --, so that no (nc, nd) array of
// wave speeds is ever written (ibh_timestep_euler).
struct ArrayLoad {
    const float* __restrict__ C;
    int64_t ldc;
    __device__ __forceinline__ float operator()(int d, int64_t c) const { return (C + (int64_t)d * ldc)[c]; }
};
struct AcousticLoad {
    const float* __restrict__ P;
    int64_t ldp;
    float Rgas, gamma;
    __device__ __forceinline__ float operator()(int d, int64_t c) const {
        return fabsf(P[(int64_t)(2 + d) * ldp + c]) + sqrtf(gamma * Rgas * ibh_max(P[ldp + c], 10.0f));
    }
};

// (device bodies with the workgroup's index and count as arguments: the same code runs as its own launch and beside the
// BC-set workgroups of a march step, k_bcinterp_dt / k_bcscatter_dt of ibh_timestep.hip)
// CELLS: the local time step of every cell, (0.5 / max_d(...)[c]) * scale, goes to dt_cells as well
template <int ND, bool TILED, class Load, bool CELLS = false>
__device__ __forceinline__ void dt_partial_wg(int wg, int nwg, int32_t nc, const GradDims& G, const Load& load,
                                              float* __restrict__ partial, float scale = 1.0f,
                                              float* __restrict__ dt_cells = nullptr) {
    // Julia's maximum has no floor at zero: the maximum starts below every value (an all-negative C gives a negative dt).
    // fmaxf stays -- it drops a NaN where Julia's max keeps it; ibh_max here cost the march 6.5 %
    float m = -INFINITY;
#ifdef IBH_NO_XCD_CELLS
    const int64_t first = wg;
#else
    const int64_t first = ibh_xcd_chunk(wg, nwg);
#endif
    for (int64_t c = first * (int64_t)blockDim.x + threadIdx.x; c < nc; c += (int64_t)nwg * blockDim.x) {
        int32_t sd[2 * ND];
#pragma unroll
        for (int s = 0; s < 2 * ND; ++s) {
            if (TILED) {
                const int pos = ((int)c >> (3 * (s >> 1))) & 7, st = 1 << (3 * (s >> 1));
                const bool inb = (s & 1) ? pos < 7 : pos > 0;
                sd[s] = inb ? (int32_t)c + ((s & 1) ? st : -st) : G.side[(int64_t)s * nc + c];
            } else sd[s] = G.side[(int64_t)s * nc + c];
        }
        float mc = -INFINITY;
#pragma unroll
        for (int d = 0; d < ND; ++d) {
            const float hc = G.h[d][c], uc = load(d, c);
            const int32_t l = sd[2 * d], r = sd[2 * d + 1];
            float ar, al;
            if (r >= 0) ar = dt_face_avg(uc, load(d, r), hc, G.h[d][r]) * 1.0f;
            else if (r == -2) ar = 0.0f;
            else ar = dt_csr_mean_face_avg(G.d[d].roff, G.d[d].ridx, (int32_t)c, G.d[d].owners, G.d[d].neighbors, G.h[d], load, d);
            if (l >= 0) al = dt_face_avg(load(d, l), uc, G.h[d][l], hc) * 1.0f;
            else if (l == -2) al = 0.0f;
            else al = dt_csr_mean_face_avg(G.d[d].loff, G.d[d].lidx, (int32_t)c, G.d[d].owners, G.d[d].neighbors, G.h[d], load, d);
            const float g = (ar + al) / hc;
            m = fmaxf(m, g);
            if constexpr (CELLS) mc = fmaxf(mc, g);
        }
        if constexpr (CELLS) dt_cells[c] = (0.5f / mc) * scale;  // (the expression of dt_final_wg, per cell)
    }
    m = ibh_red::wg_reduce<DT_BLOCK, ibh_red::FMax>(m);
    if (threadIdx.x == 0) partial[wg] = m;
}
__device__ __forceinline__ void dt_final_wg(int n, const float* __restrict__ partial, float scale, float* __restrict__ dt) {
    const float b = ibh_red::wg_reduce_partials<DT_BLOCK, ibh_red::FMax>(n, partial);
    if (threadIdx.x == 0) *dt = (0.5f / b) * scale;  // advection.jl:53 and :65
}

}  // namespace dt_dev

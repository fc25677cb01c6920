// libibhip: device bodies of the thread-per-cell gradient on face-list partitions -- the expressions of the tuple
// cell_gradient (k_cell_gradient, k_cell_gradient_all: ibh_ops.hip), shared with the face-list forms of the fused closures
// (the *_cells kernels of ibh_turb.hip), whose gradients never leave the registers.  Float32, the reference's operation
// order (-ffp-contract=off): bit for bit the operator kernels.
#pragma once
#include "ibh_common.h"
#include "ibh_dt_dev.h"

namespace grad_dev {

using dt_dev::GradDims;

__device__ __forceinline__ float face_avg(float uo, float un, float ho, float hn) {
    // at_faces (:907-909): (u_o*h_n + u_n*h_o)/(h_n + h_o)
    return (uo * hn + un * ho) / (hn + ho);
}

// cell_gradient = green_gauss(at_faces(u)) without materialising the face field (:965-972): mean over a CSR row, the walk of
// csr_mean (ibh_ops.hip) with the face value made on the way
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

// the 2 ND entries of cell c in the side table of the partition (ibh_common.h)
template <int ND>
__device__ __forceinline__ void cell_sides(const GradDims& G, int32_t nc, int64_t c, int32_t (&sd)[2 * ND]) {
#pragma unroll
    for (int s = 0; s < 2 * ND; ++s) sd[s] = G.side[(int64_t)s * nc + c];
}

// gradient of one field at cell c in every dimension.  Sides with ONE face are evaluated directly from the cell across --
// the same expression the CSR walk evaluates for its single entry (weight 1.0f) -- the others walk the lists.
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

// the way out of the table g[i][j] = d u_i / d x_j when the gradients are asked for (column ND j + i: the tuple
// cell_gradient's layout)
template <int ND>
__device__ __forceinline__ void store_gradients(const float (&g)[ND][ND], float* __restrict__ Gout, int64_t ldg, int64_t c) {
#pragma unroll
    for (int i = 0; i < ND; ++i)
#pragma unroll
        for (int j = 0; j < ND; ++j) Gout[(int64_t)(ND * j + i) * ldg + c] = g[i][j];
}

}  // namespace grad_dev

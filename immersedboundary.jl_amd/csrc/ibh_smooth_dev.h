// libibhip: one Jacobi iteration of implicit residual smoothing for ONE cell,
//     S_i = (R_i + eps * sum_{f in F(i)} Sprev_{across(f, i)}) / (1 + eps * float(n_i)),
// Jacobi on (I + eps L) S = R with L the unweighted Laplacian of the face graph.  F(i): dimensions ascending, in a dimension the
// left faces (the cell across is the face's owner) in CSR order, then the right faces (its neighbour); n_i = |F(i)|.  The sum
// starts from its first term and adds in that order; every product, sum and the divide is rounded on its own (contract(off),
// IEEE divide), so a numpy model that walks the same lists gives the same bits (tests/smooth_model.py).  smooth_row is the
// only place the formula exists: the body of k_smooth_residual and, in front of euler_step::update_row / blend_row, of
// k_update_euler_smoothed (ibh_smooth.hip).  The library's own operator: the reference has none.
#pragma once
#include "ibh_common.h"

namespace smooth {

// the face lists of a partition and its side table (ibh_part::side: the cell across a one-face side, -2 no face, -1 walk)
struct Faces {
    DimData d[IBH_MAXD];
    const int32_t* side;
};

inline Faces faces(const ibh_part* p) {
    Faces G;
    for (int d = 0; d < p->nd; ++d) G.d[d] = p->dim[d];
    G.side = p->side;
    return G;
}

// one iteration for cell c: r = the row of R, out = the row of S, Sprev (leading dimension lds) the previous iterate that
// the cells across are gathered from.  The 2 ND side-table entries are read once and serve all NV variables; an entry >= 0 is
// the cell across the side's one face, -2 contributes nothing, -1 walks the CSR list of that side.  A cell without faces
// (n = 0) gets r + eps * 0
template <int ND, int NV>
__device__ __forceinline__ void smooth_row(const Faces& G, int32_t nc, int32_t c, const float (&r)[NV],
                                           const float* __restrict__ Sprev, int64_t lds, float eps, float (&out)[NV]) {
#pragma clang fp contract(off)
    int32_t sd[2 * ND];
#pragma unroll
    for (int s = 0; s < 2 * ND; ++s) sd[s] = G.side[(int64_t)s * nc + c];
    float acc[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[v] = 0.0f;
    int n = 0;
#pragma unroll
    for (int s = 0; s < 2 * ND; ++s) {
        const int32_t t = sd[s];
        if (t >= 0) {
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                const float x = Sprev[t + v * lds];
                acc[v] = n == 0 ? x : acc[v] + x;
            }
            ++n;
        } else if (t != -2) {
            const DimData& D = G.d[s >> 1];
            const int32_t* __restrict__ off = (s & 1) ? D.roff : D.loff;
            const int32_t* __restrict__ idx = (s & 1) ? D.ridx : D.lidx;
            const int32_t* __restrict__ across = (s & 1) ? D.neighbors : D.owners;
            for (int32_t k = off[c], e = off[c + 1]; k < e; ++k) {
                const int32_t o = across[idx[k]];
#pragma unroll
                for (int v = 0; v < NV; ++v) {
                    const float x = Sprev[o + v * lds];
                    acc[v] = n == 0 ? x : acc[v] + x;
                }
                ++n;
            }
        }
    }
    const float den = 1.0f + eps * (float)n;
#pragma unroll
    for (int v = 0; v < NV; ++v) out[v] = (r[v] + eps * acc[v]) / den;
}

}  // namespace smooth

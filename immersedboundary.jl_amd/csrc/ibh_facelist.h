// libibhip: the face-list bodies of the two-kernel sweeps, and the literal (IEEE) form of the 2-D block bodies.
//   pass A  per cell : Green-Gauss gradients of every variable along every dim + JST sensor
//                      (cell_gradient :965, JST_sensor :1077)          -> workspace G
//   pass B  per cell : for each face of the cell MUSCL(high_order) states, flux, and the
//                      Green-Gauss sum of the fluxes (MUSCL :1113, green_gauss :918)
// *_cell walk the CSR left / right face lists of a cell, *_flat the flattened stencil records, *_block2 take an 8x8 block per
// wavefront with the arithmetic of the face-list bodies (IBH_EXACT).  All call the same per-face functions (ibh_flux.h) in
// the same order, so they agree bit for bit with each other and with the oracle's array-at-a-time evaluation.  The kernels
// that call them: ibh_fused_general.hip (every cell, or the cells outside blocks) and the two-kernel 3-D block kernels of
// ibh_fused3d.hip (the cells outside blocks ride in the same launch).
#pragma once
#include "ibh_common.h"
#include "ibh_flux.h"

namespace {

// Kernel parameters.  (In the unnamed namespace like the kernels that take them: a kernel's symbol names its parameter types.)
struct PartView {
    int32_t nc;
    const float* spacing;
    DimData dim[IBH_MAXD];
    const int32_t* side;  // side table (ibh_common.h): the cell across the one face of a side, -2 none, -1 walk the lists
};

// flattened stencil records of the face-list cells (ibh_part::irr_rec), or rec == null
struct FlatRec {
    const int32_t* rec;
    int32_t n;
};

}  // namespace

namespace flist {

using namespace ibhf;

// The faces of cell c on one side of dimension d.  A side with ONE face is taken from the side table -- the cell across,
// no offsets / face ids / owner and neighbour lookups (four dependent loads become one) -- with the weight 1.0f / 1 the
// walk would use; anything else walks the CSR lists.  Same faces, same order, same arithmetic.
struct SideIter {
    int32_t b, e, o, n;
    const int32_t* idx;
    bool direct;
};
__device__ __forceinline__ SideIter side_iter(const PartView& p, int d, int side, int32_t c) {
    const DimData& dd = p.dim[d];
    SideIter it;
    it.idx = side ? dd.ridx : dd.lidx;
    const int32_t t = p.side[(int64_t)(2 * d + side) * p.nc + c];
    it.direct = t >= 0;
    it.o = side ? c : t;
    it.n = side ? t : c;
    if (t >= 0) {
        it.b = 0;
        it.e = 1;
    } else if (t == -2) {
        it.b = it.e = 0;
    } else {
        const int32_t* off = side ? dd.roff : dd.loff;
        it.b = off[c];
        it.e = off[c + 1];
    }
    return it;
}
__device__ __forceinline__ void side_face(const DimData& dd, const SideIter& it, int32_t k, int32_t& o, int32_t& n) {
    if (it.direct) {
        o = it.o;
        n = it.n;
    } else {
        const int32_t f = it.idx[k];
        o = dd.owners[f];
        n = dd.neighbors[f];
    }
}

// ------------------------------------------------------------------------------------------
// face-list bodies
// ------------------------------------------------------------------------------------------
// G layout: gradient of variable v along dim d at G[(d*NV + v)*nc + c]; sensor at G[ND*NV*nc + c].
template <int ND, int NV>
__device__ __forceinline__ void passA_cell(const PartView& p, const float* __restrict__ u, int64_t ldu,
                                           float* __restrict__ G, int32_t c) {
    const int64_t nc = p.nc;
    float D = 1e-7f;
    float uc[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) uc[v] = u[c + v * ldu];
#pragma unroll
    for (int d = 0; d < ND; ++d) {
        const DimData& dd = p.dim[d];
        const float* h = p.spacing + d * nc;
        float hc = h[c];
        float s2[2][NV];
        float ds[2] = {0.f, 0.f}, as[2] = {0.f, 0.f};
#pragma unroll
        for (int side = 1; side >= 0; --side) {   // right faces, then left faces
            float* s = s2[side];
#pragma unroll
            for (int v = 0; v < NV; ++v) s[v] = 0.f;
            const SideIter it = side_iter(p, d, side, c);
            if (it.direct) {
                // one face: own values from registers, the cell across gathered (weight 1.0f / 1)
                const int32_t x = side ? it.n : it.o;
                const float hx = h[x];
#pragma unroll
                for (int v = 0; v < NV; ++v) {
                    const float ux = u[x + v * ldu];
                    const float uo = side ? uc[v] : ux, un = side ? ux : uc[v];
                    s[v] = face_avg(uo, un, side ? hc : hx, side ? hx : hc) * 1.0f;
                    if (v == 0) {
                        const float df = un - uo;
                        ds[side] = df * 1.0f;
                        as[side] = fabsf(df) * 1.0f;
                    }
                }
                continue;
            }
            const int32_t b = it.b, e = it.e;
            float w = (e > b) ? 1.0f / (float)(e - b) : 0.f;
            for (int32_t k = b; k < e; ++k) {
                int32_t o, n;
                side_face(dd, it, k, o, n);
                float ho = h[o], hn = h[n];
#pragma unroll
                for (int v = 0; v < NV; ++v) {
                    float uo = u[o + v * ldu], un = u[n + v * ldu];
                    float t = face_avg(uo, un, ho, hn) * w;
                    s[v] = (k == b) ? t : s[v] + t;
                    if (v == 0) {
                        float df = un - uo;
                        float td = df * w, ta = fabsf(df) * w;
                        ds[side] = (k == b) ? td : ds[side] + td;
                        as[side] = (k == b) ? ta : as[side] + ta;
                    }
                }
            }
        }
#pragma unroll
        for (int v = 0; v < NV; ++v) G[(int64_t)(d * NV + v) * nc + c] = (s2[1][v] - s2[0][v]) / hc;
        float gg = (ds[1] - ds[0]) / hc;
        float ugg = (as[1] + as[0]) / hc;
        D = fmaxf(D, (1e-7f + fabsf(gg)) / (1e-7f + ugg));
    }
    G[(int64_t)(ND * NV) * nc + c] = D;
}

template <int ND>
__device__ __forceinline__ void passB_adv_cell(const PartView& p, const float* __restrict__ u,
                                               const float* __restrict__ C, int64_t ldc, const float* __restrict__ G,
                                               float* __restrict__ ud, int32_t c) {
    const int64_t nc = p.nc;
    const float* Ds = G + (int64_t)ND * nc;
    float r = 0.0f;
#pragma unroll
    for (int d = 0; d < ND; ++d) {
        const DimData& dd = p.dim[d];
        const float* h = p.spacing + d * nc;
        const float* g = G + (int64_t)d * nc;
        const float* Cd = C + (int64_t)d * ldc;
        float fr = 0.f, fl = 0.f;
        {
            const SideIter it = side_iter(p, d, 1, c);
            const int32_t b = it.b, e = it.e;
            float w = (e > b) ? 1.0f / (float)(e - b) : 0.f;
            for (int32_t k = b; k < e; ++k) {
                int32_t o, n;
                side_face(dd, it, k, o, n);
                float t = adv_flux(u[o], u[n], g[o], g[n], Ds[o], Ds[n], Cd[o], Cd[n], h[o], h[n]) * w;
                fr = (k == b) ? t : fr + t;
            }
        }
        {
            const SideIter it = side_iter(p, d, 0, c);
            const int32_t b = it.b, e = it.e;
            float w = (e > b) ? 1.0f / (float)(e - b) : 0.f;
            for (int32_t k = b; k < e; ++k) {
                int32_t o, n;
                side_face(dd, it, k, o, n);
                float t = adv_flux(u[o], u[n], g[o], g[n], Ds[o], Ds[n], Cd[o], Cd[n], h[o], h[n]) * w;
                fl = (k == b) ? t : fl + t;
            }
        }
        r = r - (fr - fl) / h[c];
    }
    ud[c] = r;
}

// EULER_SENSOR: nu per face from `nu` (nc values), or from the sensor column of the workspace when `nu` is null
template <int ND, int SCH = EULER_HLL>
__device__ __forceinline__ void passB_euler_cell(const PartView& p, const float* __restrict__ P, int64_t ldp,
                                                 const float* __restrict__ G, float* __restrict__ Rr, int64_t ldr,
                                                 float Rgas, float gamma, int32_t c, const float* __restrict__ nu = nullptr) {
    constexpr int NV = ND + 2;
    typedef typename flux_of<SCH>::type FT;
    const int64_t nc = p.nc;
    const float* Ds = G + (int64_t)(ND * NV) * nc;
    const float* Nu = SCH == EULER_SENSOR && nu ? nu : Ds;
    float res[NV], Pc[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        res[v] = 0.0f;
        Pc[v] = P[c + v * ldp];
    }
    const float Dc = Ds[c];
    float Nc = 0.0f;
    if constexpr (SCH == EULER_SENSOR) Nc = Nu[c];
#pragma unroll
    for (int d = 0; d < ND; ++d) {
        const DimData& dd = p.dim[d];
        const float* h = p.spacing + d * nc;
        FT fr[NV], fl[NV];
        float dPc[NV];
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            fr[v] = fl[v] = 0;
            dPc[v] = G[(int64_t)(d * NV + v) * nc + c];
        }
        const float hcf = h[c];
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            FT* acc = side ? fr : fl;
            const SideIter it = side_iter(p, d, side, c);
            if (it.direct) {
                // one face: the cell's own values are in registers, only the cell across is gathered (weight 1.0f / 1)
                const int32_t x = side ? it.n : it.o;
                float Px[NV], dPx[NV];
#pragma unroll
                for (int v = 0; v < NV; ++v) {
                    Px[v] = P[x + v * ldp];
                    dPx[v] = G[(int64_t)(d * NV + v) * nc + x];
                }
                const float Dx = Ds[x], hx = h[x];
                float Nx = 0.0f;
                if constexpr (SCH == EULER_SENSOR) Nx = Nu[x];
                FT F[NV];
                if (side) euler_face_flux<ND, SCH>(Pc, Px, dPc, dPx, Dc, Dx, hcf, hx, d, Rgas, gamma, F, Nc, Nx);
                else euler_face_flux<ND, SCH>(Px, Pc, dPx, dPc, Dx, Dc, hx, hcf, d, Rgas, gamma, F, Nx, Nc);
#pragma unroll
                for (int v = 0; v < NV; ++v) acc[v] = F[v] * (FT)1.0f;
                continue;
            }
            const int32_t b = it.b, e = it.e;
            float w = (e > b) ? 1.0f / (float)(e - b) : 0.f;
            for (int32_t k = b; k < e; ++k) {
                int32_t o, n;
                side_face(dd, it, k, o, n);
                float Po[NV], Pn[NV], dPo[NV], dPn[NV];
#pragma unroll
                for (int v = 0; v < NV; ++v) {
                    Po[v] = P[o + v * ldp];
                    Pn[v] = P[n + v * ldp];
                    dPo[v] = G[(int64_t)(d * NV + v) * nc + o];
                    dPn[v] = G[(int64_t)(d * NV + v) * nc + n];
                }
                float No = 0.0f, Nn = 0.0f;
                if constexpr (SCH == EULER_SENSOR) {
                    No = Nu[o];
                    Nn = Nu[n];
                }
                FT F[NV];
                euler_face_flux<ND, SCH>(Po, Pn, dPo, dPn, Ds[o], Ds[n], h[o], h[n], d, Rgas, gamma, F, No, Nn);
#pragma unroll
                for (int v = 0; v < NV; ++v) {
                    FT t = F[v] * (FT)w;
                    acc[v] = (k == b) ? t : acc[v] + t;
                }
            }
        }
        FT hc = (FT)hcf;
#pragma unroll
        for (int v = 0; v < NV; ++v) res[v] = (float)((FT)res[v] - (fr[v] - fl[v]) / hc);
    }
#pragma unroll
    for (int v = 0; v < NV; ++v) Rr[c + v * ldr] = res[v];
}

// ------------------------------------------------------------------------------------------
// face-list bodies over flattened stencil records (same arithmetic and summation order as the CSR
// walk above, two dependent memory trips instead of four)
// ------------------------------------------------------------------------------------------
template <int ND, int NV>
__device__ __forceinline__ void passA_flat(const PartView& p, const FlatRec& R, int32_t t, int32_t c,
                                           const float* __restrict__ u, int64_t ldu, float* __restrict__ G) {
    const int64_t nc = p.nc;
    float D = 1e-7f;
#pragma unroll
    for (int d = 0; d < ND; ++d) {
        const float* h = p.spacing + d * nc;
        const float hc = h[c];
        float s[2][NV], sd[2] = {0.f, 0.f}, sa[2] = {0.f, 0.f};
        float uc[NV];
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            uc[v] = u[c + v * ldu];
            s[0][v] = s[1][v] = 0.f;
        }
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            const int64_t q = 2 * d + side;
            const int cnt = R.rec[(q * 5) * R.n + t];
            const float w = cnt > 0 ? 1.0f / (float)cnt : 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (k < cnt) {
                    const int32_t o = R.rec[(q * 5 + 1 + k) * R.n + t];
                    const float ho = h[o];
#pragma unroll
                    for (int v = 0; v < NV; ++v) {
                        const float uo = u[o + v * ldu];
                        // side 1 (right face): owner = this cell, neighbour = o; side 0: owner = o
                        const float fa = side ? face_avg(uc[v], uo, hc, ho) : face_avg(uo, uc[v], ho, hc);
                        const float tt = fa * w;
                        s[side][v] = (k == 0) ? tt : s[side][v] + tt;
                        if (v == 0) {
                            const float df = side ? (uo - uc[v]) : (uc[v] - uo);
                            const float td = df * w, ta = fabsf(df) * w;
                            sd[side] = (k == 0) ? td : sd[side] + td;
                            sa[side] = (k == 0) ? ta : sa[side] + ta;
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int v = 0; v < NV; ++v) G[(int64_t)(d * NV + v) * nc + c] = (s[1][v] - s[0][v]) / hc;
        const float gg = (sd[1] - sd[0]) / hc;
        const float ugg = (sa[1] + sa[0]) / hc;
        D = fmaxf(D, (1e-7f + fabsf(gg)) / (1e-7f + ugg));
    }
    G[(int64_t)(ND * NV) * nc + c] = D;
}

template <int ND>
__device__ __forceinline__ void passB_adv_flat(const PartView& p, const FlatRec& R, int32_t t, int32_t c,
                                               const float* __restrict__ u, const float* __restrict__ C, int64_t ldc,
                                               const float* __restrict__ G, float* __restrict__ ud) {
    const int64_t nc = p.nc;
    const float* Ds = G + (int64_t)ND * nc;
    const float uc = u[c], Dc = Ds[c];
    float r = 0.0f;
#pragma unroll
    for (int d = 0; d < ND; ++d) {
        const float* h = p.spacing + d * nc;
        const float* g = G + (int64_t)d * nc;
        const float* Cd = C + (int64_t)d * ldc;
        const float hc = h[c], gc = g[c], Cc = Cd[c];
        float fs[2] = {0.f, 0.f};
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            const int64_t q = 2 * d + side;
            const int cnt = R.rec[(q * 5) * R.n + t];
            const float w = cnt > 0 ? 1.0f / (float)cnt : 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (k < cnt) {
                    const int32_t o = R.rec[(q * 5 + 1 + k) * R.n + t];
                    const float fl = side ? adv_flux(uc, u[o], gc, g[o], Dc, Ds[o], Cc, Cd[o], hc, h[o])
                                          : adv_flux(u[o], uc, g[o], gc, Ds[o], Dc, Cd[o], Cc, h[o], hc);
                    const float tt = fl * w;
                    fs[side] = (k == 0) ? tt : fs[side] + tt;
                }
            }
        }
        r = r - (fs[1] - fs[0]) / hc;
    }
    ud[c] = r;
}

// ------------------------------------------------------------------------------------------
// block fast path, 2-D, 8x8 blocks.  LDS per wave and per field: tile[64] + halo[4][8][2].
// halo slot (s, t, k): side s, boundary cell t along the side, k-th face (k = 1 only on FINE sides)
// ------------------------------------------------------------------------------------------

// Fetch the neighbour across direction s (0:x- 1:x+ 2:y- 3:y+) of the field staged in `tile`/`halo`.
__device__ __forceinline__ void nb_fetch(const float* tile, const float* halo, int lane, int i, int j, int s, float self,
                                         float& v0, float& v1) {
    bool edge = (s == 0) ? (i == 0) : (s == 1) ? (i == 7) : (s == 2) ? (j == 0) : (j == 7);
    int t = (s < 2) ? j : i;
    if (!edge) {
        int off = (s == 0) ? -1 : (s == 1) ? 1 : (s == 2) ? -8 : 8;
        v0 = tile[lane + off];
        v1 = v0;
    } else {
        v0 = halo[(s * 8 + t) * 2];
        v1 = halo[(s * 8 + t) * 2 + 1];
    }
    (void)self;
}

// Stage one field: tile[lane] = own value, halo slots gathered by lanes 0..63 (slot = lane).
// MIRROR sides take the boundary cell's own value (o == n faces, ImmersedBoundary.jl:653-660).
__device__ __forceinline__ float stage_field(const float* __restrict__ f, const BlockDesc2& b, int lane, float* tile,
                                             float* halo, int32_t hc_idx, int32_t mirror_idx) {
    float self = f[b.base + lane];
    tile[lane] = self;
    float hv = 0.0f;
    if (hc_idx >= 0) hv = f[hc_idx];
    else if (mirror_idx >= 0) hv = f[mirror_idx];
    halo[lane] = hv;
    return self;
}

// lane -> halo slot (s, t, k) = lane; its cell comes from the per-block table built by ibh_analyze.cpp
// (single-face sides repeat sub-face 0 in slot k=1, MIRROR sides name the boundary cell itself).
__device__ __forceinline__ void lane_halo_role(const int32_t* __restrict__ htab, int32_t blk, int lane,
                                               int32_t& hc_idx, int32_t& mirror_idx) {
    hc_idx = htab[(size_t)blk * 64 + lane];
    mirror_idx = -1;
}

template <int NV>
__device__ __forceinline__ void passA_block2(const BlockDesc2* __restrict__ blocks, const int32_t* __restrict__ htab,
                                             int32_t blk, const float* spacing,
                                             int64_t nc, const float* __restrict__ u, int64_t ldu, float* __restrict__ G,
                                             float* lds, int lane) {
    const BlockDesc2& b = blocks[blk];
    const int i = lane & 7, j = lane >> 3;
    int32_t hc_idx, mirror_idx;
    lane_halo_role(htab, blk, lane, hc_idx, mirror_idx);
    float* tile = lds;         // [NV][64]
    float* halo = lds + NV * 64;  // [NV][64]
    float self[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) self[v] = stage_field(u + v * ldu, b, lane, tile + v * 64, halo + v * 64, hc_idx, mirror_idx);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

    const int32_t c = b.base + lane;
    float D = 1e-7f;
    const bool general = (i == 0 && b.type[0] == SIDE_GENERAL) || (i == 7 && b.type[1] == SIDE_GENERAL) ||
                         (j == 0 && b.type[2] == SIDE_GENERAL) || (j == 7 && b.type[3] == SIDE_GENERAL);
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        const float hc = b.h[d];
        const int sL = 2 * d, sR = 2 * d + 1;
        const bool edgeL = d == 0 ? (i == 0) : (j == 0);
        const bool edgeR = d == 0 ? (i == 7) : (j == 7);
        const int tyL = b.type[sL], tyR = b.type[sR];
        // neighbour spacing: same inside the block; 2h / h/2 across a 2:1 side (exact: powers of two
        // times h would also be exact, but take the stored value to stay literal)
        float hL = hc, hR = hc;
        bool twoL = false, twoR = false;
        if (edgeL) { hL = (tyL == SIDE_COARSE) ? hc * 2.0f : (tyL == SIDE_FINE) ? hc * 0.5f : hc; twoL = tyL == SIDE_FINE; }
        if (edgeR) { hR = (tyR == SIDE_COARSE) ? hc * 2.0f : (tyR == SIDE_FINE) ? hc * 0.5f : hc; twoR = tyR == SIDE_FINE; }
        float sr[NV], sl[NV], dr = 0.f, ar = 0.f, dl = 0.f, al = 0.f;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            float l0, l1, r0, r1;
            nb_fetch(tile + v * 64, halo + v * 64, lane, i, j, sL, self[v], l0, l1);
            nb_fetch(tile + v * 64, halo + v * 64, lane, i, j, sR, self[v], r0, r1);
            // right faces: owner = this cell; left faces: neighbour = this cell
            float fr0 = face_avg(self[v], r0, hc, hR);
            float fl0 = face_avg(l0, self[v], hL, hc);
            float wr = twoR ? 0.5f : 1.0f, wl = twoL ? 0.5f : 1.0f;
            float a = fr0 * wr;
            if (twoR) a = a + face_avg(self[v], r1, hc, hR) * wr;
            float bb = fl0 * wl;
            if (twoL) bb = bb + face_avg(l1, self[v], hL, hc) * wl;
            sr[v] = a;
            sl[v] = bb;
            if (v == 0) {
                float d0 = r0 - self[v];
                dr = d0 * wr;
                ar = fabsf(d0) * wr;
                if (twoR) { float d1 = r1 - self[v]; dr = dr + d1 * wr; ar = ar + fabsf(d1) * wr; }
                float e0 = self[v] - l0;
                dl = e0 * wl;
                al = fabsf(e0) * wl;
                if (twoL) { float e1 = self[v] - l1; dl = dl + e1 * wl; al = al + fabsf(e1) * wl; }
            }
        }
        if (!general) {
#pragma unroll
            for (int v = 0; v < NV; ++v) G[(int64_t)(d * NV + v) * nc + c] = (sr[v] - sl[v]) / hc;
        }
        float gg = (dr - dl) / hc;
        float ugg = (ar + al) / hc;
        D = fmaxf(D, (1e-7f + fabsf(gg)) / (1e-7f + ugg));
    }
    if (!general) G[(int64_t)(2 * NV) * nc + c] = D;
    (void)spacing;
}

__device__ __forceinline__ void passB_adv_block2(const BlockDesc2* __restrict__ blocks,
                                                 const int32_t* __restrict__ htab, int32_t blk, int64_t nc,
                                                 const float* __restrict__ u, const float* __restrict__ C, int64_t ldc,
                                                 const float* __restrict__ G, float* __restrict__ ud, float* lds,
                                                 int lane) {
    const BlockDesc2& b = blocks[blk];
    const int i = lane & 7, j = lane >> 3;
    int32_t hc_idx, mirror_idx;
    lane_halo_role(htab, blk, lane, hc_idx, mirror_idx);
    // fields: 0:u 1:D 2:gx 3:gy 4:Cx 5:Cy   (halo of gx/Cx only meaningful on x sides, gy/Cy on y sides;
    // every slot is gathered anyway: one instruction per field)
    float* tile = lds;
    float* halo = lds + 6 * 64;
    const float* fld[6] = {u, G + 2 * nc, G, G + nc, C, C + ldc};
    float self[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) self[q] = stage_field(fld[q], b, lane, tile + q * 64, halo + q * 64, hc_idx, mirror_idx);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

    const int32_t c = b.base + lane;
    float r = 0.0f;
    const bool general = (i == 0 && b.type[0] == SIDE_GENERAL) || (i == 7 && b.type[1] == SIDE_GENERAL) ||
                         (j == 0 && b.type[2] == SIDE_GENERAL) || (j == 7 && b.type[3] == SIDE_GENERAL);
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        const float hc = b.h[d];
        const int sL = 2 * d, sR = 2 * d + 1;
        const bool edgeL = d == 0 ? (i == 0) : (j == 0);
        const bool edgeR = d == 0 ? (i == 7) : (j == 7);
        const int tyL = b.type[sL], tyR = b.type[sR];
        float hL = hc, hR = hc;
        bool twoL = false, twoR = false;
        if (edgeL) { hL = (tyL == SIDE_COARSE) ? hc * 2.0f : (tyL == SIDE_FINE) ? hc * 0.5f : hc; twoL = tyL == SIDE_FINE; }
        if (edgeR) { hR = (tyR == SIDE_COARSE) ? hc * 2.0f : (tyR == SIDE_FINE) ? hc * 0.5f : hc; twoR = tyR == SIDE_FINE; }
        const int qg = 2 + d, qc = 4 + d;
        float uL0, uL1, uR0, uR1, gL0, gL1, gR0, gR1, DL0, DL1, DR0, DR1, CL0, CL1, CR0, CR1;
        nb_fetch(tile, halo, lane, i, j, sL, self[0], uL0, uL1);
        nb_fetch(tile, halo, lane, i, j, sR, self[0], uR0, uR1);
        nb_fetch(tile + 64, halo + 64, lane, i, j, sL, self[1], DL0, DL1);
        nb_fetch(tile + 64, halo + 64, lane, i, j, sR, self[1], DR0, DR1);
        nb_fetch(tile + qg * 64, halo + qg * 64, lane, i, j, sL, self[qg], gL0, gL1);
        nb_fetch(tile + qg * 64, halo + qg * 64, lane, i, j, sR, self[qg], gR0, gR1);
        nb_fetch(tile + qc * 64, halo + qc * 64, lane, i, j, sL, self[qc], CL0, CL1);
        nb_fetch(tile + qc * 64, halo + qc * 64, lane, i, j, sR, self[qc], CR0, CR1);
        float wr = twoR ? 0.5f : 1.0f, wl = twoL ? 0.5f : 1.0f;
        float fr = adv_flux(self[0], uR0, self[qg], gR0, self[1], DR0, self[qc], CR0, hc, hR) * wr;
        if (twoR) fr = fr + adv_flux(self[0], uR1, self[qg], gR1, self[1], DR1, self[qc], CR1, hc, hR) * wr;
        float fl = adv_flux(uL0, self[0], gL0, self[qg], DL0, self[1], CL0, self[qc], hL, hc) * wl;
        if (twoL) fl = fl + adv_flux(uL1, self[0], gL1, self[qg], DL1, self[1], CL1, self[qc], hL, hc) * wl;
        r = r - (fr - fl) / hc;
    }
    if (!general) ud[c] = r;
}

// ---- host side
inline PartView view(const ibh_part* p) { return {p->nc, p->spacing, {p->dim[0], p->dim[1], p->dim[2]}, p->side}; }
// flattened records apply only when a launch walks exactly the partition's face-list cell list
inline FlatRec flat_of(const ibh_part* p, const int32_t* cells) {
    return cells && cells == p->irr_cells && p->irr_rec ? FlatRec{p->irr_rec, p->n_irr} : FlatRec{nullptr, 0};
}

}  // namespace flist

// Wave-per-block frame of the 3-D kernels ("plane marching"): ONE wavefront per 8x8x8 block, lane = (i, j), the eight
// z-planes of the block handled in turn.  Each lane keeps its whole z-column in registers; x/y neighbours go through
// wave-private LDS (no workgroup barrier anywhere), z neighbours are the registers of the planes above and below.  All
// loads of a block -- the eight own values and the six halo slots of every lane -- are issued up front: one memory trip.
// The halo slots are reduced by the lanes that load them to (mean value, mean |difference to the boundary cell|), so
// a side facing finer blocks (four cells per slot) costs the consumers nothing.
// Holds: the halo ids of a lane's six slots (halo_cell3s, halo_ids), the gas constants of the 3-D Euler sweeps (Gas3) and
// the ONE gradient sweep of a block (wave_gradient_pass) behind pass A of the two-kernel sweeps (ibh_fused3d.hip), the
// tuple cell_gradient and the closures that consume the gradients where they are made (ibh_turb.hip).
// (wave_gradients_written_out at the end is the one copy kept beside it, for one kernel; the reason stands there.)
// Contraction: the functions here are compiled with fp contract(fast), as the block kernels always were; the pragma is
// switched off again at the end of the file, and ibh_turb.hip's pointwise formulas after its include rely on that.
#pragma once
#include "ibh_block2d.h"

namespace blk3 {

#pragma clang fp contract(fast)

using blk2::ldg;
using blk2::stg;

struct Gas3 {
    float R, gamma;
};

// halo cell of boundary cell t of side S (compile-time) -- the arithmetic of halo_cell3 (ibh_block3d.h)
template <int S>
__device__ __forceinline__ uint32_t halo_cell3s(const BlockDesc3& bb, const int32_t* __restrict__ htab, int32_t blk,
                                                int t) {
    const int ty = bb.type[S];
    // wave-uniform: FINE sides, and sides whose neighbour block is not complete in this partition (nb < 0: a skirt
    // fragment, image-only sweeps) take the ids from the table
    if (ty == SIDE_FINE || ((ty == SIDE_SAME || ty == SIDE_COARSE) && bb.nb[S] < 0))
        return (uint32_t)htab[(size_t)blk * 384 + S * 64 + t];
    constexpr int d = S >> 1;
    constexpr bool low = (S & 1) == 0;
    constexpr int sd = d == 0 ? 1 : d == 1 ? 8 : 64;
    constexpr int sa = d == 0 ? 8 : 1;
    constexpr int sb = d == 2 ? 8 : 64;
    int t1 = t & 7, t2 = t >> 3;
    int n, base;
    if (ty == SIDE_SAME) {
        n = low ? 7 : 0;
        base = bb.nb[S];
    } else if (ty == SIDE_COARSE) {
        n = low ? 7 : 0;
        base = bb.nb[S];
        t1 = 4 * (bb.sub[S] & 1) + (t1 >> 1);
        t2 = 4 * (bb.sub[S] >> 1) + (t2 >> 1);
    } else {
        n = low ? 0 : 7;
        base = bb.base;
    }
    return (uint32_t)(base + n * sd + t1 * sa + t2 * sb);
}

// this lane loads slot t = lane of every side
__device__ __forceinline__ void halo_ids(const BlockDesc3& bb, const int32_t* __restrict__ htab, int32_t blk, int lane,
                                         uint32_t (&hid)[6]) {
    hid[0] = halo_cell3s<0>(bb, htab, blk, lane);
    hid[1] = halo_cell3s<1>(bb, htab, blk, lane);
    hid[2] = halo_cell3s<2>(bb, htab, blk, lane);
    hid[3] = halo_cell3s<3>(bb, htab, blk, lane);
    hid[4] = halo_cell3s<4>(bb, htab, blk, lane);
    hid[5] = halo_cell3s<5>(bb, htab, blk, lane);
}

// LDS per wave: tile 512 | Hm 6x64 | Ha 6x64 = 1280 floats
#define BLK3W_PASSA_LDS (512 + 384 + 384)

// Gradients of NV cell fields of one block, one field after the other through the same LDS region: field(v) is the
// v-th field's pointer, and sink(v, k, g, D, general) receives, for the lane's cell in plane k, the gradient g[3] of
// field v, its JST sensor D and whether the cell has a GENERAL side (its gradient belongs to the face-list body).
// SENSOR = false: no Ha, no |difference| and no sensor (D = 0) -- for the kernels that consume the gradients where they
// are made.  Order of the up-front loads: the six halo ids, then per field its eight cells and its six slots.
template <int NV, bool SENSOR, class Field, class Sink>
__device__ __forceinline__ void wave_gradient_pass(const BlockDesc3& bb, const int32_t* __restrict__ htab,
                                                   const int32_t* __restrict__ ftab, int32_t blk, Field field, float* lds,
                                                   int lane, Sink sink) {
    float* tile = lds;          // [k][lane]
    float* Hm = lds + 512;      // [side][t]: mean neighbour value across the side
    float* Ha = lds + 896;      // [side][t]: mean |neighbour - boundary cell|
    uint32_t hid[6];
    halo_ids(bb, htab, blk, lane, hid);
    const int i = lane & 7, j = lane >> 3;
    const bool e0 = i == 0, e1 = i == 7, e2 = j == 0, e3 = j == 7;
    const bool general = (e0 && bb.type[0] == SIDE_GENERAL) || (e1 && bb.type[1] == SIDE_GENERAL) ||
                         (e2 && bb.type[2] == SIDE_GENERAL) || (e3 && bb.type[3] == SIDE_GENERAL);
    const float q0 = e0 ? bb.q[0] : 0.5f, q1 = e1 ? bb.q[1] : 0.5f, q2 = e2 ? bb.q[2] : 0.5f, q3 = e3 ? bb.q[3] : 0.5f;
    float uka[NV][8], hva[NV][6];
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const float* u = field(v);
#pragma unroll
        for (int k = 0; k < 8; ++k) uka[v][k] = ldg(u, (uint32_t)bb.base + lane + 64 * k);
#pragma unroll
        for (int s = 0; s < 6; ++s) hva[v][s] = ldg(u, hid[s]);
    }
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const float* u = field(v);
        const float(&uk)[8] = uka[v];
        const float(&hv)[6] = hva[v];
        if (v) blk2::wave_lds_sync();  // the previous field's LDS reads are done
#pragma unroll
        for (int k = 0; k < 8; ++k) tile[k * 64 + lane] = uk[k];
        if constexpr (SENSOR) blk2::wave_lds_sync();
        // reduce every slot to (mean value, mean |difference|) against its boundary cell: slot t of side s belongs to
        // cell pos(s, t) = n*sd + t1*sa + t2*sb of the tile
#pragma unroll
        for (int s = 0; s < 6; ++s) {
            const int d = s >> 1;
            const bool low = (s & 1) == 0;
            const int sd = d == 0 ? 1 : d == 1 ? 8 : 64, sa = d == 0 ? 8 : 1, sb = d == 2 ? 8 : 64;
            const int pos = (low ? 0 : 7) * sd + (lane & 7) * sa + (lane >> 3) * sb;
            const float ub = SENSOR ? tile[pos] : 0.0f;  // (the mean needs no boundary cell)
            float vm = hv[s], am = fabsf(hv[s] - ub);
            if (bb.type[s] == SIDE_FINE) {  // wave-uniform: three more fine cells behind this slot
                const int32_t* ft = ftab + (((size_t)bb.fine * 6 + s) * 64 + lane) * 3;
                const float v1 = ldg(u, (uint32_t)ft[0]), v2 = ldg(u, (uint32_t)ft[1]), v3 = ldg(u, (uint32_t)ft[2]);
                vm = 0.25f * (hv[s] + v1 + v2 + v3);
                am = 0.25f * (fabsf(hv[s] - ub) + fabsf(v1 - ub) + fabsf(v2 - ub) + fabsf(v3 - ub));
            }
            Hm[s * 64 + lane] = vm;
            if constexpr (SENSOR) Ha[s * 64 + lane] = am;
        }
        blk2::wave_lds_sync();
        const float zlm = Hm[4 * 64 + lane], zhm = Hm[5 * 64 + lane];
        const float zla = SENSOR ? Ha[4 * 64 + lane] : 0.0f, zha = SENSOR ? Ha[5 * 64 + lane] : 0.0f;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float uc = uk[k];
            const float* tk = tile + k * 64;
            // x, y: inside the plane or the side's reduced slot (x sides: t = j + 8k, y sides: t = i + 8k)
            float vm[6], am[6];
            vm[0] = e0 ? Hm[0 * 64 + j + 8 * k] : tk[lane - 1];
            vm[1] = e1 ? Hm[1 * 64 + j + 8 * k] : tk[lane + 1];
            vm[2] = e2 ? Hm[2 * 64 + i + 8 * k] : tk[lane - 8];
            vm[3] = e3 ? Hm[3 * 64 + i + 8 * k] : tk[lane + 8];
            // z: registers
            vm[4] = k == 0 ? zlm : uk[k > 0 ? k - 1 : 0];
            vm[5] = k == 7 ? zhm : uk[k < 7 ? k + 1 : 7];
            if constexpr (SENSOR) {
                am[0] = e0 ? Ha[0 * 64 + j + 8 * k] : fabsf(vm[0] - uc);
                am[1] = e1 ? Ha[1 * 64 + j + 8 * k] : fabsf(vm[1] - uc);
                am[2] = e2 ? Ha[2 * 64 + i + 8 * k] : fabsf(vm[2] - uc);
                am[3] = e3 ? Ha[3 * 64 + i + 8 * k] : fabsf(vm[3] - uc);
                am[4] = k == 0 ? zla : fabsf(vm[4] - uc);
                am[5] = k == 7 ? zha : fabsf(vm[5] - uc);
            }
            const float ql[3] = {q0, q2, k == 0 ? bb.q[4] : 0.5f}, qh[3] = {q1, q3, k == 7 ? bb.q[5] : 0.5f};
            float D = SENSOR ? 1e-7f : 0.0f, g[3];
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const float rh = bb.rh[d];
                const float fr = uc + qh[d] * (vm[2 * d + 1] - uc);
                const float fl = uc + ql[d] * (vm[2 * d] - uc);
                g[d] = (fr - fl) * rh;
                if constexpr (SENSOR) {
                    const float gg = ((vm[2 * d + 1] - uc) - (uc - vm[2 * d])) * rh;
                    const float ugg = (am[2 * d + 1] + am[2 * d]) * rh;
                    D = fmaxf(D, (1e-7f + fabsf(gg)) * __builtin_amdgcn_rcpf(1e-7f + ugg));
                }
            }
            sink(v, k, g, D,
                 general || (k == 0 && bb.type[4] == SIDE_GENERAL) || (k == 7 && bb.type[5] == SIDE_GENERAL));
        }
    }
}

// the gradients of NV cell fields F[v] of one block in registers, g[v][k][d] (plane k of this lane's column, dimension d):
// for the kernels that consume them where they are made (ibh_turb.hip).  Blocks without GENERAL sides only.
template <int NV>
__device__ __forceinline__ void wave_gradients(const BlockDesc3& bb, const int32_t* __restrict__ htab,
                                               const int32_t* __restrict__ ftab, int32_t blk, const float* const* F,
                                               float* lds, int lane, float (&g)[NV][8][3]) {
    wave_gradient_pass<NV, false>(bb, htab, ftab, blk, [&](int v) { return F[v]; }, lds, lane,
                                  [&](int v, int k, const float (&gv)[3], float, bool) {
                                      g[v][k][0] = gv[0], g[v][k][1] = gv[1], g[v][k][2] = gv[2];
                                  });
}

// wave_gradients as it was before wave_gradient_pass, the same arithmetic written out: kept for k_wray_agarwal_of3
// (ibh_turb.hip) alone, which measured 0.5 - 0.8 % slower over the shared body in three processes of three
// (profiles/wave3d_gradients/README.md); with this form the kernel is the parent's, instruction for instruction.
template <int NV>
__device__ __forceinline__ void wave_gradients_written_out(const BlockDesc3& bb,
                                                           const int32_t* __restrict__ htab,
                                                           const int32_t* __restrict__ ftab, int32_t blk,
                                                           const float* const* F, float* lds, int lane,
                                                           float (&g)[NV][8][3]) {
    float* tile = lds;          // [k][lane]
    float* Hm = lds + 512;      // [side][t]: mean neighbour value across the side
    uint32_t hid[6];
    halo_ids(bb, htab, blk, lane, hid);
    const int i = lane & 7, j = lane >> 3;
    const bool e0 = i == 0, e1 = i == 7, e2 = j == 0, e3 = j == 7;
    const float q0 = e0 ? bb.q[0] : 0.5f, q1 = e1 ? bb.q[1] : 0.5f, q2 = e2 ? bb.q[2] : 0.5f, q3 = e3 ? bb.q[3] : 0.5f;
    float uka[NV][8], hva[NV][6];
#pragma unroll
    for (int v = 0; v < NV; ++v) {
#pragma unroll
        for (int k = 0; k < 8; ++k) uka[v][k] = ldg(F[v], (uint32_t)bb.base + lane + 64 * k);
#pragma unroll
        for (int s = 0; s < 6; ++s) hva[v][s] = ldg(F[v], hid[s]);
    }
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const float* u = F[v];
        if (v) blk2::wave_lds_sync();  // the previous field's LDS reads are done
#pragma unroll
        for (int k = 0; k < 8; ++k) tile[k * 64 + lane] = uka[v][k];
#pragma unroll
        for (int s = 0; s < 6; ++s) {
            float vm = hva[v][s];
            if (bb.type[s] == SIDE_FINE) {  // wave-uniform: three more fine cells behind this slot
                const int32_t* ft = ftab + (((size_t)bb.fine * 6 + s) * 64 + lane) * 3;
                const float v1 = ldg(u, (uint32_t)ft[0]), v2 = ldg(u, (uint32_t)ft[1]), v3 = ldg(u, (uint32_t)ft[2]);
                vm = 0.25f * (hva[v][s] + v1 + v2 + v3);
            }
            Hm[s * 64 + lane] = vm;
        }
        blk2::wave_lds_sync();
        const float zlm = Hm[4 * 64 + lane], zhm = Hm[5 * 64 + lane];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float uc = uka[v][k];
            const float* tk = tile + k * 64;
            float vm[6];
            vm[0] = e0 ? Hm[0 * 64 + j + 8 * k] : tk[lane - 1];
            vm[1] = e1 ? Hm[1 * 64 + j + 8 * k] : tk[lane + 1];
            vm[2] = e2 ? Hm[2 * 64 + i + 8 * k] : tk[lane - 8];
            vm[3] = e3 ? Hm[3 * 64 + i + 8 * k] : tk[lane + 8];
            vm[4] = k == 0 ? zlm : uka[v][k > 0 ? k - 1 : 0];
            vm[5] = k == 7 ? zhm : uka[v][k < 7 ? k + 1 : 7];
            const float ql[3] = {q0, q2, k == 0 ? bb.q[4] : 0.5f}, qh[3] = {q1, q3, k == 7 ? bb.q[5] : 0.5f};
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const float fr = uc + qh[d] * (vm[2 * d + 1] - uc);
                const float fl = uc + ql[d] * (vm[2 * d] - uc);
                g[v][k][d] = (fr - fl) * bb.rh[d];
            }
        }
    }
}

#pragma clang fp contract(off)

}  // namespace blk3

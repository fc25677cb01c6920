// Per-lane geometry of the side planes and the sensor reduction shared by the 3-D column sweeps (ibh_cols3d.h: scalar,
// ibh_strip3d_euler.h: Euler).  ONE wavefront sweeps an 8x8x8 block and lane L owns slot t = L of each of the six sides
// (boundary cell t1 = L & 7, t2 = L >> 3 in the side's tangential coordinates).  Lateral neighbours of the halo cells come
// from the side's plane ((n + 2)^2 at pitch 18, n = 8, or 16 on a FINE side) with its border from the rim table; the
// positions a lane writes and reads in that plane depend on the lane alone and are worked out here.
// (The file is named after the strip form of the scalar sweep, which it held until the column form replaced it: DESIGN.md.)
#pragma once
#include "ibh_wave3d.h"
#include "ibh_quad2d.h"

namespace strip3 {

#pragma clang fp contract(fast)

// lane-only geometry of the slots, computed once per wave
struct LaneGeo {
    int pc;              // this slot's position in an 8 x 8 plane (pitch 18)
    int b1, b2;          // t1 & 1, t2 & 1: position inside the 2 x 2 group in front of a coarse cell
    int rpos8, radj8;    // lanes < 32: plane position of this lane's rim cell and of the halo cell next to it (n = 8)
    int rpos16, radj16;  // the same for the 16 x 16 plane of a FINE side (all lanes)
};
__device__ __forceinline__ LaneGeo lane_geo(int lane) {
    LaneGeo L;
    L.pc = ((lane & 7) + 1) + 18 * ((lane >> 3) + 1);
    L.b1 = lane & 1;
    L.b2 = (lane >> 3) & 1;
    auto rim = [](int r, int i, int n, int& pos, int& adj) {
        const int p1 = r == 0 ? 0 : r == 1 ? n + 1 : i + 1, p2 = r == 2 ? 0 : r == 3 ? n + 1 : i + 1;
        const int a1 = r == 0 ? 1 : r == 1 ? n : i + 1, a2 = r == 2 ? 1 : r == 3 ? n : i + 1;
        pos = p1 + 18 * p2;
        adj = a1 + 18 * a2;
    };
    rim((lane >> 3) & 3, lane & 7, 8, L.rpos8, L.radj8);
    rim(lane >> 4, lane & 15, 16, L.rpos16, L.radj16);
    return L;
}

// max of three JST ratios n_i / d_i and 1e-7 with ONE reciprocal (v_rcp_f32 is a quarter-rate instruction)
__device__ __forceinline__ float jst_max3(float g1, float a1, float r1, float g2, float a2, float r2, float g3, float a3,
                                          float r3) {
    const float n1 = fmaf(fabsf(g1), r1, 1e-7f), d1 = fmaf(a1, r1, 1e-7f);
    const float n2 = fmaf(fabsf(g2), r2, 1e-7f), d2 = fmaf(a2, r2, 1e-7f);
    const float n3 = fmaf(fabsf(g3), r3, 1e-7f), d3 = fmaf(a3, r3, 1e-7f);
    const float d12 = d1 * d2;
    const float m = fmaxf(fmaxf(n1 * d2, n2 * d1) * d3, n3 * d12);
    return fmaxf(m * __builtin_amdgcn_rcpf(d12 * d3), 1e-7f);
}

#pragma clang fp contract(off)

}  // namespace strip3

// Quad sweep (2-D scalar advection-JST-MUSCL residual, test/advection.jl:67-83): ONE wavefront sweeps the 16x16 tile
// of four sibling 8x8 blocks, 4 cells per lane.  Same arithmetic as blk2::sweep_adv (ibh_sweep2d.h) -- undivided
// slopes, flux_w -- but the 64 halo cells of the tile are 1/4 of its cells instead of as many as the block's own,
// and the neighbours of a cell come from registers, a few cross-row permutes and one 18-row LDS tile per field that
// holds the quad's halo in its frame.  tests/quad_model.py is the lane-by-lane numpy statement of this file, checked
// against the oracle.
//
// Lane L = 16*g + t.
//   own cells:  x = 4*g + r (r = 0..3: one float4 per field), y = t.
//     y neighbours: the rows t -/+ 1 of the tile (one 16-byte LDS read per field and direction; rows -1 / 16 of tile U
//                   hold the means of the bottom / top halo cells, so no lane is special);
//     x neighbours: r -/+ 1 in registers; across strips the columns 4g - 1 / 4g + 4 of tile U (columns -1 / 16: the
//                   means of the left / right halo cells), for slopes and fluxes lane -/+ 16 -> ds_bpermute.
//   halo slots: the two sub-faces k = 0, 1 of boundary cell t of side [left, bottom, top, right][g] (arithmetic on
//     (k0, k1) pairs); every side writes the mean of its two halo values into the frame of tile U.
//   edge faces: the same lane computes both sub-faces of its boundary cell and hands their mean to the cell's lane
//     (left / right: its own; bottom / top: through the frame of tile U, which carries the y fluxes by then).
// A face between cell a (towards -) and cell b (towards +) seen from the other side: F(a,b) = -F(b,a) with slopes
// and velocities negated (every term of flux_w is odd or even under that swap), so low and high sides share one
// evaluation: own cell first, halo cell second, sign = +1 on top / right, -1 on left / bottom.
#pragma once
#include "ibh_sweep2d.h"

namespace quad2 {

#pragma clang fp contract(fast)

typedef float v2f __attribute__((ext_vector_type(2)));
typedef float v4f __attribute__((ext_vector_type(4)));
typedef int v2i __attribute__((ext_vector_type(2)));
// float4 in global memory at any 4-byte aligned address: a quad's first cell is a multiple of 4 only on partitions
// without skirt fragments in front of it (global_load/store_dwordx4 need dword alignment only)
typedef float v4f_g __attribute__((ext_vector_type(4), aligned(4)));

// LDS per wave (floats): tile U | tile SY | tile D | tile CY | lateral lines ext[8][20] | rings F, Q [4 rows][16] (row 0
// bottom, 1 top, 2 neutral, 3 dump).
// A tile is a frame of 18 rows, pitch 20 (conflict-free ds_write_b128): frame row r + 1 holds tile row r = -1 .. 16, cell
// (x, r) at column x.  Tile U carries the quad's halo in its frame: the means of the bottom / top halo cells in rows -1 /
// 16 (pair tiles: 8), those of the left / right halo cells in columns -1 (column 19 of the row before) / 16 -- so the
// four neighbours of a cell are plain reads of the tile, whatever the lane.  Once the slopes are taken, the same frame
// hands the y fluxes down the rows: FT of row r in row r, the bottom edge flux in row -1, the top edge flux over FT of
// the top row (QuadLane::p_exw).  Rows -1 and 16 of the other tiles are never written: what lanes t = 15 read there is
// not used.
#define QUAD_PITCH 20
#define QUAD_TILE (18 * QUAD_PITCH)
#define QUAD_OFF_EXT (4 * QUAD_TILE)
#define QUAD_OFF_RING (QUAD_OFF_EXT + 160)
#define QUAD_LDS (QUAD_OFF_RING + 2 * 64)

__device__ __forceinline__ float dpp_shr1(float old, float v) {  // lane i <- lane i-1 in rows of 16; lane 0 keeps old
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(v), 0x111, 0xf, 0xf, false));
}
__device__ __forceinline__ float dpp_shl1(float old, float v) {  // lane i <- lane i+1; lane 15 keeps old
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(v), 0x101, 0xf, 0xf, false));
}
__device__ __forceinline__ float bperm(int byte_addr, float v) {  // value of lane byte_addr/4
    return __int_as_float(__builtin_amdgcn_ds_bpermute(byte_addr, __float_as_int(v)));
}
__device__ __forceinline__ float max3(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }
// an LDS read every lane performs: keeps the compiler from sinking it into a divergent branch of a later select
__device__ __forceinline__ float lds_read(const float* p) {
    float v = *p;
    asm volatile("" : "+v"(v));
    return v;
}

// interior faces (both cells same level, wa = 1/2), four at a time
__device__ __forceinline__ v4f flux_half4(v4f ua, v4f ub, v4f Sa, v4f Sb, v4f Da, v4f Db, v4f Ca, v4f Cb) {
    const v4f d = ub - ua;
    // (x + (-0.5) d instead of x - 0.5 d would spare the two instructions per pair that negate d -- measured: the compiler
    // then contracts uf and A differently, the bits change; so it stays)
    const v4f gu = Sa - 0.5f * d;
    const v4f Du = Sb - 0.5f * d;
    v4f s, Df;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        s[c] = __builtin_amdgcn_fmed3f(Du[c], gu[c], 0.0f);
        Df[c] = max3(Da[c], Db[c], 1e-7f);
    }
    const v4f t16 = (Sa - Sb) * 0.0625f;
    const v4f uf = (ua + 0.5f * d) + t16;
    const v4f A = uf - Df * t16;
    const v4f Cf = 0.5f * (Ca + Cb);
    const v4f B = Df * (s - 0.5f * d);
    const v4f CA = Cf * A;
    v4f F;
#pragma unroll
    for (int c = 0; c < 4; ++c) F[c] = fmaf(fabsf(Cf[c]), B[c], CA[c]);
    return F;
}

// edge faces: two sub-faces at a time, a = the quad's boundary cell (broadcast), b = the halo cells
__device__ __forceinline__ v2f flux_w2(float ua, v2f ub, float Sa, v2f Sb, float Da, v2f Db, float Ca, v2f Cb, float wa) {
    const v2f d = ub - ua;
    const v2f gu = Sa - d * wa;
    const v2f Du = Sb - d * (1.0f - wa);
    const v2f s = v2f{__builtin_amdgcn_fmed3f(Du.x, gu.x, 0.0f), __builtin_amdgcn_fmed3f(Du.y, gu.y, 0.0f)};
    const v2f t16 = (Sa - Sb) * 0.0625f;
    const v2f uf = (ua + wa * d) + t16;
    const v2f mu = d * (0.5f - wa) - t16;
    const v2f Df = v2f{max3(Da, Db.x, 1e-7f), max3(Da, Db.y, 1e-7f)};
    const v2f A = uf + Df * mu;
    const v2f Cf = Ca + wa * (Cb - Ca);
    const v2f B = Df * (s - 0.5f * d);
    const v2f CA = Cf * A;
    return v2f{fmaf(fabsf(Cf.x), B.x, CA.x), fmaf(fabsf(Cf.y), B.y, CA.y)};
}

// JST ratio (1e-7 + |g| rh) / (1e-7 + a rh)  (JST_sensor :1077-1097, undivided sums)
__device__ __forceinline__ float jst(float g, float a, float rh) {
    return fmaf(fabsf(g), rh, 1e-7f) * __builtin_amdgcn_rcpf(fmaf(a, rh, 1e-7f));
}
// max(1e-7, ratio of direction 1, ratio of direction 2) with ONE reciprocal (v_rcp_f32 is a quarter-rate instruction:
// it costs four issue slots): n1/d1 vs n2/d2 -> max(n1 d2, n2 d1) / (d1 d2); all four terms are positive
__device__ __forceinline__ float jst_max2(float g1, float a1, float rh1, float g2, float a2, float rh2) {
    const float n1 = fmaf(fabsf(g1), rh1, 1e-7f), d1 = fmaf(a1, rh1, 1e-7f);
    const float n2 = fmaf(fabsf(g2), rh2, 1e-7f), d2 = fmaf(a2, rh2, 1e-7f);
    return fmaxf(fmaxf(n1 * d2, n2 * d1) * __builtin_amdgcn_rcpf(d1 * d2), 1e-7f);
}

// Lane table of the quad sweep, built at compile time: per lane 8 words.  w0..w5: twelve LDS byte offsets packed two per
// word (see QuadLane for the meaning of the fields), w6: byte offset of the lane's first cell inside the quad, w7: what
// the second halo pair adds to its halo id (quad_load_halo_paired).
// Everything a lane class decides and that is a constant of the lane is here or in a wave-wide constant mask (QL_MASK),
// not in the instruction stream.
// HALF: the tile of a PAIR of blocks (16 x 8 cells: lower-left, lower-right), swept by the same wave code -- lanes t >= 8
// own no cells (they still own the slots of bottom / top boundary cells x = t), the top side sits on row 7
template <bool HALF>
struct QuadLaneTab {
    uint32_t w[64][8];
    constexpr QuadLaneTab() : w() {
        for (int lane = 0; lane < 64; ++lane) {
            const int g = lane >> 4, t = lane & 15, tl = lane & 7, lhs = lane >> 3;
            const int ytop = HALF ? 7 : 15;
            const bool g0 = g == 0, g3 = g == 3, lr = g0 || g3, t0 = t == 0, t15 = t == ytop;
            const int bx = g0 ? 0 : g3 ? 15 : t, by = lr ? t : g == 1 ? 0 : ytop;
            const int pos_b = (by + 1) * QUAD_PITCH + bx;
            const int pos_b1 = lr ? ((t ^ 1) + 1) * QUAD_PITCH + bx : (by + 1) * QUAD_PITCH + (t ^ 1);
            const int pos_up = t * QUAD_PITCH + 4 * g;  // tile row t - 1
            // halo slot of this lane's side in the frame of tile U; where its edge flux goes (left / right: a free slot)
            const int pos_hm = g0 ? (t + 1) * QUAD_PITCH - 1 : g3 ? (t + 1) * QUAD_PITCH + 16 : g == 1 ? t : (ytop + 2) * QUAD_PITCH + t;
            const int pos_exw = g == 1 ? t : g == 2 ? (ytop + 1) * QUAD_PITCH + t : 17 * QUAD_PITCH + 19;
            const int myrow = t0 ? 0 : t15 ? 1 : 2, rowB = t0 ? 0 : 2, rowT = t15 ? 1 : 2;
            const int wrow = g == 1 ? 0 : g == 2 ? 1 : 3;
            const int eline = (lane & 31) >> 2, ee = lane & 3;
            const int epos = QUAD_OFF_EXT + eline * 20 + (ee < 2 ? ee : 16 + ee);
            const int line = QUAD_OFF_EXT + lhs * 20;
            const uint32_t f[12] = {
                (uint32_t)pos_up, (uint32_t)pos_b, (uint32_t)pos_b1, (uint32_t)epos,
                (uint32_t)(QUAD_OFF_RING + wrow * 16 + t), (uint32_t)(QUAD_OFF_RING + myrow * 16 + 4 * g),
                (uint32_t)(QUAD_OFF_RING + rowB * 16 + 4 * g), (uint32_t)(QUAD_OFF_RING + rowT * 16 + 4 * g),
                (uint32_t)(line + 2 * tl), (uint32_t)(line + 2 * (tl & ~1)), (uint32_t)pos_hm, (uint32_t)pos_exw};
            for (int k = 0; k < 6; ++k) w[lane][k] = (4u * f[2 * k]) | ((4u * f[2 * k + 1]) << 16);
            w[lane][6] = 4u * (64u * ((g >> 1) + (HALF ? 0 : 2 * (t >> 3))) + 4u * (g & 1) + 8u * (t & 7));
            w[lane][7] = (uint32_t)(g0 ? -1 : g == 1 ? -8 : g == 2 ? 8 : 0);
        }
    }
};
__device__ const QuadLaneTab<false> lane_tab = QuadLaneTab<false>();
__device__ const QuadLaneTab<true> lane_tab_half = QuadLaneTab<true>();

// a lane class as a wave-wide constant: the select takes its condition from a scalar register pair that holds the
// literal, where a compare of the lane id would cost a vector instruction per class
#define QL_MASK(m) __builtin_amdgcn_inverse_ballot_w64(m)

// ---- the wave's lane-only state: LDS pointers from a compile-time table (two 16-byte loads; computing them costs
// ~90 vector instructions per wave, a fifth of a quad's arithmetic), lane classes from constant masks
struct QuadLane {
    float *p_up;     // the four cells BELOW this lane's in a tile (its own: + QUAD_PITCH, the ones above: + 2 QUAD_PITCH)
    float *p_hm;     // where the mean of this lane's two halo cells goes in the frame of tile U
    float *p_exw;    // where the edge flux of a bottom / top lane goes in that frame (left / right: a free slot)
    float *p_b;      // boundary cell of this lane's halo slots (in tile U)
    float *p_b1;     // its pair mate t ^ 1 (COARSE sides)
    float *p_epos;   // where lane & 31 puts its end value
    float *p_ringw;  // ring entry this lane's side writes (dump row for left / right)
    float *p_ringm;  // ring row this lane reads: bottom (t = 0), top (t = 15), neutral
    float *p_ringB;  // ring row for the low y side: bottom or neutral
    float *p_ringT;  // ... high y side: top or neutral
    float *p_LbS;    // low lateral pair of this lane's slots, SAME / FINE half-sides (high pair: + 4; the lane's own
                     // two slots in the lateral line: + 2)
    float *p_LbC;    // ... COARSE half-sides (high pair: + 6)
    uint32_t a0off4; // byte offset of this lane's first cell relative to the quad's
    int offB;        // second halo pair: left -1 (the pair starts at the deeper cell), bottom -8, top +8, right 0
    int lane;
    bool g0, g3, lr, dny;
    bool tl0, tl7;   // first / last lane of its half-side
    bool active;     // this lane owns cells (pair tiles: t < 8)
    float sgn;       // +1: the quad's cell is the owner of the edge face (top / right), -1 on left / bottom
};

template <bool HALF = false>
__device__ __forceinline__ QuadLane quad_lane(float* lds, int lane) {
    QuadLane G;
    char* const L = (char*)lds;
    const uint32_t* const tab = HALF ? lane_tab_half.w[lane] : lane_tab.w[lane];
    const uint4 w0 = *(const uint4*)(tab);
    const uint4 w1 = *(const uint4*)(tab + 4);
#define QL_LO(w) ((w) & 0xffffu)
#define QL_HI(w) ((w) >> 16)
    G.p_up = (float*)(L + QL_LO(w0.x));
    G.p_b = (float*)(L + QL_HI(w0.x));
    G.p_b1 = (float*)(L + QL_LO(w0.y));
    G.p_epos = (float*)(L + QL_HI(w0.y));
    G.p_ringw = (float*)(L + QL_LO(w0.z));
    G.p_ringm = (float*)(L + QL_HI(w0.z));
    G.p_ringB = (float*)(L + QL_LO(w0.w));
    G.p_ringT = (float*)(L + QL_HI(w0.w));
    G.p_LbS = (float*)(L + QL_LO(w1.x));
    G.p_LbC = (float*)(L + QL_HI(w1.x));
    G.p_hm = (float*)(L + QL_LO(w1.y));
    G.p_exw = (float*)(L + QL_HI(w1.y));
#undef QL_LO
#undef QL_HI
    G.sgn = QL_MASK(0xffffffff00000000ull) ? 1.0f : -1.0f;
    // (pair tiles: lanes t >= 8 repeat the cells of t - 8 -- valid loads, nothing stored)
    G.a0off4 = w1.z;
    G.offB = (int)w1.w;
    G.lane = lane;
    G.g0 = QL_MASK(0x000000000000ffffull);
    G.g3 = QL_MASK(0xffff000000000000ull);
    G.lr = QL_MASK(0xffff00000000ffffull);
    G.dny = QL_MASK(0x0000ffffffff0000ull);
    G.tl0 = QL_MASK(0x0101010101010101ull);
    G.tl7 = QL_MASK(0x8080808080808080ull);
    G.active = QL_MASK(HALF ? 0x00ff00ff00ff00ffull : ~0ull);
    // neutral ring rows: sensor correction 0, weight 1/2 (read by lanes that are not on the y edges)
    ((float*)(L + 4 * (QUAD_OFF_RING + 32)))[lane & 15] = 0.0f;
    ((float*)(L + 4 * (QUAD_OFF_RING + 64 + 32)))[lane & 15] = 0.5f;
    return G;
}

// ---- what a wave fetches for a quad, in three dependent steps
struct QuadTab {   // needs the quad's index only
    QuadDesc2 d;   // wave-uniform
    uint32_t ty;   // side class of this lane's half-side (lane >> 3)
    v2i hid;       // halo cells of this lane's two slots
    uint32_t eid;  // end cell of lane & 31
};
struct QuadOwn {   // needs the descriptor
    v4f U, CX, CY;
};
struct QuadHalo {  // needs the table entries
    v2f hu, hd, hc;
    float eu;
};
// qaux (or null): the compact companion rows (IBH_QAUX, ibh_common.h) -- half-sides with arithmetic halo ids are computed
// from one origin id, only FINE half-sides (and the rare others) read their part of the 640-byte row
__device__ __forceinline__ QuadTab quad_load_tab(const QuadDesc2* __restrict__ qd, const int32_t* __restrict__ qtab,
                                                 int32_t q, int lane, const int32_t* __restrict__ qaux = nullptr) {
    QuadTab T;
    T.d = qd[q];
    T.ty = (T.d.cls >> ((lane >> 1) & 28)) & 15u;
    const int32_t* row = qtab + (size_t)q * IBH_QROW;
    if (qaux) {
        const int32_t* aux = qaux + (size_t)q * IBH_QAUX;
        const int lhs = lane >> 3, tl = lane & 7;
        const int32_t orig = aux[32 + lhs];
        T.eid = (uint32_t)aux[lane & 31];
        const bool isC = T.ty == SIDE_COARSE;
        const bool lr = QL_MASK(0xffff00000000ffffull);
        const int32_t id = orig + (lr ? 8 : 1) * (isC ? tl >> 1 : tl);
        T.hid = v2i{id, id};
        if (orig < 0) T.hid = *(const v2i*)(row + 2 * lane);
        return T;
    }
    T.hid = *(const v2i*)(row + 2 * lane);
    T.eid = (uint32_t)row[128 + (lane & 31)];
    return T;
}
__device__ __forceinline__ size_t quad_base4(const QuadTab& T) { return (size_t)(uint32_t)T.d.base << 2; }
__device__ __forceinline__ QuadOwn quad_load_own(const QuadLane& G, const QuadTab& T, const float* __restrict__ u,
                                                 const float* __restrict__ C, uint32_t ldc) {
    QuadOwn O;
    // the quad's base is wave-uniform: it goes into the scalar base address, the lane adds a 32-bit byte offset < 1 KB
    const size_t b4 = quad_base4(T);
    O.U = *(const v4f_g*)((const char*)u + b4 + G.a0off4);
    O.CX = *(const v4f_g*)((const char*)C + b4 + G.a0off4);
    O.CY = *(const v4f_g*)((const char*)(C + ldc) + b4 + G.a0off4);
    return O;
}
// Halo gathers: seven per quad.  Measured (scripts/probe_sweep.py, profiles/r2_final/README.md): alone each costs
// about as much as a float4 load of the whole tile; inside the sweep, dropping ALL second-slot gathers is worth 0.35 us
// of 4.95 (wrong on FINE half-sides), but every exact way of skipping them where the second slot names the same cell
// as the first -- a wave-uniform branch, a second code path for quads without a FINE side, exec-masked loads, a paired
// 8-byte load of halo + deeper cell -- measured equal or slower than gathering everything: the sweep ends with its
// slowest waves, and those are the quads with a FINE side either way.
//
// The seven values with FOUR full gathers and one that only the lanes of FINE left / right half-sides issue:
// every gather is 8 bytes per lane.  Left / right lanes: the halo cell and the cell one step deeper are x neighbours
// (one pair per sub-face slot).  Bottom / top lanes: the two sub-face cells of a FINE half-side are x neighbours (the
// builder checks it: ibh_build_quads2), so (slot 0, slot 1) of the halo cells, of the deeper cells and of the velocity
// come as pairs; on SAME / COARSE half-sides slot 1 repeats slot 0 and the second element is not used.
__device__ __forceinline__ QuadHalo quad_load_halo_paired(const QuadLane& G, const QuadTab& T, const float* __restrict__ u,
                                                          const float* __restrict__ C, uint32_t ldc) {
    using blk2::ldg;
    typedef float v2f_g __attribute__((ext_vector_type(2), aligned(4)));
    auto pair = [](const float* p, int i) { return *(const v2f_g*)((const char*)p + ((size_t)(uint32_t)i << 2)); };
    QuadHalo H;
    const float* Cn = C + (G.dny ? ldc : 0u);
    const bool isF = T.ty == SIDE_FINE;
    // left side: the pair starts at the deeper cell, one in front of the halo cell
    const v2f PA = pair(u, T.hid.x - (int)G.g0);
    const v2f PB = pair(u, (G.lr ? T.hid.y : T.hid.x) + G.offB);
    const v2f PC = pair(Cn, T.hid.x);
    H.eu = ldg(u, T.eid);
    float hc1 = 0.0f;
    if (G.lr && isF) hc1 = ldg(Cn, (uint32_t)T.hid.y);              // few lanes, few quads
    asm volatile("" : "+v"(hc1));
    // which element of which pair is which value (one select per class that differs, conditions are scalar masks):
    //            left (g0)      right (g3)     bottom / top FINE   bottom / top SAME, COARSE
    //   hu.x     PA.y           PA.x           PA.x                PA.x
    //   hd.x     PA.x           PA.y           PB.x                PB.x
    //   hu.y     PB.y           PB.x           PA.y                PA.x
    //   hd.y     PB.x           PB.y           PB.y                PB.x
    const bool dF = G.dny && isF;
    const float a = dF ? PA.y : PA.x;
    H.hu.x = G.g0 ? PA.y : PA.x;
    H.hd.x = G.g0 ? PA.x : (G.g3 ? PA.y : PB.x);
    H.hu.y = G.g0 ? PB.y : (G.g3 ? PB.x : a);
    H.hd.y = (G.g3 || dF) ? PB.y : PB.x;
    H.hc.x = PC.x;
    H.hc.y = isF ? (G.lr ? hc1 : PC.y) : PC.x;
    return H;
}

// ---- the arithmetic of one quad.  STAMP: phase time stamps of the wave (100 MHz ticks) for scripts/wave_timeline.py
// STEP: the explicit update u + dt * residual is stored instead of the residual (ibh_step_advection)
template <bool STAMP, bool STEP = false, bool HALF = false>
__device__ __forceinline__ void quad_compute(const QuadLane& G, const QuadTab& T, const QuadOwn& O, const QuadHalo& H,
                                             float* __restrict__ ud, unsigned long long* stamps, float dt = 0.0f) {
    using blk2::wave_lds_sync;
    auto stamp = [&](int k) {
        if constexpr (STAMP) {
            __builtin_amdgcn_s_waitcnt(0);
            if (stamps && G.lane == 0) stamps[k] = __builtin_amdgcn_s_memrealtime();
        }
    };
    const v4f U = O.U, CX = O.CX, CY = O.CY;
    const v2f hu = H.hu, hd = H.hd, hc = H.hc;
    const bool g0 = G.g0, g3 = G.g3, lr = G.lr, dny = G.dny;
    const int lane = G.lane;
    const float sgn = G.sgn;
    const uint32_t ty = T.ty;
    const bool isC = ty == SIDE_COARSE, isF = ty == SIDE_FINE;
    const float qs = isC ? (1.0f / 3.0f) : isF ? (2.0f / 3.0f) : 0.5f;  // at_faces weight of the quad's cell
    const float irt = isC ? 0.5f : isF ? 2.0f : 1.0f;                   // h / h_halo
    const float rhx = T.d.rh[0], rhy = T.d.rh[1];

    // ---- stage: u tile, lateral lines
    float* const p_own = G.p_up + QUAD_PITCH;
    *(v4f*)p_own = U;
    *(v4f*)(p_own + 3 * QUAD_TILE) = CY;
    *(v2f*)(G.p_LbS + 2) = hu;
    *G.p_epos = H.eu;
    wave_lds_sync();
    stamp(4);
    const float m0 = lds_read(G.p_b);
    const float m1r = lds_read(G.p_b1);
    const float m1 = isC ? m1r : m0;
    const float hm = 0.5f * (hu.x + hu.y);
    // sensor correction of a boundary cell that faces two finer cells: its |d| sum counts both of them
    const float fix = 0.5f * (fabsf(hu.x - m0) + fabsf(hu.y - m0)) - fabsf(hm - m0);
    *G.p_hm = hm;
    G.p_ringw[0] = fix;
    G.p_ringw[64] = qs;
    wave_lds_sync();
    stamp(5);

    // ---- own cells: undivided slopes + sensor
    v4f SX, SY, D;
    v4f uT;
    {
        // the neighbours across the lane's edges, from the frame of tile U: cells of the tile or the halo means
        const v4f UL = v4f{p_own[-1], U.x, U.y, U.z};
        const v4f UR = v4f{U.y, U.z, U.w, p_own[4]};
        const v4f qL = v4f{g0 ? qs : 0.5f, 0.5f, 0.5f, 0.5f};
        const v4f qR = v4f{0.5f, 0.5f, 0.5f, g3 ? qs : 0.5f};
        const v4f dR = UR - U, dL = U - UL;
        // one multiply and one fma per cell, as the packed form qR * dR + qL * dL contracts: dR of a cell is dL of the next
        // one, so packed operands would be register pairs that overlap and have to be copied apart first
#pragma unroll
        for (int c = 0; c < 4; ++c) SX[c] = fmaf(qR[c], dR[c], qL[c] * dL[c]);
        const v4f gx = dR - dL;
        const v4f rF = *(const v4f*)G.p_ringm;
        const v4f qB = *(const v4f*)(G.p_ringB + 64);
        const v4f qT = *(const v4f*)(G.p_ringT + 64);
        const v4f uB = *(const v4f*)G.p_up;
        uT = *(const v4f*)(G.p_up + 2 * QUAD_PITCH);
        const v4f dT = uT - U, dB = U - uB;
        SY = qT * dT + qB * dB;
        const v4f gy = dT - dB;
        const float fx0 = g0 ? fix : 0.0f, fx3 = g3 ? fix : 0.0f;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float ax = fabsf(dR[c]) + fabsf(dL[c]);
            if (c == 0) ax += fx0;
            if (c == 3) ax += fx3;
            const float ay = (fabsf(dT[c]) + fabsf(dB[c])) + rF[c];
            D[c] = jst_max2(gx[c], ax, rhx, gy[c], ay, rhy);
        }
    }
    *(v4f*)(p_own + QUAD_TILE) = SY;
    *(v4f*)(p_own + 2 * QUAD_TILE) = D;

    // ---- halo cells of this lane's two slots: slope along the side normal and sensor
    v2f Shn, Dh;  // Shn: slope of the halo cell seen from the quad outwards (sign folded for the edge flux below)
    {
        const float ihn = (dny ? rhy : rhx) * irt, iht = (dny ? rhx : rhy) * irt;
        const v2f dm0 = m0 - hu, dm1 = m1 - hu, dde = hd - hu;
        const v2f din = 0.5f * (dm0 + dm1);
        // -(1 - qs) din + dde / 2  (= -x of blk2::sweep_adv)
        Shn = 0.5f * dde - (1.0f - qs) * din;
        // lateral neighbours (ibh_sweep2d.h:246-255 in pair form; quad_model.py checks the equivalence)
        const v2f Lp = *(const v2f*)(isC ? G.p_LbC : G.p_LbS);
        const v2f Hp = *(const v2f*)((isC ? G.p_LbC + 2 : G.p_LbS) + 4);
        const bool t0l = G.tl0, t7l = G.tl7;
        const v2f lo0 = v2f{(isF && !t0l) ? Lp.y : Lp.x, isF ? hu.x : Lp.x};
        const v2f lo1 = v2f{Lp.y, isF ? hu.x : Lp.y};
        const v2f hi0 = v2f{isF ? hu.y : Hp.x, Hp.x};
        const v2f hi1 = v2f{isF ? hu.y : Hp.y, (isF && !t7l) ? Hp.x : Hp.y};
        const v2f e0 = lo0 - hu, e1 = lo1 - hu, e2 = hi0 - hu, e3 = hi1 - hu;
        const v2f gn = (dm0 + dm1) + (dde + dde);
        const v2f gt = (e0 + e1) + (e2 + e3);
        const float hn = 0.5f * ihn, ht = 0.5f * iht;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const float an = (fabsf(dm0[k]) + fabsf(dm1[k])) + 2.0f * fabsf(dde[k]);
            const float at = (fabsf(e0[k]) + fabsf(e1[k])) + (fabsf(e2[k]) + fabsf(e3[k]));
            Dh[k] = jst_max2(gn[k], an, hn, gt[k], at, ht);
        }
    }

    // ---- interior faces: right (x+) and top (y+) face of every cell
    wave_lds_sync();  // SY, D tiles
    stamp(6);
    v4f FR, FT;
    {
        const int up = (lane + 16) << 2;
        const v4f Ub = v4f{U.y, U.z, U.w, bperm(up, U.x)};
        const v4f Sb = v4f{SX.y, SX.z, SX.w, bperm(up, SX.x)};
        const v4f Db = v4f{D.y, D.z, D.w, bperm(up, D.x)};
        const v4f Cb = v4f{CX.y, CX.z, CX.w, bperm(up, CX.x)};
        FR = flux_half4(U, Ub, SX, Sb, D, Db, CX, Cb);
        // the cells above are the next row of the tiles: one LDS read per field instead of four DPP moves.  Lanes t = 15
        // read row 16, which nobody writes in these tiles: whatever is there, their top face is an edge face -- the top
        // edge flux replaces their FT below (pair tiles: lanes t = 7, and what t >= 8 compute is never stored)
        const v4f St = *(const v4f*)(p_own + QUAD_TILE + QUAD_PITCH);
        const v4f Dt = *(const v4f*)(p_own + 2 * QUAD_TILE + QUAD_PITCH);
        const v4f Ct = *(const v4f*)(p_own + 3 * QUAD_TILE + QUAD_PITCH);
        FT = flux_half4(U, uT, SY, St, D, Dt, CY, Ct);
    }
    *(v4f*)p_own = FT;  // tile U is done with u: its frame now hands the y fluxes down the rows

    // ---- edge faces: both sub-faces of this lane's boundary cell
    float edge;
    {
        // the sensor of the boundary cell is in tile D for every side (left / right lanes read back their own D.x / D.w);
        // there is no tile of SX and CX
        const float So_lr = g3 ? SX.w : SX.x, Co_lr = g3 ? CX.w : CX.x;
        const float So_bt = lds_read(G.p_b + QUAD_TILE), Do = lds_read(G.p_b + 2 * QUAD_TILE),
                    Co_bt = lds_read(G.p_b + 3 * QUAD_TILE);
        const float So = lr ? So_lr : So_bt;
        const float Co = lr ? Co_lr : Co_bt;
        // own cell first, halo second; on low sides everything that is odd under the swap is negated (sgn = -1)
        const v2f F = flux_w2(m0, hu, sgn * So, Shn, Do, Dh, sgn * Co, sgn * hc, qs);
        edge = sgn * (0.5f * (F.x + F.y));
    }
    *G.p_exw = edge;  // bottom: row -1; top: over FT of the top row
    wave_lds_sync();
    stamp(7);

    // ---- Green-Gauss
    {
        const float FRm = bperm((lane - 16) << 2, FR.w);
        const v4f FL = v4f{g0 ? edge : FRm, FR.x, FR.y, FR.z};
        const v4f FRf = v4f{FR.x, FR.y, FR.z, g3 ? edge : FR.w};
        // the flux through the lower face is what the row below stored, through the upper face what this row holds now
        const v4f FB = *(const v4f*)G.p_up;
        const v4f FTf = *(const v4f*)p_own;
        const v4f res = -((FRf - FL) * rhx) - ((FTf - FB) * rhy);
        float* const out = (float*)((char*)ud + quad_base4(T) + G.a0off4);
        // the residual is not read again by this sweep: stores that do not allocate in L2 (`nt`) -- 6.03 -> 5.86 us per sweep at
        // 0.87 M cells, 15.05 -> 14.89 at 3.47 M (same box, alternating builds).  Not for STEP, whose output the next step reads.
#ifdef Q2_NO_NT_STORE   // (A/B)
        if (!HALF || G.active) *(v4f_g*)out = STEP ? U + dt * res : res;
#else
        if (!HALF || G.active) {
            if constexpr (STEP) *(v4f_g*)out = U + dt * res;
            else __builtin_nontemporal_store(res, (v4f_g*)out);
        }
#endif
    }
}

// ---- one quad by one wave.  (Sweeping several quads per wave with the next quad's loads in flight was measured and
// dropped: the prefetch registers cost a wave per SIMD -- 124 VGPRs against 89 -- and the sweep lives on wave-level
// parallelism: 6.1 us against 5.5 us at 0.87 M cells, no gain at 3.47 M.)
template <bool STAMP, bool STEP = false, bool HALF = false>
__device__ __forceinline__ void sweep_quad(const QuadDesc2* __restrict__ qd, const int32_t* __restrict__ qtab, int32_t q,
                                           const float* __restrict__ u, const float* __restrict__ C, uint32_t ldc,
                                           float* __restrict__ ud, float* lds, int lane,
                                           unsigned long long* stamps = nullptr, float dt = 0.0f,
                                           const int32_t* __restrict__ qaux = nullptr) {
    const QuadLane G = quad_lane<HALF>(lds, lane);
    const QuadTab T = quad_load_tab(qd, qtab, q, lane, qaux);  // everything that needs the quad's index only is in flight
    const QuadOwn O = quad_load_own(G, T, u, C, ldc);
    const QuadHalo H = quad_load_halo_paired(G, T, u, C, ldc);
    quad_compute<STAMP, STEP, HALF>(G, T, O, H, ud, stamps, dt);
}

#pragma clang fp contract(off)

}  // namespace quad2

// libibhip: fused residual sweeps, 2-D single-kernel forms -- no gradient workspace, one launch per phase.
//   k_sweep_adv / k_sweep_euler             one wavefront per 8x8 block (blk2::sweep_adv / sweep_euler, ibh_sweep2d.h)
//   k_sweep_quad / k_sweep_quad_euler       one wavefront per 2x2 group of sibling blocks (ibh_quad2d.h, ibh_quad2d_euler.h),
//                                           the blocks outside such groups by the per-block body in the same launch
//   k_sweep_rows                            one wavefront per eight blocks (ibh_rows2d.h)
//   k_step_quad                             a rank's step: xGMI halo exchange + image-only quad sweep in one launch
// and their launchers (adv2_*, euler2_single; ibh_fused.hip decides which one runs).  The two-kernel form of the blocks these
// sweeps do not take is in ibh_fused_general.hip.
#include <algorithm>

#include <string.h>

#include "ibh_block2d.h"
#include "ibh_sweep2d.h"
#include "ibh_quad2d.h"
#include "ibh_quad2d_euler.h"
#include "ibh_rows2d.h"
#include "ibh_halo_dev.h"
#include "ibh_fused_int.h"

using namespace fused;

namespace {

// Single-kernel sweep over a range of eligible blocks (blk2::sweep_adv): no workspace traffic, one launch.
// A workgroup owns WPB*iters consecutive blocks; wave w takes block (first + k*WPB + w), k = 0..iters-1, so the
// waves of a workgroup always work on adjacent blocks and the lane-only index arithmetic is paid once per wave.
#ifndef IBH_SWEEP_WAVES
#define IBH_SWEEP_WAVES 5
#endif
template <bool DT>
__global__ __launch_bounds__(64 * WPB) __attribute__((amdgpu_waves_per_eu(IBH_SWEEP_WAVES, IBH_SWEEP_WAVES))) void k_sweep_adv(const float* __restrict__ u, const float* __restrict__ C,
                                                        uint32_t ldc, float* __restrict__ ud,
                                                        const BlockDesc2* __restrict__ blocks,
                                                        const int32_t* __restrict__ htab,
                                                        const int32_t* __restrict__ etab,
                                                        const int32_t* __restrict__ dtab, int32_t nblk, int32_t nwg,
                                                        int32_t iters, const int32_t* __restrict__ blist) {
    __shared__ float lds[WPB * BLK2_SWEEP_LDS];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;  // uniform LDS base
    const int32_t first = __builtin_amdgcn_readfirstlane(xcd_remap(blockIdx.x, nwg) * (WPB * iters) + wave);
    if (first >= nblk) return;
    const int32_t nb = __builtin_amdgcn_readfirstlane(min(iters, (nblk - first + WPB - 1) / WPB));
    blk2::sweep_adv<DT>(blocks, htab, etab, dtab, blist, first, WPB, nb, u, C, ldc, ud, lds + wave * BLK2_SWEEP_LDS, lane);
}

// Quad sweep (quad2::sweep_quad): one wavefront per 2x2 group of sibling blocks; the blocks outside such groups take the
// per-block single kernel (blk2::sweep_adv) in the SAME launch: grid = [quad workgroups | single-block workgroups]
// (the other order measured 0.5 us slower).  Measured and dropped (profiles/r2_*/README.md): a persistent form (about
// two waves per SIMD splitting the item list by estimated cost, next item's loads in flight: 7.2 us against 5.5 us) and
// several quads per wave with prefetch (6.1 us) -- the sweep lives on wave-level parallelism.
#define QUAD_WG_LDS (WPB * (QUAD_LDS > BLK2_SWEEP_LDS ? QUAD_LDS : BLK2_SWEEP_LDS))
// wave timeline of a launch (STAMP, ibh_debug_buffer): per wave {start, end} in 100 MHz ticks and the HW_ID register
__device__ unsigned long long* ibh_dbg_buf = nullptr;
__device__ __forceinline__ void dbg_stamp(int32_t slot, int k, unsigned long long v) {
    if (ibh_dbg_buf && threadIdx.x % 64 == 0) ibh_dbg_buf[(size_t)slot * 8 + k] = v;
}

// RS: the blocks outside quads take the row sweep, EIGHT per wave (rows2::sweep_rows over the list), instead of the per-block
// body -- `nwgs`, `siters` then count waves of eight
template <bool DT, bool STAMP, bool STEP = false, bool RS = false>
#ifndef QS_WAVES
#define QS_WAVES 5
#endif
__global__ __launch_bounds__(64 * WPB) __attribute__((amdgpu_waves_per_eu(QS_WAVES, QS_WAVES))) void k_sweep_quad(const float* __restrict__ u, const float* __restrict__ C,
                                                         uint32_t ldc, float* __restrict__ ud,
                                                         const QuadDesc2* __restrict__ qd,
                                                         const int32_t* __restrict__ qtab, int32_t nq, int32_t nwgq,
                                                         const BlockDesc2* __restrict__ blocks,
                                                         const int32_t* __restrict__ htab,
                                                         const int32_t* __restrict__ etab,
                                                         const int32_t* __restrict__ dtab,
                                                         const int32_t* __restrict__ singles, int32_t ns, int32_t nwgs,
                                                         int32_t singles_first, int32_t siters,
                                                         const float* __restrict__ dtp = nullptr, int32_t npair = 0,
                                                         const int32_t* __restrict__ qaux = nullptr) {
    __shared__ __attribute__((aligned(16))) float lds[RS && WPB * ROWS_LDS > QUAD_WG_LDS ? WPB * ROWS_LDS : QUAD_WG_LDS];
    float dt = 0.0f;
    if constexpr (STEP) dt = *dtp;  // (scalar load: the time step lives on the device, ibh_timestep_advection)
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int32_t slot = blockIdx.x * WPB + wave;
    if constexpr (STAMP) {
        dbg_stamp(slot, 0, __builtin_amdgcn_s_memrealtime());
        dbg_stamp(slot, 2, __builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11)));  // HW_REG_HW_ID, all 32 bits
    }
    const int32_t wgq = singles_first ? (int32_t)blockIdx.x - nwgs : (int32_t)blockIdx.x;
    const bool isq = wgq >= 0 && wgq < nwgq;
    if (isq) {
        const int32_t q = __builtin_amdgcn_readfirstlane(xcd_remap(wgq, nwgq) * WPB + wave);
        if (q < nq)
            quad2::sweep_quad<STAMP, STEP>(qd, qtab, q, u, C, ldc, ud, lds + wave * QUAD_LDS, lane,
                                           STAMP && ibh_dbg_buf ? ibh_dbg_buf + (size_t)slot * 8 : nullptr, dt, qaux);
        else if (q < nq + npair)  // pair tiles: entries nq .. of the same arrays, the HALF form of the same wave code
            quad2::sweep_quad<STAMP, STEP, true>(qd, qtab, q, u, C, ldc, ud, lds + wave * QUAD_LDS, lane,
                                                 STAMP && ibh_dbg_buf ? ibh_dbg_buf + (size_t)slot * 8 : nullptr, dt, qaux);
    } else {
        const int32_t wgs = singles_first ? (int32_t)blockIdx.x : (int32_t)blockIdx.x - nwgq;
        if constexpr (RS) {
            const int32_t first8 = __builtin_amdgcn_readfirstlane((xcd_remap(wgs, nwgs) * WPB + wave) * 8);
            if (first8 < ns) {
                __builtin_amdgcn_s_setprio(3);  // a row wave is the longest-lived wave of the launch
                rows2::sweep_rows(blocks, etab, first8, ns, u, C, ldc, ud, lds + wave * ROWS_LDS, lane, singles);
            }
            return;
        }
        const int32_t first = __builtin_amdgcn_readfirstlane(xcd_remap(wgs, nwgs) * (WPB * siters) + wave);
        if (first < ns) {
            const int32_t nb = __builtin_amdgcn_readfirstlane(min(siters, (ns - first + WPB - 1) / WPB));
            blk2::sweep_adv<DT, STEP>(blocks, htab, etab, dtab, singles, first, WPB, nb, u, C, ldc, ud,
                                      lds + wave * BLK2_SWEEP_LDS, lane, dt);
        }
    }
    if constexpr (STAMP) {
        __builtin_amdgcn_s_waitcnt(0);
        dbg_stamp(slot, 1, __builtin_amdgcn_s_memrealtime());
        dbg_stamp(slot, 3, (unsigned long long)isq);
    }
}

// Row / column sweep (rows2::sweep_rows): one wavefront per EIGHT blocks, every complete block of a one-partition mesh
#ifndef WPBR
#define WPBR 4
#endif
__global__ __launch_bounds__(64 * WPBR) void k_sweep_rows(const float* __restrict__ u, const float* __restrict__ C,
                                                          uint32_t ldc, float* __restrict__ ud,
                                                          const BlockDesc2* __restrict__ blocks,
                                                          const int32_t* __restrict__ etab, int32_t b0, int32_t n,
                                                          int32_t nwg, const int32_t* __restrict__ list) {
    __shared__ __attribute__((aligned(16))) float lds[WPBR * ROWS_LDS];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int32_t first = __builtin_amdgcn_readfirstlane((xcd_remap(blockIdx.x, nwg) * WPBR + wave) * 8);
    if (first < n)
        rows2::sweep_rows(blocks + b0, etab + (size_t)b0 * 16, first, n, u, C, ldc, ud, lds + wave * ROWS_LDS, lane, list);
}

// One step of a rank of a multi-GPU run in ONE launch: the xGMI halo exchange of u (ibh_halo_dev.h) and the image-only
// quad sweep.  Grid = [E exchange workgroups | interior quads | interior single blocks | boundary quads | boundary
// single blocks]: the exchange workgroups push this rank's skirt rows to the peers, wait for the peers' rows and unpack
// them while the interior waves -- which read no skirt cell -- already compute; a boundary wave first waits (bounded
// spin) until every exchange workgroup of ITS launch has unpacked.  fstate (device, zeroed once): [0] tickets of the
// boundary workgroups (launch index = ticket / boundary workgroups per launch: the grid of an exchanger never
// changes), [1] exchange workgroups done.  A time-out sets bit 1 of state[2] (XgmiHalo.healthy()).
template <bool DT>
__global__ __launch_bounds__(64 * WPB) void k_step_quad(float* __restrict__ u, const float* __restrict__ C, uint32_t ldc,
                                                        float* __restrict__ ud, const QuadDesc2* __restrict__ qd,
                                                        const int32_t* __restrict__ qtab, int32_t nq_int, int32_t nq,
                                                        const BlockDesc2* __restrict__ blocks,
                                                        const int32_t* __restrict__ htab,
                                                        const int32_t* __restrict__ etab,
                                                        const int32_t* __restrict__ dtab,
                                                        const int32_t* __restrict__ singles, int32_t ns_int, int32_t ns,
                                                        const int32_t* __restrict__ send_all,
                                                        const int32_t* __restrict__ recv_all,
                                                        const float* __restrict__ src0, const float* __restrict__ src1,
                                                        XchgArgs A, uint32_t* __restrict__ state, uint32_t max_spins,
                                                        int32_t E, unsigned long long* __restrict__ fstate) {
    __shared__ __attribute__((aligned(16))) float lds[QUAD_WG_LDS];
    const int32_t b0 = (int32_t)blockIdx.x;
    if (b0 < E) {
        halo_exchange_wg(u, 1, 0, send_all, recv_all, src0, src1, A, state, max_spins, b0, E);
        __threadfence();  // the unpacked skirt rows before the count
        __syncthreads();
        if (threadIdx.x == 0) atomicAdd(&fstate[1], 1ull);
        return;
    }
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int32_t nwg_qi = (nq_int + WPB - 1) / WPB, nwg_si = (ns_int + WPB - 1) / WPB;
    const int32_t nwg_qb = (nq - nq_int + WPB - 1) / WPB, nwg_sb = (ns - ns_int + WPB - 1) / WPB;
    int32_t b = b0 - E;
    const bool boundary = b >= nwg_qi + nwg_si;
    if (boundary) {
        __shared__ unsigned long long want;
        if (threadIdx.x == 0) {
            const unsigned long long t = atomicAdd(&fstate[0], 1ull);
            want = (t / (unsigned long long)(nwg_qb + nwg_sb) + 1ull) * (unsigned long long)E;
        }
        __syncthreads();
        if (lane == 0) {
            const unsigned long long w = want;
            // bounded like the exchange wait, but strictly longer (4 x the spins at half the sleep): a peer that is late
            // yet inside the exchange bound must not make these waves give up first and compute on stale skirt rows
            unsigned long long spins = 0;
            const unsigned long long bound = 4ull * (unsigned long long)max_spins;
            while (__hip_atomic_load(&fstate[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < w) {
                if (++spins >= bound) {  // every wave reaches the exit
                    atomicOr(&state[2], 2u);
                    break;
                }
                __builtin_amdgcn_s_sleep(4);
            }
        }
        __threadfence();  // acquire: the loads below see the unpacked rows
        b -= nwg_qi + nwg_si;
    }
    // [quads | single blocks] of this phase
    const int32_t nwq = boundary ? nwg_qb : nwg_qi, q0 = boundary ? nq_int : 0, q1 = boundary ? nq : nq_int;
    const int32_t nws = boundary ? nwg_sb : nwg_si, s0 = boundary ? ns_int : 0, s1 = boundary ? ns : ns_int;
    if (b < nwq) {
        const int32_t q = __builtin_amdgcn_readfirstlane(q0 + xcd_remap(b, nwq) * WPB + wave);
        if (q < q1) quad2::sweep_quad<false>(qd, qtab, q, u, C, ldc, ud, lds + wave * QUAD_LDS, lane);
    } else {
        const int32_t first = __builtin_amdgcn_readfirstlane(s0 + xcd_remap(b - nwq, nws) * WPB + wave);
        if (first < s1)
            blk2::sweep_adv<DT>(blocks, htab, etab, dtab, singles, first, WPB, 1, u, C, ldc, ud,
                                lds + wave * BLK2_SWEEP_LDS, lane);
    }
}

// Single-kernel Euler sweep (blk2::sweep_euler); 1 / 2 / 4 waves per workgroup measured equal within 2 %
#ifndef WPBE
#define WPBE 4
#endif
// FORM (EulerForm, ibh_euler_step_dev.h): beyond FORM_RESIDUAL `R` is P_out and receives the updated primitives; dt = *dtp,
// one scalar load per wave as in k_sweep_quad<..., STEP>, or (DTC, the stage forms) dtp holds one time step per cell and is
// read where the cell is.  P0, ld0, c, sa, sb, Sd, ldsd, g: euler_step::FormArgs (Sd, ldsd: the source S of FORM_DUAL)
template <int SCH = EULER_HLL, int FORM = FORM_RESIDUAL, bool DTC = false>
__global__ __launch_bounds__(64 * WPBE) void k_sweep_euler(const float* __restrict__ P, uint32_t ldp,
                                                           float* __restrict__ R, uint32_t ldr, float Rgas, float gamma,
                                                           const BlockDesc2* __restrict__ blocks,
                                                           const int32_t* __restrict__ htab,
                                                           const int32_t* __restrict__ etab,
                                                           const int32_t* __restrict__ dtab, int32_t nblk, int32_t nwg,
                                                           int32_t iters, const int32_t* __restrict__ blist,
                                                           const float* __restrict__ dtp = nullptr,
                                                           const float* P0 = nullptr, uint32_t ld0 = 0, float c = 1.0f,
                                                           float sa = 0.0f, float sb = 1.0f, const float* Sd = nullptr,
                                                           uint32_t ldsd = 0, float g = 0.0f) {
    __shared__ float lds[WPBE * BLK2_SWEEP_EULER_LDS];
    float dt = 0.0f;
    if constexpr (FORM != FORM_RESIDUAL && !DTC) dt = *dtp;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int32_t first = __builtin_amdgcn_readfirstlane(xcd_remap(blockIdx.x, nwg) * (WPBE * iters) + wave);
    if (first >= nblk) return;
    const int32_t nb = __builtin_amdgcn_readfirstlane(min(iters, (nblk - first + WPBE - 1) / WPBE));
    blk2::sweep_euler<SCH, FORM, DTC>(blocks, htab, etab, dtab, blist, first, WPBE, nb, P, ldp, R, ldr, blk2::Gas{Rgas, gamma},
                                      lds + wave * BLK2_SWEEP_EULER_LDS, lane, dt,
                                      euler_step::FormArgs{P0, ld0, c, dtp, sa, sb, Sd, ldsd, g});
}

// Quad form of the Euler sweep (quad2::sweep_quad_euler): grid = [quad workgroups | single-block workgroups], like
// k_sweep_quad
#define QUADE_WG_LDS (WPBE * (QE_LDS > BLK2_SWEEP_EULER_LDS ? QE_LDS : BLK2_SWEEP_EULER_LDS))
// Waves per SIMD (QE_WAVES).  Round 2: 206 VGPRs = 2 waves; forcing 3 spilled 25 registers (15.4 against 12.1 us for the quads
// of the 0.87 M-cell mesh).  Round 3: HLL regrouped by state (the physical fluxes of the two sides are never held), edge
// faces first, residual accumulated direction by direction -> 188 VGPRs as the compiler schedules it freely, 136 with no
// spill when asked for 3 waves, 128 with 6 spilled for 4.  Same box, whole sweep: 2 / 3 / 4 waves 15.8 / 14.8 / 15.0 us at
// 0.87 M cells, 48.1 / 41.9 / 43.2 us at 3.47 M (profiles/r3_final/euler2d_waves.json).
#ifndef QE_WAVES
#define QE_WAVES 3
#endif
template <int SCH = EULER_HLL, int FORM = FORM_RESIDUAL, bool DTC = false>
__global__ __launch_bounds__(64 * WPBE) __attribute__((amdgpu_waves_per_eu(QE_WAVES, QE_WAVES))) void k_sweep_quad_euler(const float* __restrict__ P, uint32_t ldp,
                                                                float* __restrict__ R, uint32_t ldr, float Rgas,
                                                                float gamma, const QuadDesc2* __restrict__ qd,
                                                                const int32_t* __restrict__ qtab, int32_t nq,
                                                                int32_t nwgq, const BlockDesc2* __restrict__ blocks,
                                                                const int32_t* __restrict__ htab,
                                                                const int32_t* __restrict__ etab,
                                                                const int32_t* __restrict__ dtab,
                                                                const int32_t* __restrict__ singles, int32_t ns,
                                                                int32_t nwgs, int32_t singles_first,
                                                                const float* __restrict__ dtp = nullptr,
                                                                const float* P0 = nullptr, uint32_t ld0 = 0,
                                                                float c = 1.0f, float sa = 0.0f,
                                                                float sb = 1.0f, const float* Sd = nullptr,
                                                                uint32_t ldsd = 0, float g = 0.0f) {
    __shared__ __attribute__((aligned(16))) float lds[QUADE_WG_LDS];
    float dt = 0.0f;
    if constexpr (FORM != FORM_RESIDUAL && !DTC) dt = *dtp;  // (scalar load: the time step lives on the device, ibh_timestep_euler)
    const euler_step::FormArgs fa{P0, ld0, c, dtp, sa, sb, Sd, ldsd, g};
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int32_t wg = singles_first ? ((int32_t)blockIdx.x < nwgs ? (int32_t)blockIdx.x + nwgq : (int32_t)blockIdx.x - nwgs)
                                     : (int32_t)blockIdx.x;
    if (wg < nwgq) {
        const int32_t q = __builtin_amdgcn_readfirstlane(xcd_remap(wg, nwgq) * WPBE + wave);
        if (q < nq)
            quad2::sweep_quad_euler<SCH, FORM, DTC>(qd, qtab, q, P, ldp, R, ldr, blk2::Gas{Rgas, gamma}, lds + wave * QE_LDS, lane,
                                                    dt, fa);
    } else {
        const int32_t first = __builtin_amdgcn_readfirstlane(xcd_remap(wg - nwgq, nwgs) * WPBE + wave);
#ifndef IBH_QE_NO_SINGLES  // (instruction counts of the quad path alone: scripts/isa_count.py)
        if (first < ns)
            blk2::sweep_euler<SCH, FORM, DTC>(blocks, htab, etab, dtab, singles, first, WPBE, 1, P, ldp, R, ldr, blk2::Gas{Rgas, gamma},
                                              lds + wave * BLK2_SWEEP_EULER_LDS, lane, dt, fa);
#endif
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Host side

// measured (profiles/r3_final/rows_for_singles.json): 1 441 single blocks 5.96 -> 10.6 us, 5 937: 15.5 -> 19.0 us (a row wave
// lives ~3 us whatever the load, and the second launch is serial), 47 272: 126.1 -> 119.0 us
#define IBH_ROWS_SINGLES_MIN 24000

// ---- set-up shared by the advection and the Euler launchers (only the kernel and its physics arguments differ)
// quad launch: the quads and the single blocks of quad set `k` in phase `ph`
struct QuadRange { Range q, s; };
QuadRange quad_range(const ibh_part* p, int k, Phase ph) {
    QuadRange r{ph.of(p->nq_int[k], p->nq[k]), ph.of(p->nqs_int[k], p->nqs[k])};
    if (T.quad_parts == 1) r.s.last = r.s.first;  // measurement: quads only / single blocks only
    if (T.quad_parts == 2) r.q.last = r.q.first;
    return r;
}

// per-block list launch: positions `r` of `list`, or of the block table itself (list == null), `wpb` blocks per workgroup
struct BlockList { const BlockDesc2* bl; const int32_t *ht, *et, *ls; int32_t count, iters, nwg; };
BlockList block_list(const ibh_part* p, const int32_t* list, Range r, int wpb, int max_iters) {
    // blocks per wave: keep enough waves to fill the chip before a wave takes a second block
    // (measured on 13.5 k and 54 k blocks, scripts/sweep_iters.sh: 2-3 and 4-6 blocks per wave are best)
    const int32_t count = r.count(), iters = T.sweep_iters > 0 ? T.sweep_iters : std::min(max_iters, std::max(1, count / 6000));
    return {list ? p->blocks2 : p->blocks2 + r.first, list ? p->htab : p->htab + (size_t)r.first * 64,
            list ? p->etab : p->etab + (size_t)r.first * 16, list ? list + r.first : nullptr, count, iters,
            (count + wpb * iters - 1) / (wpb * iters)};
}

// The map (scheme, form, per-cell dt) -> instantiation of an Euler sweep kernel template K, written once for k_sweep_euler and
// k_sweep_quad_euler: sixteen of each.  FORM_STEP with a per-cell dt is none of them (ibh_step_euler sends it to two launches)
#define EULER_FORM_OF(K, S, e)                                                            \
    ((e).form == FORM_DUAL    ? ((e).dt_cells ? K<S, FORM_DUAL, true> : K<S, FORM_DUAL>)   \
     : (e).form == FORM_SSP   ? ((e).dt_cells ? K<S, FORM_SSP, true> : K<S, FORM_SSP>)     \
     : (e).form == FORM_STAGE ? ((e).dt_cells ? K<S, FORM_STAGE, true> : K<S, FORM_STAGE>) \
     : (e).form == FORM_STEP  ? K<S, FORM_STEP>                                            \
                              : K<S>)
#define EULER_KERNEL(K, e) ((e).scheme == EULER_SENSOR ? EULER_FORM_OF(K, EULER_SENSOR, e) : EULER_FORM_OF(K, EULER_HLL, e))
}  // namespace

namespace fused {

// single-kernel sweep (blk2::sweep_adv) over the eligible blocks: list positions `r`
void adv2_block_list(const ibh_part* p, const AdvArgs& a, const int32_t* list, Range r) {
    if (r.count() <= 0) return;
    const BlockList L = block_list(p, list, r, WPB, 6);
    // <true>: some blocks take their deeper cells from the table (skirt fragments)
    hipLaunchKernelGGL(p->n_dt > 0 ? k_sweep_adv<true> : k_sweep_adv<false>, dim3(L.nwg), dim3(64 * WPB), 0, ibh_stream, a.u,
                       a.C, (uint32_t)a.ldc, a.ud, L.bl, L.ht, L.et, p->dtab, L.count, L.nwg, L.iters, L.ls);
}

// quad sweep over quad set `k` (0: all blocks, 1: image blocks), one phase of it or all
static void adv2_quads(const ibh_part* p, const AdvArgs& a, int k, Phase ph) {
    const Range q = quad_range(p, k, ph).q;
    Range s = quad_range(p, k, ph).s;
    // pair tiles (set 0, whole sweeps or the interior phase -- they exist only where every block is interior): the
    // single blocks are then the ones outside quads AND pairs
    const int32_t npair = (k == 0 && T.pairs && p->npair > 0 && !ph.boundary && q.first == 0 && q.last == p->nq[k] &&
                           T.quad_parts == 3) ? p->npair : 0;
    const int32_t* slist = p->qsingles[k];
    if (npair) {
        slist = p->qsingles2;
        s = {0, p->nqs2};
    } else if (k == 0 && p->npair > 0 && ph.boundary) {
        s.last = s.first;  // (all blocks are interior blocks there: nothing in the boundary phase)
    }
    // The blocks outside quads by the row sweep (rows2::sweep_rows over the list: any eight complete blocks per wave,
    // 110 vector instructions per block against 365 in the per-block kernel), as a SECOND launch where that is cheap
    // against the sweep, or inside the quad launch ("rows_singles")
    const bool rows_able = k == 0 && p->rows_ok && p->n_dt == 0 && T.quad_variant == 0 && s.count() > 0;
    const bool rows_inside = rows_able && T.rows_singles == 2;
    const bool rows_second = rows_able && !rows_inside &&
                             (T.rows_singles < 0 ? s.count() >= IBH_ROWS_SINGLES_MIN : T.rows_singles > 0);
    const Range rs = s;
    if (rows_second) s.last = s.first;
    const int32_t siters = T.quad_singles_iters > 0 ? T.quad_singles_iters : 1;
    const int32_t nwgq = (q.count() + npair + WPB - 1) / WPB,
                  nwgs = rows_inside ? (s.count() + WPB * 8 - 1) / (WPB * 8) : (s.count() + WPB * siters - 1) / (WPB * siters);
    auto kq = k_sweep_quad<false, false>;
    if (rows_inside) kq = k_sweep_quad<false, false, false, true>;
    else if (p->n_dt > 0) kq = k_sweep_quad<true, false>;
    else if (T.quad_variant == QV_STAMPS) kq = k_sweep_quad<false, true>;
    if (nwgq + nwgs > 0)
        hipLaunchKernelGGL(kq, dim3(nwgq + nwgs), dim3(64 * WPB), 0, ibh_stream, a.u, a.C, (uint32_t)a.ldc, a.ud,
                           p->qd[k] + q.first, p->qtab[k] + (size_t)q.first * IBH_QROW, q.count(), nwgq, p->blocks2, p->htab,
                           p->etab, p->dtab, slist + s.first, s.count(), nwgs, T.quad_singles_first, siters,
                           (const float*)nullptr, npair,
                           T.arith_ids ? p->qaux[k] + (size_t)q.first * IBH_QAUX : (const int32_t*)nullptr);
    if (rows_second) {
        const int32_t nw = (rs.count() + 7) / 8, nwgr = (nw + WPBR - 1) / WPBR;
        hipLaunchKernelGGL(k_sweep_rows, dim3(nwgr), dim3(64 * WPBR), 0, ibh_stream, a.u, a.C, (uint32_t)a.ldc, a.ud,
                           p->blocks2, p->etab, 0, rs.count(), nwgr, slist + rs.first);
    }
}

// One launch per phase, no workspace.  k = 0: every block is eligible, the whole sweep; k = 1: only the image cells are
// wanted (a rank of a multi-GPU run) and every image block is eligible, nothing for the skirt fragments
void adv2_single(const ibh_part* p, const AdvArgs& a, int flags, Phase ph, int k) {
    const Range b = k ? ph.of(p->n_img_int, p->n_img) : ph.of(p->nB1, p->nblk);
    if (k == 0 && p->rows_ok && T.rows && !(flags & IBH_NO_QUAD) && T.quad_variant == 0) {
        // row / column sweep: eight blocks per wavefront, arithmetic halo ids (`quad_variant` != 0: the quad forms)
        const int32_t nw = (b.count() + 7) / 8, nwg = (nw + WPBR - 1) / WPBR;
        if (nwg > 0)
            hipLaunchKernelGGL(k_sweep_rows, dim3(nwg), dim3(64 * WPBR), 0, ibh_stream, a.u, a.C, (uint32_t)a.ldc, a.ud,
                               p->blocks2, p->etab, b.first, b.count(), nwg, (const int32_t*)nullptr);
    } else if (quads_usable(p, k, flags)) adv2_quads(p, a, k, ph);
    else adv2_block_list(p, a, k ? p->img_list : nullptr, b);
}

// every block eligible, or only the image blocks wanted and all of them eligible: one launch per phase, no workspace
// e.form beyond FORM_RESIDUAL (ibh_step_euler, ibh_stage_euler, ibh_stage_euler_ssp, ibh_stage_euler_dual): that form of the
// same kernels -- e.R is P_out and receives the updated primitives
void euler2_single(const ibh_part* p, const EulerArgs& e, int flags, Phase ph) {
    const int k = p->fuse_all ? 0 : 1;  // quad set; block list: all blocks / the image blocks
    if (quads_usable(p, k, flags)) {
        const QuadRange r = quad_range(p, k, ph);
        const int32_t nwgq = (r.q.count() + WPBE - 1) / WPBE, nwgs = (r.s.count() + WPBE - 1) / WPBE;
        if (nwgq + nwgs > 0)
            hipLaunchKernelGGL(EULER_KERNEL(k_sweep_quad_euler, e), dim3(nwgq + nwgs), dim3(64 * WPBE), 0, ibh_stream, e.P,
                               (uint32_t)e.ldp, e.R, (uint32_t)e.ldr, e.fluid->R, e.fluid->gamma, p->qd[k] + r.q.first,
                               p->qtab[k] + (size_t)r.q.first * IBH_QROW, r.q.count(), nwgq, p->blocks2, p->htab, p->etab,
                               p->dtab, p->qsingles[k] + r.s.first, r.s.count(), nwgs, T.quad_singles_first, e.dt, e.P0,
                               (uint32_t)e.ld0, e.c, e.a, e.b, e.S, (uint32_t)e.lds, e.g);
        return;
    }
    const Range b = p->fuse_all ? ph.of(p->nB1, p->nblk) : ph.of(p->n_img_int, p->n_img);
    if (b.count() <= 0) return;
    const BlockList L = block_list(p, p->fuse_all ? nullptr : p->img_list, b, WPBE, 4);
    hipLaunchKernelGGL(EULER_KERNEL(k_sweep_euler, e), dim3(L.nwg), dim3(64 * WPBE), 0, ibh_stream, e.P, (uint32_t)e.ldp, e.R,
                       (uint32_t)e.ldr, e.fluid->R, e.fluid->gamma, L.bl, L.ht, L.et, p->dtab, L.count, L.nwg, L.iters, L.ls, e.dt,
                       e.P0, (uint32_t)e.ld0, e.c, e.a, e.b, e.S, (uint32_t)e.lds, e.g);
}

// sweep and update in one launch: the quad sweep stores u + dt * residual (its cells of u are in registers)
void adv2_step_quads(const ibh_part* p, const float* u, float* u_out, const float* C, int64_t ldc, const float* dt_dev) {
    const int32_t npair = T.pairs ? p->npair : 0;
    const int32_t nq = p->nq[0], ns = npair ? p->nqs2 : p->nqs[0];
    const int32_t nwgq = (nq + npair + WPB - 1) / WPB, nwgs = (ns + WPB - 1) / WPB;
    hipLaunchKernelGGL((k_sweep_quad<false, false, true>), dim3(nwgq + nwgs), dim3(64 * WPB), 0, ibh_stream, u, C,
                       (uint32_t)ldc, u_out, p->qd[0], p->qtab[0], nq, nwgq, p->blocks2, p->htab, p->etab, p->dtab,
                       npair ? p->qsingles2 : p->qsingles[0], ns, nwgs, T.quad_singles_first, 1, dt_dev, npair,
                       T.arith_ids ? p->qaux[0] : (const int32_t*)nullptr);
}

int debug_buffer2d(unsigned long long* buf) {
    IBH_HIP(hipMemcpyToSymbol(HIP_SYMBOL(ibh_dbg_buf), &buf, sizeof(buf)));
    return 0;
}

}  // namespace fused

extern "C" {

// One step of a rank in one launch: xGMI halo exchange of u + image-only quad sweep (k_step_quad).  Needs a partition
// whose image blocks are all eligible and carry quads (the ranks of the benchmark meshes); otherwise the caller runs
// ibh_halo_exchange and ibh_residual_advection(IBH_IMAGE_ONLY) one after the other (same result).
int ibh_step_advection_xgmi(ibh_part* p, float* u, const float* C, int64_t ldc, float* ud, const int32_t* send_all,
                            int n_send_peers, const int32_t* send_seg, float* const* dst0, float* const* dst1,
                            uint32_t* const* send_flags, const int32_t* recv_all, const float* src0, const float* src1,
                            int n_recv_peers, const int32_t* recv_seg, const uint32_t* const* recv_flags,
                            uint32_t* state, uint32_t max_spins, unsigned long long* fstate) {
    IBH_REQUIRE(p && u && C && ud && state && fstate, "ibh_step_advection_xgmi: null argument");
    IBH_REQUIRE(fused2(p, 0) && p->img_all_fz && !p->fuse_all && quads_usable(p, 1, 0),
                "ibh_step_advection_xgmi: needs a 2-D partition with skirt fragments whose image blocks are all eligible "
                "for the quad sweep");
    IBH_REQUIRE(n_send_peers >= 0 && n_send_peers <= IBH_MAX_PEERS && n_recv_peers >= 0 && n_recv_peers <= IBH_MAX_PEERS &&
                    n_send_peers + n_recv_peers > 0,
                "ibh_step_advection_xgmi: 1 to 16 peers");
    XchgArgs A;
    memset(&A, 0, sizeof(A));
    A.ns = n_send_peers;
    A.nr = n_recv_peers;
    if (n_send_peers) {
        IBH_REQUIRE(send_all && send_seg && dst0 && dst1 && send_flags, "ibh_step_advection_xgmi: null send argument");
        for (int q = 0; q < n_send_peers; ++q) {
            A.dst[0][q] = dst0[q];
            A.dst[1][q] = dst1[q];
            A.sflag[q] = send_flags[q];
            A.sseg[q] = send_seg[q];
            IBH_REQUIRE(send_seg[q + 1] >= send_seg[q], "ibh_step_advection_xgmi: segments must ascend");
        }
        A.sseg[n_send_peers] = send_seg[n_send_peers];
    }
    if (n_recv_peers) {
        IBH_REQUIRE(recv_all && src0 && src1 && recv_seg && recv_flags, "ibh_step_advection_xgmi: null receive argument");
        for (int q = 0; q < n_recv_peers; ++q) {
            A.rflag[q] = recv_flags[q];
            A.rseg[q] = recv_seg[q];
            IBH_REQUIRE(recv_seg[q + 1] >= recv_seg[q], "ibh_step_advection_xgmi: segments must ascend");
        }
        A.rseg[n_recv_peers] = recv_seg[n_recv_peers];
    }
    const int32_t big = std::max(A.ns ? A.sseg[A.ns] : 0, A.nr ? A.rseg[A.nr] : 0);
    int E = (big + 255) / 256;
    E = E < 1 ? 1 : E > 64 ? 64 : E;
    const int32_t nq = p->nq[1], nqi = p->nq_int[1], ns = p->nqs[1], nsi = p->nqs_int[1];
    const int32_t nwg = (nqi + WPB - 1) / WPB + (nsi + WPB - 1) / WPB + (nq - nqi + WPB - 1) / WPB + (ns - nsi + WPB - 1) / WPB;
    static_assert(WPB == 4, "the exchange workgroups of k_step_quad are 256 threads");
    hipLaunchKernelGGL(p->n_dt > 0 ? k_step_quad<true> : k_step_quad<false>, dim3(E + nwg), dim3(64 * WPB), 0, ibh_stream, u, C,
                       (uint32_t)ldc, ud, p->qd[1], p->qtab[1], nqi, nq, p->blocks2, p->htab, p->etab, p->dtab, p->qsingles[1],
                       nsi, ns, send_all, recv_all, src0, src1, A, state, max_spins, E, fstate);
    IBH_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"

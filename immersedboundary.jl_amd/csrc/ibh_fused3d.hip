// libibhip: fused residual sweeps, 3-D (8x8x8 blocks).
//   single-kernel sweeps, no gradient workspace:
//     k_sweep3_cols / k_sweep3_euler_cols   one wavefront per block, columns of eight cells per lane (ibh_cols3d.h,
//                                           ibh_strip3d_euler.h): the default forms
//     k_sweep3_adv / k_sweep3_euler         thread per cell, one 512-thread workgroup per block (ibh_block3d.h), A/B
//   two-kernel form through the workspace, the face-list cells (ibh_facelist.h) in the same launch as the blocks:
//     k_passA3_wave, k_passA3e_wave         pass A, one wavefront per block: the gradient sweep of ibh_wave3d.h
//     k_passB3_adv_blk, k_passB3e_blk       pass B, one 512-thread workgroup per block (ibh_block3d.h)
// and their launchers (adv3_*, euler3_*; ibh_fused.hip decides which one runs).
#include "ibh_facelist.h"
#include "ibh_strip3d_euler.h"
#include "ibh_cols3d.h"
#include "ibh_block3d.h"
#include "ibh_fused_int.h"

using namespace flist;
using namespace fused;

namespace {

// 3-D pass B block kernels: one 512-thread workgroup per 8x8x8 block
// grid = [face-list workgroups over `cells` | nblk block workgroups]: the face-list cells (sides facing finer
// blocks, partial skirt blocks) are few but latency-bound (a ~20 us chain of dependent loads); dispatched FIRST
// in the same launch they run underneath the block work instead of forming a tail.
__global__ __launch_bounds__(512) void k_passB3_adv_blk(PartView p, const float* __restrict__ u,
                                                        const float* __restrict__ C, int64_t ldc,
                                                        const float* __restrict__ G, float* __restrict__ ud,
                                                        const BlockDesc3* __restrict__ blocks,
                                                        const int32_t* __restrict__ htab,
                                                        const int32_t* __restrict__ ftab, int32_t nblk,
                                                        const int32_t* __restrict__ cells, int32_t ncells,
                                                        FlatRec flat, const int32_t* __restrict__ blist) {
    __shared__ float lds[BLK3_PASSB_LDS];
    const int32_t gI = (ncells + 511) / 512;
    if ((int32_t)blockIdx.x >= gI) {
        int32_t blk = xcd_remap(blockIdx.x - gI, nblk);
        if (blist) blk = blist[blk];
        blk3::passB_adv(blocks, htab, ftab, blk, (uint32_t)p.nc, u, C, (uint32_t)ldc, G, ud, lds, threadIdx.x);
        return;
    }
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < ncells) {
        if (flat.rec) passB_adv_flat<3>(p, flat, (int32_t)t, cells[t], u, C, ldc, G, ud);
        else passB_adv_cell<3>(p, u, C, ldc, G, ud, cells[t]);
    }
}

// 3-D single-kernel scalar sweep (blk3::sweep_adv): one 512-thread workgroup per block, every block of the partition
__global__ __launch_bounds__(512) void k_sweep3_adv(const float* __restrict__ u, const float* __restrict__ C, uint32_t ldc,
                                                    float* __restrict__ ud, const BlockDesc3* __restrict__ blocks,
                                                    const int32_t* __restrict__ htab, const int32_t* __restrict__ ftab,
                                                    const int32_t* __restrict__ rtab, const int32_t* __restrict__ r4tab,
                                                    int32_t n) {
    __shared__ float lds[BLK3_SWEEP_LDS];
    const int32_t blk = xcd_remap(blockIdx.x, n);
    blk3::sweep_adv(blocks, htab, ftab, rtab + (size_t)blk * 384, r4tab, blk, u, C, ldc, ud, lds, threadIdx.x);
}

// 3-D single-kernel Euler sweep (blk3::sweep_euler): one 512-thread workgroup per block, every block of the partition
__global__ __launch_bounds__(512) void k_sweep3_euler(const float* __restrict__ P, uint32_t ldp, float* __restrict__ R,
                                                      uint32_t ldr, float Rgas, float gamma,
                                                      const BlockDesc3* __restrict__ blocks,
                                                      const int32_t* __restrict__ htab, const int32_t* __restrict__ ftab,
                                                      const int32_t* __restrict__ rtab, const int32_t* __restrict__ r4tab,
                                                      int32_t n) {
    __shared__ float lds[BLK3_SWEEP_EULER_LDS];
    const int32_t blk = xcd_remap(blockIdx.x, n);
    blk3::sweep_euler(blocks, htab, ftab, rtab + (size_t)blk * 384, r4tab, blk, P, ldp, R, ldr, blk3::Gas3{Rgas, gamma}, lds,
                      threadIdx.x);
}

// Column form of the 3-D scalar sweep (cols3::sweep_cols): one wavefront per block
#ifndef WPB3C
#define WPB3C 2
#endif
// TAB: the block table is that of the IMAGE blocks of a partition with skirt fragments (ibh_analyze3_image.cpp): sides
// towards a fragment take halo and deeper cells from tables (dtab)
template <int WAVES, bool TAB = false>
__global__ __launch_bounds__(64 * WPB3C) __attribute__((amdgpu_waves_per_eu(WAVES, WAVES))) void k_sweep3_cols(
    const float* __restrict__ u, const float* __restrict__ C, uint32_t ldc, float* __restrict__ ud,
    const BlockDesc3* __restrict__ blocks, const int32_t* __restrict__ htab, const int32_t* __restrict__ ftab,
    const int32_t* __restrict__ rtab, const int32_t* __restrict__ r4tab, int32_t n, int32_t nwg,
    const int32_t* __restrict__ dtab = nullptr) {
    __shared__ __attribute__((aligned(16))) float lds[WPB3C * C3_LDS];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int32_t blk = __builtin_amdgcn_readfirstlane(xcd_remap(blockIdx.x, nwg) * WPB3C + wave);
    if (blk < n)
        cols3::sweep_cols(blocks, htab, ftab, rtab, r4tab, blk, u, C, ldc, ud, lds + wave * C3_LDS, lane,
                          TAB ? dtab : nullptr);
}

// Column form of the 3-D Euler sweep (strip3e::sweep_euler_cols): one wavefront per 8^3 block, grid = blocks.
// (Persistent waves with the next block's first loads in flight were tried in rounds 3 and 4 and measured slower; the
// record is in DESIGN.md and profiles/r4_final/README.md.)
#ifndef WPB3E
#define WPB3E 1
#endif
// wave timeline of a launch (STAMP, ibh_debug_buffer), as in ibh_fused2d.hip: this code object's own pointer
__device__ unsigned long long* ibh_dbg_buf = nullptr;
template <int WAVES, bool STAMP = false, bool TAB = false, int SCH = EULER_HLL>
__global__ __launch_bounds__(64 * WPB3E) __attribute__((amdgpu_waves_per_eu(WAVES, WAVES))) void k_sweep3_euler_cols(
    const float* __restrict__ P, uint32_t ldp, float* __restrict__ R, uint32_t ldr, float Rgas, float gamma,
    const BlockDesc3* __restrict__ blocks, const int32_t* __restrict__ htab, const int32_t* __restrict__ ftab,
    const int32_t* __restrict__ rtab, const int32_t* __restrict__ r4tab, int32_t n, int32_t nwg,
    const int32_t* __restrict__ dtab = nullptr) {
    __shared__ __attribute__((aligned(16))) float lds[WPB3E * S3E_LDS];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int32_t blk = __builtin_amdgcn_readfirstlane(xcd_remap(blockIdx.x, nwg) * WPB3E + wave);
    strip3e::sweep_euler_cols<STAMP, SCH>(blocks, htab, ftab, rtab, r4tab, blk, n, P, ldp, R, ldr, blk3::Gas3{Rgas, gamma},
                                     lds + wave * S3E_LDS, lane, STAMP ? ibh_dbg_buf : nullptr, TAB ? dtab : nullptr);
}

// wave-per-block form of the 3-D scalar pass A (blk3::wave_gradient_pass, ibh_wave3d.h): 4 blocks per 256-thread
// workgroup; G layout: gradient along dim d at G[d*nc + c], sensor at G[3*nc + c]
__global__ __launch_bounds__(256) void k_passA3_wave(PartView p, const float* __restrict__ u, float* __restrict__ G,
                                                     const BlockDesc3* __restrict__ blocks,
                                                     const int32_t* __restrict__ htab,
                                                     const int32_t* __restrict__ ftab, int32_t nblk, int32_t nwg,
                                                     const int32_t* __restrict__ cells, int32_t ncells, FlatRec flat,
                                                     const int32_t* __restrict__ blist) {
    __shared__ float lds[4 * BLK3W_PASSA_LDS];
    const int32_t gI = (ncells + 255) / 256;
    if ((int32_t)blockIdx.x >= gI) {
        const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
        const int32_t pos = __builtin_amdgcn_readfirstlane(xcd_remap(blockIdx.x - gI, nwg) * 4 + wave);
        if (pos < nblk) {
            const int32_t blk = blist ? __builtin_amdgcn_readfirstlane(blist[pos]) : pos;
            const BlockDesc3 bb = blocks[blk];
            const uint32_t nc = (uint32_t)p.nc;
            blk3::wave_gradient_pass<1, true>(
                bb, htab, ftab, blk, [&](int) { return u; }, lds + wave * BLK3W_PASSA_LDS, lane,
                [&](int, int k, const float (&g)[3], float D, bool general) {
                    if (general) return;
                    const uint32_t c = (uint32_t)bb.base + lane + 64 * k;
                    blk2::stg(G, c, g[0]);
                    blk2::stg(G + nc, c, g[1]);
                    blk2::stg(G + (size_t)2 * nc, c, g[2]);
                    blk2::stg(G + (size_t)3 * nc, c, D);
                });
        }
        return;
    }
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < ncells) {
        if (flat.rec) passA_flat<3, 1>(p, flat, (int32_t)t, cells[t], u, (int64_t)p.nc, G);
        else passA_cell<3, 1>(p, u, (int64_t)p.nc, G, cells[t]);
    }
}

// wave-per-block form of the 3-D Euler pass A, the five primitives through the same body; G layout of the face-list
// kernels: grad of var v along dim d at G[(d*5 + v)*nc + c], sensor of the pressure (var 0) at G[15*nc + c]
__global__ __launch_bounds__(256) void k_passA3e_wave(PartView p, const float* __restrict__ P, int64_t ldp,
                                                      float* __restrict__ G, const BlockDesc3* __restrict__ blocks,
                                                      const int32_t* __restrict__ htab,
                                                      const int32_t* __restrict__ ftab, int32_t nblk, int32_t nwg,
                                                      const int32_t* __restrict__ cells, int32_t ncells, FlatRec flat) {
    __shared__ float lds[4 * BLK3W_PASSA_LDS];
    const int32_t gI = (ncells + 255) / 256;
    if ((int32_t)blockIdx.x >= gI) {
        const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
        const int32_t blk = __builtin_amdgcn_readfirstlane(xcd_remap(blockIdx.x - gI, nwg) * 4 + wave);
        if (blk < nblk) {
            const BlockDesc3 bb = blocks[blk];
            const uint32_t nc = (uint32_t)p.nc;
            blk3::wave_gradient_pass<5, true>(
                bb, htab, ftab, blk, [&](int v) { return P + (size_t)v * (uint32_t)ldp; }, lds + wave * BLK3W_PASSA_LDS, lane,
                [&](int v, int k, const float (&g)[3], float D, bool general) {
                    if (general) return;
                    const uint32_t c = (uint32_t)bb.base + lane + 64 * k;
                    blk2::stg(G + (size_t)(0 * 5 + v) * nc, c, g[0]);
                    blk2::stg(G + (size_t)(1 * 5 + v) * nc, c, g[1]);
                    blk2::stg(G + (size_t)(2 * 5 + v) * nc, c, g[2]);
                    if (v == 0) blk2::stg(G + (size_t)(3 * 5) * nc, c, D);
                });
        }
        return;
    }
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < ncells) {
        if (flat.rec) passA_flat<3, 5>(p, flat, (int32_t)t, cells[t], P, ldp, G);
        else passA_cell<3, 5>(p, P, ldp, G, cells[t]);
    }
}

// 3-D Euler pass B block kernel (5 primitives)
__global__ __launch_bounds__(512) void k_passB3e_blk(uint32_t nc, const float* __restrict__ P, uint32_t ldp,
                                                     const float* __restrict__ G, float* __restrict__ R, uint32_t ldr,
                                                     float Rgas, float gamma, const BlockDesc3* __restrict__ blocks,
                                                     const int32_t* __restrict__ htab,
                                                     const int32_t* __restrict__ ftab, int32_t nblk) {
    __shared__ float lds[BLK3_EULER_LDS];
    const int32_t blk = xcd_remap(blockIdx.x, nblk);
    blk3::passB_euler(blocks, htab, ftab, blk, nc, P, ldp, G, R, ldr, blk3::Gas3{Rgas, gamma}, lds, threadIdx.x);
}

// ---------------------------------------------------------------------------------------------------------------------
// Host side

// 3-D two-kernel block launch: block kernels over the block ranges of the phase + face-list threads over the rest
// (a, b: pass A / pass B block range; nI, gI: face-list cells, their 512-thread workgroups)
struct Blocks3 { Range a, b; int32_t nI, gI; bool doA, doB; PartView v; FlatRec flat; };
Blocks3 blocks3_setup(const ibh_part* p, int flags, Phase ph) {
    const Range a = ph.of(p->nA1, p->nblk), b = ph.of(p->nB1, p->nblk);
    const int32_t nI = ph.interior ? 0 : p->n_irr, gI = (nI + 511) / 512;
    return {a, b, nI, gI, !(flags & IBH_PASS_B_ONLY) && (a.count() > 0 || gI), !(flags & IBH_PASS_A_ONLY) && (b.count() > 0 || gI),
            view(p), flat_of(p, p->irr_cells)};
}
}  // namespace

namespace fused {

int debug_buffer3d(unsigned long long* buf) {
    IBH_HIP(hipMemcpyToSymbol(HIP_SYMBOL(ibh_dbg_buf), &buf, sizeof(buf)));
    return 0;
}

// only the image cells are wanted (a rank of a multi-GPU run) and every image block qualifies: no workspace, no skirt cells
void adv3_image_cols(const ibh_part* p, const AdvArgs& a) {
    const int32_t nwg = (p->n_img3 + WPB3C - 1) / WPB3C;
    hipLaunchKernelGGL((k_sweep3_cols<3, true>), dim3(nwg), dim3(64 * WPB3C), 0, ibh_stream, a.u, a.C, (uint32_t)a.ldc, a.ud,
                       p->iblocks3, p->ihtab3, p->iftab3, p->irtab3, p->ir4tab3, p->n_img3, nwg, p->idtab3);
}
// every block qualifies for the single-kernel sweep: one launch, nothing through the workspace
void adv3_single(const ibh_part* p, const AdvArgs& a) {
    if (T.quad_variant == QV_THREAD_PER_CELL) {
        hipLaunchKernelGGL(k_sweep3_adv, dim3(p->nblk), dim3(512), 0, ibh_stream, a.u, a.C, (uint32_t)a.ldc, a.ud, p->blocks3,
                           p->htab3, p->ftab3, p->rtab3, p->r4tab3, p->nblk);
        return;
    }
    const int32_t nwg = (p->nblk + WPB3C - 1) / WPB3C;
    hipLaunchKernelGGL((k_sweep3_cols<3>), dim3(nwg), dim3(64 * WPB3C), 0, ibh_stream, a.u, a.C, (uint32_t)a.ldc, a.ud,
                       p->blocks3, p->htab3, p->ftab3, p->rtab3, p->r4tab3, p->nblk, nwg);
}

int adv3_blocks(ibh_part* p, const AdvArgs& a, int flags, Phase ph) {
    if (const int rc = ensure_G(p)) return rc;
    const Blocks3 s = blocks3_setup(p, flags, ph);
    const int32_t na = s.a.count(), nb = s.b.count();
    if (s.doA) {
        const int32_t nwgA = (na + 3) / 4, gIw = (s.nI + 255) / 256;
        hipLaunchKernelGGL(k_passA3_wave, dim3(nwgA + gIw), dim3(256), 0, ibh_stream, s.v, a.u, p->G, p->blocks3 + s.a.first,
                           p->htab3 + (size_t)s.a.first * 384, p->ftab3, na, nwgA, p->irr_cells, s.nI, s.flat,
                           (const int32_t*)nullptr);
    }
    if (s.doB)
        hipLaunchKernelGGL(k_passB3_adv_blk, dim3(nb + s.gI), dim3(512), 0, ibh_stream, s.v, a.u, a.C, a.ldc, p->G, a.ud,
                           p->blocks3 + s.b.first, p->htab3 + (size_t)s.b.first * 384, p->ftab3, nb, p->irr_cells, s.nI,
                           s.flat, (const int32_t*)nullptr);
    return 0;
}

// image blocks of a partition with skirt fragments: one launch, nothing through the workspace
void euler3_image_cols(const ibh_part* p, const EulerArgs& e) {
    const int32_t nwg = (p->n_img3 + WPB3E - 1) / WPB3E;
    const auto k = e.scheme == EULER_SENSOR ? k_sweep3_euler_cols<2, false, true, EULER_SENSOR>
                                            : k_sweep3_euler_cols<2, false, true>;
    hipLaunchKernelGGL(k, dim3(nwg), dim3(64 * WPB3E), 0, ibh_stream, e.P, (uint32_t)e.ldp, e.R, (uint32_t)e.ldr, e.fluid->R,
                       e.fluid->gamma, p->iblocks3, p->ihtab3, p->iftab3,
                       p->irtab3, p->ir4tab3, p->n_img3, nwg, p->idtab3);
}
// 3-D, every block qualifies for the single-kernel sweep: one launch, nothing through the workspace
void euler3_single(const ibh_part* p, const EulerArgs& e) {
    const int32_t nwg = (p->nblk + WPB3E - 1) / WPB3E;
    // (the sensor scheme has the column form alone: residual_euler() in ibh_fused.hip has refused every other value of
    // quad_variant before this is reached, so the tests on quad_variant below see the HLL scheme only)
    const auto k = e.scheme == EULER_SENSOR      ? k_sweep3_euler_cols<2, false, false, EULER_SENSOR>
                   : T.quad_variant == QV_STAMPS ? k_sweep3_euler_cols<2, true, false>
                                                 : k_sweep3_euler_cols<2, false, false>;
    if (T.quad_variant == QV_THREAD_PER_CELL)
        hipLaunchKernelGGL(k_sweep3_euler, dim3(p->nblk), dim3(512), 0, ibh_stream, e.P, (uint32_t)e.ldp, e.R, (uint32_t)e.ldr,
                           e.fluid->R, e.fluid->gamma, p->blocks3, p->htab3, p->ftab3, p->rtab3, p->r4tab3, p->nblk);
    else
        hipLaunchKernelGGL(k, dim3(nwg), dim3(64 * WPB3E), 0, ibh_stream, e.P, (uint32_t)e.ldp, e.R, (uint32_t)e.ldr, e.fluid->R,
                           e.fluid->gamma, p->blocks3, p->htab3, p->ftab3, p->rtab3, p->r4tab3, p->nblk, nwg,
                           (const int32_t*)nullptr);
}

// 3-D block path: block kernels + the face-list kernels over the cells the analysis left out (whole sweeps only)
int euler3_blocks(ibh_part* p, const EulerArgs& e, int flags) {
    if (const int rc = ensure_G(p)) return rc;
    const Blocks3 s = blocks3_setup(p, flags, Phase(0));
    if (s.doA) {
        const int32_t nwgA = (p->nblk + 3) / 4, gIw = (s.nI + 255) / 256;
        hipLaunchKernelGGL(k_passA3e_wave, dim3(nwgA + gIw), dim3(256), 0, ibh_stream, s.v, e.P, e.ldp, p->G, p->blocks3,
                           p->htab3, p->ftab3, p->nblk, nwgA, p->irr_cells, s.nI, s.flat);
    }
    if (s.doB) {
        hipLaunchKernelGGL(k_passB3e_blk, dim3(p->nblk), dim3(512), 0, ibh_stream, (uint32_t)p->nc, e.P, (uint32_t)e.ldp,
                           p->G, e.R, (uint32_t)e.ldr, e.fluid->R, e.fluid->gamma, p->blocks3, p->htab3, p->ftab3, p->nblk);
        if (s.nI) euler_passB_cells(p, e, p->irr_cells, s.nI);  // (the face-list pass B is a kernel of its own)
    }
    return 0;
}

}  // namespace fused

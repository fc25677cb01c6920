// libibhip: fused residual sweeps, the two-kernel form through the gradient workspace.
//
// One sweep = two kernels:
//   pass A  per cell : Green-Gauss gradients of every variable along every dim + JST sensor      -> workspace G
//   pass B  per cell : for each face of the cell MUSCL(high_order) states, flux, and the Green-Gauss sum of the fluxes
// Each pass has two bodies launched together in ONE grid:
//   * block fast path (2-D, 8x8 blocks): one 64-lane wavefront per block, lane = cell,
//     x-fastest like the reference's cell numbering (mesher.jl:1064-1112).  Cell values are
//     staged in LDS; the halo across the four block sides (same level, mirror, 2:1 coarse,
//     2:1 fine -- classified and verified against the face lists by ibh_analyze.cpp) is
//     fetched by one gather instruction per field and staged next to the tile.  No index
//     arrays are read for these cells.  Tuned arithmetic: ibh_block2d.h; literal: ibh_facelist.h.
//   * face-list path (ibh_facelist.h): one thread per cell walking the CSR left/right face lists; used for
//     cells of partial (skirt) blocks, sides the analysis could not classify, 3-D, and when
//     IBH_FORCE_GENERAL is set.
// This is the form of every partition without block structure, of IBH_NO_FUSE / IBH_EXACT / IBH_FORCE_GENERAL calls, of
// pass A alone (the tuple cell_gradient) and of the blocks a mixed 2-D launch leaves over; the single-kernel sweeps that
// are the default elsewhere are in ibh_fused2d.hip and ibh_fused3d.hip (which also has the 3-D block kernels of this form).
#include "ibh_facelist.h"
#include "ibh_block2d.h"
#include "ibh_fused_int.h"

using namespace flist;
using namespace fused;

namespace {

// ------------------------------------------------------------------------------------------
// kernels: grid = [fast-path workgroups | face-list workgroups]
// EXACT = literal IEEE arithmetic in the block path (bit-comparable with the face-list path);
// otherwise the tuned block path of ibh_block2d.h.
// ------------------------------------------------------------------------------------------
template <int ND, int NV, bool EXACT>
__global__ __launch_bounds__(64 * WPB) void k_passA(PartView p, const float* __restrict__ u, int64_t ldu,
                                               float* __restrict__ G, const BlockDesc2* __restrict__ blocks,
                                               const int32_t* __restrict__ htab, int32_t nblk, int32_t nwg_fast,
                                               const int32_t* __restrict__ cells, int32_t ncells, FlatRec flat,
                                               const int32_t* __restrict__ blist) {
    // `blocks`/`htab`/`nblk` describe the sub-range of the block table this launch covers, or, with `blist`,
    // the whole table and the list of the nblk block indices to take.
    // grid = [face-list workgroups | block workgroups]: the latency-bound face-list cells go first
    __shared__ float lds[WPB * NV * 128];
    const int32_t gI = (ncells + 64 * WPB - 1) / (64 * WPB);
    if ((int32_t)blockIdx.x >= gI) {
        const int32_t wg = blockIdx.x - gI;
        if constexpr (ND == 2) {
            int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
            int32_t blk = __builtin_amdgcn_readfirstlane(xcd_remap(wg, nwg_fast) * WPB + wave);
            if (blk < nblk) {
                if (blist) blk = blist[blk];
                if constexpr (EXACT)
                    passA_block2<NV>(blocks, htab, blk, p.spacing, p.nc, u, ldu, G, lds + wave * NV * 128, lane);
                else
                    blk2::passA<NV>(blocks, htab, blk, (uint32_t)p.nc, u, (uint32_t)ldu, G, lds + wave * NV * 128, lane);
            }
        }
        return;
    }
#ifdef IBH_NO_XCD_CELLS
    int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
#else
    int64_t t = (int64_t)ibh_xcd_chunk((int32_t)blockIdx.x, gI) * blockDim.x + threadIdx.x;   // (the face-list workgroups)
#endif
    if (t >= ncells) return;
    int32_t c = cells ? cells[t] : (int32_t)t;
    if (flat.rec) passA_flat<ND, NV>(p, flat, (int32_t)t, c, u, ldu, G);
    else passA_cell<ND, NV>(p, u, ldu, G, c);
}

template <int ND, bool EXACT>
__global__ __launch_bounds__(64 * WPB) void k_passB_adv(PartView p, const float* __restrict__ u, const float* __restrict__ C,
                                                   int64_t ldc, const float* __restrict__ G, float* __restrict__ ud,
                                                   const BlockDesc2* __restrict__ blocks,
                                                   const int32_t* __restrict__ htab, int32_t nblk, int32_t nwg_fast,
                                                   const int32_t* __restrict__ cells, int32_t ncells, FlatRec flat,
                                                   const int32_t* __restrict__ blist) {
    constexpr int LDSW = EXACT ? 6 * 128 : BLK2_PASSB_LDS;  // floats per wave
    __shared__ float lds[WPB * LDSW];
    const int32_t gI = (ncells + 64 * WPB - 1) / (64 * WPB);
    if ((int32_t)blockIdx.x >= gI) {
        const int32_t wg = blockIdx.x - gI;
        if constexpr (ND == 2) {
            int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
            int32_t blk = __builtin_amdgcn_readfirstlane(xcd_remap(wg, nwg_fast) * WPB + wave);
            if (blk < nblk) {
                if (blist) blk = blist[blk];
                if constexpr (EXACT)
                    passB_adv_block2(blocks, htab, blk, p.nc, u, C, ldc, G, ud, lds + wave * LDSW, lane);
                else
                    blk2::passB_adv(blocks, htab, blk, (uint32_t)p.nc, u, C, (uint32_t)ldc, G, ud, lds + wave * LDSW,
                                    lane);
            }
        }
        return;
    }
    int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ncells) return;
    int32_t c = cells ? cells[t] : (int32_t)t;
    if (flat.rec) passB_adv_flat<ND>(p, flat, (int32_t)t, c, u, C, ldc, G, ud);
    else passB_adv_cell<ND>(p, u, C, ldc, G, ud, c);
}

// Euler pass B: the block body and the face-list body are separate kernels (the Float64 flux combine of
// the literal face-list body needs ~120 VGPRs and would halve the occupancy of the block body).
__global__ __launch_bounds__(64 * WPB) void k_passB_euler_blk(uint32_t nc, const float* __restrict__ P, uint32_t ldp,
                                                         const float* __restrict__ G, float* __restrict__ R,
                                                         uint32_t ldr, float Rgas, float gamma,
                                                         const BlockDesc2* __restrict__ blocks,
                                                         const int32_t* __restrict__ htab, int32_t nblk, int32_t nwg) {
    __shared__ float lds[WPB * BLK2_EULER_LDS];
    int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int32_t blk = __builtin_amdgcn_readfirstlane(xcd_remap(blockIdx.x, nwg) * WPB + wave);
    if (blk < nblk)
        blk2::passB_euler(blocks, htab, blk, nc, P, ldp, G, R, ldr, blk2::Gas{Rgas, gamma}, lds + wave * BLK2_EULER_LDS,
                          lane);
}

// (127 VGPRs = four waves per SIMD.  Six and eight waves per SIMD by capping the registers -- what paid in the viscous sum --
// were measured here: 216 and 293 against 171 us on 1.67 M cells; this pass is arithmetic in Float64, the spills cost more.)
// EULER_SENSOR (Float32 flux and accumulators): nu from `nu`, or the sensor column of G when `nu` is null
template <int ND, int SCH = EULER_HLL>
__global__ __launch_bounds__(64 * WPB) void k_passB_euler(PartView p, const float* __restrict__ P, int64_t ldp,
                                                     const float* __restrict__ G, float* __restrict__ R, int64_t ldr,
                                                     float Rgas, float gamma, const int32_t* __restrict__ cells,
                                                     int32_t ncells, const float* __restrict__ nu) {
    int64_t t = IBH_WG_X() * blockDim.x + threadIdx.x;
    if (t >= ncells) return;
    int32_t c = cells ? cells[t] : (int32_t)t;
    passB_euler_cell<ND, SCH>(p, P, ldp, G, R, ldr, Rgas, gamma, c, nu);
}

// ---------------------------------------------------------------------------------------------------------------------
// Host side

// face-list threads of a two-kernel sweep: pass A over the cells outside blocks (`fast`; the interior phase has none) or
// over every cell (skirt cells feed the faces of image cells), pass B over the same cells or over the image cells only
struct CellLists { const int32_t *cellsA, *cellsB; int32_t nA, nB; };
CellLists cell_lists(const ibh_part* p, int flags, bool fast, Phase ph) {
    const bool image = (flags & IBH_IMAGE_ONLY) && !fast;
    const int32_t* cellsA = fast ? p->irr_cells : nullptr;
    const int32_t nA = fast ? (ph.interior ? 0 : p->n_irr) : p->nc;
    return {cellsA, image ? p->image_in_domain : cellsA, nA, image ? p->n_image : nA};
}
}  // namespace

namespace fused {

// Gradient workspace of the two-kernel forms: allocated ONCE, on the first sweep that needs it, for the largest sweep
// of the partition ((nd (nd + 2) + 1) nc floats: the Euler sweep), and kept until ibh_partition_destroy -- a HIP
// graph captured earlier keeps the pointer, so it must never be freed or moved by a later, larger request.  The
// single-kernel / quad / image-only paths never touch it and do not allocate it.
int ensure_G(ibh_part* p) {
    if (p->G) return 0;
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (ibh_stream && hipStreamIsCapturing(ibh_stream, &st) == hipSuccess && st != hipStreamCaptureStatusNone)
        return ibh_fail(-1, "the gradient workspace is allocated on the first two-kernel sweep of a partition: run one "
                            "sweep before capturing it into a HIP graph", __FILE__, __LINE__);
    const size_t bytes = (size_t)(p->nd * (p->nd + 2) + 1) * (size_t)p->nc * sizeof(float);
    IBH_TRY(p->own.alloc(&p->G, bytes / sizeof(float)));
    p->G_bytes = bytes;
    return 0;
}

// mixed: eligible blocks in one kernel; the rest (skirt blocks, blocks next to face-list cells) in the
// two-kernel form, with the gradient workspace filled only where it is read (ng_list)
int adv2_mixed(ibh_part* p, const AdvArgs& a, int flags, Phase ph) {
    // interior phase without blocks of the two-kernel form: nothing reads the workspace before the boundary
    // phase, so all of pass A is done there and the interior phase is one launch
    const bool defer = p->n_nf_int == 0;
    const Range g = ph.of(defer ? 0 : p->n_ng_int, p->n_ng), r = ph.of(p->n_nf_int, p->n_nf);
    const int32_t nI = ph.interior ? 0 : p->n_irr, gI = (nI + 64 * WPB - 1) / (64 * WPB);
    if (const int rc = ensure_G(p)) return rc;
    const int32_t nwgA = (g.count() + WPB - 1) / WPB, nwgB = (r.count() + WPB - 1) / WPB;
    if (!(flags & IBH_SWEEP_ONLY)) {
        const PartView v = view(p);
        if (nwgA + gI)
            hipLaunchKernelGGL((k_passA<2, 1, false>), dim3(nwgA + gI), dim3(64 * WPB), 0, ibh_stream, v, a.u, (int64_t)p->nc,
                               p->G, p->blocks2, p->htab, g.count(), nwgA, p->irr_cells, nI, flat_of(p, p->irr_cells),
                               p->ng_list + g.first);
        if (nwgB + gI)
            hipLaunchKernelGGL((k_passB_adv<2, false>), dim3(nwgB + gI), dim3(64 * WPB), 0, ibh_stream, v, a.u, a.C, a.ldc,
                               p->G, a.ud, p->blocks2, p->htab, r.count(), nwgB, p->irr_cells, nI,
                               flat_of(p, p->irr_cells), p->nf_list + r.first);
    }
    adv2_block_list(p, a, p->fz_list, ph.of(p->n_fz_int, p->n_fz));
    return 0;
}

// two-kernel form through the gradient workspace: block kernels where the partition is 2-D with blocks (`fast`), face-list
// threads for the other cells
int adv_general(ibh_part* p, const AdvArgs& a, int flags, Phase ph, AdvPath path) {
    if (const int rc = ensure_G(p)) return rc;
    const bool fast = p->nd == 2 && has_blocks(p) && !(flags & IBH_FORCE_GENERAL);
    // overlap phases: INTERIOR = blocks independent of skirt data, BOUNDARY = the rest + face-list cells
    IBH_REQUIRE(!ph.any() || fast, "overlap phases need the block path (2-D, block_size 8, domain given)");
    const Range ra = ph.of(p->nA1, p->nblk), rb = ph.of(p->nB1, p->nblk);  // pass A / pass B block range
    const int32_t nwgA = fast ? (ra.count() + WPB - 1) / WPB : 0, nwgB = fast ? (rb.count() + WPB - 1) / WPB : 0;
    const CellLists c = cell_lists(p, flags, fast, ph);
    const PartView v = view(p);
    const dim3 blk(64 * WPB), gA(nwgA + (c.nA + 64 * WPB - 1) / (64 * WPB)), gB(nwgB + (c.nB + 64 * WPB - 1) / (64 * WPB));
    const bool doA = gA.x && !(flags & IBH_PASS_B_ONLY), doB = gB.x && !(flags & IBH_PASS_A_ONLY);
    // (without `fast` the block ranges are the whole, unused tables: null in 3-D)
    const BlockDesc2 *blkA = p->blocks2 ? p->blocks2 + ra.first : nullptr, *blkB = p->blocks2 ? p->blocks2 + rb.first : nullptr;
    const int32_t* htA = p->htab ? p->htab + (size_t)ra.first * 64 : nullptr;
    const int32_t* htB = p->htab ? p->htab + (size_t)rb.first * 64 : nullptr;
    const bool d3 = path == ADV_GENERAL_3D, exact = path == ADV_GENERAL_2D_EXACT;
    auto kA = d3 ? k_passA<3, 1, true> : exact ? k_passA<2, 1, true> : k_passA<2, 1, false>;
    auto kB = d3 ? k_passB_adv<3, true> : exact ? k_passB_adv<2, true> : k_passB_adv<2, false>;
    if (doA)
        hipLaunchKernelGGL(kA, gA, blk, 0, ibh_stream, v, a.u, (int64_t)p->nc, p->G, blkA, htA, ra.count(), nwgA, c.cellsA, c.nA,
                           flat_of(p, c.cellsA), (const int32_t*)nullptr);
    if (doB)
        hipLaunchKernelGGL(kB, gB, blk, 0, ibh_stream, v, a.u, a.C, a.ldc, p->G, a.ud, blkB, htB, rb.count(), nwgB, c.cellsB,
                           c.nB, flat_of(p, c.cellsB), (const int32_t*)nullptr);
    return 0;
}

// face-list pass B of the Euler sweep over `n` cells of a list (null: the first n cells); also the cells outside blocks of
// the 3-D block path (ibh_fused3d.hip)
void euler_passB_cells(const ibh_part* p, const EulerArgs& e, const int32_t* cells, int32_t n) {
    if (n <= 0) return;
    const bool d3 = p->nd == 3;
    const auto k = e.scheme == EULER_SENSOR ? (d3 ? k_passB_euler<3, EULER_SENSOR> : k_passB_euler<2, EULER_SENSOR>)
                                            : (d3 ? k_passB_euler<3> : k_passB_euler<2>);
    hipLaunchKernelGGL(k, dim3((n + 64 * WPB - 1) / (64 * WPB)), dim3(64 * WPB), 0, ibh_stream, view(p), e.P, e.ldp, p->G, e.R,
                       e.ldr, e.fluid->R, e.fluid->gamma, cells, n, e.nu);
}

// two-kernel form, 2-D (block kernels where `fast`) and 3-D face-list (whole sweeps only)
int euler_general(ibh_part* p, const EulerArgs& e, int flags, EulerPath path) {
    if (const int rc = ensure_G(p)) return rc;
    const PartView v = view(p);
    const bool fast = path == EUL2_FAST;
    const int32_t nwg_fast = fast ? (p->nblk + WPB - 1) / WPB : 0;
    const CellLists c = cell_lists(p, flags, fast, Phase(0));
    const dim3 blk(64 * WPB), gA(nwg_fast + (c.nA + 64 * WPB - 1) / (64 * WPB));
    const bool doA = gA.x && !(flags & IBH_PASS_B_ONLY), doB = !(flags & IBH_PASS_A_ONLY);
    auto kA = fast ? k_passA<2, 4, false> : path == EUL2_FACE_LIST ? k_passA<2, 4, true> : k_passA<3, 5, true>;
    if (doA)
        hipLaunchKernelGGL(kA, gA, blk, 0, ibh_stream, v, e.P, e.ldp, p->G, p->blocks2, p->htab, p->nblk, nwg_fast, c.cellsA,
                           c.nA, flat_of(p, c.cellsA), (const int32_t*)nullptr);
    if (doB && nwg_fast)
        hipLaunchKernelGGL(k_passB_euler_blk, dim3(nwg_fast), blk, 0, ibh_stream, (uint32_t)p->nc, e.P, (uint32_t)e.ldp, p->G,
                           e.R, (uint32_t)e.ldr, e.fluid->R, e.fluid->gamma, p->blocks2, p->htab, p->nblk, nwg_fast);
    if (doB) euler_passB_cells(p, e, c.cellsB, c.nB);
    return 0;
}

}  // namespace fused

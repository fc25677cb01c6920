// libibhip: what the units of the fused sweeps share on the host -- the tuning state, the partition predicates, the path
// names and one launcher per path.  ibh_fused.hip decides the path and switches over it; the launchers live beside their
// kernels in ibh_fused2d.hip, ibh_fused3d.hip and ibh_fused_general.hip; ibh_turb.hip reads the predicates and the tuning
// state for its block closures.  Host code only: no kernel header is included here but the one that names the forms of an
// Euler step (EulerForm).  Internal to the library: the namespace is hidden, nothing of it is exported.
#pragma once
#include <stdlib.h>

#include "ibh_common.h"
#include "ibh_euler_step_dev.h"

namespace fused __attribute__((visibility("hidden"))) {

inline int env_int(const char* name, int dflt) {
    const char* s = getenv(name);
    return s ? atoi(s) : dflt;
}
// "quad_variant": the kernel form of a single-kernel sweep (0 = the default form of every path).  These are all the values
// there are: ibh_set_tuning rejects any other, and any other in the environment counts as 0.
enum : int {
    QV_STAMPS = 4,             // wave time stamps (scripts/wave_timeline.py, scripts/wave_timeline_3d.py)
    QV_THREAD_PER_CELL = 512,  // A/B: thread-per-cell form of the 3-D sweeps
};
inline bool quad_variant_known(int v) { return v == 0 || v == QV_STAMPS || v == QV_THREAD_PER_CELL; }
inline int quad_variant_or_0(int v) { return quad_variant_known(v) ? v : 0; }

// Tuning state: ibh_set_tuning(key, v) at run time, the environment for the defaults (profiling a variant under bench.py)
struct Tuning {
    int sweep_iters = env_int("IBH_SWEEP_ITERS", 0);  // blocks per wave of the per-block single-kernel sweep; 0 = automatic
    int quad = env_int("IBH_QUAD", 1);                // 0: per-block single kernel everywhere (A/B runs)
    // row / column sweep (ibh_rows2d.h) where the partition qualifies: OFF by default -- measured slower than the quad sweep
    // (8.4 against 6.1 us at 0.87 M cells, 21.7 against 17.0 at 3.47 M: profiles/r3_final/probe_rows.json)
    int rows = env_int("IBH_ROWS", 0);
    int quad_variant = quad_variant_or_0(env_int("IBH_QUAD_VARIANT", 0));  // 0 or one of the QV_* forms above
    // 1 / 2 = only the quads / only the single blocks of a quad sweep (measurement); single blocks per wave in a quad sweep
    int quad_parts = 3, quad_singles_iters = 1;
    int quad_singles_first = env_int("IBH_SINGLES_FIRST", 0);  // grid order of a quad sweep
    int pairs = env_int("IBH_PAIRS", 1);          // pair tiles for the blocks outside quads
    int arith_ids = env_int("IBH_ARITH_IDS", 1);  // quad sweep: halo ids from the companion rows
    int transport_blocks = 1;  // 0: the face-list transport kernel everywhere (A/B, tests)
    // blocks outside quads by the row sweep: -1 = by size, 0 / 1 = never / always a second launch, 2 = inside the quad launch
    int rows_singles = env_int("IBH_ROWS_SINGLES", -1);
};
extern Tuning T;  // (ibh_fused.hip)

// Flag groups of the eligibility conditions
constexpr int F_LITERAL = IBH_FORCE_GENERAL | IBH_EXACT;                       // not the tuned block arithmetic
constexpr int F_TWO_KERNEL = IBH_NO_FUSE | IBH_PASS_A_ONLY | IBH_PASS_B_ONLY;  // the workspace form is asked for
constexpr int F_PHASES = IBH_PHASE_INTERIOR | IBH_PHASE_BOUNDARY;

// Partition predicates.  The partition has a block structure (complete 8^nd blocks found by the analysis):
inline bool has_blocks(const ibh_part* p) { return p->bs == 8 && p->nblk > 0 && (p->nd == 2 ? !!p->blocks2 : !!p->blocks3); }
// ... and the call may take the tuned block kernels / the single-kernel sweeps
inline bool tuned2(const ibh_part* p, int flags) { return p->nd == 2 && has_blocks(p) && !(flags & F_LITERAL); }
inline bool tuned3(const ibh_part* p, int flags) { return p->nd == 3 && has_blocks(p) && !(flags & F_LITERAL); }
inline bool fused2(const ibh_part* p, int flags) { return tuned2(p, flags) && !(flags & F_TWO_KERNEL); }
inline bool whole3(const ibh_part* p, int flags) { return tuned3(p, flags) && !(flags & (F_TWO_KERNEL | F_PHASES)); }
// 3-D, only the image cells wanted (a rank of a multi-GPU run) and every image block qualifies / every block qualifies
inline bool image3(const ibh_part* p, int flags) { return whole3(p, flags) && (flags & IBH_IMAGE_ONLY) && p->img_all3; }
inline bool single3(const ibh_part* p, int flags) { return whole3(p, flags) && !(flags & IBH_IMAGE_ONLY) && p->sweep3; }
// every cell of the partition in a complete 8^3 block without a GENERAL side (what the fused closures need)
inline bool all_blocks3(const ibh_part* p) {
    return p->nd == 3 && has_blocks(p) && p->n_irr == 0 && (int64_t)p->nblk * 512 == p->nc &&
           p->sum.sides[SIDE_GENERAL] == 0;
}
// quad set `k` (0: all blocks, 1: image blocks) carries quads and the call may use them
inline bool quads_usable(const ibh_part* p, int k, int flags) { return T.quad && !(flags & IBH_NO_QUAD) && p->nq[k] > 0; }

// Overlap phases: INTERIOR = the leading n_int entries of a list (blocks independent of skirt data), BOUNDARY = the rest
struct Range { int32_t first, last; int32_t count() const { return last - first; } };
struct Phase {
    bool interior, boundary;
    explicit Phase(int flags) : interior((flags & IBH_PHASE_INTERIOR) != 0), boundary((flags & IBH_PHASE_BOUNDARY) != 0) {}
    bool any() const { return interior || boundary; }
    bool valid() const { return !(interior && boundary); }
    Range of(int32_t n_int, int32_t n_all) const { return {boundary ? n_int : 0, interior ? n_int : n_all}; }
};
#define IBH_PHASES_EXCLUSIVE "IBH_PHASE_INTERIOR and IBH_PHASE_BOUNDARY are exclusive"

struct AdvArgs { const float *u, *C; int64_t ldc; float* ud; };
// `nu`: the caller's sensor of the sensor scheme (nc values), or null = the pressure JST sensor the sweep computes anyway
struct EulerArgs {  // (the entries' fields)
    const float* P; int64_t ldp; float* R; int64_t ldr; const ibh_fluid* fluid;
    EulerScheme scheme = EULER_HLL; const float* nu = nullptr;
    // ibh_step_euler, ibh_stage_euler, ibh_stage_euler_ssp, ibh_stage_euler_dual on a single-kernel path: the form the sweep
    // stores (R is then P_out)
    // and what the form reads (euler_step::FormArgs) -- from FORM_STEP on dt, one value or (dt_cells, the stage forms only) one
    // per cell; from FORM_STAGE on the base state P0 (it may be R) and the coefficient c of dt; FORM_SSP the weights a and b;
    // FORM_DUAL the source S of the physical step and the coefficient g
    EulerForm form = FORM_RESIDUAL;
    const float* dt = nullptr; bool dt_cells = false;
    const float* P0 = nullptr; int64_t ld0 = 0; float c = 1.0f;
    float a = 0.0f, b = 1.0f;
    const float* S = nullptr; int64_t lds = 0; float g = 0.0f;
};

// ---- advection: paths
enum AdvPath {
    ADV3_IMAGE_COLS,      // 3-D, image blocks only: one launch of the column sweep
    ADV3_SINGLE,          // 3-D single-kernel sweep: column or thread-per-cell form by quad_variant
    ADV3_BLOCKS,          // 3-D two-kernel block path
    ADV2_IMAGE,           // 2-D, image blocks only: quads or per-block list
    ADV2_FUSE_ALL,        // 2-D, every block eligible: rows, quads or per-block
    ADV2_MIXED,           // 2-D: per-block sweep over fz_list + two-kernel form over ng_list / nf_list
    ADV_GENERAL_2D,       // two-kernel form: 2-D (block kernels where tuned + face-list threads)
    ADV_GENERAL_2D_EXACT, //                  2-D, literal arithmetic
    ADV_GENERAL_3D,       //                  3-D face-list
};

// ---- Euler: paths
enum EulerPath {
    EUL2_SINGLE,      // 2-D single launch per phase: quads or per-block
    EUL3_IMAGE_COLS,  // 3-D, image blocks only: one launch of the column sweep
    EUL3_SINGLE,      // 3-D single-kernel sweep: column / stamped / thread-per-cell form by quad_variant
    EUL2_FAST,        // two-kernel form: 2-D block kernels + face-list threads
    EUL2_FACE_LIST,   //                  2-D face-list
    EUL3_BLOCKS,      //                  3-D block kernels + face-list threads
    EUL3_FACE_LIST,   //                  3-D face-list
};

// ---- launchers, one per path (a return value is an error code; the void ones only launch)
// ibh_fused2d.hip
void adv2_block_list(const ibh_part* p, const AdvArgs& a, const int32_t* list, Range r);
void adv2_single(const ibh_part* p, const AdvArgs& a, int flags, Phase ph, int k);
void adv2_step_quads(const ibh_part* p, const float* u, float* u_out, const float* C, int64_t ldc, const float* dt_dev);
void euler2_single(const ibh_part* p, const EulerArgs& e, int flags, Phase ph);
// ibh_fused3d.hip
void adv3_image_cols(const ibh_part* p, const AdvArgs& a);
void adv3_single(const ibh_part* p, const AdvArgs& a);
int adv3_blocks(ibh_part* p, const AdvArgs& a, int flags, Phase ph);
void euler3_image_cols(const ibh_part* p, const EulerArgs& e);
void euler3_single(const ibh_part* p, const EulerArgs& e);
int euler3_blocks(ibh_part* p, const EulerArgs& e, int flags);
// ibh_fused_general.hip
int ensure_G(ibh_part* p);
int adv2_mixed(ibh_part* p, const AdvArgs& a, int flags, Phase ph);
int adv_general(ibh_part* p, const AdvArgs& a, int flags, Phase ph, AdvPath path);
int euler_general(ibh_part* p, const EulerArgs& e, int flags, EulerPath path);
void euler_passB_cells(const ibh_part* p, const EulerArgs& e, const int32_t* cells, int32_t n);
// the wave time stamps of a unit's kernels go to `buf` (ibh_debug_buffer): a device variable per code object
int debug_buffer2d(unsigned long long* buf);
int debug_buffer3d(unsigned long long* buf);

}  // namespace fused

// libibhip: the fused residual sweeps (the headline hot path) -- host dispatch.
//
// What a sweep call launches is decided in three steps, each written once: the tuning state and the partition predicates
// (ibh_fused_int.h), advection_path() / euler_path() below (the path of a (partition, flags, tuning) triple, nothing else),
// and one launcher per path.  The entry points are a switch over the path.  The kernels and their launchers live in one
// unit per family:
//   ibh_fused2d.hip        2-D single-kernel sweeps: per-block, quad, row and step kernels, scalar and Euler
//   ibh_fused3d.hip        3-D sweeps: column and thread-per-cell forms, the 3-D block kernels of the two-kernel form
//   ibh_fused_general.hip  the two-kernel form through the gradient workspace (face-list threads + 2-D block bodies)
// and the block closures of the turbulence model in ibh_turb.hip.  No kernel and no kernel header here.
#include <float.h>
#include <string.h>

#include "ibh_common.h"
#include "ibh_fused_int.h"

using namespace fused;

Tuning fused::T;

// ---- advection: path
static AdvPath advection_path(const ibh_part* p, int flags) {
    if (tuned3(p, flags)) return image3(p, flags) ? ADV3_IMAGE_COLS : single3(p, flags) ? ADV3_SINGLE : ADV3_BLOCKS;
    if (fused2(p, flags)) {
        if ((flags & IBH_IMAGE_ONLY) && p->img_all_fz && !p->fuse_all) return ADV2_IMAGE;
        if (p->fuse_all) return ADV2_FUSE_ALL;
        // A mixed launch is three kernels where the two-kernel form is two: at ~3 us per launch it only pays when the
        // single kernel saves more than that (0.26 ns per eligible block: scripts/mixed_ab.py).  The choice depends on
        // the partition only, never on the phase flags: a sweep split in phases reproduces the whole sweep bit for bit.
        const bool mixed_pays = p->n_fz >= 12000 || (flags & (IBH_FORCE_MIXED | IBH_SWEEP_ONLY));
        if (p->fz_list && 4 * (int64_t)p->n_fz >= p->nblk && mixed_pays) return ADV2_MIXED;
    }
    return p->nd != 2 ? ADV_GENERAL_3D : (flags & IBH_EXACT) ? ADV_GENERAL_2D_EXACT : ADV_GENERAL_2D;
}

// ---- Euler: path
// The sensor scheme has the single-kernel forms and the face-list form: an external nu (one more field with halos), the
// tuned two-kernel block bodies (EUL2_FAST, EUL3_BLOCKS) and IBH_NO_FUSE all take the face-list form there.
static EulerPath euler_path(const ibh_part* p, int flags, const EulerArgs& e) {
    const bool sensor = e.scheme == EULER_SENSOR;
    if (!(sensor && e.nu)) {
        if (fused2(p, flags) && (p->fuse_all || ((flags & IBH_IMAGE_ONLY) && p->img_all_fz))) return EUL2_SINGLE;
        if (image3(p, flags)) return EUL3_IMAGE_COLS;
        if (single3(p, flags)) return EUL3_SINGLE;
    }
    if (sensor) return p->nd == 2 ? EUL2_FACE_LIST : EUL3_FACE_LIST;
    // tuned block paths: not with IBH_EXACT (the literal arithmetic lives in the face-list body)
    if (p->nd == 2) return tuned2(p, flags) ? EUL2_FAST : EUL2_FACE_LIST;
    return tuned3(p, flags) ? EUL3_BLOCKS : EUL3_FACE_LIST;
}

extern "C" {

int ibh_debug_buffer(void* buf) {  // device buffer of 8 x uint64 per wave of the launch, or NULL
    unsigned long long* b = (unsigned long long*)buf;
    const int rc = debug_buffer2d(b);
    return rc ? rc : debug_buffer3d(b);
}

int ibh_set_tuning(const char* key, int value) {
    static const struct { const char* key; int* value; } keys[] = {
        {"viscous_per_cell", &ibh_viscous_per_cell}, {"ew_scalar", &ibh_ew_scalar_only},  // ibh_cfd.hip, ibh_ew.hip
        {"time_average_nt", &ibh_time_average_nt},                                        // ibh_stats.hip
        {"quad_variant", &T.quad_variant}, {"quad_parts", &T.quad_parts}, {"quad_singles_first", &T.quad_singles_first},
        {"quad_singles_iters", &T.quad_singles_iters}, {"rows", &T.rows}, {"rows_singles", &T.rows_singles},
        {"transport_blocks", &T.transport_blocks}, {"pairs", &T.pairs}, {"arith_ids", &T.arith_ids}};
    IBH_REQUIRE(key, "ibh_set_tuning: null key");
    for (const auto& k : keys)
        if (!strcmp(key, k.key)) {
            // a value that named a retired kernel form must not quietly time the default one
            IBH_REQUIRE(k.value != &T.quad_variant || quad_variant_known(value),
                        "ibh_set_tuning: quad_variant takes 0, 4 (wave time stamps) or 512 (thread per cell)");
            *k.value = value;
            return 0;
        }
    return ibh_fail(-1, "ibh_set_tuning: unknown key", __FILE__, __LINE__);
}

int ibh_residual_advection(ibh_part* p, const float* u, const float* C, int64_t ldc, float* ud, int flags) {
    IBH_REQUIRE(p && u && C && ud, "ibh_residual_advection: null argument");
    if (p->nc == 0) return 0;
    const Phase ph(flags);
    IBH_REQUIRE(ph.valid(), IBH_PHASES_EXCLUSIVE);
    const AdvArgs a{u, C, ldc, ud};
    const AdvPath path = advection_path(p, flags);
    int rc = 0;
    switch (path) {
    case ADV3_IMAGE_COLS: adv3_image_cols(p, a); break;
    case ADV3_SINGLE: adv3_single(p, a); break;
    case ADV3_BLOCKS: rc = adv3_blocks(p, a, flags, ph); break;
    case ADV2_IMAGE: adv2_single(p, a, flags, ph, 1); break;
    case ADV2_FUSE_ALL: adv2_single(p, a, flags, ph, 0); break;
    case ADV2_MIXED: rc = adv2_mixed(p, a, flags, ph); break;
    default: rc = adv_general(p, a, flags, ph, path);
    }
    if (!rc) IBH_LAUNCH_CHECK();
    return rc;
}

// n sweeps launched back to back from ONE call: the step loop of a compiled host (a Julia `for` around the ccall costs tens
// of nanoseconds per iteration; from Python the interpreter and ctypes would be ten times the 6 us sweep)
int ibh_residual_advection_n(ibh_part* p, const float* u, const float* C, int64_t ldc, float* ud, int flags, int n) {
    int rc = 0;
    for (int i = 0; i < n && !rc; ++i) rc = ibh_residual_advection(p, u, C, ldc, ud, flags);
    return rc;
}

// the Euler entries: one body, the scheme in `e`
static int residual_euler(ibh_part* p, const EulerArgs& e, int flags, const char* phase_msg) {
    if (p->nc == 0) return 0;
    const Phase ph(flags);
    const EulerPath path = euler_path(p, flags, e);
    if (path == EUL2_SINGLE) IBH_REQUIRE(ph.valid(), IBH_PHASES_EXCLUSIVE);
    else  // the other forms run the whole sweep: they have no overlap phases
        IBH_REQUIRE(!ph.any(), phase_msg);
    // the stamped and the thread-per-cell 3-D forms are HLL only: a variant must not quietly time another kernel
    IBH_REQUIRE(!(e.scheme == EULER_SENSOR && path == EUL3_SINGLE && T.quad_variant != 0),
                "ibh_residual_euler_sensor: quad_variant 4 (wave time stamps) and 512 (thread per cell) are forms of the "
                "HLL sweep only; set quad_variant 0");
    int rc = 0;
    switch (path) {
    case EUL2_SINGLE: euler2_single(p, e, flags, ph); break;
    case EUL3_IMAGE_COLS: euler3_image_cols(p, e); break;
    case EUL3_SINGLE: euler3_single(p, e); break;
    case EUL3_BLOCKS: rc = euler3_blocks(p, e, flags); break;
    default: rc = euler_general(p, e, flags, path);
    }
    if (!rc) IBH_LAUNCH_CHECK();
    return rc;
}

int ibh_residual_euler_hll(ibh_part* p, const float* P, int64_t ldp, float* R, int64_t ldr, const ibh_fluid* fluid,
                           int flags) {
    IBH_REQUIRE(p && P && R && fluid, "ibh_residual_euler_hll: null argument");
    return residual_euler(p, EulerArgs{P, ldp, R, ldr, fluid}, flags,
                          "ibh_residual_euler_hll: overlap phases need a partition whose (image) blocks are all "
                          "eligible for the single-kernel sweep; run the sweep unphased after the exchange");
}

// The same closure with CFD.inviscid_fluxes(fluid, PL, PR, at_owners(nu), at_neighbors(nu), dim) (cfd.jl:516-554) for the
// flux; nu = null: the pressure sensor D the sweep computes for MUSCL.  Same flags as ibh_residual_euler_hll.
int ibh_residual_euler_sensor(ibh_part* p, const float* P, int64_t ldp, const float* nu, float* R, int64_t ldr,
                              const ibh_fluid* fluid, int flags) {
    IBH_REQUIRE(p && P && R && fluid, "ibh_residual_euler_sensor: null argument");
    return residual_euler(p, EulerArgs{P, ldp, R, ldr, fluid, EULER_SENSOR, nu}, flags,
                          "ibh_residual_euler_sensor: overlap phases need a partition whose (image) blocks are all "
                          "eligible for the single-kernel sweep; run the sweep unphased after the exchange");
}

// The Euler step in its four forms (EulerForm), P_out = the form's update with R = R(P): what ibh_step_euler,
// ibh_stage_euler, ibh_stage_euler_ssp and ibh_stage_euler_dual share -- the checks, the one-launch condition and the
// two-launch tail.  `e` holds the
// entry's arguments (e.R is P_out; the step form's base state is P itself), `name` the entry for its messages.
// One launch where the 2-D single-kernel sweep takes the whole partition (EUL2_SINGLE without image / phase flags) and P_out
// != P: the sweep's store epilogue writes the form itself.  The step form also needs a global dt there; the stage forms load
// the cell's row of P0 anyway and its time step with it.  Everywhere else -- 3-D, face-list or mixed partitions,
// IBH_FORCE_GENERAL, IBH_NO_FUSE, P_out == P -- the sweep goes into `work` (nc x (nd + 2), leading dimension ldw) and the form's
// ibh_update_euler* runs: two launches.  Same bits either way.
static int euler_form(const char* name, ibh_part* p, int scheme, EulerArgs e, int dt_per_cell, float* work, int64_t ldw,
                      int flags) {
    const bool step = e.form == FORM_STEP, dual = e.form == FORM_DUAL;
    const char* const update = step ? "ibh_update_euler" : e.form == FORM_STAGE ? "ibh_update_euler_stage"
                               : dual ? "ibh_update_euler_dual" : "ibh_update_euler_ssp";
#define FORM_REQUIRE(cond, ...) IBH_REQUIRE(cond, (std::string(name) + __VA_ARGS__).c_str())  // (the text is built on failure only)
    FORM_REQUIRE(p && e.fluid && e.P && e.P0 && e.R && e.dt && (!dual || e.S), ": null argument");
    FORM_REQUIRE(scheme == EULER_HLL || scheme == EULER_SENSOR, ": scheme must be 0 (HLL) or 1 (sensor)");
    FORM_REQUIRE(!(flags & IBH_IMAGE_ONLY), ": IBH_IMAGE_ONLY is not taken: the update would read skirt rows that the sweep never "
                                            "wrote (the multi-GPU step is out of scope)");
    FORM_REQUIRE(!(flags & F_PHASES), ": the overlap phases IBH_PHASE_INTERIOR / IBH_PHASE_BOUNDARY are not taken: the update "
                                      "would read rows that the phase never wrote");
    FORM_REQUIRE(!(flags & (IBH_PASS_A_ONLY | IBH_PASS_B_ONLY)), ": a single pass of the sweep is no " + (step ? "step" : "stage"));
    FORM_REQUIRE(p->nd == 2 || p->nd == 3, ": nd must be 2 or 3");
    FORM_REQUIRE(e.ldp >= p->nc && e.ld0 >= p->nc && e.ldr >= p->nc, ": a leading dimension is smaller than the number of cells");
    FORM_REQUIRE(!work || (work != e.P && work != e.P0 && work != e.R && work != e.S),
                 ": work may not alias " + (step ? "P or P_out" : dual ? "P, P0, S or P_out" : "P, P0 or P_out"));
    if (dual) {
        FORM_REQUIRE(e.lds >= p->nc, ": lds is smaller than the number of cells");
        FORM_REQUIRE(e.g >= 0.0f && e.g <= FLT_MAX, ": g must be finite and >= 0");
        FORM_REQUIRE(e.S != e.R, ": S may not alias P_out");
    }
    if (p->nc == 0) return 0;
    e.scheme = scheme == EULER_SENSOR ? EULER_SENSOR : EULER_HLL;
    e.dt_cells = dt_per_cell != 0;
    if (euler_path(p, flags, e) == EUL2_SINGLE && p->fuse_all && !(step && e.dt_cells) && e.R != e.P) {
        euler2_single(p, e, flags, Phase(0));
        IBH_LAUNCH_CHECK();
        return 0;
    }
    FORM_REQUIRE(work, ": this partition / these arguments take the two-launch form (sweep into `work`, then " + update +
                           "): work must be nc x (nd + 2) floats");
    FORM_REQUIRE(ldw >= p->nc, ": ldw is smaller than the number of cells");
#undef FORM_REQUIRE
    const int rc = scheme == EULER_SENSOR ? ibh_residual_euler_sensor(p, e.P, e.ldp, nullptr, work, ldw, e.fluid, flags)
                                          : ibh_residual_euler_hll(p, e.P, e.ldp, work, ldw, e.fluid, flags);
    if (rc) return rc;
    if (step) return ibh_update_euler(e.fluid, p->nd, p->nc, e.P, e.ldp, work, ldw, e.dt, dt_per_cell, e.R, e.ldr);
    if (e.form == FORM_STAGE)
        return ibh_update_euler_stage(e.fluid, p->nd, p->nc, e.P0, e.ld0, work, ldw, e.dt, dt_per_cell, e.c, e.R, e.ldr);
    if (dual)
        return ibh_update_euler_dual(e.fluid, p->nd, p->nc, e.P0, e.ld0, work, ldw, e.S, e.lds, e.dt, dt_per_cell, e.c, e.g, e.R,
                                     e.ldr);
    return ibh_update_euler_ssp(e.fluid, p->nd, p->nc, e.P0, e.ld0, e.P, e.ldp, work, ldw, e.dt, dt_per_cell, e.a, e.b, e.c, e.R,
                                e.ldr);
}

// One explicit Euler step, P_out = state2primitive(primitive2state(P) + dt * R(P)): bit for bit ibh_update_euler(P,
// ibh_residual_euler_{hll,sensor}(P, flags), dt), in one launch or two (euler_form; a per-cell dt takes two).  A `work` that is
// given may alias neither P nor P_out on either path -- also on a one-launch partition, where `work` is not used: the shared
// body checks it before it knows the path.
int ibh_step_euler(ibh_part* p, const ibh_fluid* fluid, int scheme, const float* P, int64_t ldp, float* P_out, int64_t ldo,
                   const float* dt, int dt_per_cell, float* work, int64_t ldw, int flags) {
    EulerArgs e{P, ldp, P_out, ldo, fluid};
    e.form = FORM_STEP, e.dt = dt;
    e.P0 = P, e.ld0 = ldp;
    return euler_form("ibh_step_euler", p, scheme, e, dt_per_cell, work, ldw, flags);
}

// One Runge-Kutta stage of the low-storage family, P_out = state2primitive(primitive2state(P0) + (alpha * dt) * R(P)): the
// update works on the base state P0 of the step, the sweep on the previous stage P.  P_out may be P0 where P0 is not P.  Same
// bits as ibh_update_euler_stage(P0, R(P), dt, alpha) in one launch or two.
int ibh_stage_euler(ibh_part* p, const ibh_fluid* fluid, int scheme, const float* P, int64_t ldp, const float* P0, int64_t ld0,
                    float* P_out, int64_t ldo, const float* dt, int dt_per_cell, float alpha, float* work, int64_t ldw,
                    int flags) {
    EulerArgs e{P, ldp, P_out, ldo, fluid};
    e.form = FORM_STAGE, e.dt = dt;
    e.P0 = P0, e.ld0 = ld0, e.c = alpha;
    return euler_form("ibh_stage_euler", p, scheme, e, dt_per_cell, work, ldw, flags);
}

// One Shu-Osher stage of a strong-stability-preserving scheme, P_out = state2primitive((primitive2state(P0) * a +
// primitive2state(P) * b) + (c * dt) * R(P)): the sweep runs on the previous stage P, whose state also enters the blend (in one
// launch the sweep keeps the cell's own state).  Same bits as ibh_update_euler_ssp(P0, P, R(P), dt, a, b, c) in one launch or two.
int ibh_stage_euler_ssp(ibh_part* p, const ibh_fluid* fluid, int scheme, const float* P, int64_t ldp, const float* P0,
                        int64_t ld0, float* P_out, int64_t ldo, const float* dt, int dt_per_cell, float a, float b, float c,
                        float* work, int64_t ldw, int flags) {
    EulerArgs e{P, ldp, P_out, ldo, fluid};
    e.form = FORM_SSP, e.dt = dt;
    e.P0 = P0, e.ld0 = ld0, e.c = c, e.a = a, e.b = b;
    return euler_form("ibh_stage_euler_ssp", p, scheme, e, dt_per_cell, work, ldw, flags);
}

// One pseudo-time stage of a dual time step, P_out = state2primitive((primitive2state(P0) + (R(P) + S) * (alpha * dt)) / (1 +
// (alpha * dt) * g)): ibh_stage_euler with the physical time derivative g Q - S of the implicit step taken point-implicitly
// (S: ibh_dual_source, conserved variables, constant during the inner iterations).  P_out may be P0 where P0 is not P; S
// aliases neither P_out nor work.  Same bits as ibh_update_euler_dual(P0, R(P), S, dt, alpha, g) in one launch or two.
int ibh_stage_euler_dual(ibh_part* p, const ibh_fluid* fluid, int scheme, const float* P, int64_t ldp, const float* P0,
                         int64_t ld0, const float* S, int64_t lds, float* P_out, int64_t ldo, const float* dt, int dt_per_cell,
                         float alpha, float g, float* work, int64_t ldw, int flags) {
    EulerArgs e{P, ldp, P_out, ldo, fluid};
    e.form = FORM_DUAL, e.dt = dt;
    e.P0 = P0, e.ld0 = ld0, e.c = alpha;
    e.S = S, e.lds = lds, e.g = g;
    return euler_form("ibh_stage_euler_dual", p, scheme, e, dt_per_cell, work, ldw, flags);
}

// One step, u_out = u + dt * residual: in one launch where the quad sweep covers the whole partition (it stores the update,
// its cells of u are in registers), the sweep and the update one after the other elsewhere.
int ibh_step_advection(ibh_part* p, const float* u, float* u_out, const float* C, int64_t ldc, const float* dt_dev,
                       const ibh_bcset* bcs) {
    IBH_REQUIRE(p && u && u_out && C && dt_dev && u != u_out, "ibh_step_advection: null or aliased argument");
    if (p->nc == 0) return 0;
    int rc = 0;
    if (fused2(p, 0) && p->fuse_all && quads_usable(p, 0, 0) && p->n_dt == 0) {
        adv2_step_quads(p, u, u_out, C, ldc, dt_dev);
        IBH_LAUNCH_CHECK();
    } else {
        if ((rc = ibh_residual_advection(p, u, C, ldc, u_out, 0))) return rc;
        if ((rc = ibh_update_dev(p->nc, dt_dev, u, u_out, u_out))) return rc;
    }
    if (bcs) rc = ibh_bcset_apply(bcs, u_out);
    return rc;
}

// The step with the time step of the NEXT step evaluated beside its boundary conditions (ibh_bcset_apply_with_dt,
// ibh_timestep.hip): dt_next = scale * 0.5 / max(...) depends on C alone, so its two launches ride in the two launches of the BC
// set instead of standing in front of the next sweep.  dt_next may be dt_dev (the sweep has read it by then).
// (Tried and dropped: the partial maxima beside the SWEEP instead -- its workgroups then carry the sweep's 27 KB of LDS and
// its register budget, and the launch takes longer than the two side by side save: 26.8 against 26.1 us per step.)
int ibh_step_advection_dt(ibh_part* p, const float* u, float* u_out, const float* C, int64_t ldc, const float* dt_dev,
                          const ibh_bcset* bcs, float scale, float* dt_next) {
    IBH_REQUIRE(dt_next, "ibh_step_advection_dt: null dt_next");
    int rc = ibh_step_advection(p, u, u_out, C, ldc, dt_dev, nullptr);
    if (rc) return rc;
    if (bcs && bcs->ng > 0) return ibh_bcset_apply_with_dt(bcs, u_out, p, C, ldc, scale, dt_next, 0);
    return ibh_timestep_advection(p, C, ldc, scale, dt_next);
}

// pass A of the scalar sweep over field `uv`, written to `G` = [grad_1 .. grad_nd, sensor], each nc floats (velocity / output
// are not touched): `G` is the workspace for the duration of the call, so the partition's own is not even allocated
static int pass_A_into(ibh_part* p, const float* uv, float* G) {
    float* const own = p->G;
    p->G = G;
    const int rc = ibh_residual_advection(p, uv, uv, p->nc, G, IBH_PASS_A_ONLY | IBH_NO_FUSE);
    p->G = own;
    return rc;
}

// cell_gradient(part, u) -- the tuple form (ImmersedBoundary.jl:980-988): the gradients of `nv` fields along ALL
// dimensions in one sweep per field, and (optionally) the JST sensor of every field (JST_sensor(part, u), :1077-1097, the
// maximum over the dimensions).  On a block-structured partition this is pass A of the two-kernel sweeps (block kernels,
// face-list threads for the cells outside blocks; tuned arithmetic: reciprocal spacings, inside 5e-6 norm-wise of the
// operator-by-operator kernels); elsewhere it falls back to ibh_cell_gradient / ibh_jst_sensor per dimension.
//   out:    (nc, nd*nv) column-major, gradient of field v along dimension d in column d*nv + v
//   sensor: (nc, nv) or null
int ibh_cell_gradient_nd(ibh_part* p, const float* u, int nv, int64_t ldu, float* out, int64_t ldo, float* sensor,
                         int64_t lds) {
    IBH_REQUIRE(p && u && out && nv >= 1, "ibh_cell_gradient_nd: bad argument");
    if (p->nc == 0) return 0;
    const int nd = p->nd;
    if (!has_blocks(p)) {
        // no block structure (e.g. the coarse levels of multigrid()): every dimension in one face-list launch
        if (const int rc = ibh_cell_gradient_all(p, u, nv, ldu, out, ldo)) return rc;
        return sensor ? ibh_jst_sensor(p, 0, u, nv, ldu, sensor, lds) : 0;
    }
    // one field, gradients and sensor back to back: pass A writes them in place (no copy)
    if (nv == 1 && ldo == p->nc && sensor == out + (size_t)nd * ldo && lds == ldo) return pass_A_into(p, u, out);
    int rc = ensure_G(p);
    if (rc) return rc;
    for (int v = 0; v < nv; ++v) {
        const float* uv = u + (size_t)v * ldu;
        if ((rc = ibh_residual_advection(p, uv, uv, p->nc, p->G, IBH_PASS_A_ONLY | IBH_NO_FUSE))) return rc;
        for (int d = 0; d < nd; ++d)
            IBH_HIP(hipMemcpyAsync(out + (size_t)(d * nv + v) * ldo, p->G + (size_t)d * p->nc, sizeof(float) * p->nc,
                                   hipMemcpyDeviceToDevice, ibh_stream));
        if (sensor)
            IBH_HIP(hipMemcpyAsync(sensor + (size_t)v * lds, p->G + (size_t)nd * p->nc, sizeof(float) * p->nc,
                                   hipMemcpyDeviceToDevice, ibh_stream));
    }
    return 0;
}

// The same gradients FIELD by field: out is (nc, nv * (nd + 1)) column-major with leading dimension nc, the gradient of field
// v along dimension d in column v * (nd + 1) + d and the JST sensor of field v in column v * (nd + 1) + nd -- the layout pass A
// writes, so that on a block-structured partition every field's sweep writes in place (ibh_cell_gradient_nd copies nd
// columns per field out of the partition's workspace: 9 device-to-device copies for the velocity gradients of a 3-D
// closure, 0.3 ms of a configs[4] V-cycle at 7.9 M cells).  The gradient of all fields along d is the strided view
// out[:, d : nv * (nd + 1) : nd + 1] (leading dimension (nd + 1) * nc).
int ibh_cell_gradient_fields(ibh_part* p, const float* u, int nv, int64_t ldu, float* out) {
    IBH_REQUIRE(p && u && out && nv >= 1, "ibh_cell_gradient_fields: bad argument");
    if (p->nc == 0) return 0;
    const int nd = p->nd;
    for (int v = 0; v < nv; ++v) {
        const float* uv = u + (size_t)v * ldu;
        float* ov = out + (size_t)v * (nd + 1) * p->nc;
        int rc = has_blocks(p) ? pass_A_into(p, uv, ov) : ibh_cell_gradient_all(p, uv, 1, p->nc, ov, p->nc);
        if (!rc && !has_blocks(p)) rc = ibh_jst_sensor(p, 0, uv, 1, p->nc, ov + (size_t)nd * p->nc, p->nc);
        if (rc) return rc;
    }
    return 0;
}

}  // extern "C"

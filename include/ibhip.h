/*
 * libibhip -- C ABI of the MI355X (gfx950) residual hot path for
 * ImmersedBoundary.jl-style block-octree partitions.
 *
 * This header is the drop-in boundary.  The reference has no
 * FFI of its own: its plug-in hook is `conv_to_backend` / `to_backend`
 * (/root/reference/src/ImmersedBoundary.jl:846-855, src/arraybends.jl:14-77)
 * plus Julia multiple dispatch on the operators
 * (/root/reference/src/ImmersedBoundary.jl:873-1157).  Each entry point below
 * names the reference function it replaces; julia/IBHip.jl shows the `ccall`
 * binding a maintainer would add.
 *
 * Conventions
 *   - fields are Float32, column-major `(rows, nv)` with leading dimension
 *     `ld` (in elements): variable v of row i is `a[i + v*ld]`  (README.md:172);
 *   - `dim` is 1-based like the reference; `dim = 0` means "all dims" where
 *     the reference allows it (JST_sensor);
 *   - index arrays handed to the *_create functions are HOST pointers in the
 *     caller's base (`index_base` = 1 for Julia, 0 for C/Python); the library
 *     keeps its own device copies;
 *   - field pointers (`u`, `out`, ...) are DEVICE pointers (from ibh_malloc or
 *     any HIP allocation of the caller, e.g. a torch tensor's data_ptr);
 *   - every function returns 0 on success, a non-zero code otherwise and
 *     never throws; `ibh_last_error()` gives the message (thread-local);
 *   - kernels are launched on the stream given to `ibh_set_stream` (per host
 *     thread; default: the null stream) and are asynchronous.
 */
#ifndef IBHIP_H
#define IBHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ibh_part ibh_part; /* device-resident Partition  (ImmersedBoundary.jl:383-392) */
typedef struct ibh_acc ibh_acc;   /* device-resident Accumulator (accumulator.jl:12-16)        */
typedef struct ibh_bc ibh_bc;     /* device-resident Boundary    (ImmersedBoundary.jl:406-414) */

/* `Fluid` (cfd.jl:14-53).  The fused Euler residual uses R and gamma only; the transport
 * properties feed ibh_cfd_viscous_fluxes / dynamic_viscosity / heat_conductivity:
 * Sutherland's law with the reference's exponent 2/3 (cfd.jl:71-77) and k(T) = sum k[i]*T^i (:84-90). */
typedef struct ibh_fluid {
    float R;
    float gamma;
    float mu_ref;
    float Tref;
    float S;
    int32_t nk;   /* number of heat-conductivity coefficients, <= 4 */
    float k[4];
} ibh_fluid;

/* ---- runtime ---------------------------------------------------------- */
int ibh_init(int device);             /* hipSetDevice + sanity check that the device is gfx950 */
const char* ibh_last_error(void);
int ibh_set_stream(void* hip_stream); /* stream for subsequent calls of this host thread */
int ibh_sync(void);                   /* hipStreamSynchronize on that stream */
int ibh_version(void);

/* ---- memory (for hosts without their own HIP allocator, e.g. julia/IBHip.jl) */
int ibh_malloc(void** dptr, size_t bytes);
int ibh_free(void* dptr);
int ibh_h2d(void* dst, const void* src, size_t bytes);
int ibh_d2h(void* dst, const void* src, size_t bytes);
int ibh_memset(void* dst, int value, size_t bytes);
/* Device memory that the live handles of this process own (partitions, accumulators, boundaries, BC sets, domain plans --
 * the workspaces they allocate on first use included): bytes requested and number of buffers.  Every create adds to it,
 * a failed create leaves it as it was, every destroy takes its handle's share off again.  Exact, unlike hipMemGetInfo.
 * Not counted: ibh_malloc / ibh_free, the IPC and halo buffers, the per-thread reduction scratch.  Either pointer may be
 * NULL. */
int ibh_owned_device_memory(int64_t* bytes, int64_t* buffers);

/* ---- Partition: replaces `to_backend(part, conv)` (ImmersedBoundary.jl:848, :788) ----
 * Uploads once.  `spacing`/`centers` are `(nc, nd)` column-major (part.spacing,
 * part.centers).  For each dim d (0..nd-1): `nf[d]` faces with
 * `owners[d]`/`neighbors[d]` (part.face_owners_neighbors[dim]); left/right
 * incidence in CSR form (`*_off[d]` has nc+1 entries, `*_idx[d]` face ids in
 * the accumulator's stencil order) = part.face_accumulators[(dim,false/true)]
 * whose weights are 1/len (ImmersedBoundary.jl:501-506, :675-684).
 * `domain` = part.domain (global cell ids, sorted) and `block_size` let the
 * library recover the block structure for the block-structured fast path;
 * pass domain = NULL or block_size = 0 to disable it.
 */
int ibh_partition_create(ibh_part** out, int nd, int32_t nc,
                         const float* spacing, const float* centers,
                         const int32_t* nf,
                         const int32_t* const* owners, const int32_t* const* neighbors,
                         const int32_t* const* left_off, const int32_t* const* left_idx,
                         const int32_t* const* right_off, const int32_t* const* right_idx,
                         int32_t n_image, const int32_t* image_in_domain,
                         const int32_t* domain, int block_size, int index_base);
int ibh_partition_destroy(ibh_part* part);
/* Introspection of the block analysis: ibh_partition_info copies the first min(n, IBH_INFO_COUNT) of these values.
 *   FULL_BLOCKS            complete 8^nd blocks the block kernels take (0 without block information)
 *   IRREGULAR_CELLS        cells left to the face-list kernels (all of them without block information)
 *   SIDES_SAME .. GENERAL  block sides by class: same level, mirror (domain boundary), coarser, finer neighbour, anything else
 *   INTERIOR_BLOCKS        blocks whose whole sweep is independent of skirt cells (IBH_PHASE_INTERIOR)
 *   FUSABLE_BLOCKS         blocks eligible for the single-kernel sweep (3-D: all of them or none)
 *   WORKSPACE_BLOCKS       blocks whose gradients go through the workspace in a mixed launch (0 when every block is eligible)
 *   IMAGE_ALL_ELIGIBLE     1 when every image block is eligible (IBH_IMAGE_ONLY sweeps are then one launch per phase)
 *   IMAGE_BLOCKS           image blocks
 *   QUADS / RIM4_ROWS      one slot, 2-D / 3-D.  2-D: 2x2 block groups of the quad sweep when every block is eligible;
 *                          3-D: rim neighbours of halo cells that are four finer cells (single-kernel sweeps)
 *   QUAD_SINGLES           2-D: blocks outside the quads
 *   IMAGE_QUADS, IMAGE_QUAD_SINGLES  the same two among the image blocks (when they are all eligible and the rest is not)
 *   ROW_SWEEP              1 when the arithmetic halo ids of the row sweep reproduce the halo table
 *   DIRECT_SIDES           (dimension, side, cell) triples with exactly one face that names the cell where the CSR says
 *   QUAD_PAIRS             2-D: pair tiles among the blocks outside quads
 *   QUAD_ARITH_HALF_SIDES  2-D: outer half-sides of the quads (8 each) whose halo ids are computed, not read
 *   TILED                  1 when the cells are complete blocks in order: cell c is cell c % 8^nd of block c / 8^nd
 * The slots up to IBH_INFO_COUNT that have no name are zero. */
enum {
    IBH_INFO_FULL_BLOCKS = 0, IBH_INFO_IRREGULAR_CELLS = 1,
    IBH_INFO_SIDES_SAME = 2, IBH_INFO_SIDES_MIRROR = 3, IBH_INFO_SIDES_COARSE = 4, IBH_INFO_SIDES_FINE = 5,
    IBH_INFO_SIDES_GENERAL = 6,
    IBH_INFO_INTERIOR_BLOCKS = 7, IBH_INFO_FUSABLE_BLOCKS = 8, IBH_INFO_WORKSPACE_BLOCKS = 9,
    IBH_INFO_IMAGE_ALL_ELIGIBLE = 10, IBH_INFO_IMAGE_BLOCKS = 11,
    IBH_INFO_QUADS = 12, IBH_INFO_RIM4_ROWS = 12,   /* 2-D / 3-D */
    IBH_INFO_QUAD_SINGLES = 13, IBH_INFO_IMAGE_QUADS = 14, IBH_INFO_IMAGE_QUAD_SINGLES = 15,
    IBH_INFO_ROW_SWEEP = 16, IBH_INFO_DIRECT_SIDES = 17, IBH_INFO_QUAD_PAIRS = 18, IBH_INFO_QUAD_ARITH_HALF_SIDES = 19,
    IBH_INFO_TILED = 20,
    IBH_INFO_COUNT = 24
};
int ibh_partition_info(const ibh_part* part, int64_t* info, int n);

/* ---- Elementwise kernels: what `Base.Broadcast` on device arrays lowers to in the reference-side binding
 * (julia/IBHip.jl) -- the arithmetic a user closure writes between the operators, e.g.
 * `@. (uL + uR) * Cf / 2 + abs(Cf) * (uL - uR) / 2`, `ud .-= ...` (test/advection.jl:67-83), `max.(a, b)` and
 * `maximum(...)` (:52-59).  Fields are column-major (n, nv), contiguous.  An operand of ibh_ew_binary is a field of
 * the result's shape (nv* == nv), a column vector broadcast over the columns (nv* == 1) or a scalar (pointer NULL,
 * value s*).  `out` may alias an operand.  ibh_ew_reduce leaves its scalar on the device. */
enum { IBH_EW_ADD = 0, IBH_EW_SUB = 1, IBH_EW_MUL = 2, IBH_EW_DIV = 3, IBH_EW_MAX = 4, IBH_EW_MIN = 5, IBH_EW_SUM = 6 };
enum { IBH_EW_ABS = 16, IBH_EW_NEG = 17, IBH_EW_SQRT = 18, IBH_EW_COPY = 19 };
int ibh_ew_binary(int op, int64_t n, int nv, const float* a, int nva, float sa, const float* b, int nvb, float sb,
                  float* out);
int ibh_ew_unary(int op, int64_t total, const float* a, float* out);
int ibh_ew_fill(int64_t total, float value, float* out);
int ibh_ew_reduce(int op, int64_t total, const float* a, float* out_device);
/* A whole broadcast expression in ONE launch -- what Julia's broadcast fusion makes of
 * `@. (uL + uR) * Cf / 2 + abs(Cf) * (uL - uR) / 2` (test/advection.jl:76-80): a postfix program over up to 8 arrays
 * (fields (n, nv) or column vectors, nv* = 1) and 8 scalars; instruction = opcode | operand << 8 with opcodes
 * IBH_EW_ADD..MIN, IBH_EW_ABS..SQRT, IBH_EW_PUSH_ARRAY (operand = array index), IBH_EW_PUSH_SCALAR; at most 48
 * instructions, stack depth 8.  Every node is evaluated in Float32 exactly as the one-node kernels do (no contraction),
 * so the result equals the node-by-node evaluation bit for bit.  `out` may alias an array. */
enum { IBH_EW_PUSH_ARRAY = 32, IBH_EW_PUSH_SCALAR = 33 };
int ibh_ew_eval(int64_t n, int nv, int nprog, const int32_t* prog, int narr, const float* const* arrays,
                const int32_t* arr_nv, int nscal, const float* scalars, float* out);
/* The rest of Julia's elementwise Float32 math, also taken by ibh_ew_eval.  A program that uses any of these opcodes
 * (or more than 8 scalars) runs on an interpreter instantiation of its own, so the kernels of the opcodes above are
 * unchanged; its limits are 48 instructions, 8 arrays, 32 scalars and stack depth 8.  Bool values are Float32 0 / 1.
 *   binary   (a, b -> a OP b):  LT LE GT GE EQ NE (IEEE, Bool result), AND OR (Bool operands), POW (double pow,
 *            rounded once), COPYSIGN, ATAN2 (atan(a, b) in double), BMUL (a is a Bool: ifelse(a, b, copysign(0, b)))
 *   unary    EXP EXP2 LOG LOG2 LOG10 SIN COS TANH ATAN (in double, rounded once), SIGN (keeps +-0 and NaN),
 *            INV (1 / x), NOT (Bool), and Base.literal_pow: POW0 (= 1, also for NaN), SQR (x*x), CUBE ((x*x)*x),
 *            INVSQR ((1/x) * (1/x))
 *   ternary  (a, b, c): CLAMP (ifelse(a > c, c, ifelse(a < b, b, a)): NaN stays NaN), IFELSE (a != 0 ? b : c)
 *   IBH_EW_PUSH_ROW (operand = k): a row vector of nv values scalars[k .. k + nv - 1], value scalars[k + j] in column j
 *            (Julia's `u_inf'` broadcast down the rows of an (n, nv) field)
 * Rounded operations: NaN where Julia throws a DomainError (log of a negative number, a negative base under a
 * non-integer exponent). */
enum { IBH_EW_PUSH_ROW = 34 };
enum { IBH_EW_LT = 64, IBH_EW_LE = 65, IBH_EW_GT = 66, IBH_EW_GE = 67, IBH_EW_EQ = 68, IBH_EW_NE = 69, IBH_EW_AND = 70,
       IBH_EW_OR = 71, IBH_EW_POW = 72, IBH_EW_COPYSIGN = 73, IBH_EW_ATAN2 = 74, IBH_EW_BMUL = 75 };
enum { IBH_EW_EXP = 80, IBH_EW_EXP2 = 81, IBH_EW_LOG = 82, IBH_EW_LOG2 = 83, IBH_EW_LOG10 = 84, IBH_EW_SIN = 85,
       IBH_EW_COS = 86, IBH_EW_TANH = 87, IBH_EW_ATAN = 88, IBH_EW_SIGN = 89, IBH_EW_INV = 90, IBH_EW_NOT = 91,
       IBH_EW_POW0 = 92, IBH_EW_SQR = 93, IBH_EW_CUBE = 94, IBH_EW_INVSQR = 95 };
enum { IBH_EW_CLAMP = 112, IBH_EW_IFELSE = 113 };
/* `sum(a; dims = 2)` of a column-major (n, nv) field: out[i] = ((a[i, 1] + a[i, 2]) + a[i, 3]) + ..., the columns in
 * order as Julia adds them; one launch, no host sync.  `out` (n values) must not overlap `a` unless nv == 1. */
int ibh_ew_reduce_rows(int64_t n, int nv, const float* a, float* out);

/* Measurement switches of the kernels (A/B runs inside one process, no effect on results beyond rounding):
 *   "quad_variant"  kernel form of the single-kernel sweeps: 0 the default, 4 wave time stamps, 512 the thread-per-cell form
 *                   of the 3-D sweeps; any other value is an error and leaves the setting as it was
 *   "quad_parts" 1 / 2 only the quads / only the single blocks; "quad_singles_first" grid order; "quad_singles_iters"
 *   "rows" 1: the row sweep instead of the quad sweep; "rows_singles" -1 by size / 0 / 1 second launch / 2 inside the launch
 *   "pairs" 0: no pair tiles; "arith_ids" 0: halo ids from the table rows; "transport_blocks" 0: face-list transport kernel */
int ibh_set_tuning(const char* key, int value);
/* Wave timeline of the quad sweep (quad_variant 4): 8 x uint64 per wave {start, end (100 MHz ticks), HW_ID, is_quad, 4 phase stamps of a quad wave}. */
int ibh_debug_buffer(void* device_buffer);

/* Measurement probe (not on the product path): the launch of the 2-D quad sweep with the work stripped down.
 * mode 0 = dispatch only, 1 = + own-cell loads and the store (16 B per cell), 2 = + tables and halo gathers. */
int ibh_probe_sweep(ibh_part* part, const float* u, const float* C, int64_t ldc, float* ud, int mode);
/* Dispatch cost of an empty grid (measurement): nwg workgroups x threads, lds_bytes of LDS per workgroup. */
int ibh_probe_dispatch(int nwg, int threads, int lds_bytes);

/* Host-only view of the 2-D block analysis ibh_partition_create runs (block table, halo / end tables, the 2x2 block
 * groups of the quad sweep): same inputs, no device needed.  Test infrastructure for the library's host logic; not
 * part of the reference's surface.  ibh_host2d_get copies item `what` (of quad set `set`: 0 = all blocks, 1 = image
 * blocks) into dst (may be NULL to query *nbytes). */
typedef struct ibh_host2d ibh_host2d;
enum {
    IBH_H2D_BLOCKS = 0,    /* block descriptors, 120 bytes each (struct BlockDesc2 of csrc/ibh_common.h) */
    IBH_H2D_HTAB = 1,      /* int32 [nblk][64] halo cell ids */
    IBH_H2D_ETAB = 2,      /* int32 [nblk][16] side-end cell ids */
    IBH_H2D_FUSABLE = 3,   /* char  [nblk] eligible for the single-kernel sweep */
    IBH_H2D_QUAD_DESC = 4, /* {int32 base; uint32 cls; float rh[2]} per quad */
    IBH_H2D_QUAD_TAB = 5,  /* int32 [nq][160] */
    IBH_H2D_SINGLES = 6,   /* int32 block indices outside quads */
    IBH_H2D_COUNTS = 7,    /* int64 [8]: blocks, quads, interior quads, singles, interior singles, fuse_all, img_all_fz, nB1 */
    IBH_H2D_INFO = 8,      /* int64 [IBH_INFO_COUNT]: every slot of ibh_partition_info, as create would report it */
    IBH_H2D_PAIR_DESC = 9, /* pair tiles (two blocks side by side, base and base + 64) in the quad format; set 0 only */
    IBH_H2D_PAIR_TAB = 10, /* int32 [npair][160] */
    IBH_H2D_SINGLES2 = 11, /* int32 block indices outside quads and pairs */
    IBH_H2D_QUAD_AUX = 12, /* int32 [nq][40] companion rows: 32 end ids + 8 origins of arithmetic halo ids (or -1) */
    IBH_H2D_PAIR_AUX = 13  /* int32 [npair][40] */
};
int ibh_analyze2_host(ibh_host2d** out, int32_t nc, const float* spacing, const int32_t* nf,
                      const int32_t* const* owners, const int32_t* const* neighbors,
                      const int32_t* const* left_off, const int32_t* const* left_idx,
                      const int32_t* const* right_off, const int32_t* const* right_idx,
                      int32_t n_image, const int32_t* image_in_domain, const int32_t* domain, int index_base);
int ibh_host2d_get(const ibh_host2d* h, int what, int set, void* dst, int64_t cap_bytes, int64_t* nbytes);
int ibh_host2d_destroy(ibh_host2d* h);

/* ---- grid operators on a Partition (ImmersedBoundary.jl:873-1157) ----------
 * `u`: (nc, nv) cell field; `uf`: (nf_dim, nv) face field.  Outputs are new
 * arrays supplied by the caller (the reference returns fresh arrays).        */
int ibh_at_owners(const ibh_part*, int dim, const float* u, int nv, int64_t ldu, float* out, int64_t ldo);    /* :879 */
int ibh_at_neighbors(const ibh_part*, int dim, const float* u, int nv, int64_t ldu, float* out, int64_t ldo); /* :889 */
int ibh_at_faces(const ibh_part*, int dim, const float* u, int nv, int64_t ldu, float* out, int64_t ldo);     /* :899 */
int ibh_green_gauss(const ibh_part*, int dim, const float* uf, int nv, int64_t ldf, float* out, int64_t ldo,
                    int unsigned_sum);                                                                         /* :918, :934 */
int ibh_cell_gradient(const ibh_part*, int dim, const float* u, int nv, int64_t ldu, float* out, int64_t ldo); /* :965 */
/* every dimension in one face-list launch: out[(d * nv + v) * ldo + c] (what ibh_cell_gradient_nd calls on partitions
 * without the block structure) */
int ibh_cell_gradient_all(const ibh_part*, const float* u, int nv, int64_t ldu, float* out, int64_t ldo);
/* cell_gradient(part, u): the tuple form, src/ImmersedBoundary.jl:980-988 -- all dimensions in one sweep per field:
 * out (nc, nd*nv), gradient of field v along dimension d in column d*nv + v; sensor (nc, nv) or NULL: JST_sensor(part, u)
 * (:1077-1097, dim = 0) of every field for free.  Block-structured partitions: pass A of the two-kernel sweeps (tuned
 * arithmetic, inside 5e-6 norm-wise of ibh_cell_gradient / ibh_jst_sensor); others: those kernels, one dimension at a time.
 * With nv = 1, ldo = lds = nc and sensor = out + nd * nc (one (nc, nd + 1) buffer) the sweep writes in place: no copy. */
int ibh_cell_gradient_nd(ibh_part*, const float* u, int nv, int64_t ldu, float* out, int64_t ldo, float* sensor,
                         int64_t lds);
/* The same FIELD by field, every sweep in place (no copies): out (nc, nv * (nd + 1)), leading dimension nc -- gradient of field
 * v along dimension d in column v * (nd + 1) + d, JST sensor of field v in column v * (nd + 1) + nd; the gradients of all
 * fields along d are the strided view of columns d, d + (nd + 1), ... (leading dimension (nd + 1) * nc). */
int ibh_cell_gradient_fields(ibh_part*, const float* u, int nv, int64_t ldu, float* out);
int ibh_face_distance(const ibh_part*, int dim, float* out);     /* :995  */
int ibh_owner_distance(const ibh_part*, int dim, float* out);    /* :1010 */
int ibh_neighbor_distance(const ibh_part*, int dim, float* out); /* :1024 */
int ibh_face_gradient(const ibh_part*, int dim, const float* u, int nv, int64_t ldu, float* out, int64_t ldo); /* :1039 */
int ibh_jst_sensor(const ibh_part*, int dim, const float* p, int nv, int64_t ldp, float* out, int64_t ldo);    /* :1077 */
/* MUSCL(part,u,du,dim;D,high_order) :1113.  `D` may be NULL (no sensor blending). */
int ibh_muscl(const ibh_part*, int dim, const float* u, const float* du, int nv, int64_t ld,
              const float* D, int high_order, float* uL, float* uR, int64_t ldf);

/* ---- Accumulator (accumulator.jl:39-130): CSR form of the bucketed stencils ----
 * Row r sums `w[k]*v[idx[k]]` for k in [off[r], off[r+1]) in that order; `w` may
 * be NULL (unweighted).  Used for face incidence, BC image interpolation and
 * multigrid coarseners/prolongators (ImmersedBoundary.jl:1391-1392).           */
int ibh_acc_create(ibh_acc** out, int32_t n_output, int32_t n_input,
                   const int32_t* off, const int32_t* idx, const float* w, int index_base);
int ibh_acc_destroy(ibh_acc*);
int ibh_accumulate(const ibh_acc*, const float* v, int nv, int64_t ldv, float* out, int64_t ldo);
/* out .+= acc(v .- v2) in one launch (the prolongation step of FAS!, solver.jl:76: Q .+= prolong(Qc .- Qcold)); same
 * arithmetic as the three separate operations.  For 2..8 fields on a many-rows-per-donor operator (a prolongation) the donors'
 * differences are first packed side by side into a scratch buffer the accumulator allocates on its first such call (so: not
 * inside a stream capture the first time, and not from two host threads at once on the same accumulator). */
int ibh_accumulate_diff_add(const ibh_acc*, const float* v, const float* v2, int nv, int64_t ldv, float* out, int64_t ldo);

/* ---- ghost-cell BC: impose_bc! (ImmersedBoundary.jl:1197-1247) ----------------
 * Boundary data: ghost ids (global rows of `a`), image-point interpolator
 * already re-indexed to `image_domain` (Boundary ctor :436-447), and
 * eta = ghost_distances ./ image_distances (:1220).                             */
int ibh_bc_create(ibh_bc** out, int32_t n_ghost, const int32_t* ghost_indices,
                  const float* ghost_distances, const float* image_distances,
                  int32_t n_image_domain, const int32_t* image_domain,
                  const int32_t* interp_off, const int32_t* interp_idx, const float* interp_w,
                  int index_base);
int ibh_bc_destroy(ibh_bc*);
/* ia = image_interpolator(a[image_domain, :])  (:1228-1230); ia is (n_ghost, nv) */
int ibh_bc_interp(const ibh_bc*, const float* a, int nv, int64_t lda, float* ia, int64_t ldi);
/* a[ghost, :] = eta*ia + (1-eta)*ba (:1242-1245).  `ba` (n_ghost, nv), or NULL
 * to use the per-variable constants `ba_const[nv]` (closures returning a scalar,
 * test/advection.jl:34).                                                        */
int ibh_bc_blend(const ibh_bc*, float* a, int nv, int64_t lda, const float* ia, int64_t ldi,
                 const float* ba, int64_t ldb, const float* ba_const);
/* Fused interp + blend for the two closures the reference's tests use:
 * mode 0: Dirichlet constant  (ba = ba_const),  mode 1: copy / zero-gradient (ba = ia). */
int ibh_bc_apply(const ibh_bc*, float* a, int nv, int64_t lda, int mode, const float* ba_const);

/* ---- partition runtime: (dom::Domain)(f, args...) (ImmersedBoundary.jl:836-859) ----
 * gather: local[i,:] = global[domain[i],:]; scatter: global[image[j],:] = local[image_in_domain[j],:].
 * `rows` is a DEVICE index array (0-based) of length n.                          */
int ibh_gather_rows(const int32_t* rows, int32_t n, const float* src, int nv, int64_t lds, float* dst, int64_t ldd);
int ibh_scatter_rows(const int32_t* rows, int32_t n, const float* src, int nv, int64_t lds, float* dst, int64_t ldd);
/* dst[dst_rows[i],:] = src[src_rows[i],:] (halo unpack / image scatter) */
int ibh_copy_rows(const int32_t* dst_rows, const int32_t* src_rows, int32_t n,
                  const float* src, int nv, int64_t lds, float* dst, int64_t ldd);

/* ---- fused residual sweeps (the headline hot path) --------------------------------
 * ibh_residual_advection: exactly the closure of test/advection.jl:67-83,
 *     D = JST_sensor(part,u); per dim: Cf = at_faces(C[:,dim]); gu = cell_gradient(u,dim);
 *     uL,uR = MUSCL(u,gu,dim; D, high_order=true);
 *     ud -= green_gauss((uL+uR)*Cf/2 + |Cf|*(uL-uR)/2, dim)
 *   with ud starting from 0.  `C` is (nc, nd) with leading dimension ldc.
 * ibh_residual_euler_hll: R2 of SURVEY.md 8d composed from reference operators,
 *     D = JST_sensor(part,P[:,1]); per dim: gP = cell_gradient(P,dim);
 *     PL,PR = MUSCL(P,gP,dim; D, high_order=true); F = inviscid_fluxes(fluid,PL,PR,dim)
 *     (cfd.jl:459-508); R -= green_gauss(F,dim), R starting from 0;  P = [p T u v (w)].
 * ibh_residual_euler_sensor: the same closure with the second inviscid_fluxes method, the central flux with Rusanov
 *     dissipation scaled by sensors (cfd.jl:516-554), all Float32:
 *     F = inviscid_fluxes(fluid,PL,PR, at_owners(part,nu,dim), at_neighbors(part,nu,dim), dim)
 *     with `nu` nc values, or NULL for nu = D (the pressure sensor MUSCL uses).  One kernel per sweep where the HLL entry
 *     has one and nu is NULL (quad_variant must be 0 in 3-D); the literal face-list form through the gradient workspace
 *     wherever nu is given, with IBH_NO_FUSE / IBH_EXACT / IBH_FORCE_GENERAL, and on partitions whose blocks do not all
 *     qualify for a single-kernel sweep.  Same flags and phase rules as ibh_residual_euler_hll.
 *     D >= 1e-7 (JST_sensor starts its maximum there), so max(nuL,nuR) with nu = NULL is MUSCL's max(D_o,D_n,1e-7) exactly;
 *     a given nu has no floor (nu = 0 is the pure central flux) and a NaN in it stays a NaN, as through Julia's max.
 * flags: bit0 = force the general face-list kernels (no block fast path);
 *        bit1 = image cells only (skirt rows of the output are left untouched);
 *        bit2 / bit3 = run only pass A / only pass B of the two-kernel sweep.
 */
#define IBH_FORCE_GENERAL 1
#define IBH_IMAGE_ONLY 2
#define IBH_PASS_A_ONLY 4 /* launch only the gradient+sensor kernel (profiling / overlap staging) */
#define IBH_PASS_B_ONLY 8 /* launch only the flux kernel; the workspace must hold a current pass A */
#define IBH_PHASE_INTERIOR 32 /* only blocks that do not depend on skirt cells (run while the halo exchange is in flight) */
#define IBH_PHASE_BOUNDARY 64 /* the complement: remaining blocks + face-list cells (run after the exchange) */
#define IBH_NO_FUSE 128       /* keep the two-kernel form (gradient workspace) even where one kernel could do the sweep */
#define IBH_FORCE_MIXED 512    /* take the mixed launch (single kernel + two-kernel form) whatever the partition size */
#define IBH_SWEEP_ONLY 256     /* measurement: of a mixed launch run only the single-kernel part */
#define IBH_NO_QUAD 1024      /* A/B: per-block single kernel where the quad sweep (2x2 block groups per wavefront) would run */
#define IBH_EXACT 16      /* block fast path with the literal IEEE arithmetic (bit-comparable with the face-list path) */
int ibh_residual_advection(ibh_part*, const float* u, const float* C, int64_t ldc, float* ud, int flags);
/* n such sweeps launched back to back by one call (the step loop of a compiled host) */
int ibh_residual_advection_n(ibh_part*, const float* u, const float* C, int64_t ldc, float* ud, int flags, int n);
int ibh_residual_euler_hll(ibh_part*, const float* P, int64_t ldp, float* R, int64_t ldr,
                           const ibh_fluid* fluid, int flags);
int ibh_residual_euler_sensor(ibh_part*, const float* P, int64_t ldp, const float* nu /* nc values or NULL */,
                              float* R, int64_t ldr, const ibh_fluid* fluid, int flags);

/* ---- CFD pointwise physics that residual closures call (cfd.jl), rows of P are [p T u v (w)],
 * rows of Q are [rho E rho*u rho*v (rho*w)]; all arrays (n, nd+2) column-major, `dim` 1-based. ---- */
int ibh_cfd_speed_of_sound(const ibh_fluid*, int64_t n, const float* T, float* a);          /* cfd.jl:62-64  */
int ibh_cfd_dynamic_viscosity(const ibh_fluid*, int64_t n, const float* T, float* mu);      /* cfd.jl:71-77  */
int ibh_cfd_heat_conductivity(const ibh_fluid*, int64_t n, const float* T, float* k);       /* cfd.jl:84-90  */
int ibh_cfd_primitive2state(const ibh_fluid*, int nd, int64_t n, const float* P, int64_t ldp,
                            float* Q, int64_t ldq);                                          /* cfd.jl:106-123 */
int ibh_cfd_state2primitive(const ibh_fluid*, int nd, int64_t n, const float* Q, int64_t ldq,
                            float* P, int64_t ldp);                                          /* cfd.jl:137-151 */
/* HLL flux (cfd.jl:459-508).  The reference evaluates the last combine in Float64 (its `0.0`
 * literals) and returns Float64; here the combine is Float64 too and the result is rounded to Float32. */
int ibh_cfd_inviscid_fluxes_hll(const ibh_fluid*, int nd, int dim, int64_t n, const float* PL, const float* PR,
                                int64_t ld, float* F, int64_t ldf);
/* central flux + Rusanov dissipation scaled by sensors nuL/nuR (n) (cfd.jl:516-554) */
int ibh_cfd_inviscid_fluxes_sensor(const ibh_fluid*, int nd, int dim, int64_t n, const float* PL, const float* PR,
                                   int64_t ld, const float* nuL, const float* nuR, float* F, int64_t ldf);
/* viscous flux along Cartesian `dim` (cfd.jl:664-736): `Pgrad` = HOST array of nd DEVICE pointers, the
 * gradient of P along each axis, each (n, nd+2) with leading dimension ldg; mu_t per row or NULL (+ constant). */
/* CFD.JST_sensor(Pim1, Pi, Pip1) (cfd.jl:563-573), elementwise over `n` values, and CFD.shock_sensor (cfd.jl:575-617):
 * velocity_gradients[i * nd + j] = device array of d u_i / d x_j (n values each). */
int ibh_cfd_jst_sensor3(int64_t n, const float* Pim1, const float* Pi, const float* Pip1, float* out);
int ibh_cfd_shock_sensor(int nd, int64_t n, const float* const* velocity_gradients, float* out);
int ibh_cfd_viscous_fluxes(const ibh_fluid*, int nd, int dim, int64_t n, const float* P, int64_t ldp,
                           const float* const* Pgrad, int64_t ldg, const float* mu_t, float mu_t_const,
                           float* F, int64_t ldf);
/* The viscous part of a Navier-Stokes residual closure in ONE launch (round 4):
 *   R[:, 2:end] .+= sum_d green_gauss(part, viscous_fluxes(fluid, at_faces(part, P, d), face_gradient(part, P, gradP, d), d;
 *                                                          mu_t = at_faces(part, mu_t, d)), d)
 * (cfd.jl:664-736 over ImmersedBoundary.jl:899-926, 1039-1069; R[:, 1] gets the zero mass flux: untouched), operation by
 * operation in the composition's order: bit-identical to the twenty-odd operator launches per dimension it replaces.
 * Pgrad[d] = cell_gradient(part, P, d + 1), (nc, nd + 2) column-major with leading dimension ldg (grad_vel_col = 2), or the
 * gradients of the velocity columns only, (nc, nd) (grad_vel_col = 0: the gradients of p and T are not read -- the normal
 * derivative of T at a face is a face_gradient); mu_t: nc values (cells). */
int ibh_viscous_residual(const ibh_part*, const ibh_fluid*, const float* P, int64_t ldp, const float* const* Pgrad,
                         int64_t ldg, int grad_vel_col, const float* mu_t, float* R, int64_t ldr);

/* ---- direct peer halo exchange over xGMI ("or direct peer ... IPC writes") -------
 * Building blocks; the orchestration (who writes where) is host-side (halo.py / the Julia shim):
 *   - receive buffers and flag words are allocated fine-grained (coherent across devices), exported as
 *     64-byte HIP IPC handles, and mapped by the peers;
 *   - per sweep the sender packs with ibh_gather_rows straight INTO the peer's mapped receive buffer, then
 *     ibh_flag_signal bumps a sequence number in the peer's flag word (system-scope release);
 *   - the receiver runs ibh_flag_wait (bounded spin, never hangs: on timeout bit 0 of *status is set and
 *     the host falls back to the RCCL path) and unpacks with ibh_scatter_rows.
 * Everything is an ordinary kernel on the caller's stream, so whole sweeps incl. the exchange can be
 * captured in a HIP graph. */
int ibh_ipc_alloc(void** dptr, size_t bytes, int fine_grained);
int ibh_ipc_free(void* dptr);
int ibh_ipc_export(void* dptr, void* handle64);        /* hipIpcGetMemHandle: writes 64 bytes            */
int ibh_ipc_import(const void* handle64, void** dptr); /* hipIpcOpenMemHandle (lazy peer access)         */
int ibh_ipc_close(void* dptr);
/* seq = ++(*counter); *slots[q] = seq for q < n.  `counter` local device memory, `slots` DEVICE array of n
 * device pointers (into the peers' flag arrays). */
int ibh_flag_signal(uint32_t* counter, uint32_t* const* slots, int n);
/* exp = ++(*counter); wait until *slots[q] >= exp for every q < n, at most max_spins polls each. */
int ibh_flag_wait(uint32_t* counter, const uint32_t* const* slots, int n, uint32_t max_spins, uint32_t* status);
/* The whole exchange in two launches.  state = 5 device words {signal seq, wait seq, status, 0, 0}.
 * push: for every peer q the rows send_all[seg[q]..seg[q+1]) of f go to dst[q] as (n_q, nv) column-major, then the
 *   last workgroup to finish stores ++signal seq into flags[q] of every peer (system-scope release).
 * pull: waits (bounded by max_spins polls, time-out sets status bit 0) until every flags[q] >= wait seq + 1, then
 *   scatters src (the peers' blocks back to back, block q = (n_q, nv) column-major) to the rows recv_all[..] of f.
 * seg / dst / flags are host arrays, copied into the launch.  At most 16 peers. */
int ibh_halo_push(const float* f, int nv, int64_t ld, const int32_t* send_all, int n_peers, const int32_t* seg,
                  float* const* dst, uint32_t* const* flags, uint32_t* state);
int ibh_halo_pull(float* f, int nv, int64_t ld, const int32_t* recv_all, const float* src, int n_peers,
                  const int32_t* seg, const uint32_t* const* flags, uint32_t* state, uint32_t max_spins);
/* push + pull in ONE launch (the same two steps; ranks running it concurrently cannot block each other: the push part
 * waits for nothing).  Sends rows of f, receives into other rows of f.  dst0/dst1, src0/src1: the two parities of
 * the double buffer; which one a launch uses follows the device-side sequence number (state[0] & 1), so graph
 * replays and eager launches can be mixed. */
int ibh_halo_exchange(float* f, int nv, int64_t ld, const int32_t* send_all, int n_send_peers, const int32_t* send_seg,
                      float* const* dst0, float* const* dst1, uint32_t* const* send_flags, const int32_t* recv_all,
                      const float* src0, const float* src1, int n_recv_peers, const int32_t* recv_seg,
                      const uint32_t* const* recv_flags, uint32_t* state, uint32_t max_spins);
/* One step of a rank in ONE launch: ibh_halo_exchange of the scalar field u + the image-only quad sweep of
 * ibh_residual_advection(u, C) -> ud (test/advection.jl:67-83 on the rank's image cells).  The exchange workgroups run
 * beside the interior quads; a boundary wave waits (bounded by max_spins, time-out sets status bit 1) until the skirt rows
 * of ITS launch are unpacked: the overlap of exchange and interior compute that north_star asks for, without a second
 * stream.  fstate: 2 device uint64, zeroed once per exchanger.  Fails (no launch) on partitions whose image blocks are
 * not all eligible for the quad sweep; the caller then runs the two entry points one after the other. */
int ibh_step_advection_xgmi(ibh_part*, float* u, const float* C, int64_t ldc, float* ud, const int32_t* send_all,
                            int n_send_peers, const int32_t* send_seg, float* const* dst0, float* const* dst1,
                            uint32_t* const* send_flags, const int32_t* recv_all, const float* src0, const float* src1,
                            int n_recv_peers, const int32_t* recv_seg, const uint32_t* const* recv_flags,
                            uint32_t* state, uint32_t max_spins, unsigned long long* fstate);

/* ---- small device-resident vector ops for the FAS loop (solver.jl:79-88) ---------- */
/* q += clamp(omega,0,1) * r ; omega scalar */
/* ---- an explicit solver step, device resident (test/advection.jl:30-89: march! = dt, closure, u .+= ud .* dt, apply_bcs!)
 * ibh_bcset: an ordered list of impose_bc! calls (ImmersedBoundary.jl:1197-1247) whose closures the library knows --
 *   mode 0: `do bdry, u; value end`, mode 1: `do bdry, u; copy(u) end` (advection.jl:30-46) -- applied with the semantics
 *   of the sequential calls: boundaries that do not read each other's ghost cells form a level; a level is two launches
 *   (interpolate + closure + blend into a side buffer, then scatter) whatever the number of boundaries.
 * ibh_timestep_advection: dt = scale * 0.5 / maximum(max.(unsigned_green_gauss(at_faces(C_d, d), d)...)) (:52-59, :65)
 *   written to device memory; ibh_step_advection: u_out = u + dt * R(u) in ONE launch where the quad sweep applies (else
 *   sweep + update), then the boundary conditions on u_out.  u and u_out must not alias. */
typedef struct ibh_bcset ibh_bcset;
int ibh_bcset_create(ibh_bcset** out, int n_bc, const ibh_bc* const* bcs, const int32_t* modes, const float* values);
int ibh_bcset_destroy(ibh_bcset*);
/* n_ghost: ghost cells of all boundaries (never negative); n_levels: low 16 bits = levels, high 16 bits = levels none of
 * whose ghost cells is a donor of the level (one launch).  Host code only: no device call, no synchronisation. */
int ibh_bcset_info(const ibh_bcset*, int32_t* n_ghost, int32_t* n_levels);
int ibh_bcset_apply(const ibh_bcset*, float* a);
int ibh_timestep_advection(ibh_part*, const float* C, int64_t ldc, float scale, float* dt_device);
int ibh_update_dev(int64_t n, const float* dt_device, const float* u, const float* r, float* out);
int ibh_step_advection(ibh_part*, const float* u, float* u_out, const float* C, int64_t ldc, const float* dt_device,
                       const ibh_bcset* bcs /* or NULL */);
/* The same step with the time step of the NEXT one evaluated on the way: dt_next = ibh_timestep_advection(p, C, ldc, scale)
 * -- it depends on C alone -- computed by extra workgroups of the BC set's own launches (partial maxima beside the first,
 * final reduction beside the second) instead of two launches in front of the next sweep.  Results identical to the separate
 * calls; dt_next may alias dt_dev. */
int ibh_step_advection_dt(ibh_part* p, const float* u, float* u_out, const float* C, int64_t ldc, const float* dt_dev,
                          const ibh_bcset* bcs, float scale, float* dt_next);
/* ---- an explicit Euler step, device resident: what connects the fused Euler sweeps, impose_flow_bc and TimeAverage.push
 * into a time march without the host.  Rows of P are [p T u v (w)], rows of R [rho E rho*u rho*v (rho*w)] as the sweeps write.
 * ibh_timestep_euler: the advection script's CFL formula (advection.jl:52-59, :65) with the acoustic speed in place of C,
 *     C_d = abs(u_d) + sqrt(gamma R max(T, 10))   (ibh_cfd_speed_of_sound, then the IEEE broadcasts abs and +)
 *     dt = (0.5 / max_cells max_d unsigned_green_gauss(at_faces(C_d, d), d)) * scale        -> dt_device (1 float, or NULL)
 *     dt_cells[c] = (0.5 / max_d(...)[c]) * scale, the local time step of a pseudo-time march  -> dt_cells (nc, or NULL)
 *   bit for bit ibh_timestep_advection on the materialised C; no (nc, nd) array of wave speeds is written.  Two launches,
 *   one when only dt_cells is asked for; one of the two outputs must be given.
 * ibh_update_euler: P_out = state2primitive(primitive2state(P) + dt * R) in one launch, bit for bit ibh_cfd_primitive2state,
 *   ibh_update_dev per column and ibh_cfd_state2primitive.  dt: one device value, or n of them (dt_per_cell != 0).  P_out may
 *   be P (a row is read whole before it is written); R may alias neither.
 * ibh_step_euler: P_out = that update with R = ibh_residual_euler_hll / _sensor(P, flags) (scheme IBH_EULER_HLL /
 *   IBH_EULER_SENSOR, the pressure sensor).  ONE launch where the 2-D single-kernel sweep takes the whole partition (every
 *   block eligible, no face-list cells; by quads or, with IBH_NO_QUAD, per block), dt is global and P_out != P: the
 *   sweep stores the updated primitives itself.  Two launches everywhere else (3-D, face-list or mixed partitions, dt_per_cell,
 *   IBH_FORCE_GENERAL, IBH_NO_FUSE, IBH_EXACT, P_out == P): the sweep into `work`, nc x (nd + 2) floats with leading dimension
 *   ldw -- an argument check there, never an allocation -- then ibh_update_euler.  Same bits either way.  A `work` that is
 *   given may alias neither P nor P_out, whichever form runs.  IBH_IMAGE_ONLY and
 *   the overlap phases are rejected: the update would read rows the sweep never wrote (the multi-GPU step is out of scope).
 * Every misuse (null pointer, nd other than 2 or 3, a leading dimension below n, the aliasing above) is an error before any
 * launch. */
#define IBH_EULER_HLL 0
#define IBH_EULER_SENSOR 1
int ibh_timestep_euler(ibh_part*, const ibh_fluid*, const float* P, int64_t ldp, float scale,
                       float* dt_device /* 1 float, may be NULL */, float* dt_cells /* nc floats, may be NULL */);
int ibh_update_euler(const ibh_fluid*, int nd, int64_t n, const float* P, int64_t ldp, const float* R, int64_t ldr,
                     const float* dt, int dt_per_cell, float* P_out, int64_t ldo);
int ibh_step_euler(ibh_part*, const ibh_fluid*, int scheme /* IBH_EULER_HLL | IBH_EULER_SENSOR */, const float* P, int64_t ldp,
                   float* P_out, int64_t ldo, const float* dt, int dt_per_cell, float* work /* nc x (nd+2) or NULL */,
                   int64_t ldw, int flags);
/* ---- multi-stage (Runge-Kutta) steps of the low-storage family: stage k of m is
 *     P_k = state2primitive(primitive2state(P_0) + (alpha_k * dt) * R(P_{k-1})),   P_0 the step's input, P_m the new state;
 *   alpha_k = 1/(m-k+1) has the degree-m Taylor polynomial as its linear amplification factor, m = 1 is ibh_step_euler.
 * ibh_update_euler_stage: P_out = state2primitive(primitive2state(P0) + (alpha * dt) * R) in one launch, bit for bit
 *   ibh_update_euler(P0, R, dt .* alpha) with the Float32 product taken by the broadcast layer.  dt: one device value, or n of
 *   them (dt_per_cell != 0).  P_out may be P0; R may alias neither.
 * ibh_stage_euler: P_out = that update with R = ibh_residual_euler_hll / _sensor(P, flags); P is the previous stage, P0 the
 *   base state (they may be the same array).  ONE launch where the 2-D single-kernel sweep takes the whole partition and
 *   P_out != P -- with a global and with a per-cell dt, with P0 == P or not: the sweep loads the cell's row of P0 and its time
 *   step in its store epilogue.  Two launches everywhere else (3-D, face-list or mixed partitions, IBH_FORCE_GENERAL,
 *   IBH_NO_FUSE, IBH_EXACT, P_out == P): the sweep into `work` -- an argument check there, never an allocation -- then
 *   ibh_update_euler_stage.  Same bits either way.  P_out may be P0 when P0 is not P (a cell reads only its own row of P0,
 *   before it writes); work may alias none of P, P0, P_out.  IBH_IMAGE_ONLY, the overlap phases and the single-pass flags are
 *   rejected as by ibh_step_euler; every misuse is an error before any launch. */
int ibh_update_euler_stage(const ibh_fluid*, int nd, int64_t n, const float* P0, int64_t ld0, const float* R, int64_t ldr,
                           const float* dt, int dt_per_cell, float alpha, float* P_out, int64_t ldo);
int ibh_stage_euler(ibh_part*, const ibh_fluid*, int scheme /* IBH_EULER_HLL | IBH_EULER_SENSOR */, const float* P, int64_t ldp,
                    const float* P0, int64_t ld0, float* P_out, int64_t ldo, const float* dt, int dt_per_cell, float alpha,
                    float* work /* nc x (nd+2) or NULL */, int64_t ldw, int flags);
/* ---- Shu-Osher stages of the strong-stability-preserving Runge-Kutta schemes: a stage is a convex combination of the step's
 *   input P_0 and a forward-Euler step of the previous stage P,
 *     P_out = state2primitive((primitive2state(P0) * a + primitive2state(P) * b) + (c * dt) * R(P)),
 *   every product and sum rounded on its own, in this order; nothing is dropped for a == 0 or b == 0.
 *   SSPRK2: (a, b, c) = (0, 1, 1), (1/2, 1/2, 1/2); SSPRK3: (0, 1, 1), (3/4, 1/4, 1/4), (1/3, 2/3, 2/3).
 * ibh_update_euler_ssp: that update in one launch for a given R, bit for bit the composition primitive2state(P0),
 *   primitive2state(P), the broadcasts dt .* c and Q0 .* a .+ Q .* b, ibh_update_dev per column (per-cell dt: the broadcasts
 *   R .* dts and +), state2primitive.  dt: one device value, or n of them (dt_per_cell != 0).  P_out may be P0 or P, P0 may be
 *   P; R may alias none of them.  n == 0 launches nothing.
 * ibh_stage_euler_ssp: the update with R = ibh_residual_euler_hll / _sensor(P, flags).  ibh_stage_euler's dispatch: ONE launch
 *   where the 2-D single-kernel sweep takes the whole partition and P_out != P, with a global and with a per-cell dt (the
 *   sweep keeps the cell's own state and loads its row of P0 and its time step in its store epilogue); two launches
 *   everywhere else (3-D, face-list or mixed partitions, IBH_FORCE_GENERAL, IBH_NO_FUSE, IBH_EXACT, P_out == P): the sweep
 *   into `work` -- an argument check there, never an allocation -- then ibh_update_euler_ssp.  Same bits either way.  P_out
 *   may be P0 when P0 is not P; work may alias none of P, P0, P_out.  IBH_IMAGE_ONLY, the overlap phases and the single-pass
 *   flags are rejected as by ibh_stage_euler; every misuse is an error before any launch. */
int ibh_update_euler_ssp(const ibh_fluid*, int nd, int64_t n, const float* P0, int64_t ld0, const float* P, int64_t ldp,
                         const float* R, int64_t ldr, const float* dt, int dt_per_cell, float a, float b, float c,
                         float* P_out, int64_t ldo);
int ibh_stage_euler_ssp(ibh_part*, const ibh_fluid*, int scheme /* IBH_EULER_HLL | IBH_EULER_SENSOR */, const float* P,
                        int64_t ldp, const float* P0, int64_t ld0, float* P_out, int64_t ldo, const float* dt, int dt_per_cell,
                        float a, float b, float c, float* work /* nc x (nd+2) or NULL */, int64_t ldw, int flags);
/* ---- implicit residual smoothing (not in the reference): between the sweep and the update of a stage the residual R is
 *   replaced by n_iter Jacobi iterations on (I + eps L) S = R, L the unweighted Laplacian of the partition's face graph.
 *   With F(i) the faces of cell i -- dimensions ascending, in a dimension its left faces in list order (the cell across is the
 *   face's owner), then its right faces (the face's neighbour; a mirror face is across from i itself) -- and n_i = |F(i)|:
 *     S^m_i = (R_i + eps * sum_{f in F(i)} S^{m-1}_{across(f, i)}) / (1 + eps * float(n_i)),   S^0 = R,   m = 1 .. n_iter,
 *   per variable, the sum started from its first term and added in the order of F(i), every product, sum and the divide
 *   rounded on its own in Float32.  eps >= 0 is one value for all variables; eps = 0 returns R (a zero may change its sign).
 *   Ghost cells take part like any other cell.  The converged S keeps sum(S) = sum(R); a constant R is a fixed point.
 * ibh_smooth_residual: n_iter >= 1 iterations on the nv <= 8 columns of R, one launch each; the result lands in S.  tmp, the
 *   ping-pong partner of S, is required from n_iter = 2.  S and tmp may alias neither each other nor R.
 * ibh_update_euler_smoothed: ONE more iteration from (R, Sprev) inside the update, in one launch; the smoothed residual is
 *   never written.  blend = 0: ibh_update_euler_stage(P0, S, dt, c) -- P, a and b are ignored; blend = 1:
 *   ibh_update_euler_ssp(P0, P, S, dt, a, b, c).  Bit for bit ibh_smooth_residual(n_iter = 1 from Sprev) followed by that
 *   update.  Sprev == R is the only iteration.  P_out may be P0 or P; it may not be R or Sprev, which other cells
 *   gather.  A smoothed stage with n_iter iterations is the sweep, ibh_smooth_residual(n_iter - 1) and this: n_iter + 1
 *   launches.
 * Every misuse (null pointer, nd other than 2 or 3, nv outside 1 .. 8, a leading dimension below nc, eps negative or not
 * finite, n_iter < 1, a missing tmp, a partition without side table, the aliasing above) is an error before any launch; nc == 0
 * is no error and no launch. */
int ibh_smooth_residual(const ibh_part*, const float* R, int nv, int64_t ldr, float eps, int n_iter, float* S, int64_t lds,
                        float* tmp /* NULL for n_iter == 1 */, int64_t ldt);
int ibh_update_euler_smoothed(const ibh_part*, const ibh_fluid*, int blend /* 0 stage, 1 Shu-Osher */, const float* P0,
                              int64_t ld0, const float* P, int64_t ldp, const float* R, int64_t ldr, const float* Sprev,
                              int64_t lds, float eps, const float* dt, int dt_per_cell, float a, float b, float c,
                              float* P_out, int64_t ldo);
/* ---- dual time stepping (not in the reference): a physical step of size dt_real is the implicit backward-difference equation
 *     g * Q^{n+1} = R(P^{n+1}) + S,   S = cn * Q^n + cm * Q^{n-1},   Q = primitive2state(P), dQ/dt = R(P),
 *   BDF2: cn = 2/dt_real, cm = -0.5/dt_real, g = 1.5/dt_real; BDF1 (the first step): cn = g = 1/dt_real, no Q^{n-1}.  It is
 *   solved by a march in pseudo-time whose stage takes the g * Q term point-implicitly (Melson, Sanetrik and Atkins): with
 *   h = alpha * dt, dt the pseudo-time step (global or per cell),
 *     P_out = state2primitive((primitive2state(P0) + (R(P) + S) * h) / (1 + h * g)),
 *   every sum, product and the IEEE divide rounded on its own, in this order.  The fixed point P_out = P = P0 is the
 *   backward-difference equation whatever alpha and dt are; g = 0 with S = 0 gives ibh_update_euler_stage's values (a zero may
 *   change its sign).  The entries take any cn, cm, g: a variable dt_real is the caller's arithmetic.
 * ibh_dual_source: S = primitive2state(Pn) * cn + primitive2state(Pm) * cm in one launch, or primitive2state(Pn) * cn with Pm
 *   NULL (ldm and cm are then ignored); bit for bit primitive2state and the broadcasts.  S may alias neither state.
 * ibh_update_euler_dual: the update above in one launch for a given R, bit for bit the composition primitive2state(P0), the
 *   broadcasts R .+ S, dt .* alpha and h .* g .+ 1, ibh_update_dev per column (per-cell dt: the broadcasts * and +), the
 *   broadcast ./ and state2primitive.  dt: one device value, or n of them (dt_per_cell != 0).  P_out may be P0; R and S may
 *   alias neither each other nor P_out, R not P0.  n == 0 launches nothing.
 * ibh_stage_euler_dual: the update with R = ibh_residual_euler_hll / _sensor(P, flags).  ibh_stage_euler's dispatch: ONE launch
 *   where the 2-D single-kernel sweep takes the whole partition and P_out != P, with a global and with a per-cell dt (the
 *   sweep loads the cell's rows of P0 and of S and its time step in its store epilogue); two launches everywhere else (3-D,
 *   face-list or mixed partitions, IBH_FORCE_GENERAL, IBH_NO_FUSE, IBH_EXACT, P_out == P): the sweep into `work` -- an
 *   argument check there, never an allocation -- then ibh_update_euler_dual.  Same bits either way.  P_out may be P0 when P0 is
 *   not P; S may alias neither P_out nor work; work may alias none of P, P0, S, P_out.  IBH_IMAGE_ONLY, the overlap phases
 *   and the single-pass flags are rejected as by ibh_stage_euler.
 * Every misuse (null pointer, nd other than 2 or 3, a leading dimension below n, g negative or not finite, the aliasing above)
 * is an error before any launch. */
int ibh_dual_source(const ibh_fluid*, int nd, int64_t n, const float* Pn, int64_t ldn, const float* Pm /* NULL: BDF1 */,
                    int64_t ldm, float cn, float cm, float* S, int64_t lds);
int ibh_update_euler_dual(const ibh_fluid*, int nd, int64_t n, const float* P0, int64_t ld0, const float* R, int64_t ldr,
                          const float* S, int64_t lds, const float* dt, int dt_per_cell, float alpha, float g, float* P_out,
                          int64_t ldo);
int ibh_stage_euler_dual(ibh_part*, const ibh_fluid*, int scheme /* IBH_EULER_HLL | IBH_EULER_SENSOR */, const float* P,
                         int64_t ldp, const float* P0, int64_t ld0, const float* S, int64_t lds, float* P_out, int64_t ldo,
                         const float* dt, int dt_per_cell, float alpha, float g, float* work /* nc x (nd+2) or NULL */,
                         int64_t ldw, int flags);
/* ---- multigrid for the Euler march (not in the reference, whose FAS! hands its operators whatever columns it is given): the
 *   transfers between two levels in CONSERVED variables.  The coarsener and the prolongator are the Accumulators of
 *   multigrid(dom) (ibh_acc_create); their n_input / n_output are the row counts of the fine and the coarse arrays.  The
 *   stencil arithmetic is ibh_accumulate's -- t = x * w, the sum started from the first entry and added in entry order -- and
 *   the state arithmetic ibh_cfd_primitive2state's / ibh_cfd_state2primitive's, nothing contracted.
 * ibh_restrict_euler: P_c = state2primitive(coarsener(primitive2state(P_f))) and D_c = coarsener(R_f .+ S_f) -- S_f NULL:
 *   coarsener(R_f), ldsf ignored -- in ONE launch, one thread per coarse row; r + s is rounded before the multiply, as the
 *   broadcast does.  Bit for bit primitive2state, the broadcast +, ibh_accumulate twice and state2primitive.  R_f, S_f and D_c
 *   are in conserved variables; the coarse forcing of a full-approximation-scheme cycle is D_c .- R_c(P_c), the caller's
 *   broadcast.  P_c and D_c may overlap neither each other nor P_f, R_f, S_f.
 * ibh_prolong_euler: P_out = state2primitive(primitive2state(P_f) .+ prolongator(primitive2state(Pc_new) .-
 *   primitive2state(Pc_old))), the correction of a fine state by the change of the coarse one, in TWO launches: a pre-pass over
 *   the coarse rows writes pack[j][0 .. 7] = primitive2state(Pc_new[j]) - primitive2state(Pc_old[j]), zeros past nd + 2, then
 *   one thread per fine row takes each donor with two 16-byte gathers (a coarse row has ~4^nd readers: converting it inside
 *   the gather would repeat both conversions that often).  Bit for bit primitive2state three times,
 *   ibh_accumulate_diff_add and state2primitive.  pack: 8 * n_input floats of the caller's, 32-byte aligned, overlapping no
 *   state; Pc_new and Pc_old share ldc.  P_out may be P_f itself (a thread reads its row whole before it writes, and nobody
 *   else reads fine rows) and may overlap no other argument.
 * Every misuse (null pointer, nd other than 2 or 3, a leading dimension below the row count, pack missing or misaligned, the
 * aliasing above) is an error before any launch; an operator with zero output rows is no error and no launch. */
int ibh_restrict_euler(const ibh_acc* coarsener, const ibh_fluid*, int nd, const float* P_f, int64_t ldpf, const float* R_f,
                       int64_t ldrf, const float* S_f /* may be NULL */, int64_t ldsf, float* P_c, int64_t ldpc, float* D_c,
                       int64_t lddc);
int ibh_prolong_euler(const ibh_acc* prolongator, const ibh_fluid*, int nd, const float* Pc_new, const float* Pc_old,
                      int64_t ldc, float* pack /* n_input x 8 floats, 32-byte aligned */, const float* P_f, int64_t ldpf,
                      float* P_out, int64_t ldo);
/* ---- cell roles of an immersed-boundary march (not in the reference, which blanks nothing): one byte per row says what the
 *   row IS -- fluid, a ghost row of a boundary, or a solid row behind the ghost layer (cell_roles(dom) on the host).  Only
 *   fluid rows carry a defect, a forcing or a norm; every test below is a SELECT, so a NaN in a masked row stops there.
 * ibh_restrict_euler_roles: ibh_restrict_euler with D_c = coarsener(t), t_i = R_f[i] .+ S_f[i] (rounded; S_f NULL: R_f[i])
 *   where roles_f[i] == IBH_ROLE_FLUID and +0 elsewhere -- bit for bit ibh_restrict_euler on that t with S_f NULL.  P_c is
 *   ibh_restrict_euler's: the state of a masked row is restricted like any other.  One launch, one byte more per fine row.
 * ibh_forcing_roles: the coarse forcing in place, D[i] = D[i] - R[i] where roles[i] == IBH_ROLE_FLUID and +0 elsewhere, for
 *   the nv <= 8 columns of (n, nv) arrays, one launch: the broadcast D .- R and the select.  D overlaps neither R nor roles.
 * ibh_sumsq_roles: out[v] (device, double) = the sum of x[i, v]^2 over the rows with roles[i] == IBH_ROLE_FLUID, for the
 *   nv <= 8 columns in one launch and the one-launch final stage of ibh_sumsq; out is assigned, never added to.
 * Every misuse (null pointer, nd / nv out of range, a leading dimension below the row count, an output that overlaps an
 * input) is an error before any launch; zero rows are no error and no launch (ibh_sumsq_roles then leaves out as it was). */
#define IBH_ROLE_FLUID 0
#define IBH_ROLE_GHOST 1
#define IBH_ROLE_SOLID 2
int ibh_restrict_euler_roles(const ibh_acc* coarsener, const ibh_fluid*, int nd, const float* P_f, int64_t ldpf,
                             const float* R_f, int64_t ldrf, const float* S_f /* may be NULL */, int64_t ldsf,
                             const uint8_t* roles_f, float* P_c, int64_t ldpc, float* D_c, int64_t lddc);
int ibh_forcing_roles(int64_t n, int nv, float* D, int64_t ldd, const float* R, int64_t ldr, const uint8_t* roles);
int ibh_sumsq_roles(int64_t n, int nv, const float* x, int64_t ldx, const uint8_t* roles, double* out /* nv */);
int ibh_axpy_clamped(int64_t n, float omega, const float* r, float* q);
/* y = a*x + y */
int ibh_axpy(int64_t n, float a, const float* x, float* y);
/* *out (device, double) = sum(x^2) */
int ibh_sumsq(int64_t n, const float* x, double* out);
/* q += clamp(omega,0,1) * r and *out = sum(r^2) in one pass (solver.jl:82 + the norm of :84 on the same array) */
int ibh_axpy_clamped_sumsq(int64_t n, float omega, const float* r, float* q, double* out);
/* One pass of FAS! over a residual array (solver.jl:80-84): rr = r [+ source]; [q += clamp(omega,0,1) * rr]; [*out_sumsq =
 * sum(rr^2)] -- `r .+= source`, the update and the norm on one read of r; source, q and out_sumsq may each be NULL. */
int ibh_fas_update(int64_t n, float omega, const float* r, const float* source, float* q, double* out_sumsq);

/* push!(::CFD.TimeAverage, Q, dt) (cfd.jl:775-800), mu and sigma updated in place in one launch:
 *   eta = dt / tau;  sigma = sqrt(sigma^2 * (1 - eta) + (mu - Q)^2 * eta);  mu = mu * (1 - eta) + Q * eta
 * sigma from the old mu.  Q is (n, nv) with leading dimension ldq; mu and sigma are compact (n * nv), 16-byte aligned.
 * Precision P of eta (flags & IBH_TA_F64: Float64, else Float32) follows Julia's promotion: sigma^2, mu - Q and
 * (mu - Q)^2 stay Float32, everything with eta is in P, rounded to Float32 on store.  dt_form:
 *   IBH_TA_DT_HOST     eta (already dt / tau in P, computed by the caller) by value; dt unused
 *   IBH_TA_DT_DEVICE   dt: one device element (dt_numel == 1), read on the device -- no host sync
 *   IBH_TA_DT_PER_VAR  dt: nv device elements, one per variable (the reference's reshape along Q's last axis)
 *   IBH_TA_DT_ELEMENT  dt: device array of Q's shape with leading dimension ldd (dt_numel >= (nv-1)*ldd + n)
 * tau (in P) divides the device dt forms.  flags & IBH_TA_FIRST: the first registry, mu = Q and sigma = mu .* 0 (-0.0
 * where Q < 0, NaN where Q is not finite); dt, eta and tau are then ignored. */
#define IBH_TA_DT_HOST 0
#define IBH_TA_DT_DEVICE 1
#define IBH_TA_DT_PER_VAR 2
#define IBH_TA_DT_ELEMENT 3
#define IBH_TA_F64 1
#define IBH_TA_FIRST 2
int ibh_time_average_push(int64_t n, int nv, const float* Q, int64_t ldq, float* mu, float* sigma, int dt_form,
                          const float* dt, int64_t dt_numel, int64_t ldd, double eta, double tau, int flags);

/* ---- domain call on device-resident global arrays: `(dom::Domain)(f, args...)` (ImmersedBoundary.jl:820-864) ------
 * A plan holds the gather and scatter tables of all partitions of a Domain.  Per partition p (host arrays in
 * `index_base`): domain[p] (n_domain[p] global rows, part.domain), image[p] and image_in_domain[p] (n_image[p] entries:
 * part.image, part.image_in_domain).  Every index must be in range and the images disjoint (the scatter of all
 * partitions is one launch); images need not cover all n_global rows -- uncovered rows are left as they are.
 * The local arrays are stacked in ONE workspace per field: partition p's block starts at element nv * ws_off[p], where
 * ws_off[p] = sum over q < p of (n_domain[q] rounded up to 64) (256-byte boundaries), and is column-major
 * (n_domain[p], nv) with leading dimension n_domain[p].  A field of nv variables needs nv * ws_off[n_parts] elements.
 *   ibh_domain_gather   ws[k][block_p + v*n_p + i] = src[k][domain_p[i] + v*ld[k]]                 (:835-840)
 *   ibh_domain_scatter  dst[k][image_p[j] + v*ld[k]] = ws[k][block_p + v*n_p + image_in_domain_p[j]]  (:857-859)
 * one launch each for all partitions and up to IBH_DOM_MAXF fields (more fields: one launch per IBH_DOM_MAXF).
 * nfields, src/ws/dst (device pointers), nv and ld: host arrays of nfields entries.
 * ibh_domain_plan_info: ws_off[0 .. n_parts] (n = n_parts + 1). */
#define IBH_DOM_MAXF 8
typedef struct ibh_domain_plan ibh_domain_plan;
int ibh_domain_plan_create(ibh_domain_plan** out, int n_parts, const int32_t* const* domain, const int32_t* n_domain,
                           const int32_t* const* image, const int32_t* const* image_in_domain, const int32_t* n_image,
                           int64_t n_global, int index_base);
int ibh_domain_plan_destroy(ibh_domain_plan* plan);
int ibh_domain_plan_info(const ibh_domain_plan* plan, int64_t* ws_off, int n);
int ibh_domain_gather(const ibh_domain_plan* plan, int nfields, const float* const* src, const int* nv,
                      const int64_t* ld, float* const* ws);
int ibh_domain_scatter(const ibh_domain_plan* plan, int nfields, const float* const* ws, const int* nv,
                       const int64_t* ld, float* const* dst);

/* FlowBC call (cfd.jl:243-300): boundary state [p T u v (w)] from the image-point primitives P and the unit normals.
 * u_inf: nd components, or ONE component (the normal velocity) when normal_flow != 0.  image_distances / dudn: both
 * null or both given (wall-function slip scaling :287-292); transpiration: scalar, or per-row array when
 * transpiration_v != null.  Host array u_inf; everything else device. */
int ibh_cfd_flow_bc(const ibh_fluid* f, int nd, int64_t n, const float* P, int64_t ldp, const float* normals, int64_t ldn,
                    float p_inf, float T_inf, const float* u_inf, int normal_flow, const float* image_distances,
                    const float* dudn, float transpiration, const float* transpiration_v, float* out, int64_t ldo);

/* ---- turbulence closures (src/turbulence.jl), pointwise, Float32 ------------------------------------------------
 * params8 (host) = {kappa, C, A, beta, betastar, D, Aplus, omega_fixed_point}; velocity gradients g: host table of
 * nd*nd device pointers, g[i*nd + j] = d u_i / d x_j. */
/* wall_function(Rey) :27-70 -> y+, u+, mu+, k+, du+/dy+ */
int ibh_turb_wall_function_rey(int64_t n, const float* Rey, const float* params8, int n_iter, float* yplus, float* uplus,
                               float* muplus, float* kplus, float* dudy);
/* wall_function(y, u, nu) :72-100 -> u_tau, nu_t, k, omega, epsilon, du/dn */
int ibh_turb_wall_function(int64_t n, const float* y, const float* u, const float* nu, const float* params8, int n_iter,
                           float* utau, float* nut, float* k, float* omega, float* eps, float* dudn);
/* shear_rate :110-124 = sqrt(2 Sij Sij) */
int ibh_turb_shear_rate(int nd, int64_t n, const float* const* g, float* S);
/* Smagorinsky_nuSGS :135-138 = (Cs Delta)^2 S */
int ibh_turb_smagorinsky(int64_t n, const float* Delta, const float* S, float Cs, float* out);
/* standard_k-epsilon :176-196; params5 (host) = {Cmu, sigma_k, sigma_eps, C1eps, C2eps} */
int ibh_turb_k_epsilon(int64_t n, const float* k, const float* eps, const float* S, const float* params5, float* nuk,
                       float* nue, float* Sk, float* Se, float* nut);
/* Wray_Agarwal :222-241; gradR, gradS (n, nd) column-major */
int ibh_turb_wray_agarwal(int nd, int64_t n, const float* R, const float* S, const float* gradR, int64_t ldr,
                          const float* gradS, int64_t lds, float sigmaR, float C1, float kappa, float* nut, float* nuR,
                          float* Sout);
/* Ducros_sensor :252-282; WALE_nuSGS :291-337 (3-D only) */
/* transport of a scalar with variable diffusivity, all dimensions in one launch:
 *   out = S + sum_d green_gauss(at_faces(nu + nuR, d) .* face_gradient(R, d) .- at_faces(vel[:, d] .* R, d), d)
 * (the right-hand side a one-equation turbulence model such as Wray_Agarwal, turbulence.jl:222-241, is closed with):
 * the operator composition of ImmersedBoundary.jl:899-943, 1039-1043 evaluated face by face, bit-identical to calling the
 * operators one after the other. */
int ibh_scalar_transport(const ibh_part*, const float* R, const float* nuR, float nu, const float* vel, int64_t ldv,
                         const float* S, float* out);
/* On a 3-D partition made of complete 8^3 blocks (ibh_partition_info: full_blocks * 512 == nc, no face-list cells, no
 * GENERAL sides) or on a partition without block structure (full_blocks == 0: the coarse levels of multigrid()) -- an
 * error otherwise: compose the operators then -- the gradients consumed where they are made:
 *   S = shear_rate(cell_gradient(part, u), cell_gradient(part, v), cell_gradient(part, w))        turbulence.jl:110-124
 *   (nut, nuR, Sout) = Wray_Agarwal(R, S, cell_gradient(part, R), cell_gradient(part, S))          turbulence.jl:222-241
 * with the arithmetic of the tuple cell_gradient's block sweep (ibh_cell_gradient_nd) and of the pointwise kernels. */
int ibh_shear_rate_of_velocity(ibh_part*, const float* vel, int64_t ldv, float* S);
/* The same with the velocity gradients kept: G (nc, nd * nd), leading dimension ldg, d u_i / d x_j in column nd * j + i -- the
 * layout of the tuple cell_gradient (ibh_cell_gradient_nd), so that G + nd * j * ldg is `cell_gradient(part, vel)[j]` for
 * ibh_viscous_residual (grad_vel_col = 0): a Navier-Stokes closure with a turbulence model needs both, and the gradients
 * are made once.  G may be NULL (= ibh_shear_rate_of_velocity). */
int ibh_shear_rate_of_velocity_grad(ibh_part*, const float* vel, int64_t ldv, float* S, float* G, int64_t ldg);
int ibh_wray_agarwal_of(ibh_part*, const float* R, const float* S, float sigmaR, float C1, float kappa, float* nut,
                        float* nuR, float* Sout);
/* The LES closure of a velocity field with the gradients consumed where they are made, one launch on the partitions of
 * ibh_shear_rate_of_velocity_grad (an error otherwise: compose cell_gradient and the pointwise closures then).  With
 * g[i][j] = cell_gradient(part, u_i)[j]:
 *   nusgs  = Smagorinsky_nuSGS(Delta, shear_rate(g); Cs = Cmodel)   (model 1)            turbulence.jl:134-137
 *          = WALE_nuSGS(Delta, g; Cw = Cmodel)                      (model 2, 3-D only)  turbulence.jl:292-337
 *   ducros = Ducros_sensor(g)                                                            turbulence.jl:253-283
 *   shock  = CFD.shock_sensor(g)                                                         cfd.jl:589-617
 *   S      = shear_rate(g)                                                               turbulence.jl:110-124
 *   G      = the gradients, (nc, nd * nd) with leading dimension ldg, d u_i / d x_j in column nd * j + i
 * in the arithmetic of ibh_cell_gradient_nd and of the pointwise kernels (bit-identical to their composition).  model 0: no
 * eddy viscosity (nusgs must be NULL); every output may be NULL, at least one is not; Delta (nc) is read with a model only. */
int ibh_les_of(ibh_part*, const float* vel, int64_t ldv, const float* Delta, int model, float Cmodel, float* nusgs,
               float* ducros, float* shock, float* S, float* G, int64_t ldg);
/* The right-hand sides of the standard k-epsilon model (turbulence.jl:175-194) in ONE launch (dispatch as ibh_les_of):
 *   k_t   = -div(u k)   + div[(nu + nu_k)   grad k]   + S_k
 *   eps_t = -div(u eps) + div[(nu + nu_eps) grad eps] + S_eps
 * with g[i][j] = cell_gradient(part, vel_i)[j]:
 *   S    = shear_rate(g)                                                                       turbulence.jl:110-124
 *   (nuk, nue, Sk, Se, nut) = standard_kϵ(k, eps, S; params5...)                               turbulence.jl:175-194
 *   rk   = Sk + sum_d green_gauss(at_faces(nu + nuk, d) .* face_gradient(k, d)   .- at_faces(vel_d .* k, d),   d)
 *   reps = Se + sum_d green_gauss(at_faces(nu + nue, d) .* face_gradient(eps, d) .- at_faces(vel_d .* eps, d), d)
 *   G    = the gradients, (nc, nd * nd) with leading dimension ldg, d u_i / d x_j in column nd * j + i
 * bit-identical to ibh_shear_rate_of_velocity_grad, ibh_turb_k_epsilon and two ibh_scalar_transport; nuk, nue, Sk and Se are
 * never written (nut = Cmu k^2 / eps is pointwise: a neighbour's diffusivity is made from the neighbour's own k and eps).
 * params5 (host) = {Cmu, sigma_k, sigma_eps, C1eps, C2eps} as for ibh_turb_k_epsilon; nut, S and G may be NULL. */
int ibh_k_epsilon_rhs(ibh_part*, const float* vel, int64_t ldv, const float* k, const float* eps, float nu,
                      const float* params5, float* rk, float* reps, float* nut, float* S, float* G, int64_t ldg);
int ibh_turb_ducros(int nd, int64_t n, const float* const* g, float* out);
int ibh_turb_wale(int64_t n, const float* Delta, const float* const* g, float Cw, float* out);

/* ---- impose_bc! with a FlowBC closure in ONE launch (ImmersedBoundary.jl:1197-1247 over cfd.jl:243-300 and, on a wall,
 * turbulence.jl:72-98): what a solver script writes as
 *   impose_bc!(dom, bname, P, s...) do b, Pi, si...
 *       wf = wall_function(b.image_distances, |u_tangential|, mu(T) / rho)                 (wall_function != 0)
 *       bc(Pi, b.normals; du!dn = wf.du!dn, image_distances = b.image_distances, transpiration), values of s...
 *   end
 * for one Boundary: interpolation at the image points, the closure and the blend, per ghost cell, in the arithmetic of
 * ibh_bc_interp, ibh_cfd_dynamic_viscosity, ibh_turb_wall_function, ibh_cfd_flow_bc and ibh_bc_blend (bit-identical to
 * their composition with the glue evaluated left to right in Float32:
 *   rho = p / (R T), nu = mu(T) / rho, un = sum_j u_j n_j, t_j = u_j - un n_j, ut = sqrt(sum_j t_j^2)). */
typedef struct ibh_flow_bc_spec {
    int32_t normal_flow;     /* 0: Dirichlet state [p_inf T_inf u_inf[0..nd-1]]; 1: u_inf[0] is the normal velocity (slip wall) */
    float p_inf;
    float T_inf;
    float u_inf[3];
    float transpiration;     /* added to the normal velocity (normal_flow only), a constant */
    int32_t wall_function;   /* 0 or 1: du!dn (and the wall-function scalar modes) from wall_function(y, ut, nu) */
    float wall_params[8];    /* {kappa, C, A, beta, betastar, D, Aplus, omega_fixed_point} as for ibh_turb_wall_function */
    int32_t n_iter;
} ibh_flow_bc_spec;
/* boundary value of scalar field i: scalar_mode[i] = */
#define IBH_BC_SCALAR_CONST 0    /* scalar_value[i]                                   */
#define IBH_BC_SCALAR_COPY 1     /* the interpolated value (zero gradient)            */
#define IBH_BC_SCALAR_NUT 2      /* wall_function's nu_t  (needs wall_function != 0)  */
#define IBH_BC_SCALAR_K 3        /* ... k                                             */
#define IBH_BC_SCALAR_OMEGA 4    /* ... omega                                         */
#define IBH_BC_SCALAR_EPSILON 5  /* ... epsilon                                       */
/* P: (n, nd + 2) rows [p T u v (w)] of the global array, leading dimension ldp, ghost rows updated in place; normals
 * (n_ghost, nd) with leading dimension ldn and image_distances (n_ghost): device copies of the Boundary's; scalars: HOST
 * table of ns <= 4 DEVICE vectors (global rows, updated in place), scalar_mode / scalar_value: host arrays of ns.
 * *direct (ibh_bc_flow_info) = 1: no ghost cell of the boundary is a donor of its stencils, the launch writes the ghost cells
 * themselves and `staging` may be NULL; 0: every ghost cell is interpolated from the arrays as they were before any is
 * written, through `staging` (device, n_ghost * (nd + 2 + ns) floats) and a second launch that scatters it.
 * Every misuse is reported before anything is launched. */
int ibh_bc_flow_info(const ibh_bc*, int32_t* direct);
int ibh_bc_flow(const ibh_bc*, const ibh_fluid*, int nd, const float* normals, int64_t ldn, const float* image_distances,
                float* P, int64_t ldp, const ibh_flow_bc_spec* spec, int ns, float* const* scalars,
                const int32_t* scalar_mode, const float* scalar_value, float* staging);

/* ---- point-implicit smoother (reference: the orphan file src/point_implicit.jl) ------------------------------
 * Arrays are dense column-major (n points, nv variables) with leading dimension n, i.e. n*nv contiguous floats;
 * the block diagonal D is (n, nv, nv) column-major: D[p + n*(k + nv*i)] = d f_k / d x_i at point p (:56-91). */
/* z[i] = +1 / -1 from a counter-based hash of (seed, i)  (the Rademacher samples of :36-38) */
int ibh_pi_rademacher(int64_t n, uint64_t seed, float* z);
/* out = x + v*h  (:30, :112) */
int ibh_pi_perturb(int64_t n, const float* x, const float* v, float h, float* out);
/* out = (fxb - fx) / h : the Jacobian-vector product of a Linearization (:110-114) */
int ibh_pi_fd(int64_t n, const float* fxb, const float* fx, float h, float* out);
/* s[p,k] += z[p] * (fxb[p,k] - fx[p,k]) / h  (:40) */
int ibh_pi_hutch_accum(int64_t n, int nv, const float* fxb, const float* fx, const float* z, float h, float* s);
/* s /= d  (:43) */
int ibh_pi_div_scalar(int64_t n, float d, float* s);
/* in place: nv == 1: D = 1/(eps + D) (:124-126); else per-point Moore-Penrose inverse of the nv x nv block
 * (:127-135; one-sided Jacobi SVD, tolerance eps*nv*sigma_max like LinearAlgebra.pinv).  1 <= nv <= 8. */
int ibh_pi_invert_blocks(int64_t n, int nv, float* D);
/* out[p,k] = sum_i v[p,i] * invD[p,k,i]  (:153-161; nv == 1: out = v .* invD :141-146) */
int ibh_pi_apply_blocks(int64_t n, int nv, const float* invD, const float* v, float* out);
/* *out (device, double) = sum(a .* b);  *out (device, float) = maximum(abs, a).  Both are two-stage reductions without
 * atomics: the result of ibh_dot is reproducible -- the same input gives the same bits in every call. */
int ibh_dot(int64_t n, const float* a, const float* b, double* out);
int ibh_maxabs(int64_t n, const float* a, float* out);
/* alpha = dots[0] / (dots[1] + eps) read on the device; x += s*alpha; r -= As*alpha  (:229-236, :291-294) */
int ibh_pi_update(int64_t n, const double* dots, float eps, const float* s, const float* As, float* x, float* r);
/* s = r / (eps + *maxabs)  (:297-299) */
int ibh_pi_normalize(int64_t n, const float* r, const float* maxabs, float eps, float* s);

#ifdef __cplusplus
}
#endif
#endif /* IBHIP_H */

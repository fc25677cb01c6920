// libibhip: the transfers of a multigrid cycle of the Euler march, in conserved variables (not in the reference, whose FAS!
// applies its coarsener and prolongator to whatever columns it is handed):
//   * ibh_restrict_euler: P_c = state2primitive(coarsener(primitive2state(P_f))) and D_c = coarsener(R_f [.+ S_f]) in ONE
//     launch, one thread per coarse row.  Every fine row is a donor of one coarse row, so the rows of P_f, R_f and S_f are
//     read once each.
//   * ibh_prolong_euler: P_out = state2primitive(primitive2state(P_f) .+ prolongator(primitive2state(Pc_new) .-
//     primitive2state(Pc_old))) in TWO launches: a pre-pass over the coarse rows leaves the difference of the two conserved
//     states in `pack`, 8 floats per row (a coarse row is gathered by ~4^nd fine rows: converting inside the gather would
//     repeat both conversions that many times), then one thread per fine row takes a donor with two 16-byte gathers.
// Arithmetic: the row functions of ibh_euler_step_dev.h and the stencil sums of k_accumulate_rows / k_accumulate_packed_add
// (ibh_transfer.hip) -- the row walk of ibh_stencil_dev.h, which states the order -- without contraction: bit for bit the
// compositions of those launches.
// With cell roles (IBH_ROLE_*: one byte per fine row) the restricted defect takes fluid rows only:
//   * ibh_restrict_euler_roles: the same launch, D_c = coarsener(t) with t = R_f [.+ S_f] in fluid rows and +0 elsewhere -- a
//     select, so a NaN in a ghost or solid row never reaches D_c; P_c is ibh_restrict_euler's;
//   * ibh_forcing_roles: the coarse forcing D = D .- R in fluid rows, +0 elsewhere, in place, one launch.
#include <cstdint>

#include "ibh_common.h"
#include "ibh_euler_step_dev.h"
#include "ibh_stencil_dev.h"

#define MG_BLOCK 256

namespace {

using stencil_dev::Entries;
using stencil_dev::load1;
using stencil_dev::load4;

// N donors of a coarse row: their conserved states and residuals [plus sources] times their weights, added to sq and sd in
// entry order; `first`: entry 0 of these is the row's first and is assigned.  All gathers are issued before the arithmetic
// ROLES: the donor's role byte rides with its gathers, and a donor that is not fluid gives +0 to sd (never to sq)
template <int ND, bool SRC, bool ROLES, int N>
__device__ __forceinline__ void restrict_entries(float Rgas, float gamma, const Entries<N>& e, bool first,
                                                 const float* __restrict__ P, int64_t ldp, const float* __restrict__ R,
                                                 int64_t ldr, const float* __restrict__ S, int64_t lds,
                                                 const uint8_t* __restrict__ roles, float (&sq)[ND + 2],
                                                 float (&sd)[ND + 2]) {
    constexpr int NV = ND + 2;
    float Pr[N][NV], d[N][NV], s[N][NV];
    uint8_t role[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        if constexpr (ROLES) role[i] = roles[e.j[i]];
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            Pr[i][v] = P[e.j[i] + v * ldp];
            d[i][v] = R[e.j[i] + v * ldr];
            if constexpr (SRC) s[i][v] = S[e.j[i] + v * lds];
        }
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
        float Q[NV];
        euler_step::p2s_row<ND>(Rgas, gamma, Pr[i], Q);
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            float x = d[i][v];
            if constexpr (SRC) x = x + s[i][v];       // the broadcast R .+ S, rounded before the multiply
            if constexpr (ROLES) x = role[i] == IBH_ROLE_FLUID ? x : 0.0f;   // a select: a masked NaN stops here
            const float tq = Q[v] * e.w[i], td = x * e.w[i];
            sq[v] = (first && i == 0) ? tq : sq[v] + tq;
            sd[v] = (first && i == 0) ? td : sd[v] + td;
        }
    }
}

// One thread per coarse row.  P_c and D_c alias nothing the kernel reads (ibh_restrict_euler checks it)
template <int ND, bool SRC, bool ROLES>
__global__ __launch_bounds__(MG_BLOCK) void k_restrict_euler(float Rgas, float gamma, int32_t n_out,
                                                             const int32_t* __restrict__ off, const int32_t* __restrict__ idx,
                                                             const float* __restrict__ w, const float* __restrict__ P,
                                                             int64_t ldp, const float* __restrict__ R, int64_t ldr,
                                                             const float* __restrict__ S, int64_t lds,
                                                             const uint8_t* __restrict__ roles, float* __restrict__ Pc,
                                                             int64_t ldpc, float* __restrict__ Dc, int64_t lddc) {
    constexpr int NV = ND + 2;
    for (int64_t r = IBH_WG_X() * (int64_t)blockDim.x + threadIdx.x; r < n_out; r += (int64_t)gridDim.x * blockDim.x) {
        const int32_t b = off[r], e = off[r + 1];
        float sq[NV], sd[NV], o[NV];
#pragma unroll
        for (int v = 0; v < NV; ++v) sq[v] = sd[v] = 0.0f;   // (a row without entries: the sums of k_accumulate_rows)
        int32_t k = b;
        if ((b & 3) == 0)
            for (; k + 4 <= e; k += 4)
                restrict_entries<ND, SRC, ROLES, 4>(Rgas, gamma, load4(idx, w, k), k == b, P, ldp, R, ldr, S, lds, roles, sq,
                                                    sd);
        for (; k < e; ++k)
            restrict_entries<ND, SRC, ROLES, 1>(Rgas, gamma, load1(idx, w, k), k == b, P, ldp, R, ldr, S, lds, roles, sq, sd);
        euler_step::s2p_row<ND>(Rgas, gamma, sq, o);
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            Pc[r + v * ldpc] = o[v];
            Dc[r + v * lddc] = sd[v];
        }
    }
}

// The pre-pass of the prolongation, one thread per coarse row: pack[j][0 .. 7] = primitive2state(Pc_new[j]) -
// primitive2state(Pc_old[j]), zeros past nd + 2 (k_pack_diff8 on the two conserved states, which are never written)
template <int ND>
__global__ __launch_bounds__(MG_BLOCK) void k_pack_dq8(float Rgas, float gamma, int32_t n_in, const float* __restrict__ Pn,
                                                       const float* __restrict__ Po, int64_t ldc, float4* __restrict__ pack) {
    constexpr int NV = ND + 2;
    for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < n_in; j += (int64_t)gridDim.x * blockDim.x) {
        float a[NV], b[NV], Qa[NV], Qb[NV], d[8] = {};
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            a[v] = Pn[j + v * ldc];
            b[v] = Po[j + v * ldc];
        }
        euler_step::p2s_row<ND>(Rgas, gamma, a, Qa);
        euler_step::p2s_row<ND>(Rgas, gamma, b, Qb);
#pragma unroll
        for (int v = 0; v < NV; ++v) d[v] = Qa[v] - Qb[v];
        pack[2 * j] = float4{d[0], d[1], d[2], d[3]};
        pack[2 * j + 1] = float4{d[4], d[5], d[6], d[7]};
    }
}

// N donors of a fine row from the packed differences: two 16-byte gathers each (one for nd = 2), all issued first
template <int ND, int N>
__device__ __forceinline__ void prolong_entries(const Entries<N>& e, bool first, const float4* __restrict__ pack,
                                                float (&s)[ND + 2]) {
    constexpr int NV = ND + 2;
    float4 lo[N], hi[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        lo[i] = pack[2 * (int64_t)e.j[i]];
        if constexpr (NV > 4) hi[i] = pack[2 * (int64_t)e.j[i] + 1];
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const float x[5] = {lo[i].x, lo[i].y, lo[i].z, lo[i].w, NV > 4 ? hi[i].x : 0.0f};
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const float t = x[v] * e.w[i];
            s[v] = (first && i == 0) ? t : s[v] + t;
        }
    }
}

// One thread per fine row: its own row of P_f is read whole before the row of P_out is written, and no other thread reads
// fine rows, so P_out may be P_f (no __restrict__ on the two)
template <int ND>
__global__ __launch_bounds__(MG_BLOCK) void k_prolong_euler(float Rgas, float gamma, int32_t n_out,
                                                            const int32_t* __restrict__ off, const int32_t* __restrict__ idx,
                                                            const float* __restrict__ w, const float4* __restrict__ pack,
                                                            const float* Pf, int64_t ldpf, float* Pout, int64_t ldo) {
    constexpr int NV = ND + 2;
    for (int64_t r = IBH_WG_X() * (int64_t)blockDim.x + threadIdx.x; r < n_out; r += (int64_t)gridDim.x * blockDim.x) {
        const int32_t b = off[r], e = off[r + 1];
        float Pr[NV], Q[NV], s[NV], o[NV];
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            Pr[v] = Pf[r + v * ldpf];
            s[v] = 0.0f;
        }
        int32_t k = b;
        if ((b & 3) == 0)
            for (; k + 4 <= e; k += 4) prolong_entries<ND, 4>(load4(idx, w, k), k == b, pack, s);
        for (; k < e; ++k) prolong_entries<ND, 1>(load1(idx, w, k), k == b, pack, s);
        euler_step::p2s_row<ND>(Rgas, gamma, Pr, Q);
#pragma unroll
        for (int v = 0; v < NV; ++v) Q[v] = Q[v] + s[v];      // out .+= acc(a .- b)
        euler_step::s2p_row<ND>(Rgas, gamma, Q, o);
#pragma unroll
        for (int v = 0; v < NV; ++v) Pout[r + v * ldo] = o[v];
    }
}

// the bytes [lo, hi) of an (n, nv) array with leading dimension ld, and whether two such ranges meet
struct Span {
    uintptr_t lo, hi;
};
inline Span span_of(const void* p, int64_t n, int nv, int64_t ld) {
    const uintptr_t lo = (uintptr_t)p;
    return Span{lo, lo + sizeof(float) * (size_t)((int64_t)(nv - 1) * ld + n)};
}
inline bool meet(Span a, Span b) { return a.lo < b.hi && b.lo < a.hi; }

inline dim3 mg_grid(int64_t n) { return dim3(ibh_grid_cap(n, MG_BLOCK, 4096)); }

// the row kernel of an (n, nv) array against a role byte per row: D = D - R in fluid rows, +0 elsewhere
__global__ __launch_bounds__(MG_BLOCK) void k_forcing_roles(int64_t n, float* __restrict__ D, int64_t ldd,
                                                            const float* __restrict__ R, int64_t ldr,
                                                            const uint8_t* __restrict__ roles) {
    const int64_t v = blockIdx.y;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float x = D[i + v * ldd] - R[i + v * ldr];
        D[i + v * ldd] = roles[i] == IBH_ROLE_FLUID ? x : 0.0f;
    }
}

// ibh_restrict_euler and, with `roles`, ibh_restrict_euler_roles: one set of checks, said in the name of the entry `who`
int restrict_euler(const char* who, const ibh_acc* c, const ibh_fluid* f, int nd, const float* P_f, int64_t ldpf,
                   const float* R_f, int64_t ldrf, const float* S_f, int64_t ldsf, const uint8_t* roles, float* P_c,
                   int64_t ldpc, float* D_c, int64_t lddc) {
    const std::string w(who);
#define REQUIRE(cond, msg) IBH_REQUIRE(cond, (w + msg).c_str())
    REQUIRE(c && f && P_f && R_f && P_c && D_c, ": null argument");
    REQUIRE(nd == 2 || nd == 3, ": nd must be 2 or 3");
    const int64_t nf = c->n_in, ncr = c->n_out;
    const int nv = nd + 2;
    REQUIRE(ldpf >= nf && ldrf >= nf && (!S_f || ldsf >= nf),
            ": a leading dimension of the fine arrays is smaller than the coarsener's n_input");
    REQUIRE(ldpc >= ncr && lddc >= ncr,
            ": a leading dimension of the coarse arrays is smaller than the coarsener's n_output");
    const Span pc = span_of(P_c, ncr, nv, ldpc), dc = span_of(D_c, ncr, nv, lddc);
    REQUIRE(!meet(pc, dc), ": D_c may not alias P_c");
    const Span in[3] = {span_of(P_f, nf, nv, ldpf), span_of(R_f, nf, nv, ldrf), span_of(S_f, nf, nv, ldsf)};
    for (int i = 0; i < (S_f ? 3 : 2); ++i)
        REQUIRE(!meet(pc, in[i]) && !meet(dc, in[i]), ": P_c and D_c may not alias P_f, R_f or S_f");
    if (roles) {
        const Span rl{(uintptr_t)roles, (uintptr_t)roles + (size_t)nf};
        REQUIRE(!meet(pc, rl) && !meet(dc, rl), ": P_c and D_c may not alias roles_f");
    }
#undef REQUIRE
    if (ncr == 0) return 0;
    const dim3 grid = mg_grid(ncr), block(MG_BLOCK);
#define RESTRICT_LAUNCH(ND, SRC, ROLES)                                                                                 \
    hipLaunchKernelGGL((k_restrict_euler<ND, SRC, ROLES>), grid, block, 0, ibh_stream, f->R, f->gamma, c->n_out, c->off, \
                       c->idx, c->w, P_f, ldpf, R_f, ldrf, S_f, ldsf, roles, P_c, ldpc, D_c, lddc)
#define RESTRICT_SRC(ND, ROLES)                    \
    do {                                           \
        if (S_f) RESTRICT_LAUNCH(ND, true, ROLES); \
        else RESTRICT_LAUNCH(ND, false, ROLES);    \
    } while (0)
    if (nd == 2) {
        if (roles) RESTRICT_SRC(2, true);
        else RESTRICT_SRC(2, false);
    } else {
        if (roles) RESTRICT_SRC(3, true);
        else RESTRICT_SRC(3, false);
    }
#undef RESTRICT_SRC
#undef RESTRICT_LAUNCH
    IBH_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" {

int ibh_restrict_euler(const ibh_acc* c, const ibh_fluid* f, int nd, const float* P_f, int64_t ldpf, const float* R_f,
                       int64_t ldrf, const float* S_f, int64_t ldsf, float* P_c, int64_t ldpc, float* D_c, int64_t lddc) {
    return restrict_euler("ibh_restrict_euler", c, f, nd, P_f, ldpf, R_f, ldrf, S_f, ldsf, nullptr, P_c, ldpc, D_c, lddc);
}

int ibh_restrict_euler_roles(const ibh_acc* c, const ibh_fluid* f, int nd, const float* P_f, int64_t ldpf, const float* R_f,
                             int64_t ldrf, const float* S_f, int64_t ldsf, const uint8_t* roles_f, float* P_c, int64_t ldpc,
                             float* D_c, int64_t lddc) {
    IBH_REQUIRE(roles_f, "ibh_restrict_euler_roles: null argument");
    return restrict_euler("ibh_restrict_euler_roles", c, f, nd, P_f, ldpf, R_f, ldrf, S_f, ldsf, roles_f, P_c, ldpc, D_c,
                          lddc);
}

int ibh_forcing_roles(int64_t n, int nv, float* D, int64_t ldd, const float* R, int64_t ldr, const uint8_t* roles) {
    IBH_REQUIRE(D && R && roles, "ibh_forcing_roles: null argument");
    IBH_REQUIRE(n >= 0 && nv >= 1 && nv <= 8, "ibh_forcing_roles: n must be >= 0 and nv in 1 .. 8");
    IBH_REQUIRE(ldd >= n && ldr >= n, "ibh_forcing_roles: a leading dimension is smaller than n");
    const Span d = span_of(D, n, nv, ldd), r = span_of(R, n, nv, ldr), rl{(uintptr_t)roles, (uintptr_t)roles + (size_t)n};
    IBH_REQUIRE(n == 0 || (!meet(d, r) && !meet(d, rl)), "ibh_forcing_roles: D may not alias R or roles");
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_forcing_roles, dim3(ibh_grid_cap(n, MG_BLOCK, 4096), nv), dim3(MG_BLOCK), 0, ibh_stream, n, D, ldd, R,
                       ldr, roles);
    IBH_LAUNCH_CHECK();
    return 0;
}

int ibh_prolong_euler(const ibh_acc* p, const ibh_fluid* f, int nd, const float* Pc_new, const float* Pc_old, int64_t ldc,
                      float* pack, const float* P_f, int64_t ldpf, float* P_out, int64_t ldo) {
    IBH_REQUIRE(p && f && Pc_new && Pc_old && P_f && P_out, "ibh_prolong_euler: null argument");
    IBH_REQUIRE(nd == 2 || nd == 3, "ibh_prolong_euler: nd must be 2 or 3");
    IBH_REQUIRE(pack && ((uintptr_t)pack & 31) == 0, "ibh_prolong_euler: pack is missing or not 32-byte aligned");
    const int64_t nf = p->n_out, ncr = p->n_in;
    const int nv = nd + 2;
    IBH_REQUIRE(ldc >= ncr, "ibh_prolong_euler: the leading dimension of the coarse arrays is smaller than the prolongator's "
                            "n_input");
    IBH_REQUIRE(ldpf >= nf && ldo >= nf,
                "ibh_prolong_euler: a leading dimension of the fine arrays is smaller than the prolongator's n_output");
    const Span out = span_of(P_out, nf, nv, ldo), pk = span_of(pack, ncr * 8, 1, ncr * 8), pf = span_of(P_f, nf, nv, ldpf);
    const Span cn = span_of(Pc_new, ncr, nv, ldc), co = span_of(Pc_old, ncr, nv, ldc);
    IBH_REQUIRE(!meet(pk, out) && !meet(pk, pf) && !meet(pk, cn) && !meet(pk, co),
                "ibh_prolong_euler: pack may not alias a state");
    IBH_REQUIRE(!meet(out, cn) && !meet(out, co), "ibh_prolong_euler: P_out may not alias Pc_new or Pc_old");
    IBH_REQUIRE((P_out == P_f && ldo == ldpf) || !meet(out, pf),
                "ibh_prolong_euler: P_out may be P_f itself, with its leading dimension, and may not overlap it otherwise");
    if (nf == 0) return 0;
    float4* pack4 = reinterpret_cast<float4*>(pack);
    if (ncr > 0) {
        auto k = nd == 2 ? k_pack_dq8<2> : k_pack_dq8<3>;
        hipLaunchKernelGGL(k, dim3(ibh_grid_cap(ncr, MG_BLOCK, 2048)), dim3(MG_BLOCK), 0, ibh_stream, f->R, f->gamma, p->n_in,
                           Pc_new, Pc_old, ldc, pack4);
    }
    auto k = nd == 2 ? k_prolong_euler<2> : k_prolong_euler<3>;
    hipLaunchKernelGGL(k, mg_grid(nf), dim3(MG_BLOCK), 0, ibh_stream, f->R, f->gamma, p->n_out, p->off, p->idx, p->w, pack4,
                       P_f, ldpf, P_out, ldo);
    IBH_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"

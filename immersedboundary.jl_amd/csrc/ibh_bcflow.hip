// libibhip: impose_bc! with a FlowBC closure -- and, on a wall, wall_function(y, u, nu) at the image points -- as ONE launch per
// Boundary (ImmersedBoundary.jl:1197-1247 over cfd.jl:243-300 and turbulence.jl:72-98): one thread per ghost cell walks its
// interpolation row once for the nd + 2 primitives and up to 4 scalar fields, evaluates the closure and blends.  The device
// bodies are those of the kernels the composition launches (ibh_flowbc_dev.h, ibh_wall_dev.h; the row sum in the order of
// ibh_stencil_dev.h, that of k_accumulate / k_accumulate_rows; the blend of k_bc_blend), evaluated without contraction: the result is the composition's
// bit for bit.
#include <algorithm>

#include "ibh_bcset_dev.h"
#include "ibh_common.h"
#include "ibh_flowbc_dev.h"
#include "ibh_wall_dev.h"

namespace {

constexpr int BCF_BLOCK = 256;
constexpr int BCF_GRID_CAP = 4096;   // workgroups of the grid-stride launches
constexpr int BCF_MAXS = 4;

struct BcFlowArgs {
    int32_t ng;
    const int32_t *off, *idx, *remap, *ghost;
    const float *w, *eta, *nrm, *imd;
    int64_t ldn, ldp;
    float* P;
    ibh_fluid f;
    float pinf, Tinf, uinf[3], transp;
    int32_t normal_flow;
    wall_dev::WallParams wp;
    int32_t ns;
    float* S[BCF_MAXS];
    int32_t mode[BCF_MAXS];
    float value[BCF_MAXS];
    float* staging;   // null: the ghost cells themselves
};

// (P and the scalars are read at the donors and -- without staging -- written at the ghost cells by the same launch: no
// __restrict__ on them; the host has checked that no ghost cell is a donor then)
template <int ND, bool WF>
__global__ __launch_bounds__(BCF_BLOCK) void k_bc_flow(BcFlowArgs A) {
    constexpr int NP = ND + 2, NF = NP + BCF_MAXS;
    const int ns = A.ns;
    const float* fld[NF];
#pragma unroll
    for (int q = 0; q < NP; ++q) fld[q] = A.P + (int64_t)q * A.ldp;
#pragma unroll
    for (int q = 0; q < BCF_MAXS; ++q) fld[NP + q] = A.S[q];
    const int nf = NP + ns;
    for (int64_t g = IBH_WG_X() * (int64_t)blockDim.x + threadIdx.x; g < A.ng; g += (int64_t)gridDim.x * blockDim.x) {
        // 1. the row of the image-point interpolator, indices and weights read once for all fields; per field the sum of
        // k_accumulate_rows (the order of ibh_stencil_dev.h): entries in CSR order, the first term assigned
        const int32_t b = A.off[g], e = A.off[g + 1];
        float s[NF];
#pragma unroll
        for (int q = 0; q < NF; ++q) s[q] = 0.0f;
        int32_t k = b;
        if ((b & 3) == 0)
            for (; k + 4 <= e; k += 4) {
                const int4 j4 = *reinterpret_cast<const int4*>(A.idx + k);
                const float4 w4 = *reinterpret_cast<const float4*>(A.w + k);
                const int32_t jj[4] = {A.remap[j4.x], A.remap[j4.y], A.remap[j4.z], A.remap[j4.w]};
                const float ww[4] = {w4.x, w4.y, w4.z, w4.w};
                float x[4][NF];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int q = 0; q < NF; ++q)
                        if (q < nf) x[i][q] = fld[q][jj[i]];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int q = 0; q < NF; ++q)
                        if (q < nf) {
                            const float t = x[i][q] * ww[i];
                            s[q] = (k + i == b) ? t : s[q] + t;
                        }
            }
        for (; k < e; ++k) {
            const int32_t j = A.remap[A.idx[k]];
            const float wk = A.w[k];
#pragma unroll
            for (int q = 0; q < NF; ++q)
                if (q < nf) {
                    const float t = fld[q][j] * wk;
                    s[q] = (k == b) ? t : s[q] + t;
                }
        }
        const float p = s[0], T = s[1];
        float u[ND], nn[ND];
#pragma unroll
        for (int j = 0; j < ND; ++j) {
            u[j] = s[2 + j];
            nn[j] = A.nrm[g + (int64_t)j * A.ldn];
        }
        // 2. the wall function at the image point: y = image distance, u = tangential speed, nu = mu(T) / rho
        float imd = 0.0f;
        wall_dev::WallOut wf = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        if (WF) {
            imd = A.imd[g];
            const float rho = p / (A.f.R * T);
            const float nu = flowbc_dev::sutherland(A.f, T) / rho;
            float un = u[0] * nn[0];
#pragma unroll
            for (int j = 1; j < ND; ++j) un = un + u[j] * nn[j];
            float t2 = 0.0f;
#pragma unroll
            for (int j = 0; j < ND; ++j) {
                const float t = u[j] - un * nn[j];
                t2 = (j == 0) ? t * t : t2 + t * t;
            }
            wf = wall_dev::wall_eval(imd, sqrtf(t2), nu, A.wp);
        }
        // 3. the FlowBC call
        float ba[NF];
        flowbc_dev::flow_bc_point<ND>(A.f, p, T, u, nn, A.pinf, A.Tinf, A.uinf, A.normal_flow, WF, wf.dudn, imd, A.transp,
                                      ba[0], ba[1], ba + 2);
        // 4. the scalars' boundary values
#pragma unroll
        for (int q = 0; q < BCF_MAXS; ++q) {
            const int32_t m = A.mode[q];
            float v = m == IBH_BC_SCALAR_COPY ? s[NP + q] : A.value[q];
            if (WF) {
                v = m == IBH_BC_SCALAR_NUT ? wf.nut : v;
                v = m == IBH_BC_SCALAR_K ? wf.k : v;
                v = m == IBH_BC_SCALAR_OMEGA ? wf.omega : v;
                v = m == IBH_BC_SCALAR_EPSILON ? wf.eps : v;
            }
            ba[NP + q] = v;
        }
        // 5., 6. the blend of k_bc_blend, into the ghost cell or the staging buffer
        const float eta = A.eta[g];
        const int64_t row = A.staging ? g : (int64_t)A.ghost[g];
#pragma unroll
        for (int q = 0; q < NF; ++q)
            if (q < nf) {
                const float v = eta * s[q] + (1.0f - eta) * ba[q];
                if (A.staging) A.staging[g + (int64_t)q * A.ng] = v;
                else if (q < NP) A.P[row + (int64_t)q * A.ldp] = v;
                else A.S[q - NP][row] = v;
            }
    }
}

// the staged form's second launch: field blockIdx.y of the staging buffer to the ghost cells (the scatter of the BC sets)
template <int ND>
__global__ __launch_bounds__(BCF_BLOCK) void k_bc_flow_scatter(int32_t ng, const int32_t* __restrict__ ghost,
                                                               const float* __restrict__ staging, float* P, int64_t ldp,
                                                               float* S0, float* S1, float* S2, float* S3) {
    constexpr int NP = ND + 2;
    const int v = blockIdx.y;
    float* a = v < NP ? P + (int64_t)v * ldp : v == NP ? S0 : v == NP + 1 ? S1 : v == NP + 2 ? S2 : S3;
    bcset_dev::scatter_wg(blockIdx.x, gridDim.x, 0, ng, ghost, staging + (int64_t)v * ng, a);
}

// is any ghost cell of the boundary a donor of one of its stencils?  (host copies of ibh_bc_create; cached on the boundary)
int flow_direct(const ibh_bc* b) {
    if (b->flow_direct < 0) {
        std::vector<int32_t> g = b->h_ghost;
        std::sort(g.begin(), g.end());
        int direct = 1;
        for (int32_t c : b->h_donor)
            if (std::binary_search(g.begin(), g.end(), c)) {
                direct = 0;
                break;
            }
        b->flow_direct = direct;
    }
    return b->flow_direct;
}

}  // namespace

extern "C" {

int ibh_bc_flow_info(const ibh_bc* b, int32_t* direct) {
    IBH_REQUIRE(b && direct, "ibh_bc_flow_info: null argument");
    *direct = flow_direct(b);
    return 0;
}

int ibh_bc_flow(const ibh_bc* b, const ibh_fluid* f, int nd, const float* normals, int64_t ldn, const float* image_distances,
                float* P, int64_t ldp, const ibh_flow_bc_spec* spec, int ns, float* const* scalars,
                const int32_t* scalar_mode, const float* scalar_value, float* staging) {
    IBH_REQUIRE(b && f && normals && image_distances && P && spec, "ibh_bc_flow: null argument");
    IBH_REQUIRE(nd == 2 || nd == 3, "ibh_bc_flow: nd must be 2 or 3");
    IBH_REQUIRE(ns >= 0 && ns <= BCF_MAXS, "ibh_bc_flow: at most 4 scalar fields (0 <= ns <= 4)");
    IBH_REQUIRE(ns == 0 || (scalars && scalar_mode && scalar_value), "ibh_bc_flow: null scalar table");
    IBH_REQUIRE(spec->wall_function == 0 || spec->wall_function == 1, "ibh_bc_flow: wall_function must be 0 or 1");
    IBH_REQUIRE(!spec->wall_function || spec->n_iter >= 0, "ibh_bc_flow: negative n_iter");
    for (int i = 0; i < ns; ++i) {
        IBH_REQUIRE(scalars[i], "ibh_bc_flow: null scalar field");
        IBH_REQUIRE(scalar_mode[i] >= IBH_BC_SCALAR_CONST && scalar_mode[i] <= IBH_BC_SCALAR_EPSILON,
                    "ibh_bc_flow: unknown scalar mode");
        IBH_REQUIRE(scalar_mode[i] < IBH_BC_SCALAR_NUT || spec->wall_function,
                    "ibh_bc_flow: a wall-function scalar mode (nut, k, omega, epsilon) needs wall_function = 1");
    }
    IBH_REQUIRE(!spec->normal_flow || (spec->u_inf[1] == 0.0f && spec->u_inf[2] == 0.0f),
                "ibh_bc_flow: Only 3 parcels in P (p, T and normal flow) allowed for normal_flow = true BC");
    IBH_REQUIRE(ldn >= b->ng && ldp >= 1, "ibh_bc_flow: leading dimension too small");
    const int direct = flow_direct(b);
    IBH_REQUIRE(direct || staging, "ibh_bc_flow: this boundary has ghost cells among its donors (ibh_bc_flow_info: direct = "
                                   "0) and needs a staging buffer of n_ghost * (nd + 2 + ns) floats");
    if (b->ng == 0) return 0;
    BcFlowArgs A;
    A.ng = b->ng;
    A.off = b->interp.off;
    A.idx = b->interp.idx;
    A.w = b->interp.w;
    A.remap = b->image_domain;
    A.ghost = b->ghost;
    A.eta = b->eta;
    IBH_REQUIRE(A.off && A.idx && A.w && A.remap && A.ghost && A.eta, "ibh_bc_flow: boundary without an interpolator");
    A.nrm = normals;
    A.imd = image_distances;
    A.ldn = ldn;
    A.ldp = ldp;
    A.P = P;
    A.f = *f;
    A.pinf = spec->p_inf;
    A.Tinf = spec->T_inf;
    A.uinf[0] = spec->u_inf[0];   // (as ibh_cfd_flow_bc: unused components are zero)
    A.uinf[1] = spec->normal_flow ? 0.0f : spec->u_inf[1];
    A.uinf[2] = (!spec->normal_flow && nd == 3) ? spec->u_inf[2] : 0.0f;
    A.transp = spec->transpiration;
    A.normal_flow = spec->normal_flow ? 1 : 0;
    A.wp = wall_dev::wall_params(spec->wall_params, spec->n_iter);
    A.ns = ns;
    for (int i = 0; i < BCF_MAXS; ++i) {
        A.S[i] = i < ns ? scalars[i] : nullptr;
        A.mode[i] = i < ns ? scalar_mode[i] : IBH_BC_SCALAR_CONST;
        A.value[i] = i < ns ? scalar_value[i] : 0.0f;
    }
    A.staging = direct ? nullptr : staging;
    const dim3 grid(ibh_grid_cap(b->ng, BCF_BLOCK, BCF_GRID_CAP)), wg(BCF_BLOCK);
    if (nd == 2) {
        if (spec->wall_function) hipLaunchKernelGGL((k_bc_flow<2, true>), grid, wg, 0, ibh_stream, A);
        else hipLaunchKernelGGL((k_bc_flow<2, false>), grid, wg, 0, ibh_stream, A);
    } else {
        if (spec->wall_function) hipLaunchKernelGGL((k_bc_flow<3, true>), grid, wg, 0, ibh_stream, A);
        else hipLaunchKernelGGL((k_bc_flow<3, false>), grid, wg, 0, ibh_stream, A);
    }
    IBH_LAUNCH_CHECK();
    if (!direct) {
        const dim3 g2(grid.x, nd + 2 + ns);
        if (nd == 2)
            hipLaunchKernelGGL(k_bc_flow_scatter<2>, g2, wg, 0, ibh_stream, b->ng, b->ghost, staging, P, ldp, A.S[0], A.S[1],
                               A.S[2], A.S[3]);
        else
            hipLaunchKernelGGL(k_bc_flow_scatter<3>, g2, wg, 0, ibh_stream, b->ng, b->ghost, staging, P, ldp, A.S[0], A.S[1],
                               A.S[2], A.S[3]);
        IBH_LAUNCH_CHECK();
    }
    return 0;
}

}  // extern "C"

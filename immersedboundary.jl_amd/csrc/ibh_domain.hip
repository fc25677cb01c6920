// libibhip: the domain call on device-resident global arrays -- `(dom::Domain)(f, args...)` (ImmersedBoundary.jl:820-864).
//
// A domain plan holds, for all partitions of a Domain at once, what the per-partition copies of the reference need:
//     gather   dargs_p = a[part.domain]                                    (:835-840, `selectdim(a, 1, part.domain) |> copy`)
//     scatter  a[part.image] = dargs_p[part.image_in_domain]              (:857-859)
// The local arrays of all partitions are stacked in one workspace per field: partition p's block starts at element
// nv * ws_off[p] with ws_off[p] = sum over q < p of pad64(n_q), i.e. on a 256-byte boundary, and is column-major
// (n_p, nv) with leading dimension n_p -- the layout `hip()` gives a fresh array, so the per-partition views are eligible
// for the same vector loads and fused paths.
//
// One gather launch and one scatter launch cover every partition and up to IBH_DOM_MAXF fields.  A workgroup takes
// DOM_BLOCK consecutive rows of ONE partition (the table `wg` maps workgroup -> (partition, first row), a uniform load:
// scalar registers, no per-lane search); lane i handles one row, reads its index once and loops over fields and
// variables.  Consecutive lanes write consecutive workspace rows (gather) or read them (scatter); part.domain and
// part.image are sorted global ids, so the global side is coalesced as far as the partition's rows are contiguous.
#include "ibh_common.h"

#include <algorithm>
#include <memory>
#include <vector>

#define DOM_BLOCK 256

// one partition of a plan (device table)
struct Part {
    int64_t row_off;  // into rows
    int64_t img_off;  // into img (pairs)
    int64_t ws_off;   // in rows of the stacked workspace (times nv = elements)
    int32_t n;        // len(part.domain)
    int32_t n_img;    // len(part.image)
};

struct ibh_domain_plan {
    int n_parts;
    int64_t n_global;
    int64_t ws_rows;                // sum of pad64(n_p): a field of nv variables needs nv * ws_rows elements
    std::vector<int64_t> ws_off;    // host copy, n_parts + 1 entries
    // device tables
    int32_t* rows = nullptr;        // concatenated part.domain (0-based)
    int32_t* img = nullptr;         // concatenated (image, image_in_domain) pairs, interleaved
    Part* parts = nullptr;          // per partition
    int2* wg_gather = nullptr;      // workgroup -> (partition, first domain row)
    int2* wg_scatter = nullptr;     // workgroup -> (partition, first image row)
    int32_t n_wg_gather = 0, n_wg_scatter = 0;
    ibh_owner own;
};

namespace {

struct DomFields {
    const float* src[IBH_DOM_MAXF];
    float* dst[IBH_DOM_MAXF];
    int64_t ld[IBH_DOM_MAXF];  // of the global array
    int32_t nv[IBH_DOM_MAXF];
    int32_t nf;
};
static_assert(std::is_trivially_copyable<DomFields>::value, "DomFields is passed to kernels by value");

__global__ __launch_bounds__(DOM_BLOCK) void k_domain_gather(const int2* __restrict__ wg, const Part* __restrict__ parts,
                                                             const int32_t* __restrict__ rows, DomFields F) {
    const int2 w = wg[blockIdx.x];  // uniform: scalar loads
    const Part P = parts[w.x];
    const int32_t i = w.y + (int32_t)threadIdx.x;
    if (i >= P.n) return;
    const int64_t g = rows[P.row_off + i];
    for (int k = 0; k < F.nf; ++k) {
        const float* __restrict__ s = F.src[k] + g;
        float* __restrict__ d = F.dst[k] + (int64_t)F.nv[k] * P.ws_off + i;
        for (int v = 0; v < F.nv[k]; ++v) d[(int64_t)v * P.n] = s[(int64_t)v * F.ld[k]];
    }
}

__global__ __launch_bounds__(DOM_BLOCK) void k_domain_scatter(const int2* __restrict__ wg, const Part* __restrict__ parts,
                                                              const int32_t* __restrict__ img, DomFields F) {
    const int2 w = wg[blockIdx.x];
    const Part P = parts[w.x];
    const int32_t j = w.y + (int32_t)threadIdx.x;
    if (j >= P.n_img) return;
    const int2 pr = ((const int2*)img)[P.img_off + j];  // (global row, local row)
    const int64_t g = pr.x;
    for (int k = 0; k < F.nf; ++k) {
        const float* __restrict__ s = F.src[k] + (int64_t)F.nv[k] * P.ws_off + pr.y;
        float* __restrict__ d = F.dst[k] + g;
        for (int v = 0; v < F.nv[k]; ++v) d[(int64_t)v * F.ld[k]] = s[(int64_t)v * P.n];
    }
}

int64_t pad64(int64_t n) { return (n + 63) & ~(int64_t)63; }

// fields [k0, k0 + nf) of the call; `gather` selects the direction
int launch(const ibh_domain_plan* p, bool gather, int k0, int nf, const float* const* src, const int* nv,
           const int64_t* ld, float* const* dst) {
    DomFields F;
    F.nf = nf;
    for (int k = 0; k < nf; ++k) {
        F.src[k] = src[k0 + k];
        F.dst[k] = dst[k0 + k];
        F.nv[k] = nv[k0 + k];
        F.ld[k] = ld[k0 + k];
    }
    if (gather) {
        if (p->n_wg_gather == 0) return 0;
        hipLaunchKernelGGL(k_domain_gather, dim3(p->n_wg_gather), dim3(DOM_BLOCK), 0, ibh_stream, p->wg_gather, p->parts,
                           p->rows, F);
    } else {
        if (p->n_wg_scatter == 0) return 0;
        hipLaunchKernelGGL(k_domain_scatter, dim3(p->n_wg_scatter), dim3(DOM_BLOCK), 0, ibh_stream, p->wg_scatter,
                           p->parts, p->img, F);
    }
    IBH_LAUNCH_CHECK();
    return 0;
}

int run(const ibh_domain_plan* p, bool gather, int nfields, const float* const* src, const int* nv, const int64_t* ld,
        float* const* dst, const char* name) {
    IBH_REQUIRE(p, name);
    IBH_REQUIRE(nfields >= 0 && (nfields == 0 || (src && nv && ld && dst)), name);
    for (int k = 0; k < nfields; ++k) {
        IBH_REQUIRE(nv[k] >= 1, "ibh_domain_gather/scatter: nv < 1");
        IBH_REQUIRE(nv[k] == 1 || ld[k] >= p->n_global, "ibh_domain_gather/scatter: ld < number of cells");
        IBH_REQUIRE(src[k] && dst[k], "ibh_domain_gather/scatter: null field pointer");
    }
    for (int k0 = 0; k0 < nfields; k0 += IBH_DOM_MAXF) {
        const int rc = launch(p, gather, k0, std::min(IBH_DOM_MAXF, nfields - k0), src, nv, ld, dst);
        if (rc) return rc;
    }
    return 0;
}

}  // namespace

extern "C" {

int ibh_domain_plan_create(ibh_domain_plan** out, int n_parts, const int32_t* const* domain, const int32_t* n_domain,
                           const int32_t* const* image, const int32_t* const* image_in_domain, const int32_t* n_image,
                           int64_t n_global, int index_base) {
    IBH_REQUIRE(out, "ibh_domain_plan_create: null out");
    *out = nullptr;
    IBH_REQUIRE(n_parts >= 0 && n_global >= 0 && n_global <= INT32_MAX, "ibh_domain_plan_create: bad sizes");
    IBH_REQUIRE(index_base == 0 || index_base == 1, "ibh_domain_plan_create: index_base must be 0 or 1");
    IBH_REQUIRE(n_parts == 0 || (domain && n_domain && image && image_in_domain && n_image),
                "ibh_domain_plan_create: null table");
    std::vector<int32_t> rows, img;
    std::vector<Part> parts(n_parts);
    std::vector<int2> wg_g, wg_s;
    std::vector<int64_t> ws_off(n_parts + 1, 0);
    std::vector<char> covered(n_global, 0);
    for (int p = 0; p < n_parts; ++p) {
        const int32_t n = n_domain[p], m = n_image[p];
        IBH_REQUIRE(n >= 0 && m >= 0 && m <= n, "ibh_domain_plan_create: bad partition sizes");
        IBH_REQUIRE((n == 0 || domain[p]) && (m == 0 || (image[p] && image_in_domain[p])),
                    "ibh_domain_plan_create: null partition table");
        Part& P = parts[p];
        P.row_off = (int64_t)rows.size();
        P.img_off = (int64_t)img.size() / 2;
        P.ws_off = ws_off[p];
        P.n = n;
        P.n_img = m;
        for (int32_t i = 0; i < n; ++i) {
            const int64_t g = (int64_t)domain[p][i] - index_base;
            IBH_REQUIRE(g >= 0 && g < n_global, "ibh_domain_plan_create: domain index out of range");
            rows.push_back((int32_t)g);
        }
        for (int32_t j = 0; j < m; ++j) {
            const int64_t g = (int64_t)image[p][j] - index_base;
            const int64_t l = (int64_t)image_in_domain[p][j] - index_base;
            IBH_REQUIRE(g >= 0 && g < n_global, "ibh_domain_plan_create: image index out of range");
            IBH_REQUIRE(l >= 0 && l < n, "ibh_domain_plan_create: image_in_domain index out of range");
            // the scatter of all partitions is one launch: a row written twice would take whichever store lands last
            IBH_REQUIRE(!covered[g], "ibh_domain_plan_create: partition images overlap");
            covered[g] = 1;
            img.push_back((int32_t)g);
            img.push_back((int32_t)l);
        }
        for (int32_t i = 0; i < n; i += DOM_BLOCK) wg_g.push_back(make_int2(p, i));
        for (int32_t j = 0; j < m; j += DOM_BLOCK) wg_s.push_back(make_int2(p, j));
        ws_off[p + 1] = ws_off[p] + pad64(n);
    }
    IBH_REQUIRE(wg_g.size() <= (size_t)INT32_MAX && wg_s.size() <= (size_t)INT32_MAX,
                "ibh_domain_plan_create: too many workgroups");
    std::unique_ptr<ibh_domain_plan> p(new ibh_domain_plan);
    p->n_parts = n_parts;
    p->n_global = n_global;
    p->ws_rows = ws_off[n_parts];
    p->ws_off = ws_off;
    p->n_wg_gather = (int32_t)wg_g.size();
    p->n_wg_scatter = (int32_t)wg_s.size();
    IBH_TRY(p->own.upload(&p->rows, rows));
    IBH_TRY(p->own.upload(&p->img, img));
    IBH_TRY(p->own.upload(&p->parts, parts));
    IBH_TRY(p->own.upload(&p->wg_gather, wg_g));
    IBH_TRY(p->own.upload(&p->wg_scatter, wg_s));
    *out = p.release();
    return 0;
}

int ibh_domain_plan_destroy(ibh_domain_plan* p) {
    delete p;
    return 0;
}

int ibh_domain_plan_info(const ibh_domain_plan* p, int64_t* ws_off, int n) {
    IBH_REQUIRE(p && ws_off && n == p->n_parts + 1, "ibh_domain_plan_info: needs n_parts + 1 entries");
    for (int i = 0; i < n; ++i) ws_off[i] = p->ws_off[i];
    return 0;
}

int ibh_domain_gather(const ibh_domain_plan* p, int nfields, const float* const* src, const int* nv, const int64_t* ld,
                      float* const* ws) {
    return run(p, true, nfields, src, nv, ld, ws, "ibh_domain_gather: bad arguments");
}

int ibh_domain_scatter(const ibh_domain_plan* p, int nfields, const float* const* ws, const int* nv, const int64_t* ld,
                       float* const* dst) {
    return run(p, false, nfields, ws, nv, ld, dst, "ibh_domain_scatter: bad arguments");
}

}  // extern "C"

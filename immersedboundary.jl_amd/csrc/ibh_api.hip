// libibhip: runtime, memory and handle management (host side of the C ABI).
#include <string.h>

#include <memory>

#include "ibh_common.h"

thread_local std::string ibh_err;
thread_local hipStream_t ibh_stream = nullptr;

int ibh_fail(int code, const char* what, const char* file, int line) {
    ibh_err = std::string(what) + " (" + file + ":" + std::to_string(line) + ")";
    return code ? code : -1;
}

static std::vector<int32_t> rebased(const int32_t* p, size_t n, int base) {
    std::vector<int32_t> v(n);
    for (size_t i = 0; i < n; ++i) v[i] = p[i] - base;
    return v;
}

struct ibh_host2d : Host2D {};

static int make_view(HostPartView& v, int nd, int32_t nc, const float* spacing, const int32_t* nf,
                     const int32_t* const* owners, const int32_t* const* neighbors, const int32_t* const* left_off,
                     const int32_t* const* left_idx, const int32_t* const* right_off, const int32_t* const* right_idx,
                     const int32_t* domain, int block_size, int index_base) {
    v.nd = nd;
    v.nc = nc;
    v.spacing = spacing;
    v.nf = nf;
    v.domain = domain;
    v.index_base = index_base;
    v.bs = block_size;
    v.owners.resize(nd); v.neighbors.resize(nd);
    v.loff.resize(nd); v.lidx.resize(nd); v.roff.resize(nd); v.ridx.resize(nd);
    for (int d = 0; d < nd; ++d) {
        IBH_REQUIRE(nf[d] >= 0, "ibh_partition_create: negative face count");
        v.owners[d] = rebased(owners[d], nf[d], index_base);
        v.neighbors[d] = rebased(neighbors[d], nf[d], index_base);
        // offsets: accept either base (first entry tells)
        int32_t ob = left_off[d][0];
        v.loff[d] = rebased(left_off[d], (size_t)nc + 1, ob);
        v.lidx[d] = rebased(left_idx[d], v.loff[d][nc], index_base);
        ob = right_off[d][0];
        v.roff[d] = rebased(right_off[d], (size_t)nc + 1, ob);
        v.ridx[d] = rebased(right_idx[d], v.roff[d][nc], index_base);
        for (int32_t f = 0; f < nf[d]; ++f)
            IBH_REQUIRE(v.owners[d][f] >= 0 && v.owners[d][f] < nc && v.neighbors[d][f] >= 0 && v.neighbors[d][f] < nc,
                        "ibh_partition_create: owner/neighbour index out of range");
        for (int32_t c = 0; c < nc; ++c)
            IBH_REQUIRE(v.loff[d][c + 1] >= v.loff[d][c] && v.roff[d][c + 1] >= v.roff[d][c],
                        "ibh_partition_create: CSR offsets not monotone");
        for (int32_t x : v.lidx[d]) IBH_REQUIRE(x >= 0 && x < nf[d], "ibh_partition_create: left face id out of range");
        for (int32_t x : v.ridx[d]) IBH_REQUIRE(x >= 0 && x < nf[d], "ibh_partition_create: right face id out of range");
    }
    return 0;
}

// ---- the uploads of ibh_partition_create, in its order
static int upload_faces(ibh_part* p, const HostPartView& v, const float* spacing, const float* centers) {
    IBH_TRY(p->own.upload(&p->spacing, spacing, (size_t)v.nc * v.nd));
    if (centers) IBH_TRY(p->own.upload(&p->centers, centers, (size_t)v.nc * v.nd));
    for (int d = 0; d < v.nd; ++d) {
        DimData& D = p->dim[d];
        D.nf = v.nf[d];
        IBH_TRY(p->own.upload(&D.owners, v.owners[d]));
        IBH_TRY(p->own.upload(&D.neighbors, v.neighbors[d]));
        IBH_TRY(p->own.upload(&D.loff, v.loff[d]));
        IBH_TRY(p->own.upload(&D.lidx, v.lidx[d]));
        IBH_TRY(p->own.upload(&D.roff, v.roff[d]));
        IBH_TRY(p->own.upload(&D.ridx, v.ridx[d]));
    }
    return 0;
}

static int upload_image_ids(ibh_part* p, int32_t n_image, const int32_t* image_in_domain, int index_base) {
    p->n_image = n_image;
    if (n_image > 0 && image_in_domain) {
        std::vector<int32_t> iid = rebased(image_in_domain, n_image, index_base);
        for (int32_t x : iid) IBH_REQUIRE(x >= 0 && x < p->nc, "ibh_partition_create: image_in_domain out of range");
        IBH_TRY(p->own.upload(&p->image_in_domain, iid));
    }
    return 0;
}

template <class T>
static std::vector<T> joined(std::vector<T> a, const std::vector<T>& b) {
    a.insert(a.end(), b.begin(), b.end());
    return a;
}
// quad set k; the pair tiles of set 0 go behind the quads, in the same arrays (the kernel tells them apart by index)
static int upload_quads2(ibh_part* p, int k, const QuadSet2& Q) {
    p->nq[k] = (int32_t)Q.qd.size();
    p->nq_int[k] = Q.nq_int;
    p->nqs[k] = (int32_t)Q.singles.size();
    p->nqs_int[k] = Q.ns_int;
    if (k == 0 && !Q.pd.empty()) {
        p->npair = (int32_t)Q.pd.size();
        p->nqs2 = (int32_t)Q.singles2.size();
        IBH_TRY(p->own.upload(&p->qd[k], joined(Q.qd, Q.pd)));
        IBH_TRY(p->own.upload(&p->qtab[k], joined(Q.qtab, Q.ptab)));
        IBH_TRY(p->own.upload(&p->qsingles2, Q.singles2));
        IBH_TRY(p->own.upload(&p->qaux[k], joined(Q.qaux, Q.paux)));
    } else {
        IBH_TRY(p->own.upload(&p->qd[k], Q.qd));
        IBH_TRY(p->own.upload(&p->qtab[k], Q.qtab));
        IBH_TRY(p->own.upload(&p->qaux[k], Q.qaux));
    }
    return p->own.upload(&p->qsingles[k], Q.singles);
}

static int upload2(ibh_part* p, const Host2D& H) {
    IBH_TRY(p->own.upload(&p->htab, H.htab));
    IBH_TRY(p->own.upload(&p->etab, H.etab));
    IBH_TRY(p->own.upload(&p->dtab, H.dtab));
    p->n_dt = (int32_t)(H.dtab.size() / 64);
    p->fuse_all = H.fuse_all;
    p->rows_ok = H.rows_ok;
    p->n_img = (int32_t)H.img.size();
    p->n_img_int = H.n_img_int;
    p->img_all_fz = H.img_all_fz;
    if (p->img_all_fz) IBH_TRY(p->own.upload(&p->img_list, H.img));
    if (!H.fuse_all && H.nfus > 0) {
        p->n_fz = (int32_t)H.fz.size();
        p->n_ng = (int32_t)H.ng.size();
        p->n_nf = (int32_t)H.nf.size();
        p->n_fz_int = H.n_fz_int;
        p->n_ng_int = H.n_ng_int;
        p->n_nf_int = H.n_nf_int;
        IBH_TRY(p->own.upload(&p->fz_list, H.fz));
        IBH_TRY(p->own.upload(&p->ng_list, H.ng));
        IBH_TRY(p->own.upload(&p->nf_list, H.nf));
    }
    for (int k = 0; k < 2; ++k) IBH_TRY(upload_quads2(p, k, H.quads[k]));
    return p->own.upload(&p->blocks2, H.blocks);
}

static int upload3(ibh_part* p, const Host3D& H) {
    p->sweep3 = H.sw.all ? 1 : 0;
    IBH_TRY(p->own.upload(&p->rtab3, H.sw.rtab));
    IBH_TRY(p->own.upload(&p->r4tab3, H.sw.r4tab));
    IBH_TRY(p->own.upload(&p->ftab3, H.ftab));
    IBH_TRY(p->own.upload(&p->blocks3, H.blocks));
    IBH_TRY(p->own.upload(&p->htab3, H.htab));
    if (H.im.all) {
        IBH_TRY(p->own.upload(&p->iblocks3, H.im.blocks));
        IBH_TRY(p->own.upload(&p->ihtab3, H.im.htab));
        IBH_TRY(p->own.upload(&p->iftab3, H.im.ftab));
        IBH_TRY(p->own.upload(&p->irtab3, H.im.rtab));
        IBH_TRY(p->own.upload(&p->ir4tab3, H.im.r4tab));
        IBH_TRY(p->own.upload(&p->idtab3, H.im.dtab));
        p->n_img3 = (int32_t)H.im.blocks.size();
        p->img_all3 = 1;
    }
    return 0;
}

// what Host = Host2D and Host3D share: the block counts, the face-list cells with their stencil records, the summary
template <class Host>
static int upload_common(ibh_part* p, const HostPartView& v, const Host& H) {
    p->nA1 = H.nph[0];
    p->nB1 = H.nph[1];
    p->bs = v.bs;
    p->nblk = (int32_t)H.blocks.size();
    p->n_irr = (int32_t)H.irr.size();
    IBH_TRY(p->own.upload(&p->irr_cells, H.irr));
    IBH_TRY(p->own.upload(&p->irr_rec, ibh_irr_records(v, H.irr)));
    p->sum = H.sum;
    return 0;
}

extern "C" {

int ibh_version(void) { return 100; }

const char* ibh_last_error(void) { return ibh_err.c_str(); }

int ibh_init(int device) {
    IBH_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    IBH_HIP(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return ibh_fail(-2, (std::string("libibhip is built for gfx950 only, device is ") + prop.gcnArchName).c_str(),
                        __FILE__, __LINE__);
    return 0;
}

int ibh_set_stream(void* s) {
    ibh_stream = (hipStream_t)s;
    return 0;
}

int ibh_sync(void) {
    IBH_HIP(hipStreamSynchronize(ibh_stream));
    return 0;
}

int ibh_malloc(void** p, size_t bytes) {
    IBH_HIP(hipMalloc(p, bytes ? bytes : 4));
    return 0;
}
int ibh_free(void* p) {
    if (p) IBH_HIP(hipFree(p));
    return 0;
}
int ibh_owned_device_memory(int64_t* bytes, int64_t* buffers) {
    if (bytes) *bytes = ibh_owned_bytes;
    if (buffers) *buffers = ibh_owned_buffers;
    return 0;
}
int ibh_h2d(void* dst, const void* src, size_t bytes) {
    IBH_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ibh_stream));
    IBH_HIP(hipStreamSynchronize(ibh_stream));
    return 0;
}
int ibh_d2h(void* dst, const void* src, size_t bytes) {
    IBH_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ibh_stream));
    IBH_HIP(hipStreamSynchronize(ibh_stream));
    return 0;
}
int ibh_memset(void* dst, int value, size_t bytes) {
    IBH_HIP(hipMemsetAsync(dst, value, bytes, ibh_stream));
    return 0;
}

int ibh_partition_create(ibh_part** out, int nd, int32_t nc, const float* spacing, const float* centers,
                         const int32_t* nf, const int32_t* const* owners, const int32_t* const* neighbors,
                         const int32_t* const* left_off, const int32_t* const* left_idx,
                         const int32_t* const* right_off, const int32_t* const* right_idx, int32_t n_image,
                         const int32_t* image_in_domain, const int32_t* domain, int block_size, int index_base) {
    IBH_REQUIRE(out && spacing && nf && owners && neighbors && left_off && left_idx && right_off && right_idx,
                "ibh_partition_create: null argument");
    *out = nullptr;
    IBH_REQUIRE(nd == 2 || nd == 3, "ibh_partition_create: nd must be 2 or 3");
    IBH_REQUIRE(nc >= 0 && (index_base == 0 || index_base == 1), "ibh_partition_create: bad nc/index_base");
    HostPartView v;
    IBH_TRY(make_view(v, nd, nc, spacing, nf, owners, neighbors, left_off, left_idx, right_off, right_idx, domain,
                      block_size, index_base));
    std::unique_ptr<ibh_part> p(new ibh_part());   // freed with all its buffers by any return before the release
    p->nd = nd;
    p->nc = nc;
    IBH_TRY(upload_faces(p.get(), v, spacing, centers));
    int64_t direct = 0;
    IBH_TRY(p->own.upload(&p->side, ibh_side_table(v, &direct)));
    IBH_TRY(upload_image_ids(p.get(), n_image, image_in_domain, index_base));
    // analysis record -> upload -> summary; without block information every cell is a face-list cell
    if (domain && block_size == 8 && nd == 2) {
        Host2D H;
        ibh_analyze2(v, image_in_domain, n_image, H);
        IBH_TRY(upload2(p.get(), H));
        IBH_TRY(upload_common(p.get(), v, H));
    } else if (domain && block_size == 8) {
        Host3D H;
        ibh_analyze3(v, image_in_domain, n_image, H);
        IBH_TRY(upload3(p.get(), H));
        IBH_TRY(upload_common(p.get(), v, H));
    } else {
        p->sum.irregular_cells = nc;
    }
    p->sum.direct_sides = direct;
    *out = p.release();
    return 0;
}

// ---- host-only introspection of the 2-D block analysis (no HIP call: runs without a GPU) ----
int ibh_analyze2_host(ibh_host2d** out, int32_t nc, const float* spacing, const int32_t* nf,
                      const int32_t* const* owners, const int32_t* const* neighbors, const int32_t* const* left_off,
                      const int32_t* const* left_idx, const int32_t* const* right_off, const int32_t* const* right_idx,
                      int32_t n_image, const int32_t* image_in_domain, const int32_t* domain, int index_base) {
    IBH_REQUIRE(out && spacing && nf && owners && neighbors && left_off && left_idx && right_off && right_idx && domain,
                "ibh_analyze2_host: null argument");
    HostPartView v;
    IBH_TRY(make_view(v, 2, nc, spacing, nf, owners, neighbors, left_off, left_idx, right_off, right_idx, domain, 8,
                      index_base));
    ibh_host2d* h = new ibh_host2d();
    ibh_analyze2(v, image_in_domain, n_image, *h);
    ibh_side_table(v, &h->sum.direct_sides);   // the table's count alone: the summary is then create's, slot for slot
    *out = h;
    return 0;
}

int ibh_host2d_get(const ibh_host2d* h, int what, int set, void* dst, int64_t cap_bytes, int64_t* nbytes) {
    IBH_REQUIRE(h && nbytes && (set == 0 || set == 1), "ibh_host2d_get: bad argument");
    const Host2D& H = *h;
    const QuadSet2& Q = H.quads[set];
    const void* src = nullptr;
    int64_t n = 0;
    int64_t counts[8] = {(int64_t)H.blocks.size(), (int64_t)Q.qd.size(), Q.nq_int, (int64_t)Q.singles.size(), Q.ns_int,
                         H.fuse_all, H.img_all_fz, H.nph[1]};
    int64_t slots[IBH_INFO_COUNT];
    ibh_summary_write(H.sum, slots);
    switch (what) {
        case IBH_H2D_BLOCKS: src = H.blocks.data(); n = (int64_t)(H.blocks.size() * sizeof(BlockDesc2)); break;
        case IBH_H2D_HTAB: src = H.htab.data(); n = (int64_t)(H.htab.size() * 4); break;
        case IBH_H2D_ETAB: src = H.etab.data(); n = (int64_t)(H.etab.size() * 4); break;
        case IBH_H2D_FUSABLE: src = H.fus.data(); n = (int64_t)H.fus.size(); break;
        case IBH_H2D_QUAD_DESC: src = Q.qd.data(); n = (int64_t)(Q.qd.size() * sizeof(QuadDesc2)); break;
        case IBH_H2D_QUAD_TAB: src = Q.qtab.data(); n = (int64_t)(Q.qtab.size() * 4); break;
        case IBH_H2D_SINGLES: src = Q.singles.data(); n = (int64_t)(Q.singles.size() * 4); break;
        case IBH_H2D_PAIR_DESC: src = Q.pd.data(); n = (int64_t)(Q.pd.size() * sizeof(QuadDesc2)); break;
        case IBH_H2D_PAIR_TAB: src = Q.ptab.data(); n = (int64_t)(Q.ptab.size() * 4); break;
        case IBH_H2D_SINGLES2: src = Q.singles2.data(); n = (int64_t)(Q.singles2.size() * 4); break;
        case IBH_H2D_QUAD_AUX: src = Q.qaux.data(); n = (int64_t)(Q.qaux.size() * 4); break;
        case IBH_H2D_PAIR_AUX: src = Q.paux.data(); n = (int64_t)(Q.paux.size() * 4); break;
        case IBH_H2D_COUNTS: src = counts; n = (int64_t)sizeof(counts); break;
        case IBH_H2D_INFO: src = slots; n = (int64_t)sizeof(slots); break;
        default: return ibh_fail(-1, "ibh_host2d_get: unknown item", __FILE__, __LINE__);
    }
    *nbytes = n;
    if (dst) {
        IBH_REQUIRE(cap_bytes >= n, "ibh_host2d_get: destination too small");
        if (n) memcpy(dst, src, (size_t)n);
    }
    return 0;
}

int ibh_host2d_destroy(ibh_host2d* h) {
    delete h;
    return 0;
}

int ibh_partition_destroy(ibh_part* p) {
    delete p;
    return 0;
}

int ibh_partition_info(const ibh_part* p, int64_t* info, int n) {
    IBH_REQUIRE(p && info, "ibh_partition_info: null argument");
    int64_t slots[IBH_INFO_COUNT];
    ibh_summary_write(p->sum, slots);
    if (n > 0) memcpy(info, slots, sizeof(int64_t) * (size_t)(n < IBH_INFO_COUNT ? n : IBH_INFO_COUNT));
    return 0;
}

static int acc_fill(ibh_acc* a, int32_t n_output, int32_t n_input, const int32_t* off, const int32_t* idx,
                    const float* w, int index_base) {
    IBH_REQUIRE(off && (n_output >= 0), "ibh_acc_create: null offsets");
    int32_t ob = off[0];
    std::vector<int32_t> o = rebased(off, (size_t)n_output + 1, ob);
    for (int32_t r = 0; r < n_output; ++r) IBH_REQUIRE(o[r + 1] >= o[r], "ibh_acc_create: offsets not monotone");
    size_t nnz = o[n_output];
    IBH_REQUIRE(nnz == 0 || idx, "ibh_acc_create: null indices");
    std::vector<int32_t> ix = rebased(idx, nnz, index_base);
    for (int32_t x : ix) IBH_REQUIRE(x >= 0 && x < n_input, "ibh_acc_create: donor index out of range");
    a->n_out = n_output;
    a->n_in = n_input;
    IBH_TRY(a->own.upload(&a->off, o));
    IBH_TRY(a->own.upload(&a->idx, ix));
    if (w) IBH_TRY(a->own.upload(&a->w, w, nnz));
    return 0;
}

int ibh_acc_create(ibh_acc** out, int32_t n_output, int32_t n_input, const int32_t* off, const int32_t* idx,
                   const float* w, int index_base) {
    IBH_REQUIRE(out, "ibh_acc_create: null out");
    *out = nullptr;
    std::unique_ptr<ibh_acc> a(new ibh_acc());
    IBH_TRY(acc_fill(a.get(), n_output, n_input, off, idx, w, index_base));
    *out = a.release();
    return 0;
}

int ibh_acc_destroy(ibh_acc* a) {
    delete a;
    return 0;
}

int ibh_bc_create(ibh_bc** out, int32_t ng, const int32_t* ghost_indices, const float* ghost_distances,
                  const float* image_distances, int32_t nid, const int32_t* image_domain,
                  const int32_t* interp_off, const int32_t* interp_idx, const float* interp_w, int index_base) {
    IBH_REQUIRE(out && ghost_indices && ghost_distances && image_distances && image_domain,
                "ibh_bc_create: null argument");
    *out = nullptr;
    std::unique_ptr<ibh_bc> b(new ibh_bc());
    b->ng = ng;
    b->nid = nid;
    std::vector<int32_t> g = rebased(ghost_indices, ng, index_base);
    std::vector<int32_t> idm = rebased(image_domain, nid, index_base);
    std::vector<float> eta(ng);
    for (int32_t i = 0; i < ng; ++i) eta[i] = ghost_distances[i] / image_distances[i];  // :1220
    IBH_TRY(b->own.upload(&b->ghost, g));
    IBH_TRY(b->own.upload(&b->image_domain, idm));
    IBH_TRY(b->own.upload(&b->eta, eta));
    IBH_TRY(acc_fill(&b->interp, ng, nid, interp_off, interp_idx, interp_w, index_base));
    // host copies (ibh_bcset_create)
    b->h_ghost = g;
    b->h_eta = eta;
    if (ng > 0 && interp_off && interp_idx) {
        const int32_t ob = interp_off[0];
        b->h_off.resize((size_t)ng + 1);
        for (int32_t i = 0; i <= ng; ++i) b->h_off[i] = interp_off[i] - ob;
        const size_t nnz = (size_t)b->h_off[ng];
        b->h_donor.resize(nnz);
        b->h_w.resize(nnz);
        for (size_t k = 0; k < nnz; ++k) {
            const int32_t j = interp_idx[k] - index_base;
            IBH_REQUIRE(j >= 0 && j < nid, "ibh_bc_create: stencil index out of range");
            b->h_donor[k] = idm[j];
            b->h_w[k] = interp_w ? interp_w[k] : 1.0f;
        }
    }
    *out = b.release();
    return 0;
}

int ibh_bc_destroy(ibh_bc* b) {
    delete b;
    return 0;
}

}  // extern "C"

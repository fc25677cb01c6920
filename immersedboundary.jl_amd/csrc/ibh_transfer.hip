// libibhip: accumulators (the reference's Accumulator: transfer operators, BC interpolation) and the ghost-cell boundary
// condition.  Threads run over the contiguous row index so loads/stores of the row-major side are coalesced.  A row is
// summed in the order of ibh_stencil_dev.h, compiled with -ffp-contract=off: bit-comparable with the oracle.
#include "ibh_common.h"
#include "ibh_stencil_dev.h"

#define OPS_BLOCK 256

namespace {

// one field per (row, field): the scalar walk, in the order of ibh_stencil_dev.h
__global__ void k_accumulate(int32_t n_out, const int32_t* __restrict__ off, const int32_t* __restrict__ idx,
                             const float* __restrict__ w, const int32_t* __restrict__ remap,
                             const float* __restrict__ v, int64_t ldv, float* __restrict__ out, int64_t ldo) {
    int64_t var = blockIdx.y;
    const float* vv = v + var * ldv;
    for (int64_t r = IBH_WG_X() * (int64_t)blockDim.x + threadIdx.x; r < n_out; r += (int64_t)gridDim.x * blockDim.x) {
        int32_t b = off[r], e = off[r + 1];
        float s = 0.0f;
        for (int32_t k = b; k < e; ++k) {
            int32_t j = idx[k];
            if (remap) j = remap[j];
            float t = w ? vv[j] * w[k] : vv[j];
            s = (k == b) ? t : s + t;
        }
        out[r + var * ldo] = s;
    }
}

// The same for several fields at once: one thread per row, the row's indices and weights read once for up to NVB
// fields (the per-(row, field) form reads them once per field).  Same sum order per field.
// v2 (optional): the stencil is applied to v - v2 (elementwise difference first, like `acc(a .- b)`); ADD: out .+= result
// Rows with weights that start on a 16-byte boundary (the 2^nd-point transfer operators: every row) take their entries four
// at a time; rows without weights take them one by one.  The walk of ibh_stencil_dev.h in one hand-written body:
// over Entries<N> the <8> instantiations take 69 VGPRs for 63 (seven waves per SIMD for eight).
template <int NVB, bool ADD = false>
__global__ void k_accumulate_rows(int32_t n_out, const int32_t* __restrict__ off, const int32_t* __restrict__ idx,
                                  const float* __restrict__ w, const int32_t* __restrict__ remap,
                                  const float* __restrict__ v, int64_t ldv, float* __restrict__ out, int64_t ldo, int nv,
                                  const float* __restrict__ v2 = nullptr) {
    const int v0 = blockIdx.y * NVB;
    const int nb = min(NVB, nv - v0);
    const float* vv = v + (int64_t)v0 * ldv;
    const float* vv2 = v2 ? v2 + (int64_t)v0 * ldv : nullptr;
    float* oo = out + (int64_t)v0 * ldo;
    for (int64_t r = IBH_WG_X() * (int64_t)blockDim.x + threadIdx.x; r < n_out; r += (int64_t)gridDim.x * blockDim.x) {
        const int32_t b = off[r], e = off[r + 1];
        float s[NVB];
#pragma unroll
        for (int q = 0; q < NVB; ++q) s[q] = 0.0f;
        int32_t k = b;
        if ((b & 3) == 0 && w)
            for (; k + 4 <= e; k += 4) {
                const int4 j4 = *reinterpret_cast<const int4*>(idx + k);
                const float4 w4 = *reinterpret_cast<const float4*>(w + k);
                int32_t jj[4] = {j4.x, j4.y, j4.z, j4.w};
                const float ww[4] = {w4.x, w4.y, w4.z, w4.w};
                if (remap) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) jj[i] = remap[jj[i]];
                }
                float x[4][NVB];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int q = 0; q < NVB; ++q)
                        if (q < nb) x[i][q] = vv[jj[i] + (int64_t)q * ldv];
                if (vv2) {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int q = 0; q < NVB; ++q)
                            if (q < nb) x[i][q] = x[i][q] - vv2[jj[i] + (int64_t)q * ldv];
                }
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int q = 0; q < NVB; ++q)
                        if (q < nb) {
                            const float t = x[i][q] * ww[i];
                            s[q] = (k + i == b) ? t : s[q] + t;
                        }
            }
        for (; k < e; ++k) {
            int32_t j = idx[k];
            if (remap) j = remap[j];
            const float wk = w ? w[k] : 1.0f;
#pragma unroll
            for (int q = 0; q < NVB; ++q) {
                if (q < nb) {
                    float x = vv[j + (int64_t)q * ldv];
                    if (vv2) x = x - vv2[j + (int64_t)q * ldv];
                    const float t = w ? x * wk : x;
                    s[q] = (k == b) ? t : s[q] + t;
                }
            }
        }
#pragma unroll
        for (int q = 0; q < NVB; ++q)
            if (q < nb) oo[r + (int64_t)q * ldo] = ADD ? oo[r + (int64_t)q * ldo] + s[q] : s[q];
    }
}

// out .+= acc(a .- b) for up to 8 fields with the donors' fields side by side: a pre-pass writes d[j][0..7] = a[j, :] - b[j, :]
// (32 bytes per donor), the row kernel then takes a donor with TWO 16-byte gathers instead of two 4-byte gathers per field
// (6 fields x 8 donors: 16 gather instructions per row instead of 96) -- same differences, same products, same order.
__global__ void k_pack_diff8(int32_t n_in, int nv, const float* __restrict__ a, const float* __restrict__ b, int64_t ld,
                             float* __restrict__ d) {
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < (int64_t)n_in * 8; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t j = t >> 3;
        const int q = (int)(t & 7);
        d[t] = q < nv ? a[j + (int64_t)q * ld] - b[j + (int64_t)q * ld] : 0.0f;
    }
}
// N donors of a row from the packed differences: two 16-byte gathers each (one up to 4 fields), all issued first
template <int NV, int N>
__device__ __forceinline__ void packed_entries(const stencil_dev::Entries<N>& en, bool first, const float4* __restrict__ d,
                                               float (&s)[8]) {
    float4 lo[N], hi[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        lo[i] = d[2 * (int64_t)en.j[i]];
        if (NV > 4) hi[i] = d[2 * (int64_t)en.j[i] + 1];
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const float x[8] = {lo[i].x, lo[i].y, lo[i].z, lo[i].w, NV > 4 ? hi[i].x : 0.0f, NV > 4 ? hi[i].y : 0.0f,
                            NV > 4 ? hi[i].z : 0.0f, NV > 4 ? hi[i].w : 0.0f};
#pragma unroll
        for (int q = 0; q < NV; ++q) {
            const float t = x[q] * en.w[i];
            s[q] = (first && i == 0) ? t : s[q] + t;
        }
    }
}
template <int NV>
__global__ void k_accumulate_packed_add(int32_t n_out, const int32_t* __restrict__ off, const int32_t* __restrict__ idx,
                                        const float* __restrict__ w, const float4* __restrict__ d, float* __restrict__ out,
                                        int64_t ldo) {
    for (int64_t r = IBH_WG_X() * (int64_t)blockDim.x + threadIdx.x; r < n_out; r += (int64_t)gridDim.x * blockDim.x) {
        const int32_t b = off[r], e = off[r + 1];
        float s[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) s[q] = 0.0f;
        int32_t k = b;
        if ((b & 3) == 0)
            for (; k + 4 <= e; k += 4) packed_entries<NV, 4>(stencil_dev::load4(idx, w, k), k == b, d, s);
        for (; k < e; ++k) packed_entries<NV, 1>(stencil_dev::load1(idx, w, k), k == b, d, s);
#pragma unroll
        for (int q = 0; q < NV; ++q) out[r + (int64_t)q * ldo] = out[r + (int64_t)q * ldo] + s[q];
    }
}

// a[ghost] = eta*ia + (1-eta)*ba (:1242-1245); ba from array, constant, or ia (copy BC)
__global__ void k_bc_blend(int32_t ng, const int32_t* __restrict__ ghost, const float* __restrict__ eta,
                           float* __restrict__ a, int64_t lda, const float* __restrict__ ia, int64_t ldi,
                           const float* __restrict__ ba, int64_t ldb, const float* __restrict__ bconst) {
    int64_t v = blockIdx.y;
    for (int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; g < ng; g += (int64_t)gridDim.x * blockDim.x) {
        float e = eta[g];
        float i = ia[g + v * ldi];
        float b = ba ? ba[g + v * ldb] : bconst[v];
        a[ghost[g] + v * lda] = e * i + (1.0f - e) * b;
    }
}

inline dim3 grid2(int64_t n, int nv) { return dim3(ibh_grid_cap(n, OPS_BLOCK, 4096), nv); }

// launch of the accumulation kernels: per (row, field) for one field, per row over blocks of up to 4 fields otherwise
static inline void launch_accumulate(int32_t n_out, const int32_t* off, const int32_t* idx, const float* w,
                                     const int32_t* remap, const float* v, int64_t ldv, float* out, int64_t ldo, int nv) {
    if (nv == 1) {
        hipLaunchKernelGGL(k_accumulate, grid2(n_out, 1), dim3(OPS_BLOCK), 0, ibh_stream, n_out, off, idx, w, remap, v, ldv,
                           out, ldo);
    } else if (nv > 4 && nv <= 8) {
        // 5..8 fields (a state vector): indices and weights read ONCE for all of them (2.0 -> 1.3 ms per application of the
        // transfer operators of a 33.6 M-cell level to 6 fields)
        hipLaunchKernelGGL(k_accumulate_rows<8>, grid2(n_out, 1), dim3(OPS_BLOCK), 0, ibh_stream, n_out, off, idx, w, remap, v,
                           ldv, out, ldo, nv, (const float*)nullptr);
    } else {
        dim3 g = grid2(n_out, (nv + 3) / 4);
        hipLaunchKernelGGL(k_accumulate_rows<4>, g, dim3(OPS_BLOCK), 0, ibh_stream, n_out, off, idx, w, remap, v, ldv, out,
                           ldo, nv, (const float*)nullptr);
    }
}

}  // namespace

#define CHECK_NV(nv) IBH_REQUIRE((nv) >= 1 && (nv) <= 65535, "nv out of range")

extern "C" {

int ibh_accumulate(const ibh_acc* a, const float* v, int nv, int64_t ldv, float* out, int64_t ldo) {
    IBH_REQUIRE(a, "ibh_accumulate: null accumulator");
    CHECK_NV(nv);
    if (a->n_out == 0) return 0;
    launch_accumulate(a->n_out, a->off, a->idx, a->w, (const int32_t*)nullptr, v, ldv, out, ldo, nv);
    IBH_LAUNCH_CHECK();
    return 0;
}

int ibh_accumulate_diff_add(const ibh_acc* a, const float* v, const float* v2, int nv, int64_t ldv, float* out,
                            int64_t ldo) {
    IBH_REQUIRE(a && v && v2 && out, "ibh_accumulate_diff_add: null argument");
    CHECK_NV(nv);
    if (a->n_out == 0) return 0;
    if (a->w && nv >= 2 && nv <= 8 && (int64_t)a->n_out >= 4 * (int64_t)a->n_in) {
        // many rows per donor (a prolongation): pack the donors' differences once, gather them 16 bytes at a time
        ibh_acc* am = const_cast<ibh_acc*>(a);
        if (!am->packed) IBH_TRY(am->own.alloc(&am->packed, 8 * (size_t)a->n_in));
        hipLaunchKernelGGL(k_pack_diff8, grid2((int64_t)a->n_in * 8, 1), dim3(OPS_BLOCK), 0, ibh_stream, a->n_in, nv, v, v2,
                           ldv, am->packed);
        const float4* d4 = reinterpret_cast<const float4*>(am->packed);
#define PACKED_LAUNCH(N)                                                                                               \
    hipLaunchKernelGGL(k_accumulate_packed_add<N>, grid2(a->n_out, 1), dim3(OPS_BLOCK), 0, ibh_stream, a->n_out, a->off,  \
                       a->idx, a->w, d4, out, ldo)
        switch (nv) {
            case 2: PACKED_LAUNCH(2); break;
            case 3: PACKED_LAUNCH(3); break;
            case 4: PACKED_LAUNCH(4); break;
            case 5: PACKED_LAUNCH(5); break;
            case 6: PACKED_LAUNCH(6); break;
            case 7: PACKED_LAUNCH(7); break;
            default: PACKED_LAUNCH(8); break;
        }
#undef PACKED_LAUNCH
        IBH_LAUNCH_CHECK();
        return 0;
    }
    for (int v0 = 0; v0 < nv; v0 += 8) {
        const int nb = nv - v0 < 8 ? nv - v0 : 8;
        hipLaunchKernelGGL((k_accumulate_rows<8, true>), grid2(a->n_out, 1), dim3(OPS_BLOCK), 0, ibh_stream, a->n_out, a->off,
                           a->idx, a->w, (const int32_t*)nullptr, v + (int64_t)v0 * ldv, ldv, out + (int64_t)v0 * ldo, ldo,
                           nb, v2 + (int64_t)v0 * ldv);
    }
    IBH_LAUNCH_CHECK();
    return 0;
}

int ibh_bc_interp(const ibh_bc* b, const float* a, int nv, int64_t lda, float* ia, int64_t ldi) {
    IBH_REQUIRE(b, "ibh_bc_interp: null boundary");
    CHECK_NV(nv);
    if (b->ng == 0) return 0;
    launch_accumulate(b->ng, b->interp.off, b->interp.idx, b->interp.w, b->image_domain, a, lda, ia, ldi, nv);
    IBH_LAUNCH_CHECK();
    return 0;
}

int ibh_bc_blend(const ibh_bc* b, float* a, int nv, int64_t lda, const float* ia, int64_t ldi, const float* ba,
                 int64_t ldb, const float* ba_const) {
    IBH_REQUIRE(b && (ba || ba_const), "ibh_bc_blend: need ba or ba_const");
    CHECK_NV(nv);
    if (b->ng == 0) return 0;
    float* dconst = nullptr;
    if (!ba) {
        IBH_HIP(hipMallocAsync((void**)&dconst, sizeof(float) * nv, ibh_stream));
        IBH_HIP(hipMemcpyAsync(dconst, ba_const, sizeof(float) * nv, hipMemcpyHostToDevice, ibh_stream));
    }
    hipLaunchKernelGGL(k_bc_blend, grid2(b->ng, nv), dim3(OPS_BLOCK), 0, ibh_stream, b->ng, b->ghost, b->eta, a, lda,
                       ia, ldi, ba, ldb, dconst);
    IBH_LAUNCH_CHECK();
    if (dconst) IBH_HIP(hipFreeAsync(dconst, ibh_stream));
    return 0;
}

int ibh_bc_apply(const ibh_bc* b, float* a, int nv, int64_t lda, int mode, const float* ba_const) {
    IBH_REQUIRE(b && (mode == 0 || mode == 1), "ibh_bc_apply: bad mode");
    CHECK_NV(nv);
    if (b->ng == 0) return 0;
    float* ia = nullptr;
    IBH_HIP(hipMallocAsync((void**)&ia, sizeof(float) * (size_t)b->ng * nv, ibh_stream));
    int rc = ibh_bc_interp(b, a, nv, lda, ia, b->ng);
    if (!rc) rc = (mode == 0) ? ibh_bc_blend(b, a, nv, lda, ia, b->ng, nullptr, 0, ba_const)
                              : ibh_bc_blend(b, a, nv, lda, ia, b->ng, ia, b->ng, nullptr);
    hipError_t e = hipFreeAsync(ia, ibh_stream);
    if (rc) return rc;
    IBH_HIP(e);
    return 0;
}

}  // extern "C"

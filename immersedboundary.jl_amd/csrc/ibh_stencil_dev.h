// libibhip: the walk over a CSR stencil row [b, e) and its loaders -- the ONE statement of the order in which a row is
// summed, on which every bit-for-bit claim about accumulators and transfer operators rests:
//   * per entry k the product t = x * w[k] (x: whatever the caller gathers for donor idx[k]; without weights t = x);
//   * the sum is ASSIGNED from the row's first entry and the others are added in entry order, s = s + t (never 0 + t, no
//     contraction);
//   * where the row starts on a 16-byte boundary its entries come four at a time -- one dwordx4 of indices, one of
//     weights -- and ALL gathers of a group are issued before its arithmetic; the arithmetic keeps the entry order.
// A walk is two loops over the loaders below, each handing its entries and the flag "entry 0 of these is the row's first"
// to the kernel's own function of Entries<N>:
//     int32_t k = b;
//     if ((b & 3) == 0)
//         for (; k + 4 <= e; k += 4) xxx_entries<.., 4>(load4(idx, w, k), k == b, ..);
//     for (; k < e; ++k) xxx_entries<.., 1>(load1(idx, w, k), k == b, ..);
// k_accumulate_packed_add (ibh_transfer.hip), k_restrict_euler and k_prolong_euler (ibh_mgrid.hip) are written so.  (One
// function that takes the kernel's part as a callable was tried for the two loops: through it k_restrict_euler<3, true> took
// 83 VGPRs for 79, five waves per SIMD for six, and the 2-D prolongation measured 2 % slower, outside the spread;
// profiles/ops_split.)  k_accumulate_rows (ibh_transfer.hip) keeps the walk in one hand-written body -- 4-wide only with
// weights, indices through `remap`, v2 subtracted before the multiply: over Entries<N> its <8> instantiations took 69 VGPRs
// for 63, seven waves per SIMD for eight.  Walks that keep the order in bodies of their own: k_accumulate
// (ibh_transfer.hip), bcset_dev::bc_interp1 (ibh_bcset_dev.h), k_bc_flow (ibh_bcflow.hip).
#pragma once
#include "ibh_common.h"

namespace stencil_dev {

// entries k .. k + n - 1 (n = 4: one dwordx4 of indices and one of weights; 1: the scalar tail) of a row
template <int N>
struct Entries {
    int32_t j[N];
    float w[N];
};
__device__ __forceinline__ Entries<4> load4(const int32_t* __restrict__ idx, const float* __restrict__ w, int32_t k) {
    const int4 j4 = *reinterpret_cast<const int4*>(idx + k);
    Entries<4> e{{j4.x, j4.y, j4.z, j4.w}, {1.0f, 1.0f, 1.0f, 1.0f}};
    if (w) {
        const float4 w4 = *reinterpret_cast<const float4*>(w + k);
        e.w[0] = w4.x, e.w[1] = w4.y, e.w[2] = w4.z, e.w[3] = w4.w;
    }
    return e;
}
__device__ __forceinline__ Entries<1> load1(const int32_t* __restrict__ idx, const float* __restrict__ w, int32_t k) {
    return Entries<1>{{idx[k]}, {w ? w[k] : 1.0f}};   // (no weights: x * 1 is x, bit for bit)
}

}  // namespace stencil_dev

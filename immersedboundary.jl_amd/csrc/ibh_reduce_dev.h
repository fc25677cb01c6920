// libibhip: the workgroup reduction of every two-stage reduction in the library, written once.
//
// The scheme: every workgroup reduces its stride of the input to ONE value and writes it into an array
// of partials (host side: ibh_red_scratch, ibh_reduce.hip); a one-workgroup launch reduces the partials and writes the
// result.  No atomics and no counters (arrivals at one address serialise across the XCDs), with one exception: k_ew_reduce
// on 2 - 8 workgroups lets the last workgroup to arrive at a counter finish (ibh_ew.hip), with the two functions below.
//
// Order of operations of wg_reduce, fixed -- it is part of the bits of every sum:
//   1. within a wave, the __shfl_down tree with offsets 32, 16, 8, 4, 2, 1: lane 0 holds the wave's value;
//   2. lane 0 of wave w writes LDS slot w;
//   3. after the barrier, thread 0 combines the slots in wave order: ((slot 0 OP slot 1) OP slot 2) OP ...
// The result is valid in thread 0 only.
#pragma once
#include "ibh_common.h"

namespace ibh_red {

// The operations: the value type, op(a, b) and the value a strided pass starts from.
template <class T>
struct Sum {   // + on double and on float
    using type = T;
    static __device__ __forceinline__ T op(T a, T b) { return a + b; }
    static __device__ __forceinline__ T identity() { return T(0); }
};
struct FMax {  // fmaxf: drops a NaN
    using type = float;
    static __device__ __forceinline__ float op(float a, float b) { return fmaxf(a, b); }
    static __device__ __forceinline__ float identity() { return -INFINITY; }
};
struct FMin {  // fminf: drops a NaN
    using type = float;
    static __device__ __forceinline__ float op(float a, float b) { return fminf(a, b); }
    static __device__ __forceinline__ float identity() { return INFINITY; }
};
struct NanMax {  // ibh_max: Julia's maximum, NaN in, NaN out
    using type = float;
    static __device__ __forceinline__ float op(float a, float b) { return ibh_max(a, b); }
    static __device__ __forceinline__ float identity() { return -INFINITY; }
};

// The per-thread values v of a workgroup of N threads (all of them must call) reduced with OP; valid in thread 0.
// The slots are static LDS of the instantiation: a kernel that reduces a second time with the same <N, OP> puts a
// __syncthreads() between the two calls, so that thread 0 has read the slots before they are written again.
template <int N, class OP>
__device__ __forceinline__ typename OP::type wg_reduce(typename OP::type v) {
    static_assert(N >= 64 && N % 64 == 0, "a workgroup of whole waves");
    __shared__ typename OP::type slot[N / 64];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = OP::op(v, __shfl_down(v, o, 64));
    if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        v = slot[0];
#pragma unroll
        for (int w = 1; w < N / 64; ++w) v = OP::op(v, slot[w]);
    }
    return v;
}

// The final stage: ONE workgroup of N threads over the n partials of the first stage -- thread t takes partials t, t + N,
// ... in that order starting from the identity, then wg_reduce.  Valid in thread 0.
template <int N, class OP>
__device__ __forceinline__ typename OP::type wg_reduce_partials(int n, const typename OP::type* __restrict__ part) {
    typename OP::type v = OP::identity();
    for (int i = threadIdx.x; i < n; i += N) v = OP::op(v, part[i]);
    return wg_reduce<N, OP>(v);
}

}  // namespace ibh_red

// libibhip: the host side of the two-stage reductions (device side: ibh_reduce_dev.h) -- the scratch
// that holds the workgroup partials between the two launches, and the final stage of the sums in double.
#include "ibh_common.h"

namespace {

// final stage of the sums in double: one workgroup adds the n workgroup sums -- thread t adds partials t, t + 256, ... in
// that order, then the 256 values go through the LDS tree (strides 128 ... 1).  A fixed order for a fixed n: it is part of
// the bits of ibh_sumsq, ibh_axpy_clamped_sumsq, ibh_fas_update and ibh_dot.
__global__ __launch_bounds__(256) void k_sum_partials(int n, const double* __restrict__ part, double* __restrict__ out) {
    __shared__ double sh[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += part[i];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = sh[0];
}

}  // namespace

// The scratch of the reductions of ONE host thread: a region of IBH_RED_BYTES per entry point, allocated together on first
// use (on the device that is current then) and kept for the life of the thread.
// The rule that makes it safe: the reductions of a host thread are launched on ibh_stream, and a stream runs them in
// order, so the second stage of one reduction has read a region before the first stage of the next one writes it.  A
// caller that switches streams (ibh_set_stream) between two reductions without synchronising the first stream breaks that
// order and races on the scratch.  Entry points that a caller may interleave on purpose have regions of their own.
void* ibh_red_scratch(ibh_red_region region) {
    static thread_local char* buf = nullptr;
    if (!buf) {   // zeroed once, on ibh_stream like the reductions that follow (no reliance on the null stream): the
                  // arrival counter of ibh_ew_reduce lives behind its partials and resets itself
        const size_t bytes = (size_t)IBH_RED_REGIONS * IBH_RED_BYTES;
        if (hipMalloc((void**)&buf, bytes) != hipSuccess) buf = nullptr;
        else if (hipMemsetAsync(buf, 0, bytes, ibh_stream) != hipSuccess) { hipFree(buf); buf = nullptr; }
    }
    return buf ? buf + (size_t)region * IBH_RED_BYTES : nullptr;
}

void ibh_launch_sum_partials(int n, const double* part, double* out) {
    hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(256), 0, ibh_stream, n, part, out);
}

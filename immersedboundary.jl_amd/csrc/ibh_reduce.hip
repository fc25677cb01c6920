// libibhip: the host side of the two-stage reductions (device side: ibh_reduce_dev.h) -- the scratch
// that holds the workgroup partials between the two launches, and the final stage of the sums in double -- and
// ibh_sumsq_roles, the sums of squares of the columns of an array over its fluid rows.
#include "ibh_common.h"
#include "ibh_reduce_dev.h"

#define RED_BLOCK 256

namespace {

// final stage of the sums in double: one workgroup adds the n workgroup sums -- thread t adds partials t, t + 256, ... in
// that order, then the 256 values go through the LDS tree (strides 128 ... 1).  A fixed order for a fixed n: it is part of
// the bits of ibh_sumsq, ibh_axpy_clamped_sumsq, ibh_fas_update and ibh_dot.  Workgroup c of the launch does so for the n
// partials from part[c * n] into out[c]: the columns of ibh_sumsq_roles; every other reduction launches one.
__global__ __launch_bounds__(256) void k_sum_partials(int n, const double* __restrict__ part, double* __restrict__ out) {
    __shared__ double sh[256];
    part += (int64_t)blockIdx.x * n;
    out += blockIdx.x;
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

// column blockIdx.y of x over the rows whose role is fluid, in double: workgroup sums (ibh_reduce_dev.h) into
// part[column * gridDim.x + workgroup], added by k_sum_partials.  A select: a NaN in a masked row is not summed.
__global__ __launch_bounds__(RED_BLOCK) void k_sumsq_roles(int64_t n, const float* __restrict__ x, int64_t ldx,
                                                           const uint8_t* __restrict__ roles, double* __restrict__ part) {
    const float* __restrict__ col = x + blockIdx.y * ldx;
    double s = 0.0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const double t = roles[i] == IBH_ROLE_FLUID ? (double)col[i] : 0.0;
        s += t * t;
    }
    s = ibh_red::wg_reduce<RED_BLOCK, ibh_red::Sum<double>>(s);
    if (threadIdx.x == 0) part[blockIdx.y * gridDim.x + blockIdx.x] = s;
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

void ibh_launch_sum_partials(int n, const double* part, double* out, int ncols) {
    hipLaunchKernelGGL(k_sum_partials, dim3(ncols), dim3(256), 0, ibh_stream, n, part, out);
}

extern "C" int ibh_sumsq_roles(int64_t n, int nv, const float* x, int64_t ldx, const uint8_t* roles, double* out) {
    IBH_REQUIRE(x && roles && out, "ibh_sumsq_roles: null argument");
    IBH_REQUIRE(n >= 0 && nv >= 1 && nv <= IBH_SUMSQ_ROLES_MAX_NV, "ibh_sumsq_roles: n must be >= 0 and nv in 1 .. 8");
    IBH_REQUIRE(ldx >= n, "ibh_sumsq_roles: the leading dimension is smaller than n");
    const uintptr_t o = (uintptr_t)out, xl = (uintptr_t)x, rl = (uintptr_t)roles;
    const uintptr_t oh = o + nv * sizeof(double), xh = xl + sizeof(float) * (size_t)((int64_t)(nv - 1) * ldx + n);
    IBH_REQUIRE(n == 0 || (!(o < xh && xl < oh) && !(o < rl + (size_t)n && rl < oh)),
                "ibh_sumsq_roles: out may not alias x or roles");
    if (n == 0) return 0;    // (nothing launched, out as it was)
    double* part = (double*)ibh_red_scratch(IBH_RED_SUMSQ_ROLES);
    IBH_REQUIRE(part, "ibh_sumsq_roles: no scratch");
    // nv columns of at most 2048 / 8 workgroup partials each share the region
    const int nwg = ibh_grid_cap(n, RED_BLOCK, (int)(IBH_RED_BYTES / sizeof(double)) / IBH_SUMSQ_ROLES_MAX_NV);
    hipLaunchKernelGGL(k_sumsq_roles, dim3(nwg, nv), dim3(RED_BLOCK), 0, ibh_stream, n, x, ldx, roles, part);
    ibh_launch_sum_partials(nwg, part, out, nv);
    IBH_LAUNCH_CHECK();
    return 0;
}

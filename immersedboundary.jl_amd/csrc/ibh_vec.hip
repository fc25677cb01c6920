// libibhip: the small vector ops of the FAS loop (solver.jl:80-84): axpy, the clamped fixed-point update and the sums of
// squares.  Thread per element, grid-stride; the sums in double through workgroup partials (ibh_reduce_dev.h).
#include "ibh_common.h"
#include "ibh_reduce_dev.h"

#define OPS_BLOCK 256

namespace {

__global__ void k_axpy_clamped(int64_t n, float omega, const float* __restrict__ r, float* __restrict__ q) {
    float w = ibh_clamp(omega, 0.0f, 1.0f);   // Julia's clamp: a NaN omega stays NaN
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        q[i] = q[i] + w * r[i];
}

__global__ void k_axpy(int64_t n, float a, const float* __restrict__ x, float* __restrict__ y) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        y[i] = a * x[i] + y[i];
}

// sum x^2 in double: workgroup sums (ibh_reduce_dev.h), added by k_sum_partials (ibh_reduce.hip)
__global__ void k_sumsq(int64_t n, const float* __restrict__ x, double* __restrict__ out) {
    double s = 0.0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        double t = (double)x[i];
        s += t * t;
    }
    s = ibh_red::wg_reduce<OPS_BLOCK, ibh_red::Sum<double>>(s);
    if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// One pass of `FAS!` over a residual array (solver.jl:80-84): rr = r [+ source]; [q += clamp(omega, 0, 1) * rr]; [sum rr^2]
// -- `r .+= source`, the fixed-point update and the norm on ONE read of r (round 3 had the sum as an ATen kernel).
// <false, true, true> is ibh_axpy_clamped_sumsq (solver.jl:82 and the norm of :84 on the same array).
template <bool SRC, bool UPD, bool NRM>
__global__ void k_fas_update(int64_t n, float omega, const float* __restrict__ r, const float* __restrict__ src,
                             float* __restrict__ q, double* __restrict__ out) {
    const float w = ibh_clamp(omega, 0.0f, 1.0f);   // Julia's clamp: a NaN omega stays NaN
    double s = 0.0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float ri = r[i];
        if (SRC) ri = ri + src[i];
        if (UPD) q[i] = q[i] + w * ri;
        if (NRM) s += (double)ri * (double)ri;
    }
    if (NRM) {
        s = ibh_red::wg_reduce<OPS_BLOCK, ibh_red::Sum<double>>(s);
        if (threadIdx.x == 0) out[blockIdx.x] = s;
    }
}

}  // namespace

extern "C" {

int ibh_axpy_clamped(int64_t n, float omega, const float* r, float* q) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_axpy_clamped, dim3(ibh_grid_cap(n, OPS_BLOCK, 2048)), dim3(OPS_BLOCK), 0, ibh_stream, n, omega, r, q);
    IBH_LAUNCH_CHECK();
    return 0;
}
int ibh_axpy_clamped_sumsq(int64_t n, float omega, const float* r, float* q, double* out) {
    IBH_REQUIRE(out, "ibh_axpy_clamped_sumsq: null argument");
    return ibh_fas_update(n, omega, r, nullptr, q, out);   // k_fas_update<false, true, true>
}
int ibh_fas_update(int64_t n, float omega, const float* r, const float* source, float* q, double* out_sumsq) {
    IBH_REQUIRE(r || n <= 0, "ibh_fas_update: null residual");
    double* part = out_sumsq ? (double*)ibh_red_scratch(IBH_RED_FAS) : nullptr;
    IBH_REQUIRE(!out_sumsq || part, "ibh_fas_update: no scratch");
    if (n <= 0) {
        if (out_sumsq) IBH_HIP(hipMemsetAsync(out_sumsq, 0, sizeof(double), ibh_stream));
        return 0;
    }
    if (!q && !out_sumsq) return 0;
    const int nwg = ibh_grid_cap(n, OPS_BLOCK, 2048);
#define FAS_LAUNCH(S, U, N) \
    hipLaunchKernelGGL((k_fas_update<S, U, N>), dim3(nwg), dim3(OPS_BLOCK), 0, ibh_stream, n, omega, r, source, q, part)
    if (source) {
        if (q && out_sumsq) FAS_LAUNCH(true, true, true);
        else if (q) FAS_LAUNCH(true, true, false);
        else FAS_LAUNCH(true, false, true);
    } else {
        if (q && out_sumsq) FAS_LAUNCH(false, true, true);
        else if (q) FAS_LAUNCH(false, true, false);
        else FAS_LAUNCH(false, false, true);
    }
#undef FAS_LAUNCH
    if (out_sumsq) ibh_launch_sum_partials(nwg, part, out_sumsq);
    IBH_LAUNCH_CHECK();
    return 0;
}
int ibh_axpy(int64_t n, float a, const float* x, float* y) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_axpy, dim3(ibh_grid_cap(n, OPS_BLOCK, 2048)), dim3(OPS_BLOCK), 0, ibh_stream, n, a, x, y);
    IBH_LAUNCH_CHECK();
    return 0;
}
int ibh_sumsq(int64_t n, const float* x, double* out) {
    double* part = (double*)ibh_red_scratch(IBH_RED_SUMSQ);
    IBH_REQUIRE(out && part, "ibh_sumsq: null argument or no scratch");
    if (n <= 0) {
        IBH_HIP(hipMemsetAsync(out, 0, sizeof(double), ibh_stream));
        return 0;
    }
    const int nwg = ibh_grid_cap(n, OPS_BLOCK, 1024);
    hipLaunchKernelGGL(k_sumsq, dim3(nwg), dim3(OPS_BLOCK), 0, ibh_stream, n, x, part);
    ibh_launch_sum_partials(nwg, part, out);
    IBH_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"

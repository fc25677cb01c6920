// libibhip: running statistics of a field -- CFD.TimeAverage (cfd.jl:738-802).
//
// One push is a pure stream: read mu, sigma and Q (and dt when it is elementwise), write mu and sigma in place.  Each lane
// moves 16 B per array (4 consecutive elements of the flat, compact mu / sigma); Q and an elementwise dt take the same
// 16-B loads when they are compact too, or one element at a time through their `ld` otherwise.
//
// Arithmetic follows Julia's promotion op by op (compiled with -ffp-contract=off, IEEE divide / sqrt): with P the
// precision of eta = dt / tau,
//     sigma = sqrt(sigma^2 * (1 - eta) + (mu - Q)^2 * eta)      sigma^2, mu - Q, (mu - Q)^2 in Float32; the rest in P
//     mu    = mu * (1 - eta) + Q * eta                          in P, rounded to Float32 on store
// and the first registry is `mu = copy(Q); sigma = mu .* 0` (-0.0 where Q < 0, NaN where Q is NaN or Inf).
#include "ibh_common.h"

#define TA_BLOCK 256

// ibh_set_tuning("time_average_nt", v): stores of mu / sigma with the non-temporal hint (1), plain (0), or plain while the
// three arrays fit the Infinity Cache and non-temporal past it (-1, the default).  Measured (profiles/time_average/): at
// 7.9 M x 5 non-temporal stores took 1-2 % less time in two runs; at 0.87 M x 1 (10 MB, resident) no consistent difference
int ibh_time_average_nt = -1;

namespace {

typedef float v4f_a __attribute__((ext_vector_type(4), aligned(16)));

enum { TA_FIRST = -1 };  // template form of the first registry; the others are IBH_TA_DT_*

__device__ __forceinline__ float ta_sqrt(float x) { return __builtin_sqrtf(x); }
__device__ __forceinline__ double ta_sqrt(double x) { return __builtin_sqrt(x); }

// one element of the push, in the reference's order: sigma from the OLD mu, then mu
template <class P>
__device__ __forceinline__ void ta_update(float& mu, float& sg, float q, P eta) {
    const P om = P(1) - eta;
    const float s2 = sg * sg;
    const float d = mu - q;
    const float d2 = d * d;
    sg = (float)ta_sqrt((P)s2 * om + (P)d2 * eta);
    mu = (float)((P)mu * om + (P)q * eta);
}

// F = dt form (IBH_TA_DT_* or TA_FIRST), P = precision of eta, VEC = Q (and an elementwise dt) compact and 16-B aligned,
// NT = non-temporal stores
template <int F, class P, bool VEC, bool NT>
__global__ __launch_bounds__(TA_BLOCK) void k_time_average(int64_t n, int64_t N, const float* __restrict__ Q, int64_t ldq,
                                                           float* __restrict__ mu, float* __restrict__ sg, P eta_h,
                                                           const float* __restrict__ dt, int64_t ldd, P tau) {
    P eta_u = eta_h;
    if (F == IBH_TA_DT_DEVICE) eta_u = (P)dt[0] / tau;  // uniform address: one scalar load per wave
    const int64_t nchunk = (N + 3) >> 2;
    for (int64_t c = blockIdx.x * (int64_t)TA_BLOCK + threadIdx.x; c < nchunk; c += (int64_t)gridDim.x * TA_BLOCK) {
        const int64_t e0 = c << 2;
        const bool full = e0 + 4 <= N;
        // (row, variable) of the four elements, for strided Q / dt and the per-variable dt
        int64_t r[4] = {0, 0, 0, 0}, v[4] = {0, 0, 0, 0};
        if (!VEC || F == IBH_TA_DT_PER_VAR) {
            v[0] = e0 / n;
            r[0] = e0 - v[0] * n;
#pragma unroll
            for (int j = 1; j < 4; ++j) {
                r[j] = r[j - 1] + 1;
                v[j] = v[j - 1];
                if (r[j] == n) r[j] = 0, ++v[j];
            }
        }
        float q[4], m[4], s[4], t[4];
        if (VEC && full) {
            const v4f_a a = *(const v4f_a*)(Q + e0);
            q[0] = a.x, q[1] = a.y, q[2] = a.z, q[3] = a.w;
            if (F == IBH_TA_DT_ELEMENT) {
                const v4f_a b = *(const v4f_a*)(dt + e0);
                t[0] = b.x, t[1] = b.y, t[2] = b.z, t[3] = b.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (e0 + j >= N) continue;
                q[j] = VEC ? Q[e0 + j] : Q[r[j] + v[j] * ldq];
                if (F == IBH_TA_DT_ELEMENT) t[j] = VEC ? dt[e0 + j] : dt[r[j] + v[j] * ldd];
            }
        }
        if (F == TA_FIRST) {
#pragma unroll
            for (int j = 0; j < 4; ++j) m[j] = q[j], s[j] = q[j] * 0.0f;  // `avg.μ .* 0`, not a fill: keeps -0.0 and NaN
        } else {
            if (full) {
                const v4f_a a = *(const v4f_a*)(mu + e0), b = *(const v4f_a*)(sg + e0);
                m[0] = a.x, m[1] = a.y, m[2] = a.z, m[3] = a.w;
                s[0] = b.x, s[1] = b.y, s[2] = b.z, s[3] = b.w;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (e0 + j < N) m[j] = mu[e0 + j], s[j] = sg[e0 + j];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (!full && e0 + j >= N) continue;  // past the end: v[j] may be nv
                P eta = eta_u;
                if (F == IBH_TA_DT_PER_VAR) eta = (P)dt[v[j]] / tau;
                if (F == IBH_TA_DT_ELEMENT) eta = (P)t[j] / tau;
                ta_update<P>(m[j], s[j], q[j], eta);
            }
        }
        if (full) {
            const v4f_a a = {m[0], m[1], m[2], m[3]}, b = {s[0], s[1], s[2], s[3]};
            if (NT) {
                __builtin_nontemporal_store(a, (v4f_a*)(mu + e0));
                __builtin_nontemporal_store(b, (v4f_a*)(sg + e0));
            } else {
                *(v4f_a*)(mu + e0) = a;
                *(v4f_a*)(sg + e0) = b;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (e0 + j < N) mu[e0 + j] = m[j], sg[e0 + j] = s[j];
        }
    }
}

template <int F, class P, bool VEC, bool NT>
void launch(int64_t n, int64_t N, const float* Q, int64_t ldq, float* mu, float* sg, double eta, const float* dt,
            int64_t ldd, double tau) {
    hipLaunchKernelGGL((k_time_average<F, P, VEC, NT>), dim3(ibh_grid((N + 3) >> 2, TA_BLOCK)), dim3(TA_BLOCK), 0,
                       ibh_stream, n, N, Q, ldq, mu, sg, (P)eta, dt, ldd, (P)tau);
}

template <int F, class P>
void launch_f(bool vec, bool nt, int64_t n, int64_t N, const float* Q, int64_t ldq, float* mu, float* sg, double eta,
              const float* dt, int64_t ldd, double tau) {
    if (vec) {
        if (nt) launch<F, P, true, true>(n, N, Q, ldq, mu, sg, eta, dt, ldd, tau);
        else launch<F, P, true, false>(n, N, Q, ldq, mu, sg, eta, dt, ldd, tau);
    } else {
        if (nt) launch<F, P, false, true>(n, N, Q, ldq, mu, sg, eta, dt, ldd, tau);
        else launch<F, P, false, false>(n, N, Q, ldq, mu, sg, eta, dt, ldd, tau);
    }
}

template <class P>
void launch_p(int form, bool vec, bool nt, int64_t n, int64_t N, const float* Q, int64_t ldq, float* mu, float* sg,
              double eta, const float* dt, int64_t ldd, double tau) {
    switch (form) {
        case IBH_TA_DT_HOST: launch_f<IBH_TA_DT_HOST, P>(vec, nt, n, N, Q, ldq, mu, sg, eta, dt, ldd, tau); break;
        case IBH_TA_DT_DEVICE: launch_f<IBH_TA_DT_DEVICE, P>(vec, nt, n, N, Q, ldq, mu, sg, eta, dt, ldd, tau); break;
        case IBH_TA_DT_PER_VAR: launch_f<IBH_TA_DT_PER_VAR, P>(vec, nt, n, N, Q, ldq, mu, sg, eta, dt, ldd, tau); break;
        default: launch_f<IBH_TA_DT_ELEMENT, P>(vec, nt, n, N, Q, ldq, mu, sg, eta, dt, ldd, tau); break;
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" {

int ibh_time_average_push(int64_t n, int nv, const float* Q, int64_t ldq, float* mu, float* sigma, int dt_form,
                          const float* dt, int64_t dt_numel, int64_t ldd, double eta, double tau, int flags) {
    IBH_REQUIRE(n >= 0 && nv >= 1, "ibh_time_average_push: bad shape");
    IBH_REQUIRE((flags & ~(IBH_TA_F64 | IBH_TA_FIRST)) == 0, "ibh_time_average_push: unknown flags");
    const bool first = flags & IBH_TA_FIRST, f64 = flags & IBH_TA_F64;
    if (nv == 1) ldq = ldd = n;
    IBH_REQUIRE(ldq >= n, "ibh_time_average_push: ldq < n");
    if (n == 0) return 0;
    IBH_REQUIRE(Q && mu && sigma, "ibh_time_average_push: null argument");
    IBH_REQUIRE(aligned16(mu) && aligned16(sigma), "ibh_time_average_push: mu and sigma must be 16-byte aligned");
    if (!first) {
        switch (dt_form) {
            case IBH_TA_DT_HOST: break;
            case IBH_TA_DT_DEVICE:
                IBH_REQUIRE(dt && dt_numel == 1, "ibh_time_average_push: device dt must have one element");
                break;
            case IBH_TA_DT_PER_VAR:
                IBH_REQUIRE(dt && dt_numel == nv, "ibh_time_average_push: per-variable dt must have nv elements");
                break;
            case IBH_TA_DT_ELEMENT:
                IBH_REQUIRE(ldd >= n, "ibh_time_average_push: ldd < n");
                IBH_REQUIRE(dt && dt_numel >= (int64_t)(nv - 1) * ldd + n,
                            "ibh_time_average_push: elementwise dt is smaller than Q");
                break;
            default: return ibh_fail(-1, "ibh_time_average_push: unknown dt form", __FILE__, __LINE__);
        }
    }
    const int64_t N = n * (int64_t)nv;
    const bool elem = !first && dt_form == IBH_TA_DT_ELEMENT;
    const bool vec = ldq == n && aligned16(Q) && (!elem || (ldd == n && aligned16(dt)));
    const bool nt = ibh_time_average_nt < 0 ? (size_t)N * 12 > ((size_t)256 << 20) : ibh_time_average_nt != 0;
    if (first) launch_f<TA_FIRST, float>(vec, nt, n, N, Q, ldq, mu, sigma, 0.0, nullptr, 0, 1.0);
    else if (f64) launch_p<double>(dt_form, vec, nt, n, N, Q, ldq, mu, sigma, eta, dt, ldd, tau);
    else launch_p<float>(dt_form, vec, nt, n, N, Q, ldq, mu, sigma, eta, dt, ldd, tau);
    IBH_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"

// libibhip: the elementwise Float32 math of Julia's broadcast beyond `+ - * / max min abs sqrt` (ibh_ew.hip, extended
// interpreter).  Bool values are Float32 0 / 1.  Exact operations follow Julia's definitions literally (clamp, sign,
// literal_pow, the strong-zero `Bool * Float`); the transcendental functions and `^` are evaluated in double and rounded
// once, which is Julia's `Float32(f(Float64(x)))` within an ulp.  Where Julia throws a DomainError (`log(-1f0)`,
// `(-2f0)^0.5f0`) the result is NaN.
#pragma once
#include "ibh_common.h"

namespace ew_math {

__device__ __forceinline__ float b2f(bool c) { return c ? 1.0f : 0.0f; }

// the rounded operations: in double, rounded once
__device__ __forceinline__ float ew1d(int op, float x) {
    switch (op) {
        case IBH_EW_EXP: return (float)exp((double)x);
        case IBH_EW_EXP2: return (float)exp2((double)x);
        case IBH_EW_LOG: return (float)log((double)x);
        case IBH_EW_LOG2: return (float)log2((double)x);
        case IBH_EW_LOG10: return (float)log10((double)x);
        case IBH_EW_SIN: return (float)sin((double)x);
        case IBH_EW_COS: return (float)cos((double)x);
        case IBH_EW_TANH: return (float)tanh((double)x);
        default: return (float)atan((double)x);
    }
}
__device__ __forceinline__ float ew2d(int op, float a, float b) {
    // C's pow already has Julia's special cases: 1^y = 1 and x^0 = 1 for NaN, the sign of a negative base under an
    // integer exponent; a negative base under a non-integer one is NaN (Julia: DomainError)
    if (op == IBH_EW_POW) return (float)pow((double)a, (double)b);
    return (float)atan2((double)a, (double)b);
}
__device__ __forceinline__ bool rounded1(int op) { return op >= IBH_EW_EXP && op <= IBH_EW_ATAN; }
__device__ __forceinline__ bool rounded2(int op) { return op == IBH_EW_POW || op == IBH_EW_ATAN2; }

// DM: the program uses a rounded operation (the host knows); without, the double code is not compiled in
template <bool DM>
__device__ __forceinline__ float ew1x(int op, float x) {
    if (DM && rounded1(op)) return ew1d(op, x);
    switch (op) {
        case IBH_EW_ABS: return fabsf(x);
        case IBH_EW_NEG: return -x;
        case IBH_EW_SQRT: return sqrtf(x);
        case IBH_EW_COPY: return x;
        // sign(x) = ifelse(x < 0, -1, ifelse(x > 0, 1, x)): keeps +-0 and NaN
        case IBH_EW_SIGN: return x < 0.0f ? -1.0f : x > 0.0f ? 1.0f : x;
        case IBH_EW_INV: return 1.0f / x;
        case IBH_EW_NOT: return b2f(x == 0.0f);
        // Base.literal_pow: x^0 = one(x) (also for NaN), x^2 = x*x, x^3 = (x*x)*x, x^-2 = (i = inv(x); i*i)
        case IBH_EW_POW0: return 1.0f;
        case IBH_EW_SQR: return x * x;
        case IBH_EW_CUBE: return (x * x) * x;
        default: {
            const float i = 1.0f / x;
            return i * i;
        }
    }
}

template <bool DM>
__device__ __forceinline__ float ew2x(int op, float a, float b) {
    if (DM && rounded2(op)) return ew2d(op, a, b);
    switch (op) {
        case IBH_EW_ADD: return a + b;
        case IBH_EW_SUB: return a - b;
        case IBH_EW_MUL: return a * b;
        case IBH_EW_DIV: return a / b;
        case IBH_EW_MAX: return fmaxf(a, b);
        case IBH_EW_MIN: return fminf(a, b);
        case IBH_EW_LT: return b2f(a < b);
        case IBH_EW_LE: return b2f(a <= b);
        case IBH_EW_GT: return b2f(a > b);
        case IBH_EW_GE: return b2f(a >= b);
        case IBH_EW_EQ: return b2f(a == b);
        case IBH_EW_NE: return b2f(a != b);
        case IBH_EW_AND: return b2f(a != 0.0f && b != 0.0f);
        case IBH_EW_OR: return b2f(a != 0.0f || b != 0.0f);
        case IBH_EW_COPYSIGN: return copysignf(a, b);
        // Bool * Float (a is the Bool): ifelse(a, b, copysign(0, b)), so false * NaN == 0, false * -2 == -0
        default: return a != 0.0f ? b : copysignf(0.0f, b);
    }
}

__device__ __forceinline__ float ew3x(int op, float a, float b, float c) {
    // clamp(x, lo, hi) = ifelse(x > hi, hi, ifelse(x < lo, lo, x)): NaN stays NaN
    if (op == IBH_EW_CLAMP) return a > c ? c : a < b ? b : a;
    return a != 0.0f ? b : c;  // ifelse(cond, a, b)
}

}  // namespace ew_math

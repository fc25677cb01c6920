"""numpy statement of every elementwise opcode of ``ibh_ew_eval`` (include/ibhip.h), in Julia's Float32 semantics.

Exact operations are stated exactly (the device must match them bit for bit, NaN matching NaN); the rounded ones are
``float32(f(float64(x)))``, which the device must meet within 2 ulp.  Bool values are Float32 0 / 1, as on the device.
Departure from Julia: where Julia throws a DomainError (``log(-1f0)``, ``(-2f0)^0.5f0``) the result is NaN."""
import numpy as np

from ibamd import hiparray as H

f32, f64 = np.float32, np.float64


def _b(c):
    return np.asarray(c).astype(f32)


def _d(fn):
    def g(*xs):
        with np.errstate(all="ignore"):
            return fn(*(np.asarray(x, dtype=f32).astype(f64) for x in xs)).astype(f32)
    return g


def _pow(a, b):
    # C / Julia pow in double, rounded once: 1^y = 1 and x^0 = 1 also for NaN (numpy's double pow already does both)
    with np.errstate(all="ignore"):
        return np.power(np.asarray(a, f32).astype(f64), np.asarray(b, f32).astype(f64)).astype(f32)


def _sign(x):
    x = np.asarray(x, f32)
    return np.where(x < 0, f32(-1), np.where(x > 0, f32(1), x)).astype(f32)


def _inv(x):
    with np.errstate(all="ignore"):
        return (f32(1) / np.asarray(x, f32)).astype(f32)


def _invsqr(x):
    i = _inv(x)
    return (i * i).astype(f32)


def _bmul(b, x):
    x = np.asarray(x, f32)
    return np.where(np.asarray(b) != 0, x, np.copysign(f32(0), x)).astype(f32)


def _clamp(x, lo, hi):
    x, lo, hi = (np.asarray(v, f32) for v in (x, lo, hi))
    return np.where(x > hi, hi, np.where(x < lo, lo, x)).astype(f32)


EXACT = {
    H.LT: lambda a, b: _b(np.less(a, b)), H.LE: lambda a, b: _b(np.less_equal(a, b)),
    H.GT: lambda a, b: _b(np.greater(a, b)), H.GE: lambda a, b: _b(np.greater_equal(a, b)),
    H.EQ: lambda a, b: _b(np.equal(a, b)), H.NE: lambda a, b: _b(np.not_equal(a, b)),
    H.AND: lambda a, b: _b((np.asarray(a) != 0) & (np.asarray(b) != 0)),
    H.OR: lambda a, b: _b((np.asarray(a) != 0) | (np.asarray(b) != 0)),
    H.COPYSIGN: lambda a, b: np.copysign(np.asarray(a, f32), np.asarray(b, f32)).astype(f32),
    H.BMUL: _bmul,
    H.SIGN: _sign, H.INV: _inv, H.NOT: lambda a: _b(np.asarray(a) == 0),
    H.POW0: lambda a: np.ones_like(np.asarray(a, f32)),
    H.SQR: lambda a: (np.asarray(a, f32) * np.asarray(a, f32)).astype(f32),
    H.CUBE: lambda a: ((np.asarray(a, f32) * np.asarray(a, f32)) * np.asarray(a, f32)).astype(f32),
    H.INVSQR: _invsqr,
    H.CLAMP: _clamp,
    H.IFELSE: lambda c, a, b: np.where(np.asarray(c) != 0, np.asarray(a, f32), np.asarray(b, f32)).astype(f32),
}
ROUNDED = {
    H.POW: _pow, H.ATAN2: _d(np.arctan2),
    H.EXP: _d(np.exp), H.EXP2: _d(np.exp2), H.LOG: _d(np.log), H.LOG2: _d(np.log2), H.LOG10: _d(np.log10),
    H.SIN: _d(np.sin), H.COS: _d(np.cos), H.TANH: _d(np.tanh), H.ATAN: _d(np.arctan),
}
ARITY = {op: fn.__code__.co_argcount if hasattr(fn, "__code__") else 1 for op, fn in EXACT.items()}
ARITY.update({op: 2 for op in (H.POW, H.ATAN2)})
ARITY.update({op: 1 for op in (H.EXP, H.EXP2, H.LOG, H.LOG2, H.LOG10, H.SIN, H.COS, H.TANH, H.ATAN)})


def model(op, *args):
    """The value of opcode ``op`` on Float32 operands (numpy arrays or scalars)."""
    return (EXACT.get(op) or ROUNDED[op])(*args)


def compare_exact(x, op, s):
    """``x OP s`` for a Float32 x against a Float64 scalar s, compared exactly (Julia's mixed-precision comparison)."""
    x = np.asarray(x, f32).astype(f64)
    fn = {H.LT: np.less, H.LE: np.less_equal, H.GT: np.greater, H.GE: np.greater_equal, H.EQ: np.equal,
          H.NE: np.not_equal}[op]
    return fn(x, f64(s))


def ulp_distance(a, b):
    """Distance in Float32 ulps (0 where both are NaN or equal; a huge value where only one is NaN)."""
    a, b = np.asarray(a, f32), np.asarray(b, f32)

    def key(x):
        i = x.view(np.int32).astype(np.int64)
        return np.where(i < 0, np.int64(-2 ** 31) - i, i)

    d = np.abs(key(a) - key(b))
    both = np.isnan(a) & np.isnan(b)
    one = np.isnan(a) ^ np.isnan(b)
    return np.where(both, 0, np.where(one, 2 ** 40, d))


def same_bits(a, b):
    """Equal bit for bit, NaN matching NaN (the payload is not Julia's to define)."""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return a.shape == b.shape and bool(np.all(ulp_distance(a, b) == 0) and
                                       np.array_equal(np.signbit(a) & ~np.isnan(a), np.signbit(b) & ~np.isnan(b)))

"""numpy models of the explicit Euler step around the fused sweeps (``ibh_timestep_euler``, ``ibh_update_euler``), built
from the oracle's operators (imported, not edited), in Float32 -- the device's operation order -- and in float64 with the
same structure.

Time step (test/advection.jl:52-59, :65 with the acoustic speed in place of C):

    C_d      = abs(u_d) + speed_of_sound(fluid, T)                       sqrt(gamma R max(T, 10))
    per[c]   = max_d unsigned_green_gauss(at_faces(C_d, d), d)[c]
    dt_cells = (0.5 / per) * scale          dt = (0.5 / max_c per) * scale

(``0.5 / max`` first, then ``* scale``: advection.jl:53 and :65, the order of ``ibh_timestep_advection``).

Update: ``state2primitive(primitive2state(P) + R * dt)`` with the oracle's two functions; ``dt`` a scalar or one per row.
"""
import numpy as np

from oracle import cfd as ocfd
from oracle import domain as od

f32, f64 = np.float32, np.float64
EPS32 = float(np.finfo(f32).eps)


def fluid_of(dtype):
    """The oracle's air with its Float32 constants, as ``dtype`` (the float64 model computes with the same numbers)."""
    f = ocfd.Fluid()
    return ocfd.Fluid(R=dtype(f.R), gamma=dtype(f.gamma))


def wave_speeds(P, dtype=f32):
    """(nc, nd): abs(u_d) + a."""
    P = np.asarray(P).astype(dtype)
    a = ocfd.speed_of_sound(fluid_of(dtype), P[:, 1])
    C = np.abs(P[:, 2:]) + a[:, None]
    assert C.dtype == dtype
    return np.ascontiguousarray(C)


def percell_max(op, C):
    """max_d unsigned_green_gauss(at_faces(C_d, d), d) per cell, in C's dtype (``op``: an oracle view of the partition)."""
    per = None
    for d in range(1, op.ndims + 1):
        a = od.unsigned_green_gauss(op, od.at_faces(op, np.ascontiguousarray(C[:, d - 1]), d), d)
        assert a.dtype == C.dtype
        per = a if per is None else np.maximum(per, a)
    return per


def timestep(op, P, scale=1.0, dtype=f32):
    """(dt, dt_cells) of the model in ``dtype``."""
    per = percell_max(op, wave_speeds(P, dtype))
    with np.errstate(divide="ignore"):
        cells = (dtype(0.5) / per) * dtype(scale)
        dt = (dtype(0.5) / per.max()) * dtype(scale)
    assert cells.dtype == dtype
    return dtype(dt), cells


def update(P, R, dt, dtype=f32):
    """state2primitive(primitive2state(P) + R * dt); dt a scalar or (n,)."""
    fl = fluid_of(dtype)
    P, R = np.asarray(P).astype(dtype), np.asarray(R).astype(dtype)
    dt = np.asarray(dt).astype(dtype)
    h = dt.reshape(-1, 1) if dt.ndim else dt
    with np.errstate(all="ignore"):
        Q = ocfd.primitive2state(fl, P)
        Q = Q + R * h
        out = ocfd.state2primitive(fl, Q)
    assert out.dtype == dtype
    return out


def update_scale(P, R, dt):
    """Per-element scale of the update's rounding error, from the float64 model's own intermediates: the magnitudes that
    enter each output before any cancellation,
        p:   (gamma - 1) (|E'| + |rho'| k')          T:   that / (|rho'| R)
        u_j: |u_j'| + (|rho u_j| + |dt R_j|) / |rho'|
    (' = after the update).  A row whose float64 result is not finite has scale NaN (compared by pattern, not by size)."""
    fl = fluid_of(f64)
    P, R = np.asarray(P).astype(f64), np.asarray(R).astype(f64)
    dt = np.asarray(dt).astype(f64)
    h = dt.reshape(-1, 1) if dt.ndim else dt
    with np.errstate(all="ignore"):
        Q0 = ocfd.primitive2state(fl, P)
        Q = Q0 + R * h
        rho = np.abs(Q[:, 0])
        u = Q[:, 2:] / Q[:, :1]
        k = 0.5 * (u * u).sum(axis=1)
        sp = (fl.gamma - 1.0) * (np.abs(Q[:, 1]) + rho * k)
        S = np.empty_like(P)
        S[:, 0] = sp
        S[:, 1] = sp / (rho * fl.R)
        S[:, 2:] = np.abs(u) + (np.abs(Q0[:, 2:]) + np.abs(R[:, 2:] * h)) / rho[:, None]
    return S


def update_deviation(got, P, R, dt):
    """max over the finite elements of |got - float64 model| / update_scale, in units of the Float32 epsilon."""
    ref = update(P, R, dt, f64)
    S = update_scale(P, R, dt)
    ok = np.isfinite(ref) & np.isfinite(S) & (S > 0)
    assert np.array_equal(np.isfinite(np.asarray(got))[ok], np.ones(int(ok.sum()), bool)), "non-finite where the model is finite"
    return float((np.abs(np.asarray(got).astype(f64) - ref)[ok] / S[ok]).max()) / EPS32


def synthetic_rows(n, nd, seed=5, per_cell=False):
    """(P, R, dt) for the update alone: rows drawn from the regimes' ranges -- p = 1e5 (1 +- 5 %), T = 288 (1 +- 5 %) with
    every eighth row cold (T in 5 .. 15: both sides of the clamp), velocities up to +-3 a with every fifth row at rest --
    and residuals that change each conserved variable by up to 10 % of its size in one step of dt ~ 1e-4."""
    rng = np.random.default_rng(seed)
    P = np.empty((n, nd + 2), f64)
    P[:, 0] = 1e5 * (1 + 0.05 * rng.uniform(-1, 1, n))
    P[:, 1] = 288.15 * (1 + 0.05 * rng.uniform(-1, 1, n))
    cold = np.arange(n) % 8 == 3
    P[cold, 1] = 10 * (1 + 0.5 * rng.uniform(-1, 1, int(cold.sum())))
    P[:, 2:] = 1000.0 * rng.uniform(-1, 1, (n, nd))
    P[np.arange(n) % 5 == 1, 2:] = 0
    P = P.astype(f32)
    Q = ocfd.primitive2state(fluid_of(f64), P.astype(f64))
    dt0 = 1e-4
    R = 0.1 * rng.uniform(-1, 1, Q.shape) * np.maximum(np.abs(Q), np.abs(Q[:, :1]) * 100.0 * (np.arange(nd + 2) >= 2)) / dt0
    dt = (dt0 * (1 + 0.5 * rng.uniform(-1, 1, n))).astype(f32) if per_cell else f32(dt0)
    return P, R.astype(f32), dt


# max over synthetic_rows(20000, nd) of the FLOAT32 MODEL's deviation from the float64 model, in Float32 epsilons under
# update_scale -- measured by tests/test_euler_step_model.py::test_float32_model_deviation, which holds the constant to
# the measurement from both sides.  The device check (tests/test_gpu_euler_step.py) allows 4 x this: the margin the LES
# and k-epsilon checks use for the same reason, rounding order inside a sum.
MODEL_DEVIATION_EPS = {2: 2.4, 3: 2.3}

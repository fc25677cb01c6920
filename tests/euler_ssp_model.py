"""numpy model of one Shu-Osher stage of a strong-stability-preserving Runge-Kutta scheme (``ibh_update_euler_ssp``,
``ibh_stage_euler_ssp``), built on the pieces of ``euler_step_model``:

    h     = c * dt                                    rounded once
    Q_new = (primitive2state(P0) * a + primitive2state(P) * b) + R * h
    P_out = state2primitive(Q_new)

``a``, ``b``, ``c`` are Float32 scalars on the device whatever the model's precision (the entry takes ``float``s).  ``dt`` is
a scalar or one value per row.  ``linear_step`` and ``integrate`` apply the stages of whole steps to scalar test equations in
float64 / complex128, in the Shu-Osher form (triples) or the low-storage form (plain coefficients).
"""
import numpy as np

import euler_step_model as em
from oracle import cfd as ocfd

f32, f64 = np.float32, np.float64


def update_ssp(P0, P, R, dt, a, b, c, dtype=f32):
    """state2primitive((primitive2state(P0) * a + primitive2state(P) * b) + R * (c * dt)); dt a scalar or (n,)."""
    fl = em.fluid_of(dtype)
    P0, P, R = (np.asarray(x).astype(dtype) for x in (P0, P, R))
    a, b, c = (dtype(f32(x)) for x in (a, b, c))
    h = (np.asarray(dt).astype(dtype) * c).astype(dtype)
    h = h.reshape(-1, 1) if h.ndim else h
    with np.errstate(all="ignore"):
        Q0, Q = ocfd.primitive2state(fl, P0), ocfd.primitive2state(fl, P)
        Qn = (Q0 * a + Q * b) + R * h
        out = ocfd.state2primitive(fl, Qn)
    assert out.dtype == dtype
    return out


def update_ssp_scale(P0, P, R, dt, a, b, c):
    """``euler_step_model.update_scale`` for a blended base state: the magnitudes that enter each output before any
    cancellation, from the float64 model's own intermediates,
        p:   (gamma - 1) (|E'| + |rho'| k')          T:   that / (|rho'| R)
        u_j: |u_j'| + (|a rho0 u0_j| + |b rho u_j| + |c dt R_j|) / |rho'|
    (' = after the update)."""
    fl = em.fluid_of(f64)
    P0, P, R = (np.asarray(x).astype(f64) for x in (P0, P, R))
    a, b, c = (f64(f32(x)) for x in (a, b, c))
    h = np.asarray(dt).astype(f64) * c
    h = h.reshape(-1, 1) if h.ndim else h
    with np.errstate(all="ignore"):
        Q0, Q1 = ocfd.primitive2state(fl, P0), ocfd.primitive2state(fl, P)
        Q = (Q0 * a + Q1 * b) + R * h
        rho = np.abs(Q[:, 0])
        u = Q[:, 2:] / Q[:, :1]
        k = 0.5 * (u * u).sum(axis=1)
        sp = (fl.gamma - 1.0) * (np.abs(Q[:, 1]) + rho * k)
        S = np.empty_like(P)
        S[:, 0] = sp
        S[:, 1] = sp / (rho * fl.R)
        S[:, 2:] = np.abs(u) + (np.abs(Q0[:, 2:] * a) + np.abs(Q1[:, 2:] * b) + np.abs(R[:, 2:] * h)) / rho[:, None]
    return S


def update_ssp_deviation(got, P0, P, R, dt, a, b, c):
    """max over the finite elements of |got - float64 model| / update_ssp_scale, in units of the Float32 epsilon: the scale
    ``euler_step_model.update_deviation`` uses, to which it reduces for (a, b) = (0, 1)."""
    ref = update_ssp(P0, P, R, dt, a, b, c, f64)
    S = update_ssp_scale(P0, P, R, dt, a, b, c)
    ok = np.isfinite(ref) & np.isfinite(S) & (S > 0)
    assert np.isfinite(np.asarray(got))[ok].all(), "non-finite where the model is finite"
    return float((np.abs(np.asarray(got).astype(f64) - ref)[ok] / S[ok]).max()) / em.EPS32


def second_rows(n, nd, per_cell=False):
    """(P0, P, R, dt): the rows of ``euler_step_model.synthetic_rows`` as the swept state ``P`` with their residuals, and a
    second row set (another seed) as the base state ``P0``."""
    P, R, dt = em.synthetic_rows(n, nd, per_cell=per_cell)
    P0, _, _ = em.synthetic_rows(n, nd, seed=11)
    return P0, P, R, dt


def _is_triples(stages):
    return any(isinstance(s, (tuple, list)) for s in stages)


def rk_step(f, y, dt, stages):
    """One step of y' = f(y): ``stages`` (a, b, c) triples -- y_k = a y_0 + b y_{k-1} + c dt f(y_{k-1}) -- or plain
    coefficients alpha_k of the low-storage form y_k = y_0 + alpha_k dt f(y_{k-1})."""
    y0 = yk = y
    if _is_triples(stages):
        for a, b, c in stages:
            yk = a * y0 + b * yk + c * dt * f(yk)
    else:
        for al in stages:
            yk = y0 + al * dt * f(yk)
    return yk


def linear_step(y, z, stages):
    """One step on y' = lambda y with z = lambda dt, in complex128."""
    return rk_step(lambda v: complex(z) * v, complex(y), 1.0, stages)


def integrate(f, y0, t_end, nsteps, stages):
    """y(t_end) by ``nsteps`` equal steps, in float64."""
    y, dt = f64(y0), f64(t_end) / nsteps
    for _ in range(nsteps):
        y = rk_step(f, y, dt, stages)
    return y

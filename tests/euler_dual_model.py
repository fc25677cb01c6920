"""numpy model of dual time stepping (``ibh_dual_source``, ``ibh_update_euler_dual``, ``ibh_stage_euler_dual``,
``solver.DualTimeMarch``), built on the pieces of ``euler_step_model``.  With ``dQ/dt = R(P)``, ``Q = primitive2state(P)``, a
physical step of size ``dt_real`` solves the backward-difference equation

    g Q^{n+1} = R(P^{n+1}) + S,      S = cn Q^n + cm Q^{n-1}
    BDF2: (cn, cm, g) = (2, -0.5, 1.5) / dt_real          BDF1: (1, 0, 1) / dt_real

by a march in pseudo-time whose stage takes ``g Q`` point-implicitly:

    h     = alpha * dtau                                  rounded once
    Q_new = (primitive2state(P0) + (R + S) * h) / (1 + h * g)
    P_out = state2primitive(Q_new)

every sum, product and the divide rounded on its own.  ``alpha``, ``g``, ``cn``, ``cm`` are Float32 scalars on the device
whatever the model's precision (the entries take ``float``s).  ``dtau`` is a scalar or one value per row.  ``march_scalar``
applies the whole scheme to ``y' = -y^2`` in float64, where the backward-difference equation has a closed form.
"""
import numpy as np

import euler_ssp_model as sp
import euler_step_model as em
from oracle import cfd as ocfd

f32, f64 = np.float32, np.float64


def bdf_coefficients(order, dt_real, dtype=f32):
    """(cn, cm, g) of the backward difference of ``order`` 1 or 2, computed in float64 and rounded once to ``dtype``."""
    if order not in (1, 2):
        raise ValueError("order must be 1 or 2")
    w = (2.0, -0.5, 1.5) if order == 2 else (1.0, 0.0, 1.0)
    return tuple(dtype(x / f64(dt_real)) for x in w)


def dual_source(Pn, Pm, cn, cm, dtype=f32):
    """primitive2state(Pn) * cn + primitive2state(Pm) * cm, or primitive2state(Pn) * cn with ``Pm`` None."""
    fl = em.fluid_of(dtype)
    cn, cm = dtype(f32(cn)), dtype(f32(cm))
    with np.errstate(all="ignore"):
        S = ocfd.primitive2state(fl, np.asarray(Pn).astype(dtype)) * cn
        if Pm is not None:
            S = S + ocfd.primitive2state(fl, np.asarray(Pm).astype(dtype)) * cm
    assert S.dtype == dtype
    return S


def _h(dt, alpha, dtype):
    h = (np.asarray(dt).astype(dtype) * dtype(f32(alpha))).astype(dtype)
    return h.reshape(-1, 1) if h.ndim else h


def update_dual(P0, R, S, dt, alpha, g, dtype=f32):
    """state2primitive((primitive2state(P0) + (R + S) * h) / (1 + h * g)), h = alpha * dt; dt a scalar or (n,)."""
    fl = em.fluid_of(dtype)
    P0, R, S = (np.asarray(x).astype(dtype) for x in (P0, R, S))
    h, g = _h(dt, alpha, dtype), dtype(f32(g))
    with np.errstate(all="ignore"):
        Q = ocfd.primitive2state(fl, P0)
        Q = (Q + (R + S) * h) / (h * g + dtype(1))
        out = ocfd.state2primitive(fl, Q)
    assert out.dtype == dtype
    return out


def update_dual_scale(P0, R, S, dt, alpha, g):
    """``euler_step_model.update_scale`` for the dual update: the magnitudes that enter each output before any cancellation,
    from the float64 model's own intermediates.  A conserved variable enters with A_v = (|Q0_v| + (|R_v| + |S_v|) h) / (1 + h g)
    -- the three terms of its numerator, which R against S and both against Q0 may cancel -- so
        p:   (gamma - 1) (A_E + A_rho k')          T:   that / (|rho'| R)          u_j: |u_j'| + A_j / |rho'|
    (' = after the update).  With S = 0 and g = 0 and no cancellation in E and rho it is ``update_scale``."""
    fl = em.fluid_of(f64)
    P0, R, S = (np.asarray(x).astype(f64) for x in (P0, R, S))
    h, g = _h(dt, alpha, f64), f64(f32(g))
    with np.errstate(all="ignore"):
        Q0 = ocfd.primitive2state(fl, P0)
        den = h * g + 1.0
        Q = (Q0 + (R + S) * h) / den
        A = (np.abs(Q0) + (np.abs(R) + np.abs(S)) * h) / den
        rho = np.abs(Q[:, 0])
        u = Q[:, 2:] / Q[:, :1]
        k = 0.5 * (u * u).sum(axis=1)
        sc = (fl.gamma - 1.0) * (A[:, 1] + A[:, 0] * k)
        out = np.empty_like(P0)
        out[:, 0] = sc
        out[:, 1] = sc / (rho * fl.R)
        out[:, 2:] = np.abs(u) + A[:, 2:] / rho[:, None]
    return out


def update_dual_deviation(got, P0, R, S, dt, alpha, g):
    """max over the finite elements of |got - float64 model| / update_dual_scale, in units of the Float32 epsilon."""
    ref = update_dual(P0, R, S, dt, alpha, g, f64)
    sc = update_dual_scale(P0, R, S, dt, alpha, g)
    ok = np.isfinite(ref) & np.isfinite(sc) & (sc > 0)
    assert np.isfinite(np.asarray(got))[ok].all(), "non-finite where the model is finite"
    return float((np.abs(np.asarray(got).astype(f64) - ref)[ok] / sc[ok]).max()) / em.EPS32


DT0 = 1e-4   # the time step of ``euler_step_model.synthetic_rows`` (per cell: within +-50 % of it)


def dual_rows(n, nd, per_cell=False):
    """(P0, R, S, dt, g): ``euler_ssp_model.second_rows`` -- ``P0`` the base state, ``R`` the residuals of the other row set
    ``P`` -- with the BDF2 source of a physical step of 8 x the rows' time step, ``P0`` as Q^n and ``P`` as Q^{n-1}, in
    Float32 (what the device is handed), and that step's ``g``.  (R up to 0.1 |Q| / dt against S ~ 0.19 |Q| / dt: the sum
    R + S cancels in part.)"""
    P0, P, R, dt = sp.second_rows(n, nd, per_cell)
    cn, cm, g = bdf_coefficients(2, 8 * DT0)
    return P0, R, dual_source(P0, P, cn, cm, f32), dt, g


# max over dual_rows(20000, nd), global and per-cell dt, alpha in (1, 1/3), of the FLOAT32 MODEL's deviation from the float64
# model, in Float32 epsilons under update_dual_scale -- measured by
# tests/test_euler_dual_model.py::test_float32_model_deviation, which holds the constant to the measurement from both sides.
# The device check (tests/test_gpu_euler_dual.py) allows 4 x this: the margin ``update_euler`` and ``update_euler_stage`` are
# held to, for rounding order inside a sum.
MODEL_DEVIATION_EPS = {2: 2.7, 3: 2.7}      # (measured: 2.592, 2.605)


# ---------------------------------------------------------------------------------------------------------------------
# the scheme on y' = R(y) = -y^2, y(0) = 1: y(t) = 1 / (1 + t)
# ---------------------------------------------------------------------------------------------------------------------
def bdf_exact_step(S, g):
    """The solution y > 0 of the backward-difference equation g y = -y^2 + S."""
    return 0.5 * (-g + np.sqrt(g * g + 4.0 * S))


def inner_iterations(y, S, g, stages, n_inner, cfl=0.9):
    """``n_inner`` pseudo-steps from ``y``: the local pseudo-time step ``cfl / |dR/dq|`` from the pseudo-step's input, then
    the stages q_k = (q_0 + (R(q_{k-1}) + S) h) / (1 + h g), h = alpha_k dtau."""
    q = f64(y)
    for _ in range(n_inner):
        q0, dtau = q, cfl / abs(2.0 * q)
        for alpha in stages:
            h = alpha * dtau
            q = (q0 + (-q * q + S) * h) / (1.0 + h * g)
    return q


def march_scalar(nsteps, order, stages=None, n_inner=40, t_end=1.0):
    """y(t_end) by ``nsteps`` physical steps in float64: BDF1 on the first step, BDF ``order`` afterwards; every step solved
    by ``inner_iterations`` from y^n, or in closed form with ``stages=None``.  Returns the list of all y^n."""
    dt = f64(t_end) / nsteps
    ys = [f64(1.0)]
    for n in range(nsteps):
        cn, cm, g = bdf_coefficients(1 if n == 0 else order, dt, f64)
        S = cn * ys[-1] + (cm * ys[-2] if n > 0 else 0.0)
        ys.append(bdf_exact_step(S, g) if stages is None else inner_iterations(ys[-1], S, g, stages, n_inner))
    return ys

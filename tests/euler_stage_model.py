"""numpy model of one Runge-Kutta stage of the low-storage family (``ibh_update_euler_stage``, ``ibh_stage_euler``), built on
``euler_step_model.update``:

    P_out = state2primitive(primitive2state(P0) + R * (alpha * dt))

``alpha`` is a Float32 scalar on the device whatever the model's precision (the entry takes a ``float``), and the product
``alpha * dt`` is rounded once in the model's ``dtype`` before it multiplies ``R`` -- the broadcast ``dt .* alpha`` followed
by ``update_euler``.  ``dt`` is a scalar or one value per row.  ``march`` applies the stages of a whole step to a linear
test equation.
"""
import numpy as np

import euler_step_model as em

f32, f64 = np.float32, np.float64


def stage_dt(dt, alpha, dtype=f32):
    """alpha * dt in ``dtype``; alpha enters as the Float32 the device receives."""
    return (np.asarray(dt).astype(dtype) * dtype(f32(alpha))).astype(dtype)


def update_stage(P0, R, dt, alpha, dtype=f32):
    """state2primitive(primitive2state(P0) + R * (alpha * dt)); dt a scalar or (n,)."""
    return em.update(P0, R, stage_dt(dt, alpha, dtype), dtype)


def update_stage_deviation(got, P0, R, dt, alpha):
    """``euler_step_model.update_deviation`` of a stage: against the float64 model whose time step is the float64 product
    of the Float32 ``alpha`` and ``dt``, on the scale of that update."""
    return em.update_deviation(got, P0, R, stage_dt(dt, alpha, f64))


def linear_step(y, z, alphas):
    """One step of the low-storage scheme on y' = lambda y with z = lambda dt: y_k = y_0 + alpha_k z y_{k-1}, in float64 /
    complex128."""
    y0 = yk = complex(y)
    for a in alphas:
        yk = y0 + float(a) * complex(z) * yk
    return yk

"""The numpy model of a Runge-Kutta stage (tests/euler_stage_model.py) against the step model it is built on, and the stage
coefficients of ``solver.rk_stages`` against the Taylor polynomial they are chosen for.  No GPU."""
import math

import numpy as np
import pytest

import euler_stage_model as sm
import euler_step_model as em
from ibamd.solver import rk_stages

f32, f64 = np.float32, np.float64


@pytest.mark.parametrize("per_cell", [False, True], ids=["global_dt", "per_cell_dt"])
@pytest.mark.parametrize("nd", [2, 3])
def test_alpha_one_on_the_same_state_is_the_step(nd, per_cell):
    P, R, dt = em.synthetic_rows(3000, nd, per_cell=per_cell)
    got, ref = sm.update_stage(P, R, dt, 1.0, f32), em.update(P, R, dt, f32)
    assert got.dtype == f32 and np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(sm.update_stage(P, R, dt, 1.0, f64), em.update(P, R, dt, f64))


@pytest.mark.parametrize("nd", [2, 3])
def test_stage_is_the_update_with_the_rounded_product(nd):
    """The base state is P0, not the state the residual came from; the time step is fl32(alpha) * dt rounded once."""
    P0, R, dt = em.synthetic_rows(3000, nd, per_cell=True)
    a = f32(1.0 / 3.0)
    h = dt * a
    assert h.dtype == f32
    assert np.array_equal(sm.update_stage(P0, R, dt, 1.0 / 3.0, f32), em.update(P0, R, h, f32))
    # float64: alpha is still the Float32 the entry receives
    assert np.array_equal(sm.update_stage(P0, R, dt, 1.0 / 3.0, f64), em.update(P0, R, dt.astype(f64) * f64(a), f64))
    # the Float32 model of a stage stays within the step model's own deviation from float64
    dev = sm.update_stage_deviation(sm.update_stage(P0, R, dt, 1.0 / 3.0, f32), P0, R, dt, 1.0 / 3.0)
    print(f"nd={nd}: Float32 stage model deviates {dev:.3f} eps from the float64 model")
    assert dev <= 4 * em.MODEL_DEVIATION_EPS[nd]


def test_rk_stages_values():
    assert rk_stages(1) == (1.0,)
    assert rk_stages(4) == (1.0 / 4, 1.0 / 3, 1.0 / 2, 1.0)
    for m in range(1, 6):
        assert rk_stages(m) == tuple(1.0 / (m - k + 1) for k in range(1, m + 1))
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            rk_stages(bad)


@pytest.mark.parametrize("z", [-1.5, -0.3 + 0.7j])
@pytest.mark.parametrize("m", [1, 2, 3, 4, 5])
def test_amplification_factor_is_the_taylor_polynomial(m, z):
    got = sm.linear_step(1.0, z, rk_stages(m))
    ref = sum(complex(z) ** j / math.factorial(j) for j in range(m + 1))
    assert abs(got - ref) <= 1e-14 * abs(ref), (m, z, got, ref)

"""The numpy model of a Shu-Osher stage (tests/euler_ssp_model.py) against the stage model it generalises, and the triples of
``solver.ssp_stages``: their values, their convexity, their linear amplification factor and their order on a nonlinear
equation.  No GPU."""
import math
from fractions import Fraction

import numpy as np
import pytest

import euler_ssp_model as sp
import euler_stage_model as sm
import euler_step_model as em
from ibamd.solver import rk_stages, ssp_stages

f32, f64 = np.float32, np.float64


def test_ssp_stages_values():
    assert ssp_stages(2) == ((0, 1, 1), (1 / 2, 1 / 2, 1 / 2))
    assert ssp_stages(3) == ((0, 1, 1), (3 / 4, 1 / 4, 1 / 4), (1 / 3, 2 / 3, 2 / 3))
    for bad in (0, 1, 4, 2.5, True, "3", None):
        with pytest.raises(ValueError):
            ssp_stages(bad)


@pytest.mark.parametrize("order", [2, 3])
def test_every_stage_is_a_convex_combination(order):
    """a, b >= 0, a + b == 1 and c == b in exact rationals: a stage is a convex combination of the step's input and one
    forward-Euler step of the previous stage, which is what makes the scheme strong-stability-preserving with CFL
    coefficient 1."""
    for a, b, c in ssp_stages(order):
        fa, fb, fc = (Fraction(x).limit_denominator(12) for x in (a, b, c))
        assert (float(fa), float(fb), float(fc)) == (a, b, c)          # the doubles are the nearest to these rationals
        assert fa >= 0 and fb >= 0 and fa + fb == 1 and fc == fb, (a, b, c)


@pytest.mark.parametrize("z", [-1.5, -0.3 + 0.7j])
@pytest.mark.parametrize("order", [2, 3])
def test_amplification_factor_is_the_taylor_polynomial(order, z):
    got = sp.linear_step(1.0, z, ssp_stages(order))
    ref = sum(complex(z) ** j / math.factorial(j) for j in range(order + 1))
    assert abs(got - ref) <= 1e-14 * abs(ref), (order, z, got, ref)


def test_nonlinear_order():
    """y' = -y^2, y(0) = 1, to t = 1 (y = 1/2) in float64 with 16, 32 and 64 steps: halving the step divides the error by 4
    (SSPRK2), 8 (SSPRK3) -- and by 4 only for the three-stage low-storage scheme, which is third-order on linear problems
    alone.  Observed ratios 16 -> 32 and 32 -> 64: ssp2 4.09, 4.05; ssp3 8.29, 8.14; rk_stages(3) 3.55, 3.80 -- all within
    15 % of the nominal factor."""
    for name, stages, factor in (("ssp2", ssp_stages(2), 4.0), ("ssp3", ssp_stages(3), 8.0), ("rk3", rk_stages(3), 4.0)):
        err = [abs(sp.integrate(lambda y: -y * y, 1.0, 1.0, n, stages) - 0.5) for n in (16, 32, 64)]
        ratios = (err[0] / err[1], err[1] / err[2])
        print(f"{name}: errors {err[0]:.3e} {err[1]:.3e} {err[2]:.3e}, ratios {ratios[0]:.3f} {ratios[1]:.3f}")
        for r in ratios:
            assert abs(r - factor) <= 0.15 * factor, (name, ratios)


@pytest.mark.parametrize("per_cell", [False, True], ids=["global_dt", "per_cell_dt"])
@pytest.mark.parametrize("nd", [2, 3])
def test_no_blend_is_the_low_storage_stage(nd, per_cell):
    """(a, b, c) = (0, 1, c) on finite rows without zero components: Q0 * 0 is +-0 and adds nothing, so the bits are
    ``update_stage(P, R, dt, c)``'s, whatever finite P0 is."""
    P0, P, R, dt = sp.second_rows(3000, nd, per_cell)
    keep = np.isfinite(P).all(axis=1) & np.isfinite(P0).all(axis=1) & (P != 0).all(axis=1) & (R != 0).all(axis=1)
    assert keep.sum() > 2000
    P0, P, R = P0[keep], P[keep], R[keep]
    dt = dt[keep] if per_cell else dt
    for c in (1.0, 0.25, 2.0 / 3.0):
        got, ref = sp.update_ssp(P0, P, R, dt, 0.0, 1.0, c, f32), sm.update_stage(P, R, dt, c, f32)
        assert got.dtype == f32 and np.array_equal(got.view(np.uint32), ref.view(np.uint32)), c


@pytest.mark.parametrize("nd", [2, 3])
def test_model_structure_and_deviation(nd):
    """The coefficients enter as the Float32 the device receives, c * dt is rounded once, and the Float32 model stays within
    a few epsilons of the float64 model on the update's own scale."""
    P0, P, R, dt = sp.second_rows(3000, nd, per_cell=True)
    a, b, c = 1.0 / 3.0, 2.0 / 3.0, 2.0 / 3.0
    fl = em.fluid_of(f32)
    from oracle import cfd as ocfd
    with np.errstate(all="ignore"):
        Q0, Q = ocfd.primitive2state(fl, P0), ocfd.primitive2state(fl, P)
        h = (dt * f32(c)).reshape(-1, 1)
        assert h.dtype == f32
        ref = ocfd.state2primitive(fl, (Q0 * f32(a) + Q * f32(b)) + R * h)
    got = sp.update_ssp(P0, P, R, dt, a, b, c, f32)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    dev = sp.update_ssp_deviation(got, P0, P, R, dt, a, b, c)
    print(f"nd={nd}: Float32 Shu-Osher stage model deviates {dev:.3f} eps from the float64 model")
    assert dev <= 4 * em.MODEL_DEVIATION_EPS[nd]
    # with no blend the scale is the step model's
    S = sp.update_ssp_scale(P0, P, R, dt, 0.0, 1.0, c)
    assert np.allclose(S, em.update_scale(P, R, sm.stage_dt(dt, c, f64)), rtol=1e-13, equal_nan=True)

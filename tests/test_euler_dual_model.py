"""The numpy model of dual time stepping (tests/euler_dual_model.py): the converged inner iteration against the closed form
of the backward-difference equation on ``y' = -y^2``, the orders of BDF1 and BDF2, the reduction to the stage model, the
Float32 model's own deviation from float64 (the constant the device check is 4 x of), and the argument checks of
``solver.bdf_coefficients`` and ``solver.DualTimeMarch``, which come before anything touches the device.  No GPU."""
import numpy as np
import pytest

import euler_dual_model as dm
import euler_stage_model as sm
import euler_step_model as em
from ibamd import backend as B
from ibamd import solver
from ibamd.solver import DualTimeMarch, bdf_coefficients, rk_stages, ssp_stages

f32, f64 = np.float32, np.float64


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("m", [1, 3])
def test_converged_inner_iteration_is_the_bdf_solution(m, order):
    """40 pseudo-steps of ``rk_stages(m)`` at the local pseudo-time step 0.9 / |dR/dq| solve every physical step to 1e-12 of
    the closed form; the two marches agree to that at every step."""
    N = 20
    exact, inner = dm.march_scalar(N, order), dm.march_scalar(N, order, rk_stages(m), 40)
    dt = 1.0 / N
    for n in range(N):      # every step on its own: from the iterated history, the closed form of ITS equation
        cn, cm, g = dm.bdf_coefficients(1 if n == 0 else order, dt, f64)
        S = cn * inner[n] + (cm * inner[n - 1] if n > 0 else 0.0)
        assert abs(inner[n + 1] - dm.bdf_exact_step(S, g)) <= 1e-12, (n, inner[n + 1])
        assert abs(g * inner[n + 1] - (-inner[n + 1] ** 2 + S)) <= 1e-11 * g        # the fixed point is the BDF equation
    worst = max(abs(a - b) for a, b in zip(exact, inner))
    print(f"rk_stages({m}), BDF{order}: inner iteration within {worst:.2e} of the closed form over {N} steps")
    assert worst <= 1e-12


def test_orders_of_accuracy():
    """Halving dt_real divides the error at T = 1 by 4 with BDF2 (after one BDF1 step) and by 2 with BDF1."""
    err = {o: [abs(dm.march_scalar(N, o, rk_stages(3), 40)[-1] - 0.5) for N in (20, 40, 80)] for o in (1, 2)}
    r2 = [err[2][i] / err[2][i + 1] for i in range(2)]
    r1 = [err[1][i] / err[1][i + 1] for i in range(2)]
    print(f"BDF2 error ratios {r2[0]:.3f} {r2[1]:.3f}; BDF1 {r1[0]:.3f} {r1[1]:.3f}")
    assert all(3.8 <= r <= 4.2 for r in r2), r2
    assert all(1.9 <= r <= 2.1 for r in r1), r1


@pytest.mark.parametrize("per_cell", [False, True], ids=["global_dt", "per_cell_dt"])
@pytest.mark.parametrize("nd", [2, 3])
def test_zero_g_and_zero_source_is_the_stage(nd, per_cell):
    """g = 0, S = 0: R + 0 and Q / 1 change no value -- ``euler_stage_model.update_stage`` exactly, in Float32."""
    P0, R, dt = em.synthetic_rows(3000, nd, per_cell=per_cell)
    S = np.zeros_like(R)
    for alpha in (1.0, 1.0 / 3.0):
        got, ref = dm.update_dual(P0, R, S, dt, alpha, 0.0, f32), sm.update_stage(P0, R, dt, alpha, f32)
        assert got.dtype == f32 and np.isfinite(ref).all()
        assert (got == ref).all()


@pytest.mark.parametrize("nd", [2, 3])
def test_dual_source_and_update_are_their_formulas(nd):
    """The source is the blend of the two conserved states; the update is the formula written out per component."""
    P0, R, S, dt, g = dm.dual_rows(500, nd, per_cell=True)
    assert S.dtype == f32 and g == f32(1.5 / (8 * dm.DT0))
    P, _, _ = em.synthetic_rows(500, nd)
    from oracle import cfd as ocfd
    fl = em.fluid_of(f32)
    cn, cm, _ = dm.bdf_coefficients(2, 8 * dm.DT0)
    Qn, Qm = ocfd.primitive2state(fl, P0), ocfd.primitive2state(fl, P)
    assert np.array_equal(S, Qn * cn + Qm * cm)
    assert np.array_equal(dm.dual_source(P0, None, cn, cm), Qn * cn)
    h = (dt * f32(1.0 / 3.0)).reshape(-1, 1)
    Q = (Qn + (R + S) * h) / (h * g + f32(1))
    assert Q.dtype == f32
    assert np.array_equal(dm.update_dual(P0, R, S, dt, 1.0 / 3.0, g), ocfd.state2primitive(fl, Q))


@pytest.mark.parametrize("nd", [2, 3])
def test_float32_model_deviation(nd):
    """The constant the device bound is 4 x of: measured here, held from both sides."""
    worst = 0.0
    for per_cell in (False, True):
        P0, R, S, dt, g = dm.dual_rows(20000, nd, per_cell)
        for alpha in (1.0, 1.0 / 3.0):
            for gg in (0.0, g):
                got = dm.update_dual(P0, R, S, dt, alpha, gg, f32)
                assert got.dtype == f32 and np.isfinite(got).all()
                worst = max(worst, dm.update_dual_deviation(got, P0, R, S, dt, alpha, gg))
    print(f"nd={nd}: Float32 model deviates {worst:.3f} eps from the float64 model (constant {dm.MODEL_DEVIATION_EPS[nd]})")
    assert 0.9 * dm.MODEL_DEVIATION_EPS[nd] <= worst <= dm.MODEL_DEVIATION_EPS[nd]


def test_bdf_coefficients():
    assert bdf_coefficients(2, 0.5) == (4.0, -1.0, 3.0)
    assert bdf_coefficients(1, 0.25) == (4.0, 0.0, 4.0)
    for order in (1, 2):        # float64 arithmetic, rounded once: the model's numbers
        got = bdf_coefficients(order, 3e-4)
        assert got == tuple(float(x) for x in dm.bdf_coefficients(order, 3e-4))
        assert all(isinstance(x, float) and x == float(f32(x)) for x in got)
    for order in (0, 3, 1.5, True, None):
        with pytest.raises(ValueError, match="order"):
            bdf_coefficients(order, 1e-3)
    for dt_real in (0.0, -1e-3, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="dt_real"):
            bdf_coefficients(2, dt_real)


def test_dual_time_march_rejects_misuse_before_the_device(monkeypatch):
    """Every refused argument raises before the march asks for the partition, an array or a launch."""
    def fail(name, *a):
        pytest.fail(f"{name} was called: the argument check did not stop it")
    monkeypatch.setattr(B, "call", fail)
    monkeypatch.setattr(B, "_part", lambda p: pytest.fail("the partition was asked for before the arguments were checked"))
    part = object()
    for order in (3, 0, None, 1.5):
        with pytest.raises(ValueError, match="order"):
            DualTimeMarch(part, 1e-3, 4, order=order)
    with pytest.raises(ValueError, match="dt_real"):
        DualTimeMarch(part, 0.0, 4)
    with pytest.raises(ValueError, match="dt_real"):
        DualTimeMarch(part, float("nan"), 4)
    for n_inner in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="n_inner"):
            DualTimeMarch(part, 1e-3, n_inner)
    with pytest.raises(ValueError, match="smooth.*fixed point"):
        DualTimeMarch(part, 1e-3, 4, smoothing=(0.5, 2))
    with pytest.raises(ValueError, match="Shu-Osher"):
        DualTimeMarch(part, 1e-3, 4, stages=ssp_stages(3))
    with pytest.raises(ValueError, match="Shu-Osher"):
        DualTimeMarch(part, 1e-3, 4, stages=((0.0, 1.0, 1.0), 0.5))
    assert solver.DualTimeMarch is DualTimeMarch and issubclass(DualTimeMarch, solver.EulerMarch)

"""The numpy models of the explicit Euler step (tests/euler_step_model.py) against closed forms and against the oracle's
operators composed by hand; the Float32 model's own deviation from the float64 model, which the device check
(tests/test_gpu_euler_step.py) takes its bound from.  No GPU."""
import numpy as np
import pytest

import euler_step_model as em
import ibamd
import regimes as rg
from conftest import ADV_FAMILIES, oracle_view
from oracle import cfd as ocfd
from oracle import domain as od

f32, f64 = np.float32, np.float64


@pytest.fixture(scope="module")
def case(adv_mesh_coarse):
    dom = ibamd.Domain(adv_mesh_coarse, hypercube_families=ADV_FAMILIES, max_partition_size=10 ** 9, boundaries=False)
    (part,) = dom.partitions.values()
    return part, oracle_view(part)


def _uniform(n, nd):
    return np.tile(f32([1e5, 288.15, 100.0, -50.0, 25.0][:nd + 2]), (n, 1))


@pytest.mark.parametrize("dtype", [f32, f64])
def test_uniform_state_closed_forms(case, dtype):
    part, op = case
    n, nd = part.spacing.shape
    P = _uniform(n, nd)
    # R = 0: the update is the round trip of the model, whatever dt
    rt = ocfd.state2primitive(em.fluid_of(dtype), ocfd.primitive2state(em.fluid_of(dtype), P.astype(dtype)))
    for dt in (f32(0.0), f32(1e-3), np.full(n, 2e-3, f32)):
        assert np.array_equal(em.update(P, np.zeros_like(P), dt, dtype), rt)
    # ... and the round trip returns P to rounding
    assert np.abs(rt - P.astype(dtype)).max() <= 8 * np.finfo(dtype).eps * 1e5
    # dt_cells * max_d(...) = 0.5 scale to rounding, and dt is the smallest of them
    scale = 0.75
    dt, cells = em.timestep(op, P, scale, dtype)
    per = em.percell_max(op, em.wave_speeds(P, dtype))
    assert np.abs(cells * per - dtype(0.5 * scale)).max() <= 4 * np.finfo(dtype).eps
    assert dt == cells.min()


@pytest.mark.parametrize("regime", ["transonic", "crossing", "rest", "cold"])
@pytest.mark.parametrize("dtype", [f32, f64])
def test_dt_is_the_oracle_composition(case, regime, dtype):
    part, op = case
    P = rg.euler_regime(part, regime).astype(dtype)
    fl = em.fluid_of(dtype)
    a = ocfd.speed_of_sound(fl, P[:, 1])
    per = None
    for d in range(1, part.ndims + 1):
        Cd = np.abs(P[:, 1 + d]) + a
        g = od.unsigned_green_gauss(op, od.at_faces(op, np.ascontiguousarray(Cd), d), d)
        per = g if per is None else np.maximum(per, g)
    scale = dtype(0.75)
    dt, cells = em.timestep(op, P, scale, dtype)
    assert dt.dtype == dtype and dt == (dtype(0.5) / per.max()) * scale          # advection.jl:53, then :65
    assert abs(float(dt) - 0.5 * 0.75 / float(per.max())) <= 2 * np.finfo(dtype).eps * float(dt)
    assert np.array_equal(cells, (dtype(0.5) / per) * scale)
    if regime == "cold":
        assert (P[:, 1] < 10).mean() > 0.25      # the clamp binds: a is that of 10 K there
        assert np.array_equal(a[P[:, 1] < 10], np.full(int((P[:, 1] < 10).sum()), np.sqrt(fl.gamma * fl.R * dtype(10))))


@pytest.mark.parametrize("dtype", [f32, f64])
def test_update_with_dt_zero_is_the_round_trip(case, dtype):
    part, _ = case
    P = rg.euler_regime(part, "transonic")
    R = np.random.default_rng(3).standard_normal(P.shape).astype(f32) * 1e6
    fl = em.fluid_of(dtype)
    rt = ocfd.state2primitive(fl, ocfd.primitive2state(fl, P.astype(dtype)))
    assert np.array_equal(em.update(P, R, f32(0.0), dtype), rt)
    assert np.array_equal(em.update(P, R, np.zeros(P.shape[0], f32), dtype), rt)


@pytest.mark.parametrize("nd", [2, 3])
def test_float32_model_deviation(nd):
    """The constant the device bound is 4 x of: measured here, held from both sides."""
    worst = 0.0
    for per_cell in (False, True):
        P, R, dt = em.synthetic_rows(20000, nd, per_cell=per_cell)
        got = em.update(P, R, dt, f32)
        assert got.dtype == f32 and np.isfinite(got).all()
        assert (P[:, 1] < 10).any() and (got[:, 1] == 10).any()        # both clamps are exercised
        worst = max(worst, em.update_deviation(got, P, R, dt))
    print(f"nd={nd}: Float32 model deviates {worst:.3f} eps from the float64 model (constant {em.MODEL_DEVIATION_EPS[nd]})")
    assert 0.9 * em.MODEL_DEVIATION_EPS[nd] <= worst <= em.MODEL_DEVIATION_EPS[nd]

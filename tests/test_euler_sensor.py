"""The Euler sweep with the sensor-scaled central + Rusanov flux, on the CPU: calibration of its per-cell bound, sensitivity,
and the C entry's declaration and host-side validation.

Calibration (``test_calibration``, Float32 oracle composition of tests/euler_sensor_model.py against its float64 evaluation
under ``sensor_scale``; maxima over the four meshes of tests/test_gpu_percell_regimes.py):

    nu = D:  supersonic+ 3.28e-07, supersonic- 3.51e-07, transonic 3.25e-07, crossing 3.46e-07, stagnation 2.79e-07,
             rest 2.76e-07, floor 1.90e-07, cold 2.31e-07, jump 5.68e-08
    transonic with an external random nu in [0, 1]: 2.81e-07;  with nu = 0: 1.39e-07
    per mesh: adv 3.21e-07, rae6k_2 3.51e-07, corner 2.83e-07, sphere_1 2.93e-07
    worst 3.51e-07, 4 x = 1.40e-06 -> BOUND_SENSOR = 2e-6

``BOUND_SENSOR`` = 4 x the worst figure, rounded up to one digit, and at most ``percell.BOUND_EULER``.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import euler_sensor_model as esm
import percell as pc
import regimes as rg
from abi import assert_bound
from conftest import oracle_view
from ibamd import _lib
from oracle import cfd as ocfd

f32, f64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NU_CASES = ("external", "zero")   # besides nu = D: a caller's random nu in [0, 1], and nu = 0 (the pure central flux)
NU_REGIME = "transonic"


@pytest.fixture(scope="module")
def parts(adv_mesh, rae_mesh_small):
    return {k: (p, oracle_view(p)) for k, p in esm.regime_partitions(adv_mesh, rae_mesh_small).items()}


def _nu(kind, n):
    return esm.external_nu(n) if kind == "external" else np.zeros(n, f32)


def _max(err):
    assert np.isfinite(err).all()
    return float(err.max())


def test_calibration(parts):
    """Float32 oracle against float64 on all nine regimes and the four meshes with nu = D, and with an external random nu and
    nu = 0: at most half the bound; the bound is 4 x the worst figure in one digit and does not exceed BOUND_EULER."""
    fluid = ocfd.Fluid()
    seen = {}
    for name, (part, op) in parts.items():
        n = part.spacing.shape[0]
        cases = [(reg, None) for reg in rg.EULER_REGIMES] + [(NU_REGIME, k) for k in NU_CASES]
        for reg, kind in cases:
            P = rg.euler_regime(part, reg)
            nu = None if kind is None else _nu(kind, n)
            r64 = esm.ref64_euler_sensor(op, P, nu)
            r32 = esm.oracle_euler_sensor_residual(op, P, fluid, nu)
            assert r32.dtype == f32 and np.isfinite(r64).all()
            e = _max(pc.percell_error(r32, r64, esm.sensor_scale(part, P, r64)))
            key = f"nu = D, {reg}" if kind is None else f"nu {kind}, {reg}"
            seen[key] = max(seen.get(key, 0.0), e)
            seen["mesh " + name] = max(seen.get("mesh " + name, 0.0), e)
    print("\nsensor-flux calibration, Float32 oracle against float64 (max over the meshes / the cases):")
    for k, v in seen.items():
        print(f"  {k}: {v:.2e}")
    worst = max(seen.values())
    print(f"  worst: {worst:.2e}; 4 x = {4 * worst:.2e}; BOUND_SENSOR = {esm.BOUND_SENSOR:.1e}")
    assert worst <= esm.BOUND_SENSOR / 2, seen
    assert esm.BOUND_SENSOR <= pc.BOUND_EULER
    # the rule: 4 x the worst figure rounded UP to one digit
    mag = 10.0 ** np.floor(np.log10(4 * worst))
    assert esm.BOUND_SENSOR == pytest.approx(np.ceil(4 * worst / mag) * mag, rel=1e-9), (worst, esm.BOUND_SENSOR)


@pytest.mark.parametrize("mesh", ["adv", "rae6k_2", "corner", "sphere_1"])
def test_sensitivity(parts, mesh):
    """A 1e-4 relative error on the coarsest level alone exceeds the bound (as tests/test_percell.py::test_sensitivity); the
    unbroken Float32 oracle passes."""
    part, op = parts[mesh]
    P = rg.euler_regime(part, NU_REGIME)
    r64 = esm.ref64_euler_sensor(op, P)
    s = esm.sensor_scale(part, P, r64)
    r32 = esm.oracle_euler_sensor_residual(op, P, ocfd.Fluid())
    classes = pc.cell_classes(part, block_classes=False)
    assert pc.check(r32, r64, s, esm.BOUND_SENSOR, part, classes=classes, what=mesh) <= esm.BOUND_SENSOR
    lev = pc.levels(part)
    bad = r32.copy()
    bad[lev == lev.max()] *= f32(1 + 1e-4)
    with pytest.raises(AssertionError, match="per-cell error"):
        pc.check(bad, r64, s, esm.BOUND_SENSOR, part, classes=classes, what=mesh)


def test_nu_zero_is_the_central_flux_and_uniform_state_gives_zero(parts):
    """Model sanity: nu = 0 leaves F = (UcL + UcR) u / 2 + p, and a uniform state has a zero residual exactly, in Float32."""
    part, op = parts["adv"]
    n = part.spacing.shape[0]
    P = np.tile(f32([1e5, 288.15, 100.0, -50.0]), (n, 1))
    for nu in (None, np.zeros(n, f32), esm.external_nu(n)):
        r = esm.oracle_euler_sensor_residual(op, P, ocfd.Fluid(), nu)
        assert not r.any()
    fluid = ocfd.Fluid()
    PL, PR = rg.euler_regime(part, "crossing")[:64], rg.euler_regime(part, "transonic")[:64]
    z = np.zeros(64, f32)
    F = ocfd.inviscid_fluxes_sensor(fluid, PL, PR, z, z, 1)
    UL, UR = ocfd.primitive2state(fluid, PL), ocfd.primitive2state(fluid, PR)
    UL[:, 1] += PL[:, 0]
    UR[:, 1] += PR[:, 0]
    Pm = (PL + PR) / f32(2)
    C = (UL + UR) * Pm[:, 2:3] / f32(2)
    C[:, 2] += Pm[:, 0]
    assert np.array_equal(F, C)


# ---------------------------------------------------------------------------------------------------------------------
# C ABI and host validation
# ---------------------------------------------------------------------------------------------------------------------
def test_entry_is_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "ibhip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+ibh_residual_euler_sensor\s*\(", text)
    assert_bound(("ibh_residual_euler_sensor",))


def test_null_arguments_are_reported_before_any_launch():
    """Null partition, P, R or fluid: non-zero with "null" in ibh_last_error, without a GPU."""
    lib = _lib.load()
    buf = (ctypes.c_float * 8)()
    a = ctypes.addressof(buf)
    fl = _lib.ibh_fluid(283.0, 1.4, 0.0, 1.0, 0.0, 0)
    part = ctypes.c_void_p(a)   # never dereferenced: the check of the other arguments comes first
    for args in ((None, a, 2, None, a, 2, ctypes.byref(fl), 0),
                 (part, None, 2, None, a, 2, ctypes.byref(fl), 0),
                 (part, a, 2, None, None, 2, ctypes.byref(fl), 0),
                 (part, a, 2, None, a, 2, None, 0)):
        assert lib.ibh_residual_euler_sensor(*args) != 0
        msg = lib.ibh_last_error()
        assert b"null" in msg and b"ibh_residual_euler_sensor" in msg, msg

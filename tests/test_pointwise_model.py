"""The per-element checker of the pointwise sensors and closures (tests/pointwise_model.py), on the CPU.

Calibration: the Float32 oracle, through the same scales on the same families as the device (tests/test_gpu_pointwise.py),
stays at or below half of each kernel's bound against its own float64 evaluation; the maxima are printed (``pytest -s``).
Blindness: on the 3-D ``divfree`` family the Float32 oracle passes the norm-wise check that was all there was
(``rel_inf <= 1e-6``) while single elements are off by more than 1e-4 relative -- the per-element scale carries them.
Planted errors: each wrong term, put into a copy of the float64 reference, fails the check on a named family.
"""
import numpy as np
import pytest

import pointwise_model as pm
from conftest import rel_inf
from oracle import cfd as ocfd
from oracle import turbulence as ot

f32, f64 = np.float32, np.float64
N_CAL = 20000


def test_the_literal_restatements_are_the_oracle():
    """Without a plant the ``*_lit`` functions give the oracle's bits, in Float32 and in float64."""
    n = 501
    for conv in (lambda x: x, pm.to64):
        for nd in (2, 3):
            for fam in pm.GRAD_FAMILIES:
                g = conv(pm.grad_family(fam, nd, n, 2))
                assert np.array_equal(pm.ducros_lit(g), ot.Ducros_sensor(g))
                assert np.array_equal(pm.shock_lit(g), ocfd.shock_sensor(g))
                if nd == 3:
                    D = conv(pm.delta_field(n, 2))
                    assert np.array_equal(pm.wale_lit(D, g), ot.WALE_nuSGS(D, g))
        x = conv(list(pm.keps_family(n, 2)))
        a, b = pm.keps_lit(*x), ot.standard_k_epsilon(*x)
        assert all(np.array_equal(a[k], b[k]) for k in b)
        Rey = conv(pm.rey_family(n, 2))
        a, b = pm.wall_rey_lit(Rey), ot.wall_function_rey(Rey)
        assert all(np.array_equal(a[k], b[k]) for k in b)
        x = conv(list(pm.jst_family("pressure", n, 2)))
        assert np.array_equal(pm.jst_lit(*x), ocfd.JST_sensor3(*x))


def _normal(a):
    a = np.abs(np.asarray(a))
    return np.isfinite(a).all() and ((a == 0) | (a >= np.finfo(f32).tiny)).all()


def calibrate(n=N_CAL, seeds=(0, 1)):
    """{(kernel, output): {family: maximum of the Float32 oracle against float64}}."""
    worst = {}
    for kernel in pm.KERNELS:
        for fam, nd in pm.families(kernel):
            name = pm.family_name(kernel, fam, nd)
            for seed in seeds:
                x, kw = pm.make(kernel, fam, nd, n, seed)
                got = pm.oracle(kernel, x, kw)
                assert all(_normal(v) for v in got.values()), name
                ref, sc = pm.reference(kernel, x, kw)
                for key, v in pm.measure(got, ref, sc, what=name, min_finite=0.99).items():
                    w = worst.setdefault((kernel, key), {})
                    w[name] = max(w.get(name, 0.0), v[0])
    return worst


def test_calibration():
    """The Float32 oracle against float64 on every family, two seeds.  Every family's reference is finite on at least
    99 % of its elements and the Float32 outputs are normal (or 0) and finite.  Each maximum is at most half of
    BOUND_POINTWISE, or the output carries 4 x its measured maximum, rounded up, as its bound (pointwise_model.BOUNDS,
    CALIBRATED: the recorded figure must still hold, within a quarter, so a bound cannot drift from its measurement)."""
    worst = calibrate()
    print("\ncalibration (per-element error of the Float32 oracle against float64; Smagorinsky in units of 2 eps):")
    for (kernel, key), fams in worst.items():
        e = max(fams.values())
        b = pm.bound_of(kernel, key)
        print(f"  {kernel} {key}: {e:.2e} (bound {b:.1e})  " + ", ".join(f"{k.split(' ', 1)[1]} {v:.1e}" for k, v in fams.items()))
        if kernel == "Smagorinsky_nuSGS":     # the arithmetic's own 2 eps, not a calibrated bound: held to it whole
            assert e <= b
        elif b == pm.BOUND_POINTWISE:
            assert e <= b / 2, (kernel, key, fams)
        else:
            rec = pm.CALIBRATED[kernel, key]
            assert e <= 1.25 * rec and 4 * rec <= b <= 8 * rec, (kernel, key, e, rec, b)
    assert set(pm.CALIBRATED) == {(k, o) for (k, o) in worst if pm.bound_of(k, o) != pm.BOUND_POINTWISE
                                  and k != "Smagorinsky_nuSGS"}


def test_exact_rows_on_the_oracle():
    """The exact rows' expected values are the float64 oracle's, and the Float32 oracle is within 2 ulps of them."""
    for name, kernel, x, expect in pm.exact_rows():
        ref = pm.oracle(kernel, x, dtype=f64)["out"]
        assert np.allclose(ref, expect, rtol=1e-15, atol=0), (name, ref, expect)
        got = pm.oracle(kernel, x)["out"]
        assert pm.ulps(got, ref).max() <= pm.ULPS_EXACT, (name, got, ref)
        if expect in (0.0, 1.0):
            assert np.all(got == f32(expect)), name


def test_edge_rows_on_the_oracle():
    """The Float32 oracle has the float64 oracle's NaN pattern and infinities on the edge rows (so the device can)."""
    for name, kernel, x, kw in pm.edge_rows():
        ref, sc = pm.reference(kernel, x, kw)
        assert any(np.isnan(v).any() for v in ref.values()), name
        pm.check(kernel, pm.oracle(kernel, x, kw), ref, sc, what=name, factor=0.5)


def test_the_norm_wise_check_is_blind_on_divfree():
    """3-D ``divfree``: the divergence is a rounding error, the shock sensor's ``div^2`` dominates its epsilon (1f-14).  The
    Float32 oracle passes rel_inf <= 1e-6 against float64 while some element is off by more than 1e-4 relative -- and
    passes the per-element check, whose scale carries the cancellation."""
    (g,), _ = pm.make("shock_sensor", "divfree", 3, N_CAL, 0)
    got = ocfd.shock_sensor(g)
    ref, sc = pm.reference("shock_sensor", (g,))
    assert rel_inf(got, ref["out"]) <= 1e-6
    rel = np.abs(got - ref["out"]) / np.abs(ref["out"])
    assert rel.max() > 1e-4, rel.max()
    pm.check("shock_sensor", {"out": got}, ref, sc, factor=0.5)


# (kernel, plant, restatement, family, nd): the family on which the planted error must fail the check
PLANTS = [
    ("Ducros_sensor", "curl_sign", "rot", 3),
    ("Ducros_sensor", "curl_sign", "rand", 2),
    ("shock_sensor", "once", "rand", 2),
    ("Ducros_sensor", "eps", "divfree", 3),
    ("shock_sensor", "eps", "divfree", 3),
    ("WALE_nuSGS", "trace", "rand", 3),
    ("WALE_nuSGS", "exponent", "rot", 3),
    ("WALE_nuSGS", "transpose", "rand", 3),
    ("standard_k_epsilon", "c1c2", "decades", 0),
    ("standard_k_epsilon", "sigma", "decades", 0),
    ("wall_function_rey", "mu_square", "decades", 0),
    ("wall_function_rey", "k_min", "decades", 0),
    ("JST_sensor", "two_pi", "unit", 0),
]


def _planted(kernel, x, plant):
    x = pm.to64(x)
    with np.errstate(all="ignore"):
        if kernel == "Ducros_sensor":
            return {"out": pm.ducros_lit(x[0], plant)}
        if kernel == "shock_sensor":
            return {"out": pm.shock_lit(x[0], plant)}
        if kernel == "WALE_nuSGS":
            return {"out": pm.wale_lit(x[0], x[1], plant=plant)}
        if kernel == "standard_k_epsilon":
            return pm.keps_lit(*x, plant=plant)
        if kernel == "wall_function_rey":
            return pm.wall_rey_lit(x[0], plant=plant)
        if kernel == "JST_sensor":
            return {"out": pm.jst_lit(*x, plant=plant)}
    raise KeyError(kernel)


@pytest.mark.parametrize("kernel,plant,family,nd", PLANTS)
def test_planted_errors(kernel, plant, family, nd):
    """A wrong term in a copy of the float64 reference fails the check on the named family; the copy without it passes
    with an error of exactly 0."""
    x, kw = pm.make(kernel, family, nd, 4099, 0)
    ref, sc = pm.reference(kernel, x, kw)
    assert max(pm.check(kernel, _planted(kernel, x, None), ref, sc).values()) == 0.0
    with pytest.raises(AssertionError, match="off by"):
        pm.check(kernel, _planted(kernel, x, plant), ref, sc, what=pm.family_name(kernel, family, nd))


def test_planted_errors_on_the_exact_rows():
    """The exact rows pin both epsilons and the 2-D double count on their own."""
    rows = {name: (kernel, x) for name, kernel, x, _ in pm.exact_rows()}
    for name, plant in (("Ducros 2-D div = 0, curl^2 = 2^-20", "eps"), ("Ducros 3-D div = 0, curl^2 = 2^-20", "eps"),
                        ("shock 2-D w = 2^-24", "eps"), ("shock 3-D w = 2^-24", "eps"), ("shock 2-D w = 2^-24", "once"),
                        ("JST (1, 2, 3) 2^-40", "two_pi")):
        kernel, x = rows[name]
        ref = pm.oracle(kernel, x, dtype=f64)["out"]
        bad = _planted(kernel, x, plant)["out"]
        assert pm.ulps(bad, ref).max() > pm.ULPS_EXACT, (name, plant)

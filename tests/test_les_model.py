"""Known answers of the LES closures and shock sensors that do not come from libibhip: ``oracle.turbulence`` and
``oracle.cfd`` on hand-made 3 x 3 and 2 x 2 velocity-gradient tables (tests/les_model.py), and the Float32 oracle
composition's own deviation from them on the meshes of tests/test_gpu_les.py -- the bounds its analytic-field check imports."""
import numpy as np
import pytest

import les_model as lm
from conftest import oracle_view
from oracle import cfd as ocfd
from oracle import turbulence as ot

f32, f64 = np.float32, np.float64


@pytest.mark.parametrize("nd", [2, 3])
@pytest.mark.parametrize("dtype", [f32, f64])
def test_pure_shear(nd, dtype):
    a = -0.7
    g = lm.table(lm.shear(nd, a), 5, dtype)
    S = ot.shear_rate(g)
    assert S.dtype == dtype and np.allclose(S, abs(dtype(f32(a))), rtol=4 * np.finfo(dtype).eps, atol=0)
    if nd == 3:   # g g = 0 for a pure shear: the WALE operator vanishes identically
        assert np.array_equal(ot.WALE_nuSGS(np.full(5, 0.1, dtype), g), np.zeros(5, dtype))


@pytest.mark.parametrize("nd", [2, 3])
def test_pure_dilatation(nd):
    for dtype in (f32, f64):
        g = lm.table(lm.dilatation(nd), 5, dtype)
        assert np.array_equal(ot.Ducros_sensor(g), np.ones(5, dtype))
        assert np.array_equal(ocfd.shock_sensor(g), np.ones(5, dtype))


def test_solid_rotation_3d():
    w = (0.3, -0.9, 0.6)
    g = lm.table(lm.rotation(3, w), 5, f64)
    curl2 = sum((2.0 * f64(f32(x))) ** 2 for x in w)      # curl(omega x r) = 2 omega
    assert np.allclose(ot.shear_rate(g), 0.0, atol=0)
    assert np.allclose(ot.Ducros_sensor(g), lm.EPS32 / (curl2 + lm.EPS32), rtol=1e-14, atol=0)
    assert np.allclose(ocfd.shock_sensor(g), lm.EPS_SHOCK / (curl2 + lm.EPS_SHOCK), rtol=1e-14, atol=0)


def test_rotation_2d_counts_the_vorticity_twice_in_the_shock_sensor():
    g = lm.table(lm.rotation(2), 5, f64)
    w2 = (2.0 * f64(f32(0.6))) ** 2
    assert np.allclose(ot.Ducros_sensor(g), lm.EPS32 / (w2 + lm.EPS32), rtol=1e-14, atol=0)
    assert np.allclose(ocfd.shock_sensor(g), lm.EPS_SHOCK / (2.0 * w2 + lm.EPS_SHOCK), rtol=1e-14, atol=0)


@pytest.mark.parametrize("nd", [2, 3])
def test_smagorinsky(nd):
    Delta = np.array([0.05, 0.1, 0.2], f64)
    for _, make in lm.FIELDS:
        ans = lm.answers(make(nd), Delta)
        assert np.allclose(ans["smagorinsky"], (f64(lm.CS) * Delta) ** 2 * ans["S"], rtol=1e-14, atol=0)
    assert np.allclose(lm.answers(lm.shear(nd, 0.7), Delta)["smagorinsky"], (f64(lm.CS) * Delta) ** 2 * f64(f32(0.7)),
                       rtol=1e-14, atol=0)


MESHES = [("octree", lm.octree_mesh), ("bs4 2d", lambda: lm.bs4_mesh(2)), ("bs4 3d", lambda: lm.bs4_mesh(3))]


@pytest.mark.parametrize("key,make", MESHES, ids=[k.replace(" ", "_") for k, _ in MESHES])
def test_oracle_composition_on_linear_fields(key, make):
    """The deviation of the Float32 oracle composition from the table answers on the cells of ``interior`` -- the device's
    bound is 4 x it -- is rounding: a few ulps of the gradients (|u| <= 8, h >= 1/16: 2^-21 / h relative to |A| ~ 1)."""
    part = lm.one_partition(make())
    sel = lm.interior(part)
    assert 2 * sel.sum() >= sel.size, f"{key}: the mask keeps {sel.sum()} of {sel.size} cells"
    bound, dev = lm.bounds(key, part, oracle_view(part))
    print(f"\n{key}: {sel.sum()} of {sel.size} cells; Float32 oracle composition against the table answers:")
    for k in sorted(dev):
        print(f"  {k}: {dev[k]:.3e}")
    assert set(dev) == set(lm.OUTPUTS) - (set() if part.ndims == 3 else {"wale"})
    assert dev["S"] <= 1e-4 and dev["ducros"] <= 1e-4 and dev["shock"] <= 1e-4

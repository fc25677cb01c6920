"""``residual_euler_sensor`` on the device: the literal form bit for bit, every tuned form per cell against float64.

Meshes, regimes and reference handling as tests/test_gpu_percell_regimes.py (its ``meshes`` fixture: ``adv``, ``rae6k_2``,
``corner``, ``sphere_1``): one float64 reference per (mesh, regime), ``percell.check`` (NaN pattern, then the bound) with
``euler_sensor_model.sensor_scale`` and ``BOUND_SENSOR`` (calibrated in tests/test_euler_sensor.py).  The literal form
(``IBH_FORCE_GENERAL``: face-list threads through the gradient workspace) follows the reference operation by operation, so it
is held to the Float32 oracle composition bit for bit, as the HLL literal form is to its own.
"""
import numpy as np
import pytest
import torch

import euler_sensor_model as esm
import ibamd
import percell as pc
import regimes as rg
from ibamd import _lib
from oracle import cfd as ocfd
from test_gpu_percell import EXACT, GENERAL, IMAGE, NO_FUSE, NO_QUAD, PH1, PH2, _euler, _tuned
from test_gpu_percell_regimes import MESHES, RegimeCase, meshes  # noqa: F401  (``meshes`` is a fixture)

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
MEASURED = {}
REFS = {}          # (mesh, regime) -> (P, float64 reference, scale)
BIT_REGIMES = ("transonic", "crossing")


def _record(form, regime, err):
    MEASURED[form, regime] = max(MEASURED.get((form, regime), 0.0), err)


@pytest.fixture(scope="module", autouse=True)
def _print_measured():
    yield
    if MEASURED:
        print("\nresidual_euler_sensor, per-cell maxima against float64 (form, regime):")
        for k in sorted(MEASURED):
            print(f"  {k[0]} | {k[1]}: {MEASURED[k]:.3e}")


def _ref(c, reg):
    if (c.name, reg) not in REFS:
        P = rg.euler_regime(c.part, reg)
        R64 = esm.ref64_euler_sensor(c.op, P)
        REFS[c.name, reg] = (P, R64, esm.sensor_scale(c.part, P, R64))
    return REFS[c.name, reg]


def _sensor(dpart, P, flags=0, nu=None, phases=False, out=None):
    """The sweep into a NaN-filled output (whole, or the two overlap phases one after the other)."""
    if out is None:
        out = torch.full((P.shape[1], P.shape[0]), float("nan"), dtype=torch.float32, device="cuda").T
    dP = ibamd.hip(P)
    dnu = None if nu is None else ibamd.hip(nu)
    for ph in ((PH1, PH2) if phases else (0,)):
        ibamd.residual_euler_sensor(dpart, dP, nu=dnu, out=out, flags=flags | ph)
    return ibamd.to_host(out)


def _check(c, reg, got, form, cells=None):
    P, R64, S = _ref(c, reg)
    assert np.isfinite(R64).all()
    e = pc.check(got, R64, S, esm.BOUND_SENSOR, c.part, cells=cells, classes=c.classes, what=f"{form} [{c.name}, regime {reg}]")
    _record(form, reg, e)


# ---------------------------------------------------------------------------------------------------------------------
# literal form: the Float32 oracle composition bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", MESHES)
def test_literal_form_is_the_oracle_bit_for_bit(meshes, mesh):
    c = meshes[mesh]
    fluid = ocfd.Fluid()
    n = c.part.spacing.shape[0]
    for reg in BIT_REGIMES:
        P = rg.euler_regime(c.part, reg)
        exp = esm.oracle_euler_sensor_residual(c.op, P, fluid)
        got = _sensor(c.dpart, P, GENERAL)
        assert np.array_equal(got, exp), (mesh, reg, int((got != exp).sum()))
        # the HLL literal form against its own restatement
        assert np.array_equal(_euler(c.dpart, P, GENERAL), pc.oracle_euler_residual(c.op, P, fluid)), (mesh, reg)
        # nu = None is nu = JST_sensor(part, p) passed explicitly
        D = ibamd.to_host(ibamd.JST_sensor(c.dpart, ibamd.hip(np.ascontiguousarray(P[:, 0]))))
        assert np.array_equal(_sensor(c.dpart, P, GENERAL, nu=D), got), (mesh, reg)
        assert np.array_equal(_sensor(c.dpart, P, 0, nu=D), got), (mesh, reg)     # a given nu takes the literal form
        # a caller's nu, and nu = 0: the pure central flux
        for nu in (esm.external_nu(n), np.zeros(n, f32)):
            exp_nu = esm.oracle_euler_sensor_residual(c.op, P, fluid, nu)
            assert np.array_equal(_sensor(c.dpart, P, GENERAL, nu=nu), exp_nu), (mesh, reg, float(nu.max()))
            assert np.array_equal(_sensor(c.dpart, P, 0, nu=nu), exp_nu), (mesh, reg, float(nu.max()))
    # a NaN in a caller's nu reaches every cell with a face on it, as through the reference's max(nuL, nuR), and no other
    P = rg.euler_regime(c.part, "transonic")
    nu = esm.external_nu(n)
    nu[::97] = np.nan
    exp_nan = esm.oracle_euler_sensor_residual(c.op, P, fluid, nu)
    assert 0 < np.isnan(exp_nan[:, 0]).sum() < n
    assert np.array_equal(_sensor(c.dpart, P, GENERAL, nu=nu), exp_nan, equal_nan=True), mesh
    # a uniform state gives exactly zero
    P = np.tile(f32([1e5, 288.15, 100.0, -50.0, 25.0][:c.nd + 2]), (n, 1))
    assert not _sensor(c.dpart, P, GENERAL).any()
    assert not _sensor(c.dpart, P, GENERAL, nu=esm.external_nu(n)).any()


# ---------------------------------------------------------------------------------------------------------------------
# tuned forms per cell against float64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", rg.EULER_REGIMES)
def test_adv_forms(meshes, regime):
    """2-D, every block eligible: quads + pairs + singles (default), the per-block kernel, the other grid order, the literal
    block arithmetic, the two-kernel request, and the overlap phases -- bit for bit the unphased sweep."""
    c = meshes["adv"]
    d = c.dpart
    P = _ref(c, regime)[0]
    whole = _sensor(d, P)
    _check(c, regime, whole, "2d quad (default)")
    _check(c, regime, _sensor(d, P, NO_QUAD), "2d per-block NO_QUAD")
    _check(c, regime, _tuned({"quad_singles_first": 1}, lambda: _sensor(d, P)), "2d quad quad_singles_first=1")
    _check(c, regime, _sensor(d, P, EXACT), "2d literal EXACT")
    _check(c, regime, _sensor(d, P, NO_FUSE), "2d NO_FUSE")
    assert np.array_equal(_sensor(d, P, phases=True), whole), regime
    assert np.array_equal(_sensor(d, P, NO_QUAD, phases=True), _sensor(d, P, NO_QUAD)), regime


@pytest.mark.parametrize("regime", rg.EULER_REGIMES)
def test_rae_image_only_and_partition(meshes, regime):
    """Skirts and face-list cells: the image quads write the image rows alone; the whole-partition call."""
    c = meshes["rae6k_2"]
    P = _ref(c, regime)[0]
    n = P.shape[0]
    for flags, form in ((IMAGE, "2d IMAGE_ONLY quads"), (IMAGE | NO_QUAD, "2d IMAGE_ONLY NO_QUAD")):
        got = _sensor(c.dpart, P, flags)
        skirt = np.ones(n, bool)
        skirt[c.img] = False
        assert np.isnan(got[skirt]).all() and not np.isnan(got[c.img]).any(), form    # skirt rows stay untouched
        _check(c, regime, got, form, cells=c.img)
    _check(c, regime, _sensor(c.dpart, P), "2d partition default")


@pytest.mark.parametrize("regime", rg.EULER_REGIMES)
def test_corner_columns(meshes, regime):
    c = meshes["corner"]
    _check(c, regime, _sensor(c.dpart, _ref(c, regime)[0]), "3d columns (default)")
    _check(c, regime, _sensor(c.dpart, _ref(c, regime)[0], NO_FUSE), "3d NO_FUSE")


def test_corner_quad_variant_512_fails_with_its_message(meshes):
    """The thread-per-cell and the stamped 3-D forms are HLL only: the entry fails, the output is untouched."""
    c = meshes["corner"]
    P = rg.euler_regime(c.part, "transonic")
    out = torch.full((P.shape[1], P.shape[0]), float("nan"), dtype=torch.float32, device="cuda").T
    try:
        _lib.call("ibh_set_tuning", b"quad_variant", 512)
        with pytest.raises(_lib.IbhError, match="quad_variant"):
            ibamd.residual_euler_sensor(c.dpart, ibamd.hip(P), out=out)
        assert np.isnan(ibamd.to_host(out)).all()
    finally:
        _lib.call("ibh_set_tuning", b"quad_variant", 0)
    assert np.isfinite(_sensor(c.dpart, P)).all()


@pytest.mark.parametrize("regime", rg.EULER_REGIMES)
def test_sphere_image_only_columns(meshes, regime):
    c = meshes["sphere_1"]
    P = _ref(c, regime)[0]
    got = _sensor(c.dpart, P, IMAGE)
    assert np.isnan(got[:, 0]).sum() == got.shape[0] - c.img.size
    _check(c, regime, got, "3d IMAGE_ONLY (cols)", cells=c.img)
    _check(c, regime, _sensor(c.dpart, P), "3d partition default")


TUNED_CALLS = {"adv": ((0, "2d quad (default)"), (NO_QUAD, "2d per-block NO_QUAD")),
               "rae6k_2": ((IMAGE, "2d IMAGE_ONLY quads"), (IMAGE | NO_QUAD, "2d IMAGE_ONLY NO_QUAD")),
               "corner": ((0, "3d columns (default)"),),
               "sphere_1": ((IMAGE, "3d IMAGE_ONLY (cols)"),)}


@pytest.mark.parametrize("mesh", MESHES)
def test_single_kernel_calls_do_not_run_the_literal_form(meshes, mesh):
    """The face-list form is inside the bound too, and leaves skirt rows alone: a dispatch that fell back to it would pass
    every per-cell check above.  The single kernels regroup the flux by state and take hardware reciprocals, the face-list
    form divides in the reference's order, so on a noisy state some bit of the two differs; the face-list form itself is
    pinned bit for bit by the first test.  The path does not depend on the state: one regime."""
    c = meshes[mesh]
    P = _ref(c, "transonic")[0]
    literal = _sensor(c.dpart, P, GENERAL)
    rows = c.img if mesh in ("rae6k_2", "sphere_1") else slice(None)
    for flags, form in TUNED_CALLS[mesh]:
        got = _sensor(c.dpart, P, flags)
        assert np.isfinite(got[rows]).all(), form
        assert not np.array_equal(got[rows], literal[rows]), f"{form} [{mesh}] gave the bits of the face-list form"
    # and the requests that are to take the face-list form do: a caller's nu (checked bit for bit above) and IBH_NO_FUSE
    assert np.array_equal(_sensor(c.dpart, P, NO_FUSE), literal), mesh


# ---------------------------------------------------------------------------------------------------------------------
# existing behaviour, front end
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", ["adv", "corner"])
def test_hll_is_unchanged_by_a_sensor_call(meshes, mesh):
    """The two entries share the gradient workspace and the tuning state: HLL before and after gives identical bits."""
    c = meshes[mesh]
    P = rg.euler_regime(c.part, "transonic")
    for flags in (0, NO_FUSE, GENERAL):
        before = _euler(c.dpart, P, flags)
        _sensor(c.dpart, P, flags)
        _sensor(c.dpart, P, GENERAL, nu=esm.external_nu(P.shape[0]))
        assert np.array_equal(_euler(c.dpart, P, flags), before), (mesh, flags)


def test_domain_call_and_graph_replay(adv_mesh_coarse):
    """``dom(f, P, R)`` on device arrays over two partitions equals the per-partition calls; a ``GraphedClosure`` of it replays
    the same bits."""
    from conftest import ADV_FAMILIES
    dp = ibamd.Domain(adv_mesh_coarse, hypercube_families=ADV_FAMILIES, max_partition_size=2048)
    assert len(dp.partitions) == 2
    n = len(dp)
    x = dp.global_centers()
    rng = np.random.default_rng(3)
    P = np.empty((n, 4), f32)
    P[:, 0] = 1e5 * (1 + 0.05 * rng.uniform(-1, 1, n))
    P[:, 1] = 288.15 * (1 + 0.05 * rng.uniform(-1, 1, n))
    P[:, 2] = 340 * np.sin(2 * np.pi * x[:, 0])
    P[:, 3] = -100 * (1 + 0.1 * rng.uniform(-1, 1, n))
    exp = np.zeros_like(P)
    for part in dp.partitions.values():
        loc = ibamd.to_host(ibamd.residual_euler_sensor(ibamd.to_backend(part, ibamd.hip),
                                                        ibamd.hip(np.ascontiguousarray(P[part.domain]))))
        exp[part.image] = loc[part.image_in_domain]
    assert np.abs(exp).max() > 0

    def f(part, P, R):
        ibamd.residual_euler_sensor(part, P, out=R)

    dP, dR = ibamd.hip(P), ibamd.hip(np.zeros_like(P))
    dp(f, dP, dR)
    assert np.array_equal(ibamd.to_host(dR), exp)

    def call(P, R):
        dp(f, P, R)

    g = ibamd.GraphedClosure(call, dP, dR)
    dR.zero_()
    g()
    assert np.array_equal(ibamd.to_host(dR), exp) and np.array_equal(ibamd.to_host(dP), P)

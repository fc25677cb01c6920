"""The pointwise sensors and LES / RANS closures on the device, per element, against the float64 oracle
(tests/pointwise_model.py: references, scales, families, bounds; tests/test_pointwise_model.py calibrates them on the CPU
and plants the errors these checks must see).

Before this module ``Ducros_sensor``, ``WALE_nuSGS``, ``Smagorinsky_nuSGS``, ``standard_k_epsilon``, the pointwise
``shear_rate``, ``shock_sensor``, the three-point ``JST_sensor`` and eight of the eleven ``wall_function`` outputs were
compared norm-wise on one field of uniform gradients.  Here every element answers to its own scale: on the states the
formulas exist for (pure rotation, dilatation, shear, zero gradients, gradients spread over decades, Pk = eps), on exact
rows that pin both epsilons and the 2-D double count of ``shock_sensor``, on NaN / Inf / zero inputs (the reference's NaN
pattern exactly), at the sizes around a workgroup, past the 4096 x 256 grid cap of csrc/ibh_turb.hip (the second trip of
the grid-stride loops) and on strided inputs.  The wrappers' argument checks (an array whose extent the kernel takes
from another argument) are tested with ``backend.call`` replaced, so that a lost check cannot reach a kernel.
"""
import numpy as np
import pytest

import ibamd
import pointwise_model as pm
from ibamd import backend as B
from ibamd import cfd
from ibamd import turbulence as T

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
MEASURED = {}


def _record(form, family, errs):
    for key, e in errs.items():
        k = (form if key == "out" else f"{form} {key}", family)
        MEASURED[k] = max(MEASURED.get(k, 0.0), e)


@pytest.fixture(scope="module", autouse=True)
def _print_measured():
    yield
    if MEASURED:
        print("\nper-element maxima against float64 (Smagorinsky in units of 2 eps), by form and family:")
        forms = {}
        for (form, fam), e in MEASURED.items():
            forms.setdefault(form, {})[fam] = e
        for form in sorted(forms):
            print(f"  {form}: {max(forms[form].values()):.3e}  " + ", ".join(f"{k} {v:.1e}" for k, v in forms[form].items()))


def _h(t):
    return ibamd.to_host(t)


def _dev(x, put=ibamd.hip):
    if isinstance(x, (list, tuple)):
        return [_dev(v, put) for v in x]
    return put(x)


def _strided(a):
    """A device view with stride 2 (``_field`` copies it; the copy must live through the launch)."""
    buf = np.full(2 * a.size, np.nan, f32)
    buf[::2] = a
    v = ibamd.hip(buf)[::2]
    assert v.stride(0) == 2
    return v


def device(kernel, x, kw=None, put=ibamd.hip):
    """The device kernel on host inputs: {output: host array}."""
    kw = dict(kw or {})
    d = _dev(x, put)
    if "C" in kw:
        kw["C_"] = kw.pop("C")
    if "omega" in kw:
        kw["omega_fixed_point"] = kw.pop("omega")
    if kernel == "shear_rate":
        out = T.shear_rate(d[0])
    elif kernel == "Ducros_sensor":
        out = T.Ducros_sensor(d[0])
    elif kernel == "shock_sensor":
        out = cfd.shock_sensor(d[0])
    elif kernel == "WALE_nuSGS":
        out = T.WALE_nuSGS(d[0], d[1])
    elif kernel == "Smagorinsky_nuSGS":
        out = T.Smagorinsky_nuSGS(d[0], d[1])
    elif kernel == "standard_k_epsilon":
        out = T.standard_k_epsilon(*d)
    elif kernel == "JST_sensor":
        out = cfd.JST_sensor(*d)
    elif kernel in ("wall_function_rey", "wall_function"):
        out = T.wall_function(*d, **kw)
    else:
        raise KeyError(kernel)
    return {k: _h(v) for k, v in out.items()} if isinstance(out, dict) else {"out": _h(out)}


def _run(kernel, family, nd, n, seed=0, put=ibamd.hip, tail=None, tag=""):
    x, kw = pm.make(kernel, family, nd, n, seed)
    ref, sc = pm.reference(kernel, x, kw)
    name = pm.family_name(kernel, family, nd)
    errs = pm.check(kernel, device(kernel, x, kw, put), ref, sc, what=f"{name} n={n}", min_finite=0.99, tail=tail)
    _record(f"{kernel} {nd}-D" if nd else kernel, family + tag, errs)


KERNEL_ND = [(k, nd) for k in pm.KERNELS for nd in sorted({nd for _, nd in pm.families(k)})]
_ids = [f"{k}-{nd}d" if nd else k for k, nd in KERNEL_ND]


@pytest.mark.parametrize("kernel,nd", KERNEL_ND, ids=_ids)
def test_families(kernel, nd):
    """Every family at n = 4099, and the first one at n = 1, 255, 256, 257 (one thread, a workgroup less one, one, one
    more)."""
    fams = [f for f, d in pm.families(kernel) if d == nd]
    for fam in fams:
        _run(kernel, fam, nd, pm.SIZES[-1])
    for n in pm.SIZES[:-1]:
        _run(kernel, fams[0], nd, n, seed=1)


@pytest.mark.parametrize("kernel,nd", KERNEL_ND, ids=_ids)
def test_past_the_grid_cap(kernel, nd):
    """n = 4096 x 256 + 3: the launches of csrc/ibh_turb.hip and csrc/ibh_cfd.hip are capped at 4096 workgroups of 256
    threads, so the elements from 1 048 576 on are the second trip of the grid-stride loop; they are among those checked.
    (``k_jst3`` and ``k_shock`` had no loop: those elements were never written.  The 3-D shock sensor passed all the same,
    on the Ducros test's result in recycled memory -- the two agree on this family -- hence the poisoned allocation.)"""
    poison = B.colmajor_empty(pm.N_WRAP)     # what the caching allocator hands to the next output of this size
    poison.fill_(float("nan"))
    del poison
    assert pm.N_WRAP > pm.WRAP == 4096 * 256
    _run(kernel, pm.families(kernel)[0][0], nd, pm.N_WRAP, seed=2, tail=pm.WRAP, tag=" (wrapped)")


def test_exact_rows():
    """Inputs whose sums and differences are exact in Float32, held to 2 ulps of the float64 value with no scale: both
    epsilons, the 2-D double count, zero gradients -> exactly 1, flat triples -> exactly 1, pure shear -> WALE exactly 0."""
    for name, kernel, x, expect in pm.exact_rows():
        ref = pm.oracle(kernel, x, dtype=f64)["out"]
        got = device(kernel, x)["out"]
        u = int(pm.ulps(got, ref).max())
        _record("exact rows (ulps)", name, {"out": float(u)})
        assert u <= pm.ULPS_EXACT, (name, got, ref)
        if expect in (0.0, 1.0):
            assert np.all(got == f32(expect)), (name, got)


def test_edge_rows():
    """k = 0, eps = 0, NaN in each k-epsilon input; a NaN or an Inf in one gradient entry; Rey in {0, -0.0, -5, 1e-12, 1e12,
    NaN, Inf}; u in {0, -5, NaN, Inf}: the float64 oracle's NaN pattern and infinities, finite rows within the bound."""
    for name, kernel, x, kw in pm.edge_rows():
        ref, sc = pm.reference(kernel, x, kw)
        errs = pm.check(kernel, device(kernel, x, kw), ref, sc, what=name)
        _record("edge rows", name, {"out": max(errs.values())})


def test_strided_inputs():
    """Non-contiguous 1-D inputs: every wrapper copies them, and the copies live through the launch."""
    for kernel, nd in KERNEL_ND:
        _run(kernel, pm.families(kernel)[0][0], nd, 4099, seed=3, put=_strided, tag=" (strided)")


# ---------------------------------------------------------------------------------------------------------------------
# argument checks: an array whose extent the kernel takes from another argument
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny3d():
    from ibamd.mesher import Mesh
    msh = Mesh(f32([-1, -1, -1]), f32([2, 2, 2]), block_size=4)
    (part,) = ibamd.Domain(msh, hypercube_families=[], boundaries=False, max_partition_size=10 ** 9).partitions.values()
    dpart = ibamd.to_backend(part, ibamd.hip)
    nc = part.centers.shape[0]
    rng = np.random.default_rng(6)
    P = np.empty((nc, 5), f32)
    P[:, 0] = 1e5
    P[:, 1] = 288.15
    P[:, 2:] = rng.uniform(-30, 30, (nc, 3))
    dP = ibamd.hip(P)
    S, gV = T.shear_rate_of_velocity(dpart, dP[:, 2:], gradients=True)
    return dict(dpart=dpart, nc=nc, P=dP, gV=gV, gP=ibamd.cell_gradient(dpart, dP), mut=ibamd.hip(np.zeros(nc, f32)))


def _no_launch(monkeypatch):
    def fail(name, *a):
        pytest.fail(f"{name} was called: the argument check did not stop the launch")
    monkeypatch.setattr(B, "call", fail)


def test_viscous_residual_rejects_velocity_gradients_without_the_flag(tiny3d, monkeypatch):
    """The tuple of ``shear_rate_of_velocity(..., gradients=True)`` -- (nc, nd) slices of one (nc, nd * nd) buffer -- without
    ``velocity_gradients_only=True`` would be read at columns 2..nd+1: past the slice, for the last one past the allocation."""
    c = tiny3d
    assert all(tuple(g.shape) == (c["nc"], 3) for g in c["gV"])
    R = ibamd.hip(np.zeros((c["nc"], 5), f32))
    _no_launch(monkeypatch)
    with pytest.raises(ValueError, match="velocity_gradients_only"):
        cfd.viscous_residual(c["dpart"], cfd.Fluid(), c["P"], c["gV"], c["mut"], R)
    with pytest.raises(ValueError):      # and the other way round: full gradients with the flag
        cfd.viscous_residual(c["dpart"], cfd.Fluid(), c["P"], c["gP"], c["mut"], R, velocity_gradients_only=True)
    with pytest.raises(ValueError):      # a P of another dimension than the partition's
        cfd.viscous_residual(c["dpart"], cfd.Fluid(), c["P"][:, :4], c["gP"][:2], c["mut"], R[:, :4])
    with pytest.raises(ValueError):      # one array short
        cfd.viscous_residual(c["dpart"], cfd.Fluid(), c["P"], c["gP"][:2], c["mut"], R)


def test_viscous_residual_takes_velocity_gradients_with_the_flag(tiny3d, monkeypatch):
    """The same tuple with the flag, and the full gradients without it, reach the launch (a recording stub: nothing runs)."""
    c = tiny3d
    R = ibamd.hip(np.zeros((c["nc"], 5), f32))
    seen = []
    monkeypatch.setattr(B, "call", lambda name, *a: seen.append((name, a)) or 0)
    cfd.viscous_residual(c["dpart"], cfd.Fluid(), c["P"], c["gV"], c["mut"], R, velocity_gradients_only=True)
    cfd.viscous_residual(c["dpart"], cfd.Fluid(), c["P"], c["gP"], c["mut"], R)
    launches = [(n, a) for n, a in seen if n == "ibh_viscous_residual"]
    assert len(launches) == 2
    assert [a[6] for _, a in launches] == [0, 2]          # grad_vel_col: velocities alone, gradients of P


def test_viscous_fluxes_rejects_short_gradients(monkeypatch):
    n = 16
    P = ibamd.hip(np.ones((n, 4), f32))
    g4, g2 = ibamd.hip(np.ones((n, 4), f32)), ibamd.hip(np.ones((n, 2), f32))
    _no_launch(monkeypatch)
    for grads in ((g2, g2), (g4, g2), (g4,), (g4, g4, g4), (g4, g4[:, 0])):
        with pytest.raises(ValueError):
            cfd.viscous_fluxes(cfd.Fluid(), P, grads, 1)


def test_inviscid_fluxes_rejects_a_PR_of_another_shape(monkeypatch):
    n = 16
    PL = ibamd.hip(np.ones((n, 4), f32))
    nu = ibamd.hip(np.ones(n, f32))
    _no_launch(monkeypatch)
    for PR in (ibamd.hip(np.ones((n - 1, 4), f32)), ibamd.hip(np.ones((n, 5), f32)), ibamd.hip(np.ones((n, 3), f32))):
        with pytest.raises(ValueError):
            cfd.inviscid_fluxes(cfd.Fluid(), PL, PR, 1)
        with pytest.raises(ValueError):
            cfd.inviscid_fluxes(cfd.Fluid(), PL, PR, nu, nu, 1)
        with pytest.raises(ValueError):
            cfd.inviscid_fluxes(cfd.Fluid(), PR, PL, 1)


def test_wale_rejects_a_2d_table(monkeypatch):
    """The kernel reads a 3 x 3 table of pointers: a 2 x 2 one raises before the launch (an ``assert`` before, which
    ``python -O`` drops)."""
    g = _dev(pm.grad_family("rand", 2, 16))
    D = ibamd.hip(pm.delta_field(16))
    _no_launch(monkeypatch)
    with pytest.raises(ValueError, match="3D"):
        T.WALE_nuSGS(D, g)

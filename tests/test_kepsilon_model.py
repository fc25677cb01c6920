"""The k-epsilon right-hand sides of tests/kepsilon_model.py against answers that do not come from libibhip -- the closed
forms on linear velocity fields with constant k and eps --, the Float32 oracle composition's own deviation from them on the
meshes of tests/test_gpu_k_epsilon.py (the bounds its checks import), and ``ibh_k_epsilon_rhs``'s argument checks, which
need no GPU: every misuse is reported through ``ibh_last_error`` before anything is launched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import kepsilon_model as km
import les_model as lm
from abi import assert_bound
from conftest import oracle_view
from ibamd import _lib

f32, f64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MESHES = [("octree", lm.octree_mesh), ("bs4 2d", lambda: lm.bs4_mesh(2)), ("bs4 3d", lambda: lm.bs4_mesh(3))]


def test_closed_form_by_hand():
    """Pure shear a: S = |a|, tr = 0.  Dilatation d: S = d sqrt(2 nd), tr = nd d.  Rotation: S = 0, tr = 0."""
    k0, e0 = f64(km.K0), f64(km.EPS0)
    Cmu, C1, C2 = (f64(km.PARAMS[x]) for x in ("Cmu", "C1", "C2"))
    nut = Cmu * k0 * k0 / e0
    a = f64(f32(0.7))
    ans = km.closed_form(lm.shear(3, 0.7), 4)
    assert np.allclose(ans["rk"], nut * a * a - e0, rtol=1e-14, atol=0)
    assert np.allclose(ans["reps"], C1 * nut * a * a * e0 / k0 - C2 * e0 * e0 / k0, rtol=1e-14, atol=0)
    for nd in (2, 3):
        d = f64(f32(1.3))
        ans = km.closed_form(lm.dilatation(nd), 4)
        S2 = 2.0 * nd * d * d
        assert np.allclose(ans["S"] ** 2, S2, rtol=1e-14, atol=0)
        assert np.allclose(ans["rk"], nut * S2 - e0 - k0 * nd * d, rtol=1e-14, atol=0)
        assert np.allclose(ans["reps"], C1 * nut * S2 * e0 / k0 - C2 * e0 * e0 / k0 - e0 * nd * d, rtol=1e-14, atol=0)
        ans = km.closed_form(lm.rotation(nd), 4)
        assert np.allclose(ans["rk"], -e0, rtol=1e-14, atol=0) and np.allclose(ans["reps"], -C2 * e0 * e0 / k0, rtol=1e-14, atol=0)
    assert np.allclose(ans["nut"], nut, rtol=1e-14, atol=0)


@pytest.mark.parametrize("key,make", MESHES, ids=[k.replace(" ", "_") for k, _ in MESHES])
def test_oracle_composition_on_linear_fields(key, make):
    """The Float64 oracle composition gives the closed forms on the cells of ``les_model.interior`` up to the one rounding
    of ``u = A x`` to Float32 (|u| <= 8: 2^-22 per value, / h >= 1/32 in a gradient or a divergence, times k0, eps0 or
    2 nut S ~ 1: below 1e-4), and the Float32 oracle composition's own deviation -- the device's bound is 4 x it -- is
    printed per output."""
    part = lm.one_partition(make())
    op = oracle_view(part)
    sel = lm.interior(part)
    assert 2 * sel.sum() >= sel.size, f"{key}: the mask keeps {sel.sum()} of {sel.size} cells"
    n = sel.size
    k, eps = np.full(n, km.K0, f32), np.full(n, km.EPS0, f32)
    for name, mk in lm.FIELDS:
        A = mk(part.ndims)
        got, _ = km.oracle_rhs(op, lm.linear_field(part, A), k, eps, dtype=f64)
        ans = km.closed_form(A, n)
        for o in km.OUTPUTS:
            e = float(np.abs(got[o] - ans[o])[sel].max())
            assert e <= 1e-4, (key, name, o, e)
    bound, dev = km.bounds(key, part, op)
    print(f"\n{key}: {sel.sum()} of {sel.size} cells; Float32 oracle composition against the closed forms:")
    for o in km.OUTPUTS:
        print(f"  {o}: {dev[o]:.3e}")
    assert set(dev) == set(km.OUTPUTS) and all(bound[o] == 4.0 * dev[o] for o in dev)
    assert max(dev.values()) <= 1e-2          # Float32 rounding, not a discretisation error


def test_fields_are_positive_and_in_range():
    part = lm.one_partition(lm.bs4_mesh(2))
    k, eps = km.k_eps_fields(part)
    assert k.dtype == f32 and eps.dtype == f32
    assert 0.5 <= k.min() and k.max() <= 2.0 and 1.0 <= eps.min() and eps.max() <= 4.0
    assert k.std() > 0.1 and eps.std() > 0.2


def test_wavy_reference_prints_the_float32_oracles_deviation():
    part = lm.one_partition(lm.bs4_mesh(2))
    _, ref, scale, dev = km.wavy_reference("bs4 2d", part, oracle_view(part))
    print("\nbs4 2d, wavy fields: Float32 oracle against the Float64 oracle, per cell / scale:")
    for o in km.WAVY_OUTPUTS:
        print(f"  {o}: {dev[o]:.3e}")
        assert 0 < dev[o] <= 64 * np.finfo(f32).eps, (o, dev[o])
        assert np.isfinite(ref[o]).all() and (scale[o] > 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# the C entry: exported, declared, bound; misuse reported before any launch
# ---------------------------------------------------------------------------------------------------------------------
ARGS = ("p", "vel", "ldv", "k", "eps", "nu", "params5", "rk", "reps", "nut", "S", "G", "ldg")


def test_exported_declared_and_bound():
    assert_bound(("ibh_k_epsilon_rhs",))
    sig = _lib._SIGS["ibh_k_epsilon_rhs"]
    assert len(sig) == len(ARGS)
    assert sig[ARGS.index("ldv")] is C.c_int64 and sig[ARGS.index("ldg")] is C.c_int64 and sig[ARGS.index("nu")] is C.c_float
    jl = open(os.path.join(ROOT, "julia", "IBHip.jl")).read()
    assert re.search(r"function k_epsilon_rhs!\(", jl) and re.search(r"ccall\(\(:ibh_k_epsilon_rhs,\s*lib\)", jl)


def _args(**over):
    """A well-formed argument list over host buffers (nothing is dereferenced before the checks: every case below returns
    from them), with single arguments replaced.  The partition is a zeroed stand-in: nd = 0, nc = 0."""
    buf = (C.c_float * 64)()
    handle = (C.c_char * 8192)()
    b = C.addressof(buf)
    a = dict(p=C.addressof(handle), vel=b, ldv=16, k=b, eps=b, nu=1.5e-5, params5=b, rk=b, reps=b, nut=b, S=b, G=b, ldg=16)
    a.update(over)
    return [a[x] for x in ARGS], (buf, handle)


CASES = [(dict([(name, None)]), b"null argument") for name in ("p", "vel", "k", "eps", "params5", "rk", "reps")]
CASES += [(dict(ldv=-1), b"ldv < nc"), (dict(ldg=-1), b"ldg < nc")]


@pytest.mark.parametrize("over,what", CASES, ids=[next(iter(o)) for o, _ in CASES])
def test_misuse_is_reported_before_any_launch(over, what):
    lib = _lib.load()
    args, keep = _args(**over)
    rc = lib.ibh_k_epsilon_rhs(*args)
    assert rc != 0 and what in lib.ibh_last_error() and b"ibh_k_epsilon_rhs" in lib.ibh_last_error(), lib.ibh_last_error()


@pytest.mark.parametrize("over", [dict(), dict(nut=None, S=None, G=None, ldg=-1)], ids=["all_outputs", "rk_reps_alone"])
def test_an_empty_partition_is_no_error(over):
    lib = _lib.load()
    args, keep = _args(**over)
    assert lib.ibh_k_epsilon_rhs(*args) == 0

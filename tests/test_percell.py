"""The per-cell checker of tests/percell.py, on the CPU: calibration and sensitivity.

Calibration: the Float32 numpy oracle and the C restatement (oracle/residual_c.py) stay at or below half of the bounds the
GPU tests use (tests/test_gpu_percell.py) against the float64 evaluation -- the bounds have room for correct Float32
arithmetic.  Sensitivity: errors a norm-wise check passes (a 1e-4 relative error on the coarsest level alone, one face
with the wrong neighbour) and a block computed from a shifted input fail the per-cell check.
"""
import os

import numpy as np
import pytest

import ibamd
import percell as pc
from conftest import ADV_FAMILIES, GOLDEN, RAE_FAMILIES, advection_mesh, euler_field, oracle_view, rae_mesh, rel_inf, \
    seeded_field
from oracle import cfd as ocfd
from oracle import residual_c as rc

f32, f64 = np.float32, np.float64


def _octree_partition():
    from test_golden import _partition
    return _partition(dict(np.load(os.path.join(GOLDEN, "octree_partition.npz"))))


@pytest.fixture(scope="module")
def cases():
    """(name, product partition) of the RAE2822 and advection test partitions and the 3-D octree with level jumps."""
    out = []
    for name, msh, fam, mps in (("rae", rae_mesh(), RAE_FAMILIES, 16384), ("adv", advection_mesh(), ADV_FAMILIES, 4096)):
        dom = ibamd.Domain(msh, hypercube_families=fam, max_partition_size=mps)
        out += [(f"{name}{k}", p) for k, p in dom.partitions.items()]
    out.append(("octree", _octree_partition()))
    return out


def _fields(part):
    x = part.centers
    n = x.shape[0]
    if part.ndims == 2:
        Cv = np.stack([np.ones(n, f32), f32(0.5) + seeded_field(x, seed=3) * f32(0.1)], axis=1)
        us = {kind: seeded_field(x, kind=kind) for kind in ("smooth", "step")}
        P = euler_field(x, seed=3)
    else:
        rng = np.random.default_rng(5)
        Cv = np.stack([np.ones(n, f32), f32(0.5) + f32(0.1) * rng.uniform(-1, 1, n).astype(f32), np.full(n, -0.25, f32)],
                      axis=1)
        smooth = (np.sin(2 * x[:, 0]) * np.cos(3 * x[:, 1]) + 0.3 * x[:, 2] + 0.1 * rng.uniform(-1, 1, n)).astype(f32)
        step = ((x[:, 1] > x[:, 0]).astype(f32) + f32(0.01) * rng.uniform(-1, 1, n).astype(f32)).astype(f32)
        us = {"smooth": smooth, "step": step}
        P = euler_field(x, seed=3)
    return us, Cv, P


def test_the_oracle_is_dtype_generic(cases):
    """Float32 inputs: the Float32 oracle (the committed golden vectors pin its bits); float64 inputs: float64 throughout."""
    name, part = cases[0]
    op = oracle_view(part)
    us, Cv, P = _fields(part)
    assert pc.oracle_advection_residual(op, us["smooth"], Cv).dtype == f32
    assert pc.oracle_euler_residual(op, P, ocfd.Fluid()).dtype == f32
    assert pc.ref64_advection(op, us["smooth"], Cv).dtype == f64
    assert pc.ref64_euler(op, P).dtype == f64


def test_calibration(cases):
    """Float32 oracle and C restatement against float64: at most half of the GPU bounds, on every case and field."""
    worst = {"numpy_scalar": 0.0, "c_scalar": 0.0, "numpy_euler": 0.0, "c_euler": 0.0}
    for name, part in cases:
        op = oracle_view(part)
        cp = rc.CPart(part)
        us, Cv, P = _fields(part)
        for kind, u in us.items():
            r64 = pc.ref64_advection(op, u, Cv)
            s = pc.scalar_scale(part, u, r64)
            worst["numpy_scalar"] = max(worst["numpy_scalar"], pc.percell_error(pc.oracle_advection_residual(op, u, Cv),
                                                                                r64, s).max())
            worst["c_scalar"] = max(worst["c_scalar"], pc.percell_error(cp.residual_advection(u, Cv), r64, s).max())
        r64 = pc.ref64_euler(op, P)
        s = pc.euler_scale(part, P, r64)
        worst["numpy_euler"] = max(worst["numpy_euler"],
                                   pc.percell_error(pc.oracle_euler_residual(op, P, ocfd.Fluid()), r64, s).max())
        worst["c_euler"] = max(worst["c_euler"], pc.percell_error(cp.residual_euler(P), r64, s).max())
    print("\ncalibration (per-cell error of the Float32 restatements against float64):", worst)
    assert worst["numpy_scalar"] <= pc.BOUND / 2 and worst["c_scalar"] <= pc.BOUND / 2, worst
    assert worst["numpy_euler"] <= pc.BOUND_EULER / 2 and worst["c_euler"] <= pc.BOUND_EULER / 2, worst


def _neighbour_swapped_views(part, x, k=6):
    """Oracle views of ``part`` in which one interior face of the coarsest level names the wrong neighbour: the cell one
    step further along the same dimension.  Of all such faces, the ``k`` whose wrong neighbour looks most like the right
    one (value and gradient of ``x`` along the face's dimension): wrong ids that a norm-wise check is least likely to see."""
    from oracle import domain as od
    lev = pc.levels(part)
    top = lev.max()
    op = oracle_view(part)
    xs = np.asarray(x, dtype=f64).reshape(x.shape[0], -1)
    cand = []
    for d in range(1, part.ndims + 1):
        o, nb = part.face_owners_neighbors[d]
        nxt = np.full(part.spacing.shape[0], -1, np.int64)   # the cell across the single far face along d
        inner = o != nb
        nxt[o[inner]] = nb[inner]
        nxt[np.bincount(o[inner], minlength=nxt.size) != 1] = -1
        far = nxt[nb]
        ok = inner & (lev[o] == top) & (lev[nb] == top) & (far >= 0) & (far != o)
        ok[ok] &= lev[far[ok]] == top
        if not ok.any():
            continue
        g = np.asarray(od.cell_gradient(op, x, d), dtype=f64).reshape(x.shape[0], -1) * part.spacing[:, d - 1:d]
        sx = np.abs(xs).max(axis=0)
        f = np.nonzero(ok)[0]
        diff = ((np.abs(xs[far[f]] - xs[nb[f]]) + np.abs(g[far[f]] - g[nb[f]])) / sx).max(axis=1)
        cand += [(float(diff[i]), d, int(f[i]), int(far[f[i]])) for i in range(f.size)]
    assert cand, "no interior face on the coarsest level"
    for _, d, f, far in sorted(cand)[:k]:
        view = oracle_view(part)
        fon = dict(view.face_owners_neighbors)
        o, nb = fon[d]
        nb2 = nb.copy()
        nb2[f] = far
        fon[d] = (o, nb2)
        view.face_owners_neighbors = fon
        yield view


def _one_block(part):
    """Cells of one complete block on the coarsest level (2-D: the library's block table; 3-D: 512 cells from a base)."""
    lev = pc.levels(part)
    if part.ndims == 2:
        from ibamd import hostview
        bases = hostview.analyze2(part)["blocks"]["base"]
        bases = bases[lev[bases] == lev.max()]
        return np.arange(64) + int(bases[len(bases) // 2])
    b = int(np.nonzero(lev == lev.max())[0][0])
    return np.arange(512) + b


@pytest.mark.parametrize("which", ["scalar", "euler"])
def test_sensitivity(cases, which):
    """Every injected error fails the per-cell check.  On the RAE2822 partitions (ten levels) the coarse-level error, and
    for the scalar step field the wrong neighbour id, also pass the norm-wise check: that is the gap this checker closes."""
    fluid = ocfd.Fluid()
    gap = 0
    for name, part in cases:
        op = oracle_view(part)
        us, Cv, P = _fields(part)
        if which == "scalar":
            u = us["step"]
            res = lambda view, x: pc.oracle_advection_residual(view, x, Cv)  # noqa: E731
            r64 = pc.ref64_advection(op, u, Cv)
            s = pc.scalar_scale(part, u, r64)
            x, bound = u, pc.BOUND
        else:
            res = lambda view, x: pc.oracle_euler_residual(view, x, fluid)  # noqa: E731
            r64 = pc.ref64_euler(op, P)
            s = pc.euler_scale(part, P, r64)
            x, bound = P, pc.BOUND_EULER
        r32 = res(op, x)
        assert pc.check(r32, r64, s, bound, part, what=name) <= bound            # the unbroken oracle passes
        lev = pc.levels(part)
        multilevel = lev.max() >= 2
        # (1) a 1e-4 relative error on the coarsest level alone
        bad = r32.copy()
        bad[lev == lev.max()] *= f32(1 + 1e-4)
        with pytest.raises(AssertionError, match="per-cell error"):
            pc.check(bad, r64, s, bound, part, what=name)
        if multilevel:
            assert rel_inf(bad, r64) <= 1e-5, name
            gap += 1
        # (2) one interior face on the coarsest level with the wrong neighbour
        # (the most inconspicuous wrong id whose effect exceeds the bound at all: a wrong neighbour with the same value
        # and gradient as the right one changes nothing any check could see)
        bad = next((b for b in (res(view, x) for view in _neighbour_swapped_views(part, x))
                    if pc.percell_error(b, r64, s).max() > bound), None)
        assert bad is not None, name
        with pytest.raises(AssertionError, match="per-cell error"):
            pc.check(bad, r64, s, bound, part, what=name)
        if multilevel and which == "scalar":   # (the Euler state is noisy on every level: there a wrong id is seen
            assert rel_inf(bad, r64) <= 1e-5, name   # norm-wise too)
        # (3) one block's residual from a shifted input
        blk = _one_block(part)
        bad = r32.copy()
        bad[blk] = res(op, np.roll(x, 1, axis=0))[blk]
        with pytest.raises(AssertionError, match="per-cell error") as e:
            pc.check(bad, r64, s, bound, part, what=name)
        if part.ndims == 2:   # the report names the block class of the bad block
            assert "level" in str(e.value) and ("quad" in str(e.value) or "single" in str(e.value))
    assert gap >= 3      # the RAE2822 partitions: ten levels, the coarsest ~700x below the finest


def test_report_points_at_the_class(cases):
    """The failure message lists the worst cell per class, and the class that holds the error stands out."""
    name, part = cases[0]
    op = oracle_view(part)
    us, Cv, _ = _fields(part)
    u = us["smooth"]
    r64 = pc.ref64_advection(op, u, Cv)
    s = pc.scalar_scale(part, u, r64)
    lev = pc.levels(part)
    bad = pc.oracle_advection_residual(op, u, Cv)
    top = lev == lev.max()
    bad[top] += f32(1e-3) * s[top].astype(f32)
    with pytest.raises(AssertionError) as e:
        pc.check(bad, r64, s, pc.BOUND, part, what=name)
    lines = {ln.split("(")[0].strip(): float(ln.split("max ")[1].split()[0]) for ln in str(e.value).splitlines()[1:]}
    assert lines[f"level{lev.max()}"] > 5e-4 and lines["level0"] < pc.BOUND

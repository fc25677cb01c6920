"""Per-cell error checks of the fused residual sweeps against a float64 evaluation of the oracle.

Test infrastructure.  A norm-wise check (``conftest.rel_inf``: max |got - exp| / max |exp|) cannot see a wrong coarse
block: for a noisy state the residual grows like 1/h, so the coarsest level sits ~700x below the finest one and a
0.1 % error on every coarsest-level cell passes 1e-5.  Here every cell is held to its own scale:

- scalar sweeps: ``conftest.stencil_scale`` = |ref| + max |u| over the cell and its face neighbours / h;
- Euler sweeps, per variable v: |ref_v| + max over the cell's two-deep face neighbourhood of sum_d |F_d,v(P)| / h, with
  F_d(P) = inviscid_fluxes(P, P, d) the physical flux (HLL consistency): the residual is a difference of such fluxes.

The reference is the numpy oracle evaluated in float64 (it is dtype-generic: Float32 inputs give the Float32 oracle
bit for bit, tests/test_golden.py).  ``check`` reports the worst cell of every class -- refinement level, image /
skirt, the side kinds of the cell's faces and, in 2-D, the block class of the partition tables (quad, pair, single,
face-list cell, deeper-cell table) -- so that a failure points at a class.
"""
import numpy as np

from oracle import cfd as ocfd
from oracle import domain as od

f32, f64 = np.float32, np.float64

# Per-cell bounds of the GPU sweeps against the float64 reference.  The Float32 oracle and its C restatement stay below
# half of them on every test case (tests/test_percell.py::test_calibration: 4.6e-7 scalar, 1.0e-6 Euler); a 1e-4 relative
# error on the coarsest level alone reads 3e-5 (tests/test_percell.py::test_sensitivity).
BOUND = 2e-6
BOUND_EULER = 2.5e-6


def oracle_advection_residual(part, u, C):
    """test/advection.jl:67-83 with ud starting from zero, in the dtype of ``u`` and ``C``."""
    ud = np.zeros_like(u)
    D = od.JST_sensor(part, u)
    for dim in range(1, part.ndims + 1):
        Cf = od.at_faces(part, np.ascontiguousarray(C[:, dim - 1]), dim)
        gu = od.cell_gradient(part, u, dim)
        uL, uR = od.MUSCL(part, u, gu, dim, D=D, high_order=True)
        ud -= od.green_gauss(part, (uL + uR) * Cf / f32(2) + np.abs(Cf) * (uL - uR) / f32(2), dim)
    return ud


def oracle_euler_residual(part, P, fluid):
    """Euler HLL residual composed from the reference operators, in the dtype of ``P``."""
    R = np.zeros_like(P)
    D = od.JST_sensor(part, np.ascontiguousarray(P[:, 0]))
    for dim in range(1, part.ndims + 1):
        gP = od.cell_gradient(part, P, dim)
        PL, PR = od.MUSCL(part, P, gP, dim, D=D, high_order=True)
        F = ocfd.inviscid_fluxes(fluid, PL, PR, dim)
        R -= od.green_gauss(part, F, dim)  # Float64 flux, rounded on the in-place update
    return R


def ref64_advection(part, u, C):
    r = oracle_advection_residual(part, np.asarray(u).astype(f64), np.asarray(C).astype(f64))
    assert r.dtype == f64
    return r


def ref64_euler(part, P, fluid=None):
    r = oracle_euler_residual(part, np.asarray(P).astype(f64), fluid or ocfd.Fluid())
    assert r.dtype == f64
    return r


def _face_max(part, a):
    """max of ``a`` over each cell and its face neighbours (rows of a 1-D or 2-D array)."""
    m = a.copy()
    for d in range(1, part.ndims + 1):
        o, nb = part.face_owners_neighbors[d]
        np.maximum.at(m, o, a[nb])
        np.maximum.at(m, nb, a[o])
    return m


def scalar_scale(part, u, ref):
    from conftest import stencil_scale
    return stencil_scale(part, u, ref)


def euler_scale(part, P, ref, fluid=None):
    """(nc, nv) scale of the Euler residual: |ref_v| + max over the two-deep face neighbourhood of sum_d |F_d,v(P)| / h."""
    fluid = fluid or ocfd.Fluid()
    P64 = np.asarray(P).astype(f64)
    F = np.zeros_like(P64)
    for d in range(1, part.ndims + 1):
        F += np.abs(ocfd.inviscid_fluxes(fluid, P64, P64, d))
    m = _face_max(part, _face_max(part, F))
    h = np.asarray(part.spacing).min(axis=1).astype(f64)
    return np.abs(np.asarray(ref, dtype=f64)) + m / h[:, None]


def percell_error(got, ref, scale):
    """|got - ref| / scale per cell (and variable)."""
    return np.abs(np.asarray(got, dtype=f64) - np.asarray(ref, dtype=f64)) / np.asarray(scale, dtype=f64)


# ---------------------------------------------------------------------------------------------------------------------
# cell classes
# ---------------------------------------------------------------------------------------------------------------------
def levels(part):
    """Refinement level per cell: 0 = finest."""
    h = np.asarray(part.spacing).min(axis=1)
    hs = np.unique(h)
    return np.searchsorted(hs, h)


def _side_classes(part):
    """Per cell: has a face to a coarser cell / to finer cells / a mirror face / no face on some side."""
    nc = part.spacing.shape[0]
    sp = np.asarray(part.spacing)
    coarse = np.zeros(nc, bool)
    fine = np.zeros(nc, bool)
    mirror = np.zeros(nc, bool)
    edge = np.zeros(nc, bool)                    # no face at all on one side: the edge of a skirt
    for d in range(1, part.ndims + 1):
        o, nb = part.face_owners_neighbors[d]
        ho, hn = sp[o, d - 1], sp[nb, d - 1]
        coarse[o[hn > ho]] = True
        coarse[nb[ho > hn]] = True
        fine[o[hn < ho]] = True
        fine[nb[ho < hn]] = True
        mirror[o[o == nb]] = True                # a mirror face names the cell twice
        nleft = np.bincount(nb, minlength=nc)    # faces on the low side of the cell (the cell is the neighbour)
        nright = np.bincount(o, minlength=nc)
        edge |= (nleft == 0) | (nright == 0)
    return dict(side_coarse=coarse, side_fine=fine, side_mirror=mirror, side_open=edge,
                side_same=~(coarse | fine | mirror | edge))


def _block_classes_2d(part):
    """Block classes of the 2-D quad sweep from the library's host-side analysis (csrc/ibh_analyze.cpp)."""
    from ibamd import hostview
    A = hostview.analyze2(part)
    nc = part.spacing.shape[0]
    out = {}

    def cells(bases, n):
        m = np.zeros(nc, bool)
        if len(bases):
            m[(np.asarray(bases, np.int64)[:, None] + np.arange(n)).ravel()] = True
        return m
    blocks = A["blocks"]
    Q = A["quads_all"]
    out["quad"] = cells(Q["desc"]["base"], 256)
    out["pair"] = cells(Q["pair_desc"]["base"], 128)
    single = Q["singles2"] if len(Q["pair_desc"]) else Q["singles"]
    out["single"] = cells(blocks["base"][single], 64)
    out["deeper_table"] = cells(blocks["base"][blocks["dt"] >= 0], 64)
    out["face_list"] = ~cells(blocks["base"], 64)
    QI = A["quads_image"]
    out["image_quad"] = cells(QI["desc"]["base"], 256)
    out["image_single"] = cells(blocks["base"][QI["singles"]], 64) if len(QI["singles"]) else np.zeros(nc, bool)
    return out


def cell_classes(part, block_classes=True):
    """{class name: boolean mask over the partition's cells}."""
    nc = part.spacing.shape[0]
    out = {}
    lev = levels(part)
    for k in range(lev.max() + 1):
        out[f"level{k}"] = lev == k
    img = np.zeros(nc, bool)
    img[np.asarray(part.image_in_domain)] = True
    out["image"] = img
    out["skirt"] = ~img
    out.update(_side_classes(part))
    if block_classes and part.ndims == 2 and getattr(part, "block_size", 8) == 8:
        out.update(_block_classes_2d(part))
    return {k: v for k, v in out.items() if v.any()}


# ---------------------------------------------------------------------------------------------------------------------
# the check
# ---------------------------------------------------------------------------------------------------------------------
def report(err, classes, got=None, ref=None, scale=None):
    """One line per class: worst cell (and variable), its error, value, reference and scale."""
    e = err if err.ndim == 2 else err[:, None]
    lines = []
    for name, mask in classes.items():
        if not mask.any():
            continue
        sub = e[mask]
        i, v = np.unravel_index(int(np.argmax(sub)), sub.shape)
        c = int(np.nonzero(mask)[0][i])
        s = f"  {name:>14s} ({int(mask.sum()):6d} cells): max {sub[i, v]:.3e} at cell {c} var {v}"
        if got is not None:
            g = np.asarray(got, dtype=f64).reshape(e.shape[0], -1)
            r = np.asarray(ref, dtype=f64).reshape(e.shape[0], -1)
            sc = np.asarray(scale, dtype=f64).reshape(e.shape[0], -1)
            s += f" (got {g[c, v]:.7g}, ref {r[c, v]:.7g}, scale {sc[c, v]:.3g})"
        lines.append(s)
    return "\n".join(lines)


def check(got, ref64, scale, bound, part, cells=None, classes=None, what=""):
    """Assert max(|got - ref64| / scale) <= bound over ``cells`` (all cells by default); return that maximum.  The
    failure message lists the worst cell of every class."""
    err = percell_error(got, ref64, scale)
    sel = np.ones(err.shape[0], bool)
    if cells is not None:
        sel = np.zeros(err.shape[0], bool)
        sel[np.asarray(cells)] = True
    e = np.where(sel if err.ndim == 1 else sel[:, None], err, 0.0)
    if np.isnan(e).any():
        worst = float("nan")
    else:
        worst = float(e.max())
    if not worst <= bound:
        cls = classes if classes is not None else cell_classes(part)
        cls = {k: m & sel for k, m in cls.items()}
        nan = np.isnan(e).any(axis=1) if e.ndim == 2 else np.isnan(e)
        msg = (f"{what}: per-cell error {worst:.3e} > bound {bound:.1e}; {int(nan.sum())} NaN cells; "
               f"worst cell per class:\n" + report(np.nan_to_num(e, nan=np.inf), cls, got, ref64, scale))
        raise AssertionError(msg)
    return worst

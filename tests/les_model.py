"""Known answers of the LES closures and shock sensors on constant velocity-gradient tables, the meshes and linear velocity
fields that carry them onto a partition, and the bounds of the device's analytic-field check.

Test infrastructure shared by tests/test_les_model.py (CPU) and tests/test_gpu_les.py (GPU).

A table is ``A[i][j] = d u_i / d x_j`` (Float32 entries, none of them a dyadic number, so that ``u = A x`` rounds on the
mesh); its answers come from ``oracle.turbulence`` / ``oracle.cfd`` evaluated on the table itself in float64 -- nothing of
libibhip is involved.  On a partition the velocity ``u = A x`` is rounded to Float32 once; the Float32 oracle composition
(``cell_gradient`` per component, then the pointwise functions) deviates from the table answers by that rounding pushed
through the gradient and the formulas.  ``bounds`` measures this deviation per output over the three fields and the
selected cells of a mesh; the device is held to 4 x it (its gradients are made with other, equally rounded, expressions
on block partitions; the factor is tests/percell.py's).
"""
import numpy as np

from oracle import cfd as ocfd
from oracle import domain as od
from oracle import turbulence as ot

f32, f64 = np.float32, np.float64
CS, CW = f32(0.17), f32(0.325)
EPS32 = f64(np.finfo(f32).eps)
EPS_SHOCK = f64(f32(1e-14))
OUTPUTS = ("S", "ducros", "shock", "smagorinsky", "wale")


# ---------------------------------------------------------------------------------------------------------------------
# tables
# ---------------------------------------------------------------------------------------------------------------------
def shear(nd, a=0.7):
    """Pure shear: d u / d y = a."""
    A = np.zeros((nd, nd), f32)
    A[0, 1] = a
    return A


def dilatation(nd, d=1.3):
    """Pure dilatation: d u_i / d x_i = d."""
    return (f32(d) * np.eye(nd)).astype(f32)


def rotation(nd, w=(0.3, -0.9, 0.6)):
    """Solid rotation u = omega x r (3-D), u = w (-y, x) (2-D, w = the z component)."""
    A = np.zeros((nd, nd), f32)
    if nd == 2:
        A[0, 1], A[1, 0] = -w[2], w[2]
    else:
        A[0, 1], A[0, 2] = -w[2], w[1]
        A[1, 0], A[1, 2] = w[2], -w[0]
        A[2, 0], A[2, 1] = -w[1], w[0]
    return A


FIELDS = (("shear", shear), ("dilatation", dilatation), ("rotation", rotation))


def table(A, n=1, dtype=f64):
    """The nd x nd table of length-n vectors the pointwise functions take."""
    nd = A.shape[0]
    return [[np.full(n, A[i, j], dtype) for j in range(nd)] for i in range(nd)]


def pointwise(g, Delta):
    """Every output of the closure from a gradient table, in the dtype of the table."""
    nd = len(g)
    S = ot.shear_rate(g)
    out = dict(S=S, ducros=ot.Ducros_sensor(g), shock=ocfd.shock_sensor(g), smagorinsky=ot.Smagorinsky_nuSGS(Delta, S, CS))
    if nd == 3:
        out["wale"] = ot.WALE_nuSGS(Delta, g, CW)
    return out


def answers(A, Delta):
    """The table answers per cell (float64): the pointwise oracle on the constant table."""
    D = np.asarray(Delta).astype(f64)
    return pointwise(table(A, D.shape[0], f64), D)


# ---------------------------------------------------------------------------------------------------------------------
# meshes and partitions
# ---------------------------------------------------------------------------------------------------------------------
def octree_mesh():
    """[-2, 2]^3, 8^3 blocks, one refined ball: SAME, MIRROR, COARSE and FINE sides."""
    from ibamd import Ball, Mesh
    return Mesh(f32([-2, -2, -2]), f32([4, 4, 4]), block_size=8,
                refinement_regions=[(Ball(np.array([1.2, 1.2, 1.2]), 0.1), f32(0.1))])


def single_block_mesh():
    """[-2, 2]^3 as ONE 8^3 block: six mirror sides."""
    from ibamd import Mesh
    return Mesh(f32([-2, -2, -2]), f32([4, 4, 4]), block_size=8)


def bs4_mesh(nd):
    """4^nd blocks with 2:1 interfaces: a partition without block structure."""
    from ibamd import Ball, Mesh
    return Mesh(f32([-2] * nd), f32([4] * nd), block_size=4,
                refinement_regions=[(Ball(np.array([1.2] * nd), 0.1), f32(0.05 if nd == 2 else 0.12))])


def one_partition(msh):
    import ibamd
    (part,) = ibamd.Domain(msh, max_partition_size=10 ** 9, boundaries=False).partitions.values()
    return part


def interior(part):
    """Cells whose 2-ring is same-level with no mirror face: every cell within two face hops has the cell's spacing, and the
    cell has a face on each of its sides, none of them a mirror face.  Such a cell has exactly one same-level neighbour
    across every side: its gradient of a linear field is the field's, up to rounding."""
    nc = part.spacing.shape[0]
    h = np.asarray(part.spacing).min(axis=1)
    lo, hi = h.copy(), h.copy()
    ok = np.ones(nc, bool)
    for d in range(1, part.ndims + 1):
        o, nb = part.face_owners_neighbors[d]
        ok[o[o == nb]] = False                      # a mirror face names the cell twice
        ok &= (np.bincount(nb, minlength=nc) >= 1) & (np.bincount(o, minlength=nc) >= 1)
    for _ in range(2):
        l2, h2 = lo.copy(), hi.copy()
        for d in range(1, part.ndims + 1):
            o, nb = part.face_owners_neighbors[d]
            np.minimum.at(l2, o, lo[nb])
            np.minimum.at(l2, nb, lo[o])
            np.maximum.at(h2, o, hi[nb])
            np.maximum.at(h2, nb, hi[o])
        lo, hi = l2, h2
    return ok & (lo == h) & (hi == h)


def filter_width(part):
    """Delta = (product of the spacings)^(1 / nd), Float32."""
    sp = np.asarray(part.spacing).astype(f64)
    return (np.prod(sp, axis=1) ** (1.0 / part.ndims)).astype(f32)


def linear_field(part, A):
    """u = A x at the cell centres, rounded to Float32 once."""
    return (np.asarray(part.centers).astype(f64) @ A.astype(f64).T).astype(f32)


def oracle_composition(op, vel, Delta):
    """The Float32 oracle composition: cell_gradient per component, then the pointwise functions."""
    nd = op.ndims
    g = [list(od.cell_gradient(op, np.ascontiguousarray(vel[:, i]))) for i in range(nd)]
    return pointwise(g, Delta), g


_BOUNDS = {}


def bounds(key, part, op):
    """{output: 4 x max over the three fields and the cells of ``interior(part)`` of |Float32 oracle composition - table
    answer|} for the mesh ``key`` (computed once), and the deviations themselves."""
    if key not in _BOUNDS:
        sel = interior(part)
        Delta = filter_width(part)
        dev = {}
        for name, make in FIELDS:
            A = make(part.ndims)
            got, _ = oracle_composition(op, linear_field(part, A), Delta)
            ans = answers(A, Delta)
            for k in got:
                assert got[k].dtype == f32, k
                dev[k] = max(dev.get(k, 0.0), float(np.abs(got[k].astype(f64) - ans[k])[sel].max()))
        _BOUNDS[key] = ({k: 4.0 * v for k, v in dev.items()}, dev)
    return _BOUNDS[key]

"""Inputs and restatements shared by the FlowBC boundary-condition tests (test_flow_bc_oracle.py, test_gpu_flow_bc.py):

* the seeded image-point family on which the Float32 oracle closure is pinned against its Float64 evaluation;
* the oracle's composed wall / far-field closures (the lines of tests/test_config5.py:87-98, any dimension, any dtype);
* synthetic ``Boundary`` structs over a random field -- no mesh --, with a ghost cell among the donors or without;
* a host loop that writes ghost cells one after the other IN GHOST ORDER (what a direct write would give where a ghost
  cell is a donor of a later row), from the same tables.
"""
import numpy as np

import ibamd
from ibamd.accumulator import Accumulator
from ibamd.domain import Boundary

f32 = np.float32
TOL = 1e-5    # the project's standing bound (test_gpu_runtime.py::test_flow_bc_in_impose_bc, test_config5.py RES_TOL)
FAR3 = [1.0e5, 288.15, 100.0, 0.0, 0.0]


def image_point_family(n, nd, seed=0):
    """p, T = 1e5, 288.15 +- 5 %; u = 100 +- 10 %, the other velocities +- 20; unit normals; y = 10^U(-3, -0.5)."""
    rng = np.random.default_rng(seed)
    P = np.empty((n, nd + 2), dtype=np.float64)
    P[:, 0] = 1e5 * (1 + 0.05 * rng.uniform(-1, 1, n))
    P[:, 1] = 288.15 * (1 + 0.05 * rng.uniform(-1, 1, n))
    P[:, 2] = 100.0 * (1 + 0.1 * rng.uniform(-1, 1, n))
    for d in range(1, nd):
        P[:, 2 + d] = 20.0 * rng.uniform(-1, 1, n)
    nrm = rng.normal(size=(n, nd))
    nrm /= np.sqrt((nrm * nrm).sum(axis=1))[:, None]
    y = 10.0 ** rng.uniform(-3, -0.5, n)
    return P.astype(f32), nrm.astype(f32), y.astype(f32)


def oracle_wall_closure(ofluid, o_wall, Pi, normals, image_distances, **wall_kw):
    """The wall closure of tests/test_config5.py:91-97 -> (boundary state, wall_function's dict)."""
    from oracle import cfd as ocfd
    from oracle import turbulence as ot
    rho = Pi[:, 0] / (ofluid.R * Pi[:, 1])
    nu = ocfd.dynamic_viscosity(ofluid, Pi[:, 1]) / rho
    un = (Pi[:, 2:] * normals).sum(axis=1)
    ut = np.sqrt(((Pi[:, 2:] - un[:, None] * normals) ** 2).sum(axis=1))
    wf = ot.wall_function(image_distances, ut, nu, **wall_kw)
    return o_wall(Pi, normals, dudn=wf["du_dn"], image_distances=image_distances), wf


def oracle_config5_bcs(view, Q, far, R_inf, wall_name, far_name="farfield"):
    """tests/test_config5.py:87-98 for any dimension: the oracle's ``impose_bc`` with the two closures, in place."""
    from oracle import cfd as ocfd
    from oracle import domain as od
    nd = Q.shape[1] - 3
    ofluid = ocfd.Fluid()
    o_free = ocfd.FlowBC(ofluid, f32(far))
    o_wall = ocfd.FlowBC(ofluid, f32([far[0], far[1], 0.0]), normal_flow=True)
    P, R = Q[:, :nd + 2], Q[:, nd + 2]
    od.impose_bc(lambda b, Pi, Ri: (o_free(Pi, b.normals), R_inf), view, far_name, P, R)

    def wall_bc(b, Pi, Ri):
        ba, wf = oracle_wall_closure(ofluid, o_wall, Pi, b.normals, b.image_distances)
        return ba, wf["nut"]
    od.impose_bc(wall_bc, view, wall_name, P, R)


class FakeDomain:
    """What ``impose_bc`` / ``impose_flow_bc`` read of a Domain: the dimension, the number of cells, the boundaries."""

    def __init__(self, nd, n, boundaries):
        self.ndims, self.n, self.boundaries = nd, n, boundaries

    def __len__(self):
        return self.n


PLANTED = ("ut0", "u0", "un_neg", "nan_T")


def synthetic_boundary(ng, nd, seed=0, staged=False, extra_cells=3000):
    """A ``Boundary`` of ``ng`` ghost cells over ``n`` cells with a seeded field ``[p T u v (w) s1..s4]`` (n, nd + 6):
    stencil rows of 0..9 entries (so rows start on and off 16-byte boundaries), every ghost cell its own cell.  Donors are
    cells that are no ghost cells; ``staged``: every third ghost cell is also a donor of the NEXT row.  With ng >= 16, rows
    3, 5, 7, 9 are planted one-donor rows (weight 1): velocity parallel to the normal, zero velocity, inflow against the
    normal, a NaN temperature."""
    rng = np.random.default_rng(1000 * nd + seed + ng)
    n = 2 * ng + extra_cells
    perm = rng.permutation(n)
    ghost = np.sort(perm[:ng]).astype(np.int32)
    others = np.sort(perm[ng:]).astype(np.int32)          # never written: free to be donors
    planted_cells = others[:4]
    image_domain = others[4:].copy()
    lens = (np.arange(ng) * 7 + 4) % 10                   # 4, 1, 8, 5, 2, 9, 6, 3, 0, 7, ...
    plant = ng >= 16
    if plant:
        lens[[3, 5, 7, 9]] = 1
    nid0 = image_domain.size
    if staged:
        image_domain = np.concatenate([image_domain, ghost[::3]]).astype(np.int32)   # positions nid0 + k: ghost 3 k
    if plant:
        image_domain = np.concatenate([image_domain, planted_cells]).astype(np.int32)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    idx = rng.integers(0, nid0, size=int(off[-1])).astype(np.int32)
    w = rng.uniform(0.05, 1.0, size=idx.size)
    row = np.repeat(np.arange(ng), lens)
    w = (w / np.maximum(np.bincount(row, weights=w, minlength=ng), 1e-30)[row]).astype(f32)
    if staged:
        for k, g in enumerate(range(0, ng, 3)):           # ghost g is a donor of row g + 1 (its first entry)
            r = g + 1
            if r < ng and lens[r] > 0 and not (plant and r in (3, 5, 7, 9)):
                idx[off[r]] = nid0 + k
    if plant:
        for q, r in enumerate((3, 5, 7, 9)):
            idx[off[r]] = image_domain.size - 4 + q
            w[off[r]] = 1.0
    P, nrm, y = image_point_family(ng, nd, seed=seed + 1)
    F = np.empty((n, nd + 6), dtype=f32)
    F[:, :nd + 2] = image_point_family(n, nd, seed=seed + 2)[0]
    F[:, nd + 2:] = rng.uniform(1e-5, 1e-3, size=(n, 4)).astype(f32)
    if plant:
        nrm[3] = 0.0
        nrm[3, 0] = 1.0
        F[planted_cells[0], 2:nd + 2] = 0.0
        F[planted_cells[0], 2] = 50.0                      # u = 50 n: no tangential part
        F[planted_cells[1], 2:nd + 2] = 0.0                # zero velocity
        F[planted_cells[2], 2:nd + 2] = (-30.0 * nrm[7].astype(np.float64)).astype(f32)
        F[planted_cells[2], 3] += 5.0                      # u . n < 0 with a tangential part
        F[planted_cells[3], 1] = np.nan                    # NaN temperature at a donor
    acc = Accumulator(csr=(off, idx, w), n_input=int(image_domain.size))
    b = Boundary(ghost, np.zeros((ng, nd), f32), nrm, y, (y * rng.uniform(0.1, 0.9, ng)).astype(f32), acc, image_domain)
    return b, F


def rows_of(b):
    """(donor cells, weights) per ghost cell, from the Boundary's tables."""
    acc = b.image_interpolator
    return [(b.image_domain[acc.idx[acc.off[g]:acc.off[g + 1]]], acc.w[acc.off[g]:acc.off[g + 1]])
            for g in range(acc.n_output)]


def host_dirichlet(b, F, nd, far, ghost_order):
    """``impose_bc`` of the Dirichlet ``FlowBC(far)`` on the columns [p T u v (w)] of F with the scalar column nd + 2 copied,
    on the host in Float32 (rows summed in entry order).  ``ghost_order`` False: every ghost cell from the arrays as they
    were (the reference); True: ghost cells written one after the other, each seeing the earlier ones."""
    from oracle import cfd as ocfd
    o_free = ocfd.FlowBC(ocfd.Fluid(), f32(far))
    src = F if ghost_order else F.copy()
    eta = (b.ghost_distances / b.image_distances).astype(f32)
    nv = nd + 3
    for g, (cells, w) in enumerate(rows_of(b)):
        ia = np.zeros(nv, f32)
        for k in range(cells.size):
            t = src[cells[k], :nv] * w[k]
            ia = t if k == 0 else ia + t
        ba = np.concatenate([o_free(ia[None, :nd + 2], b.normals[g:g + 1])[0], ia[nd + 2:]])
        F[b.ghost_indices[g], :nv] = eta[g] * ia + (f32(1) - eta[g]) * ba
    return F

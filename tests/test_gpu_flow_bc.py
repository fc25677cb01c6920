"""``impose_flow_bc`` (``ibh_bc_flow``): ``impose_bc!`` with a ``FlowBC`` closure -- on a wall with ``wall_function(y, u, nu)`` at the
image points -- in one launch per boundary partition.

The kernel calls the device functions of the kernels the composition launches, sums the stencil rows and blends in their
order, and the library is compiled without contraction: its result is the composition's BIT FOR BIT (derived, not
measured).  The composition here is the library's own launches: ``ibh_bc_interp``, the glue lines of the wall closure column
by column as ``HipArray`` broadcasts (the IEEE elementwise kernels), ``cfd.dynamic_viscosity``, ``turbulence.wall_function``,
``cfd.FlowBC``, ``ibh_bc_blend``.  A difference is a finding to trace stage by stage -- the specs isolate the stages --,
not a tolerance to loosen.  Against the oracle (real boundaries) the bound is the project's standing 1e-5, inside which the
Float32 oracle itself stays (at most 1.2e-6 from its Float64 evaluation, test_flow_bc_oracle.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ibamd
from ibamd import _lib
from conftest import oracle_boundaries_view, rel_inf
import flow_bc_model as fm
import pointwise_model as pm

f32 = np.float32
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WALL_KW = dict(kappa=pm.WALL_PARAMS["kappa"], C_=pm.WALL_PARAMS["C"], A=pm.WALL_PARAMS["A"], beta=pm.WALL_PARAMS["beta"],
               betastar=pm.WALL_PARAMS["betastar"], D=pm.WALL_PARAMS["D"], Aplus=pm.WALL_PARAMS["Aplus"],
               omega_fixed_point=pm.WALL_PARAMS["omega"], n_iter=7)
# name -> (FlowBC state, normal_flow, wall_function keywords or None, transpiration, scalar specs); 0 .. 4 scalars, every mode
SPECS = {
    "far_dirichlet": (None, False, None, 0.0, ()),
    "far_dirichlet_2_scalars": (None, False, None, 0.0, (4.5e-5, "copy")),
    "slip_wall": ([1.0e5, 288.15, 0.0], True, None, 0.0, ("copy",)),
    "slip_wall_wall_function": ([1.0e5, 288.15, 0.0], True, {}, 0.0, ("nut", "k", "omega", "epsilon")),
    "slip_wall_wall_function_params_transpiration": ([1.0e5, 288.15, -2.0], True, WALL_KW, 0.75, (1.0e-4, "nut", "copy")),
}


def _bc(name, nd):
    from ibamd import cfd
    state, normal_flow, wf, transp, specs = SPECS[name]
    far = [1.0e5, 288.15, 100.0, 10.0, -5.0][:nd + 2] if state is None else state
    return cfd.FlowBC(cfd.Fluid(), far, normal_flow=normal_flow), wf, transp, specs


def _device_fields(F, nd, ns, pad=5):
    """P = [p T u v (w)] with a leading dimension larger than n, and ns scalar vectors, on the device."""
    import torch
    n = F.shape[0]
    buf = torch.zeros((nd + 2, n + pad), dtype=torch.float32, device="cuda")
    P = buf.T[:n]
    P.copy_(ibamd.hip(F[:, :nd + 2]))
    assert P.stride() == (1, n + pad)
    return P, [ibamd.hip(np.ascontiguousarray(F[:, nd + 2 + q])) for q in range(ns)]


def composed(dom, bname, bc, P, fields, specs, wf, transp):
    """The composition of the library's own launches that ``impose_flow_bc`` replaces."""
    from ibamd import cfd
    from ibamd import turbulence as T
    H = ibamd.HipArray
    nd = dom.ndims
    fluid = bc.fluid

    def closure(b, Pi, *si):
        kw, w = {}, None
        if wf is not None:
            p, Tm = H(Pi[:, 0]), H(Pi[:, 1])
            u = [H(Pi[:, 2 + j]) for j in range(nd)]
            nn = [H(b.normals[:, j]) for j in range(nd)]
            rho = H((p / (fluid.R * Tm)).t)
            nu = H((H(cfd.dynamic_viscosity(fluid, Pi[:, 1].contiguous())) / rho).t)
            un = u[0] * nn[0]
            for j in range(1, nd):
                un = un + u[j] * nn[j]
            un = H(un.t)
            t2 = None
            for j in range(nd):
                t = H((u[j] - un * nn[j]).t)
                t2 = t * t if t2 is None else t2 + t * t
            ut = H(t2.t).sqrt().t
            w = T.wall_function(b.image_distances, ut, nu.t, **wf)
            kw = dict(du_dn=w["du_dn"], image_distances=b.image_distances)
        ba = bc(Pi, b.normals, transpiration=transp, **kw)
        vals = [si[i] if s == "copy" else w[s] if isinstance(s, str) else s for i, s in enumerate(specs)]
        return (ba, *vals)
    ibamd.impose_bc(closure, dom, bname, P, *fields)


_boundaries = {}


def _synthetic(ng, nd, staged=False):
    key = (ng, nd, staged)
    if key not in _boundaries:
        b, F = fm.synthetic_boundary(ng, nd, staged=staged)
        _boundaries[key] = (fm.FakeDomain(nd, F.shape[0], {"bc": {1: b}}), b, F)
    return _boundaries[key]


def _direct(b):
    d = C.c_int32(-1)
    _lib.call("ibh_bc_flow_info", ibamd.to_backend(b).handle, C.byref(d))
    return d.value


def _both(dom, F, nd, name):
    """(fused, composed) results [P | scalars] on the host for one spec."""
    bc, wf, transp, specs = _bc(name, nd)
    out = []
    for fused in (True, False):
        P, fields = _device_fields(F, nd, len(specs))
        if fused:
            ibamd.impose_flow_bc(dom, "bc", bc, P, scalars=list(zip(fields, specs)), wall_function=wf, transpiration=transp)
        else:
            composed(dom, "bc", bc, P, fields, specs, wf, transp)
        out.append(np.concatenate([ibamd.to_host(P)] + [ibamd.to_host(f)[:, None] for f in fields], axis=1))
    return out


def _assert_bits(got, ref, F, b, what):
    if not np.array_equal(got, ref, equal_nan=True):
        bad = np.argwhere(~((got == ref) | (np.isnan(got) & np.isnan(ref))))
        rows = {int(r): int(np.nonzero(b.ghost_indices == r)[0][0]) if r in b.ghost_indices else None for r in bad[:8, 0]}
        pytest.fail(f"{what}: {bad.shape[0]} values differ from the composition; columns {sorted(set(bad[:, 1].tolist()))}, "
                    f"cell -> ghost row {rows}, first: fused {got[tuple(bad[0])]!r} composed {ref[tuple(bad[0])]!r}")
    ghosts = np.zeros(F.shape[0], bool)
    ghosts[b.ghost_indices] = True
    nc = got.shape[1]
    assert np.array_equal(got[~ghosts], F[~ghosts, :nc], equal_nan=True), f"{what}: a cell that is no ghost cell changed"
    assert not np.array_equal(got[ghosts], F[ghosts, :nc], equal_nan=True), f"{what}: no ghost cell changed"


@pytest.mark.parametrize("name", list(SPECS))
@pytest.mark.parametrize("nd", [2, 3])
@pytest.mark.parametrize("ng", [1, 255, 256, 257, 4099])
def test_bits_against_the_composition(ng, nd, name):
    dom, b, F = _synthetic(ng, nd)
    acc = b.image_interpolator
    if ng >= 255:   # what the family is for: rows of 0 .. 9 entries that start on and off 16-byte boundaries
        starts = acc.off[:-1][acc.lengths >= 4] % 4
        assert set(acc.lengths.tolist()) == set(range(10)) and (starts == 0).any() and (starts != 0).any()
    assert _direct(b) == 1
    got, ref = _both(dom, F, nd, name)
    _assert_bits(got, ref, F, b, f"{name}, nd = {nd}, ng = {ng}")
    if ng >= 16:    # the planted rows: ut = 0, zero velocity, un < 0, NaN temperature (which must reach the ghost cell)
        assert np.isnan(got[b.ghost_indices[9], 1]) and np.isfinite(got[b.ghost_indices[[3, 5, 7]], :nd + 2]).all()


def test_direct_and_staged():
    from ibamd import cfd
    nd, ng = 3, 300
    for staged in (False, True):
        dom, b, F = _synthetic(ng, nd, staged=staged)
        assert _direct(b) == (0 if staged else 1)
        for name in ("far_dirichlet_2_scalars", "slip_wall_wall_function"):
            got, ref = _both(dom, F, nd, name)
            _assert_bits(got, ref, F, b, f"{name}, staged = {staged}")
    # the staged boundary: a write in ghost order would let row g + 1 see ghost cell g already written -- another result.
    # Both from the tables on the host (Dirichlet far field, one copied scalar): the reference order reproduces the device
    # within the bound, the ghost order does not.
    dom, b, F = _synthetic(ng, nd, staged=True)
    far = [1.0e5, 288.15, 100.0, 10.0, -5.0]
    P, fields = _device_fields(F, nd, 1)
    ibamd.impose_flow_bc(dom, "bc", cfd.FlowBC(cfd.Fluid(), far), P, scalars=[(fields[0], "copy")])
    got = np.concatenate([ibamd.to_host(P), ibamd.to_host(fields[0])[:, None]], axis=1)
    keep = np.zeros(F.shape[0], bool)
    keep[b.ghost_indices] = True
    keep[b.ghost_indices[[9, 10]]] = False       # the NaN row and the row it feeds
    ref = fm.host_dirichlet(b, F[:, :nd + 3].copy(), nd, far, ghost_order=False)
    seq = fm.host_dirichlet(b, F[:, :nd + 3].copy(), nd, far, ghost_order=True)
    e_ref = max(float(rel_inf(got[keep, v], ref[keep, v])) for v in range(nd + 3))
    e_seq = max(float(rel_inf(got[keep, v], seq[keep, v])) for v in range(nd + 3))
    print(f"staged boundary: against the host in reference order {e_ref:.3g}, in ghost order {e_seq:.3g}")
    assert e_ref <= fm.TOL and e_seq > 100 * fm.TOL
    # the C entry refuses a staged boundary without a staging buffer, before any launch
    spec = _lib.ibh_flow_bc_spec(0, far[0], far[1], (C.c_float * 3)(*far[2:]), 0.0, 0, (C.c_float * 8)(), 0)
    fluid = cfd.Fluid()._c()
    db = ibamd.to_backend(b)
    with pytest.raises(_lib.IbhError, match="staging"):
        _lib.call("ibh_bc_flow", db.handle, C.byref(fluid), nd, C.c_void_p(db.normals.data_ptr()), ng,
                        C.c_void_p(db.image_distances.data_ptr()), C.c_void_p(P.data_ptr()), int(P.stride(1)),
                        C.byref(spec), 0, None, None, None, None)


def test_past_the_grid_cap():
    """Three ghost cells more than one pass of the capped grid covers: the grid-stride loop's second trip."""
    src = open(os.path.join(ROOT, "immersedboundary.jl_amd", "csrc", "ibh_bcflow.hip")).read()
    cap = int(re.search(r"BCF_GRID_CAP = (\d+);", src).group(1))
    wg = int(re.search(r"BCF_BLOCK = (\d+);", src).group(1))
    ng, nd = cap * wg + 3, 3
    b, F = fm.synthetic_boundary(ng, nd, extra_cells=1000)
    dom = fm.FakeDomain(nd, F.shape[0], {"bc": {1: b}})
    bc, wf = _bc("slip_wall_wall_function", nd)[:2]
    out = []
    for fused in (True, False):
        P, fields = _device_fields(F, nd, 1)
        if fused:
            ibamd.impose_flow_bc(dom, "bc", bc, P, scalars=[(fields[0], "nut")], wall_function=wf)
        else:
            composed(dom, "bc", bc, P, fields, ("nut",), wf, 0.0)
        out.append(np.concatenate([ibamd.to_host(P), ibamd.to_host(fields[0])[:, None]], axis=1))
    _assert_bits(out[0], out[1], F, b, f"ng = {ng}")


@pytest.fixture(scope="module")
def sphere_levels():
    """The sphere of test_config5.py at h = 0.4 with blocks of 4^3: 29 184 cells with 1 200 wall ghost cells, one coarse level."""
    import bench
    from ibamd.mesher import Mesh
    msh = Mesh(f32([-4, -4, -4]), f32([8, 8, 8]), ("sphere", bench.icosphere(subdiv=2), f32(0.4)), block_size=4)
    fam = [("farfield", [(d, sd) for d in (1, 2, 3) for sd in (False, True)])]
    dom = ibamd.Domain(msh, hypercube_families=fam, max_partition_size=10 ** 9)
    levels = [dom] + ibamd.multigrid(dom, max_levels=1)[0]
    assert len(levels) > 1 and sum(b.ghost_indices.size for b in dom.boundaries["sphere"].values()) >= 500
    return levels


def _seeded_Q(dom, seed):
    nd, n = dom.ndims, len(dom)
    Q = np.empty((n, nd + 3), f32)
    Q[:, :nd + 2] = fm.image_point_family(n, nd, seed=seed)[0]
    Q[:, nd + 2] = 4.5e-5 * (1 + 0.5 * np.random.default_rng(seed).uniform(0, 1, n))
    return Q


def _against_oracle(dom, view, wall_name, what):
    from ibamd.closures import config5_boundary_conditions
    nd = dom.ndims
    far, R_inf = fm.FAR3[:nd + 2], f32(4.5e-5)
    Q0 = _seeded_Q(dom, 3)
    Qo = Q0.copy()
    fm.oracle_config5_bcs(view, Qo, far, R_inf, wall_name)
    ghosts = np.zeros(len(dom), bool)
    for name in (wall_name, "farfield"):
        for b in dom.boundaries[name].values():
            ghosts[b.ghost_indices] = True
    errs = {}
    for fused in (True, False):
        Qg = ibamd.hip(Q0)
        config5_boundary_conditions(dom, Qg, far, wall_name=wall_name, R_inf=float(R_inf), fused=fused)
        got = ibamd.to_host(Qg)
        errs[fused] = {v: float(rel_inf(got[ghosts, v], Qo[ghosts, v])) for v in range(nd + 3)}
        if fused:
            assert np.array_equal(got[~ghosts], Q0[~ghosts]), f"{what}: a cell that is no ghost cell changed"
            changed = (got[ghosts] != Q0[ghosts]).any(axis=1)
            assert changed.all(), f"{what}: {int((~changed).sum())} ghost cells unchanged"
    print(f"{what}: {int(ghosts.sum())} ghost cells, rel_inf per variable [p T u.. R] against the oracle: fused {errs[True]}, "
          f"composed {errs[False]}")
    assert max(errs[True].values()) <= fm.TOL, errs[True]


def test_real_boundaries_against_the_oracle_2d(rae_domains):
    dp, do = rae_domains
    print("RAE2822 boundary partitions:", {k: len(v) for k, v in dp.boundaries.items()})
    _against_oracle(dp, do, "wall", "RAE2822")


def test_real_boundaries_against_the_oracle_3d(sphere_levels):
    for l, dom in enumerate(sphere_levels):
        _against_oracle(dom, oracle_boundaries_view(dom), "sphere", f"sphere level {l}")


def test_graph_replay_equals_eager(sphere_levels):
    from ibamd.closures import config5_boundary_conditions
    dom = sphere_levels[0]
    Q0 = _seeded_Q(dom, 4)

    def bcs(Q):
        config5_boundary_conditions(dom, Q, fm.FAR3, R_inf=4.5e-5, fused=True)
    Qe = ibamd.hip(Q0)
    bcs(Qe)
    bcs(Qe)
    Qg = ibamd.hip(Q0)
    g = ibamd.GraphedClosure(bcs, Qg)
    assert np.array_equal(ibamd.to_host(Qg), Q0)          # constructing it restores the state
    g()
    g()
    assert np.array_equal(ibamd.to_host(Qg), ibamd.to_host(Qe))
    assert not np.array_equal(ibamd.to_host(Qg), Q0)


def _no_launch(monkeypatch):
    from ibamd import backend as B

    def fail(name, *a):
        pytest.fail(f"{name} was called: the argument check did not stop the launch")
    monkeypatch.setattr(B, "call", fail)


def test_argument_checks_come_before_any_launch(monkeypatch):
    from ibamd import cfd
    nd = 3
    dom, b, F = _synthetic(255, nd)
    ibamd.to_backend(b)
    P, s = _device_fields(F, nd, 4)
    s5 = ibamd.hip(np.zeros(F.shape[0], f32))
    short = ibamd.hip(np.zeros(F.shape[0] - 1, f32))
    P4, Pshort = ibamd.hip(F[:, :nd + 1]), ibamd.hip(F[:-1, :nd + 2])
    wall = cfd.FlowBC(cfd.Fluid(), [1e5, 288.15, 0.0], normal_flow=True)
    far = cfd.FlowBC(cfd.Fluid(), [1e5, 288.15, 100.0, 0.0, 0.0])
    _no_launch(monkeypatch)
    bad = [
        dict(bc=wall, P=P, scalars=[(x, "copy") for x in s + [s5]]),                    # more than four scalars
        dict(bc=wall, P=P, scalars=[(s[0], "nut")]),                                    # a wall-function mode without it
        dict(bc=wall, P=P, scalars=[(s[0], "epsilon")], wall_function=None),
        dict(bc=wall, P=P, scalars=[(s[0], "nu_t")], wall_function={}),                 # an unknown mode
        dict(bc=wall, P=P, wall_function=dict(kapa=0.4)),                               # an unknown keyword
        dict(bc=cfd.FlowBC(cfd.Fluid(), [1e5, 288.15, 0.0, 1.0], normal_flow=True), P=P),   # normal_flow, two velocities
        dict(bc=cfd.FlowBC(cfd.Fluid(), [1e5, 288.15, 100.0, 0.0]), P=P),               # a 2-D state on a 3-D domain
        dict(bc=far, P=P4),                                                             # (n, nd + 1)
        dict(bc=far, P=Pshort),                                                         # a row short
        dict(bc=far, P=P, scalars=[(short, 1.0)]),
        dict(bc=far, P=P, scalars=[(P[:, :2], 1.0)]),                                   # a scalar field that is no vector
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            ibamd.impose_flow_bc(dom, "bc", **kw)
    with pytest.raises(ValueError):
        ibamd.impose_flow_bc(fm.FakeDomain(4, F.shape[0], dom.boundaries), "bc", far, P)   # nd = 4
    with pytest.raises(TypeError):
        ibamd.impose_flow_bc(dom, "bc", far, F[:, :nd + 2])                              # a host array: no CPU path

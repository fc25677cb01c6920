"""The explicit Euler step on the device -- ``timestep_euler``, ``update_euler``, ``step_euler``, ``EulerMarch`` -- bit for bit
against the compositions of the library's own launches that they replace, and against the float64 models of
tests/euler_step_model.py.  Meshes: the four of tests/test_gpu_percell_regimes.py (``adv``: every block in quads, pairs or
singles, the one-launch step; ``rae6k_2``: skirts and face-list cells; ``corner`` and ``sphere_1``: 3-D); states:
``regimes.euler_regime``.
"""

import numpy as np
import pytest
import torch

import euler_step_model as em
import ibamd
import percell_steps as ps
import regimes as rg
from conftest import ADV_FAMILIES
from ibamd import _lib, cfd
from ibamd import backend as B
from ibamd.hiparray import HipArray as H
from ibamd.solver import EulerMarch
from test_gpu_percell_regimes import MESHES, meshes  # noqa: F401  (the module-scoped fixture of the four meshes)

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
FLUID = cfd.Fluid()
SCALE = 0.75
DT_REGIMES = ("transonic", "crossing", "rest", "cold")
GENERAL, NO_FUSE, NO_QUAD = B.IBH_FORCE_GENERAL, B.IBH_NO_FUSE, B.IBH_NO_QUAD


def same_bits(got, ref, what=""):
    """Bit for bit where the reference is finite, the same NaN / Inf pattern elsewhere."""
    g, r = ibamd.to_host(got), ibamd.to_host(ref)
    assert g.shape == r.shape, (what, g.shape, r.shape)
    assert np.array_equal(np.isnan(g), np.isnan(r)), f"{what}: NaN pattern differs"
    fin = ~np.isnan(r)
    bad = g.view(np.uint32)[fin] != r.view(np.uint32)[fin]
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values differ, first at {np.argwhere(g.view(np.uint32) != r.view(np.uint32))[:3].tolist()}"


def padded(n, nv, pad=13, fill=None):
    """(n, nv) device array with leading dimension n + pad."""
    t = torch.empty((nv, n + pad), dtype=torch.float32, device="cuda")
    if fill is not None:
        t.fill_(fill)
    return t.T[:n]


# ---------------------------------------------------------------------------------------------------------------------
# time step
# ---------------------------------------------------------------------------------------------------------------------
def materialised_C(Pd):
    """C_d = abs.(u_d) .+ speed_of_sound(fluid, T) by the IEEE path: ibh_cfd_speed_of_sound, then HipArray abs and +."""
    n, nd = Pd.shape[0], Pd.shape[1] - 2
    a = cfd.speed_of_sound(FLUID, Pd[:, 1].contiguous())
    Cd = B.colmajor_empty(n, nd)
    for d in range(nd):
        Cd[:, d] = (abs(H(Pd[:, 2 + d].contiguous())) + H(a)).t
    return Cd


def composed_dt_cells(dpart, Cd, scale):
    per = None
    for d in range(Cd.shape[1]):
        g = ibamd.unsigned_green_gauss(dpart, ibamd.at_faces(dpart, Cd[:, d].contiguous(), d + 1), d + 1)
        per = g if per is None else H(per).maximum_with(H(g)).t
    return ((0.5 / H(per)) * scale).t


@pytest.mark.parametrize("regime", DT_REGIMES)
@pytest.mark.parametrize("mesh", MESHES)
def test_timestep_bit_for_bit_and_against_float64(meshes, mesh, regime):
    c = meshes[mesh]
    P = rg.euler_regime(c.part, regime)
    if regime == "cold":
        assert (P[:, 1] < 10).any()
    Pd = ibamd.hip(P)
    Cd = materialised_C(Pd)
    ref_dt = ibamd.timestep_advection(c.dpart, Cd, scale=SCALE)
    cells = B.colmajor_empty(P.shape[0])
    cells.fill_(float("nan"))
    dt = ibamd.timestep_euler(c.dpart, Pd, FLUID, SCALE, cells=cells)
    same_bits(dt, ref_dt, f"{mesh} {regime} dt")
    same_bits(cells, composed_dt_cells(c.dpart, Cd, SCALE), f"{mesh} {regime} dt_cells")
    assert float(dt.item()) == float(ibamd.to_host(cells).min())
    # each output alone: the same values (dt_cells alone is one launch)
    same_bits(ibamd.timestep_euler(c.dpart, Pd, FLUID, SCALE), ref_dt, "dt alone")
    only = torch.full_like(cells, float("nan"))
    assert ibamd.timestep_euler(c.dpart, Pd, FLUID, SCALE, out=False, cells=only) is only
    same_bits(only, cells, "dt_cells alone")
    # padded leading dimension
    Pp = padded(P.shape[0], P.shape[1])
    Pp.copy_(Pd)
    same_bits(ibamd.timestep_euler(c.dpart, Pp, FLUID, SCALE), ref_dt, "padded P")
    # float64 model, at the bound the advection time step is held to
    ref64, _ = em.timestep(c.op, P, SCALE, f64)
    err = ps.check_dt(dt.item(), ref64, f"{mesh} {regime}")
    print(f"timestep_euler {mesh} {regime}: dt {dt.item():.6e}, {err / ps.ULP:.2f} ulp from float64")


# ---------------------------------------------------------------------------------------------------------------------
# update
# ---------------------------------------------------------------------------------------------------------------------
def composed_update(Pd, Rd, dtd):
    """primitive2state -> Q + dt R per column (ibh_update_dev; a per-cell dt by the IEEE broadcasts * and +) ->
    state2primitive"""
    n, nv = Pd.shape
    Q = cfd.primitive2state(FLUID, Pd)
    Q2 = B.colmajor_empty(n, nv)
    for v in range(nv):
        if dtd.numel() == 1:
            B._stream()
            _lib.call("ibh_update_dev", n, B._ptr(dtd), B._ptr(Q[:, v]), B._ptr(Rd[:, v].contiguous()), B._ptr(Q2[:, v]))
        else:
            t = (H(Rd[:, v].contiguous()) * H(dtd)).t
            Q2[:, v] = (H(Q[:, v].contiguous()) + H(t)).t
    return cfd.state2primitive(FLUID, Q2)


_rows = {}


def rows(n, nd, per_cell):
    if (n, nd, per_cell) not in _rows:
        P, R, dt = em.synthetic_rows(n, nd, per_cell=per_cell)
        dtd = ibamd.hip(dt) if per_cell else torch.tensor([float(dt)], dtype=torch.float32, device="cuda")
        Pd, Rd = ibamd.hip(P), ibamd.hip(R)
        _rows[n, nd, per_cell] = (P, R, dt, Pd, Rd, dtd, composed_update(Pd, Rd, dtd))
    return _rows[n, nd, per_cell]


@pytest.mark.parametrize("per_cell", [False, True], ids=["global_dt", "per_cell_dt"])
@pytest.mark.parametrize("nd", [2, 3])
@pytest.mark.parametrize("n", [1, 77, 2048 * 256 + 77])
def test_update_bit_for_bit(n, nd, per_cell):
    """One row, less than a workgroup, and past the grid cap of 2 048 workgroups of 256 (the grid-stride loop)."""
    P, R, dt, Pd, Rd, dtd, ref = rows(n, nd, per_cell)
    out = B.colmajor_empty(n, nd + 2)
    out.fill_(float("nan"))
    assert ibamd.update_euler(Pd, Rd, dtd, FLUID, out=out) is out
    same_bits(out, ref, "out of place")
    assert np.isfinite(ibamd.to_host(out)).all()
    same_bits(ibamd.update_euler(Pd, Rd, dtd, FLUID), ref, "allocated")
    inplace = Pd.clone()
    ibamd.update_euler(inplace, Rd, dtd, FLUID, out=inplace)
    same_bits(inplace, ref, "in place")
    base = torch.full((nd + 2, n + 29), float("nan"), dtype=torch.float32, device="cuda")
    Pp, Rp, Op = padded(n, nd + 2, 13), padded(n, nd + 2, 5), base.T[:n]
    Pp.copy_(Pd)
    Rp.copy_(Rd)
    ibamd.update_euler(Pp, Rp, dtd, FLUID, out=Op)
    same_bits(Op, ref, "padded")
    assert torch.isnan(base[:, n:]).all()                                       # nothing written past row n


@pytest.mark.parametrize("nd", [2, 3])
def test_update_nan_and_vacuum_rows(nd):
    """A NaN row and rows with rho -> 0 (p = 0; dt R_rho = -rho): the NaN / Inf pattern of the composition."""
    P, R, dt = em.synthetic_rows(300, nd)
    P[7] = np.nan
    P[11, 1] = np.nan
    P[19, 0] = 0.0
    R[19] = 0.0
    R[23, 0] = np.nan
    rho = P[31, 0] / (f32(283.0) * P[31, 1])
    R[31, 0] = -rho / dt
    P[40, 0] = 0.0
    Pd, Rd = ibamd.hip(P), ibamd.hip(R)
    dtd = torch.tensor([float(dt)], dtype=torch.float32, device="cuda")
    ref = composed_update(Pd, Rd, dtd)
    got = ibamd.update_euler(Pd, Rd, dtd, FLUID)
    same_bits(got, ref, "special rows")
    g, r = ibamd.to_host(got), ibamd.to_host(ref)
    assert np.array_equal(np.isinf(g), np.isinf(r)) and np.array_equal(np.signbit(g)[np.isinf(r)], np.signbit(r)[np.isinf(r)])
    assert np.isnan(g[7]).all() and not np.isfinite(g[19]).all()
    ok = np.setdiff1d(np.arange(300), [7, 11, 19, 23, 31, 40])
    assert np.isfinite(g[ok]).all()


@pytest.mark.parametrize("per_cell", [False, True], ids=["global_dt", "per_cell_dt"])
@pytest.mark.parametrize("nd", [2, 3])
def test_update_against_float64(nd, per_cell):
    """Per element against the float64 model: 4 x the Float32 model's own deviation (euler_step_model.MODEL_DEVIATION_EPS,
    measured in tests/test_euler_step_model.py) -- the margin for rounding order inside a sum."""
    P, R, dt, Pd, Rd, dtd, _ = rows(20000, nd, per_cell)
    got = ibamd.to_host(ibamd.update_euler(Pd, Rd, dtd, FLUID))
    dev = em.update_deviation(got, P, R, dt)
    model = em.update_deviation(em.update(P, R, dt, f32), P, R, dt)
    print(f"update_euler nd={nd} per_cell={per_cell}: device {dev:.3f} eps, Float32 model {model:.3f} eps, "
          f"bound {4 * em.MODEL_DEVIATION_EPS[nd]:.1f} eps")
    assert dev <= 4 * em.MODEL_DEVIATION_EPS[nd]


def test_python_layer_rejects_misuse(meshes):
    c = meshes["corner"]
    Pd = ibamd.hip(rg.euler_regime(c.part, "rest"))
    dt = torch.ones(1, dtype=torch.float32, device="cuda")
    out = torch.empty_like(Pd.T).T
    with pytest.raises(_lib.IbhError, match="work must be"):
        ibamd.step_euler(c.dpart, Pd, dt, out)                                   # 3-D: two launches, needs work
    with pytest.raises(_lib.IbhError, match="may not alias"):
        ibamd.update_euler(Pd, out, dt, out=out)
    with pytest.raises(_lib.IbhError, match="IBH_IMAGE_ONLY"):
        ibamd.step_euler(c.dpart, Pd, dt, out, work=torch.empty_like(out.T).T, flags=B.IBH_IMAGE_ONLY)
    with pytest.raises(TypeError):
        ibamd.update_euler(Pd, out, 1e-3)                                        # a host dt
    with pytest.raises(ValueError):
        ibamd.update_euler(Pd, out, torch.ones(3, dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError):
        ibamd.step_euler(c.dpart, Pd, dt, out, scheme="roe")
    with pytest.raises(TypeError):
        ibamd.step_euler(c.dpart, Pd, dt, torch.empty((Pd.shape[0], Pd.shape[1]), dtype=torch.float32, device="cuda"))
    # a work that aliases P or out is rejected on the one-launch path too, where it would not be used: nothing is launched
    a = meshes["adv"]
    Pa = ibamd.hip(rg.euler_regime(a.part, "rest"))
    oa = B.colmajor_empty(*Pa.shape)
    oa.fill_(float("nan"))
    for work in (Pa, oa):
        with pytest.raises(_lib.IbhError, match="work may not alias"):
            ibamd.step_euler(a.dpart, Pa, dt, oa, FLUID, "hll", work=work, flags=0)
        assert torch.isnan(oa).all()


# ---------------------------------------------------------------------------------------------------------------------
# step
# ---------------------------------------------------------------------------------------------------------------------
def residual(dpart, Pd, scheme, flags):
    fn = ibamd.residual_euler_hll if scheme == "hll" else ibamd.residual_euler_sensor
    return fn(dpart, Pd, flags=flags, fluid=FLUID)


STEP_CASES = [("adv", 0), ("adv", NO_QUAD), ("adv", GENERAL), ("adv", NO_FUSE), ("rae6k_2", 0), ("rae6k_2", GENERAL),
              ("rae6k_2", NO_FUSE), ("corner", 0), ("corner", GENERAL), ("corner", NO_FUSE), ("sphere_1", 0),
              ("sphere_1", GENERAL), ("sphere_1", NO_FUSE)]
ONE_LAUNCH = {("adv", 0), ("adv", NO_QUAD)}


@pytest.mark.parametrize("scheme", ["hll", "sensor"])
@pytest.mark.parametrize("mesh,flags", STEP_CASES, ids=[f"{m}-{f}" for m, f in STEP_CASES])
def test_step_bit_for_bit(meshes, mesh, flags, scheme):
    c = meshes[mesh]
    n, nv = c.part.spacing.shape[0], c.nd + 2
    for regime in ("transonic", "cold"):
        Pd = ibamd.hip(rg.euler_regime(c.part, regime))
        dt = ibamd.timestep_euler(c.dpart, Pd, FLUID, SCALE)
        R = residual(c.dpart, Pd, scheme, flags)
        ref = ibamd.update_euler(Pd, R, dt, FLUID)
        what = f"{mesh} flags={flags} {scheme} {regime}"
        work, out = B.colmajor_empty(n, nv), B.colmajor_empty(n, nv)
        work.fill_(float("nan"))                                 # a row the sweep or the update leaves unwritten shows
        out.fill_(float("nan"))
        ibamd.step_euler(c.dpart, Pd, dt, out, FLUID, scheme, work=work, flags=flags)
        same_bits(out, ref, what)
        finite_R = np.isfinite(ibamd.to_host(R)).all(axis=1)
        assert finite_R.any() and np.isfinite(ibamd.to_host(out)[finite_R]).all(), what
        if (mesh, flags) in ONE_LAUNCH:                          # the sweep stores the update itself: no work array
            out.fill_(float("nan"))
            ibamd.step_euler(c.dpart, Pd, dt, out, FLUID, scheme, flags=flags)
            same_bits(out, ref, what + " without work")
            po = padded(n, nv, 19, fill=float("nan"))
            ibamd.step_euler(c.dpart, Pd, dt, po, FLUID, scheme, flags=flags)
            same_bits(po, ref, what + " padded out")
        else:
            with pytest.raises(_lib.IbhError, match="work must be"):
                ibamd.step_euler(c.dpart, Pd, dt, out, FLUID, scheme, flags=flags)
        if regime == "transonic":
            # in place (two launches everywhere), and a per-cell time step
            inplace = Pd.clone()
            ibamd.step_euler(c.dpart, inplace, dt, inplace, FLUID, scheme, work=work, flags=flags)
            same_bits(inplace, ref, what + " in place")
            cells = ibamd.timestep_euler(c.dpart, Pd, FLUID, SCALE, out=False, cells=B.colmajor_empty(n))
            out.fill_(float("nan"))
            ibamd.step_euler(c.dpart, Pd, cells, out, FLUID, scheme, work=work, flags=flags)
            same_bits(out, ibamd.update_euler(Pd, R, cells, FLUID), what + " per-cell dt")


# ---------------------------------------------------------------------------------------------------------------------
# march
# ---------------------------------------------------------------------------------------------------------------------
NSTEPS = 20
TAU = f32(1e-3)


@pytest.fixture(scope="module")
def march_dom(adv_mesh):
    dom = ibamd.Domain(adv_mesh, hypercube_families=ADV_FAMILIES, max_partition_size=10 ** 9)
    (part,) = dom.partitions.values()
    far = cfd.FlowBC(FLUID, [1e5, 288.15, 340.0, -340.0])
    wall = cfd.FlowBC(FLUID, [1e5, 288.15, 0.0], normal_flow=True)

    def bcs(P):
        ibamd.impose_flow_bc(dom, "outlet", far, P)
        for name in ("lower", "upper"):
            ibamd.impose_flow_bc(dom, name, wall, P)
    return dom, part, ibamd.to_backend(part, ibamd.hip), bcs


def composed_march(dpart, P0, scheme, bcs, avg):
    P = P0
    for _ in range(NSTEPS):
        dt = ibamd.timestep_advection(dpart, materialised_C(P), scale=SCALE)
        P = composed_update(P, residual(dpart, P, scheme, 0), dt)
        bcs(P)
        avg.push(P, dt)
    return P


@pytest.mark.parametrize("scheme", ["hll", "sensor"])
def test_march(march_dom, scheme):
    dom, part, dpart, bcs = march_dom
    assert dpart.info["fusable_blocks"] == dpart.info["full_blocks"] > 0 and dpart.info["irregular_cells"] == 0
    assert sum(b.ghost_indices.size for name in ("outlet", "lower", "upper") for b in dom.boundaries[name].values()) > 0
    P0 = ibamd.hip(rg.euler_regime(part, "transonic"))
    start = P0.clone()
    avg_ref = cfd.TimeAverage(TAU)
    ref = composed_march(dpart, P0, scheme, bcs, avg_ref)
    assert np.isfinite(ibamd.to_host(ref)).all()

    avg = cfd.TimeAverage(TAU)
    m = EulerMarch(dpart, FLUID, scheme=scheme, scale=SCALE, bcs=bcs, average=avg)
    P = P0
    for _ in range(NSTEPS):
        P = m.step(P)
    same_bits(P, ref, f"march {scheme}")
    same_bits(avg.mu, avg_ref.mu, "mean")
    same_bits(avg.sigma, avg_ref.sigma, "sigma")
    same_bits(P0, start, "the initial array is left alone")

    # the same steps captured once and replayed: no host read-back, no allocation in a step
    g_m = EulerMarch(dpart, FLUID, scheme=scheme, scale=SCALE, bcs=bcs)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        Pw = g_m.step(g_m.step(P0))                      # warm-up: workspaces are allocated on first use
        stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            Pg = P0
            for _ in range(NSTEPS):
                Pg = g_m.step(Pg)
        Pg.fill_(float("nan"))
        graph.replay()
    stream.synchronize()
    B._stream()
    same_bits(Pg, ref, f"march {scheme}, graph replay")
    del Pw


def test_march_forms(march_dom):
    """``residual=`` (a callable followed by update_euler), ``dt_every`` and ``local_dt`` against their compositions."""
    dom, part, dpart, bcs = march_dom
    P0 = ibamd.hip(rg.euler_regime(part, "transonic"))
    m = EulerMarch(dpart, FLUID, scale=SCALE, residual=lambda p, P, out: ibamd.residual_euler_hll(p, P, out=out, fluid=FLUID))
    plain = EulerMarch(dpart, FLUID, scale=SCALE)
    same_bits(m.step(m.step(P0)), plain.step(plain.step(P0)), "residual=")
    every = EulerMarch(dpart, FLUID, scale=SCALE, dt_every=2)
    dt0 = ibamd.timestep_euler(dpart, P0, FLUID, SCALE)
    P1 = ibamd.update_euler(P0, residual(dpart, P0, "hll", 0), dt0, FLUID)
    P2 = ibamd.update_euler(P1, residual(dpart, P1, "hll", 0), dt0, FLUID)
    same_bits(every.step(every.step(P0)), P2, "dt_every=2 keeps the time step for two steps")
    local = EulerMarch(dpart, FLUID, scale=SCALE, local_dt=True)
    cells = ibamd.timestep_euler(dpart, P0, FLUID, SCALE, out=False, cells=B.colmajor_empty(P0.shape[0]))
    same_bits(local.step(P0), ibamd.update_euler(P0, residual(dpart, P0, "hll", 0), cells, FLUID), "local_dt")
    with pytest.raises(ValueError):
        EulerMarch(dpart, FLUID, local_dt=True, average=cfd.TimeAverage(TAU))

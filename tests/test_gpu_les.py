"""``les_closure_of`` / ``ibh_les_of`` -- the LES eddy viscosity (Smagorinsky, WALE), the Ducros and shock sensors, the shear
rate and the velocity gradients of a velocity field in ONE launch -- and ``navier_stokes_les_residual`` on the device.

Every output is held to the device composition (``cell_gradient`` per component, then ``shear_rate``,
``Smagorinsky_nuSGS``, ``WALE_nuSGS``, ``Ducros_sensor``, ``shock_sensor``) bit for bit: on 3-D partitions of complete 8^3
blocks (wave per block), on face-list partitions in 2-D and 3-D (thread per cell), with every single output requested alone
(a NULL pointer for each of the others), on a view into a wider state and a padded gradient buffer, with a NaN velocity,
past the grid cap, and replayed from a graph.  The composition's own kernels answer to the oracle in
tests/test_gpu_pointwise.py and tests/test_gpu_percell_closures.py; here the fused form also answers to known answers that
come from neither: linear velocity fields against the table answers of tests/les_model.py, with bounds from the Float32
oracle's own deviation (tests/test_les_model.py prints them).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import closure_cases as cc
import ibamd
import les_model as lm
import percell as pc
from closure_cases import same
from conftest import euler_field, oracle_view
from ibamd import _lib, cfd, closures
from ibamd import backend as B
from ibamd import turbulence as T

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
MEASURED = {}


@pytest.fixture(scope="module", autouse=True)
def _print_measured():
    yield
    if MEASURED:
        print("\nles_closure_of on linear fields, device maxima against the table answers (mesh, output): measured / bound")
        for k in sorted(MEASURED):
            print(f"  {k[0]} | {k[1]}: {MEASURED[k][0]:.3e} / {MEASURED[k][1]:.3e}")


class Case(cc.Case):
    def __init__(self, part):
        super().__init__(part)
        self.Delta_h = lm.filter_width(part)
        self.Delta = ibamd.hip(self.Delta_h)


@pytest.fixture(scope="module")
def cases():
    return cc.make_cases(Case)


def composition(dpart, vel, Delta):
    """The device composition: every output of the closure from ``cell_gradient`` and the pointwise kernels."""
    nd = vel.shape[1]
    g = [list(ibamd.cell_gradient(dpart, vel[:, i].contiguous())) for i in range(nd)]
    S = T.shear_rate(g)
    out = dict(S=S, ducros=T.Ducros_sensor(g), shock=cfd.shock_sensor(g), smagorinsky=T.Smagorinsky_nuSGS(Delta, S, Cs=0.17),
               g=g)
    if nd == 3:
        out["wale"] = T.WALE_nuSGS(Delta, g, Cw=0.325)
    return out


def assert_is_the_composition(c, vel, what=""):
    """Both models with every output together, and every output alone."""
    comp = composition(c.dpart, vel, c.Delta)
    nd = c.nd
    assert float(torch.nan_to_num(comp["S"]).abs().max()) > 0

    def check(got, keys, model, tag):
        assert set(got) == set(keys), (what, tag, sorted(got))
        for k in keys:
            if k == "gradients":
                assert len(got[k]) == nd
                for j in range(nd):
                    assert got[k][j].shape == (c.nc, nd)
                    for i in range(nd):
                        assert same(got[k][j][:, i], comp["g"][i][j]), (what, tag, "gradient", i, j)
            else:
                assert got[k].shape == (c.nc,)
                assert same(got[k], comp[model if k == "nusgs" else k]), (what, tag, k)

    models = ["smagorinsky"] + (["wale"] if nd == 3 else [])
    for model in models:
        got = T.les_closure_of(c.dpart, vel, c.Delta, model=model, ducros=True, shock=True, shear=True, gradients=True)
        check(got, ("nusgs", "ducros", "shock", "S", "gradients"), model, f"{model}: all")
        check(T.les_closure_of(c.dpart, vel, c.Delta, model=model), ("nusgs",), model, f"{model}: nusgs alone")
    check(T.les_closure_of(c.dpart, vel, ducros=True), ("ducros",), None, "ducros alone")
    check(T.les_closure_of(c.dpart, vel, shock=True), ("shock",), None, "shock alone")
    check(T.les_closure_of(c.dpart, vel, shear=True), ("S",), None, "S alone")
    check(T.les_closure_of(c.dpart, vel, gradients=True), ("gradients",), None, "gradients alone")
    check(T.les_closure_of(c.dpart, vel, ducros=True, shock=True, shear=True, gradients=True),
          ("ducros", "shock", "S", "gradients"), None, "no model: all")
    return comp


# ---------------------------------------------------------------------------------------------------------------------
# (a), (b), (c): the composition, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", ["octree", "single"])
def test_all_block_partitions_are_the_composition(cases, mesh):
    """Wave per 8^3 block (``k_les_of3``): the octree has SAME, MIRROR, COARSE and FINE sides and a block count that is no
    multiple of the four waves of a workgroup; the single block has six mirror sides."""
    c = cases[mesh]
    cc.assert_block_case(c, mesh)
    assert_is_the_composition(c, ibamd.hip(c.wavy()), mesh)


@pytest.mark.parametrize("nd", [2, 3])
def test_face_list_partitions_are_the_composition(cases, nd):
    """Thread per cell over the side table (``k_les_of_cells``), 2:1 interfaces; WALE is 3-D only."""
    c = cases[f"bs4 {nd}d"]
    vel = ibamd.hip(c.wavy(33))
    assert_is_the_composition(c, vel, f"bs4 {nd}d")
    if nd == 2:
        with pytest.raises(ValueError, match="WALE model only implemented for 3D"):
            T.les_closure_of(c.dpart, vel, c.Delta, model="wale")


def test_misuse_raises_value_error(cases):
    c = cases["bs4 3d"]
    vel = ibamd.hip(c.wavy())
    for kw, args in ((dict(), ()), (dict(model="dynamic"), (c.Delta,)), (dict(model="wale"), ()),
                     (dict(model="smagorinsky"), (c.Delta[:-1].contiguous(),))):
        with pytest.raises(ValueError):
            T.les_closure_of(c.dpart, vel, *args, **kw)
    with pytest.raises(ValueError):
        T.les_closure_of(c.dpart, vel[:, :2], shear=True)


def test_partition_with_skirt_fragments_composes():
    """Two partitions of the octree: blocks and skirt fragments, not all-block.  The wrapper composes; the C entry says so."""
    c = cc.skirt_case(Case)
    vel = ibamd.hip(c.wavy())
    assert_is_the_composition(c, vel, "two partitions")
    S = B.colmajor_empty(c.nc)
    B._stream()
    lib = _lib.load()
    rc = lib.ibh_les_of(c.dpart.handle, B._ptr(vel), c.nc, None, 0, 0.0, None, None, None, B._ptr(S), None, 0)
    assert rc != 0 and b"compose" in lib.ibh_last_error(), lib.ibh_last_error()


@pytest.mark.parametrize("field", ["wavy", "nan", "view"])
@pytest.mark.parametrize("mesh", ["octree", "single", "bs4 2d", "bs4 3d"])
def test_shear_rate_of_velocity_is_the_closure_without_a_model(cases, mesh, field):
    """``shear_rate_of_velocity(part, vel[, gradients=True])`` is ``les_closure_of(part, vel, shear=True[, gradients=True])``
    bit for bit with the same NaN pattern -- a cross-check: the first has kernels of its own (``k_shear_of_velocity3``,
    ``k_shear_of_velocity_cells``) over the helpers of ``k_les_of3<MODEL_NONE>`` / ``k_les_of_cells``.  ``"view"``: the
    velocity is ``P[:, 2:2 + nd]`` of a wider state and both C entries write ``G`` into a buffer with ``ldg > nc``."""
    c = cases[mesh]
    nd, nc = c.nd, c.nc
    v = c.wavy(12)
    if field == "nan":
        v[nc // 3, nd - 1] = np.nan
    P = ibamd.hip(np.concatenate([np.full((nc, 2), 1.5, f32), v, np.full((nc, 1), -2.5, f32)], axis=1))
    P0 = P.clone()
    vel = P[:, 2:2 + nd] if field == "view" else ibamd.hip(v)
    S = T.shear_rate_of_velocity(c.dpart, vel)
    S2, G = T.shear_rate_of_velocity(c.dpart, vel, gradients=True)
    les = T.les_closure_of(c.dpart, vel, shear=True, gradients=True)
    assert same(S, les["S"]) and same(S2, les["S"]) and same(T.les_closure_of(c.dpart, vel, shear=True)["S"], S)
    n_nan = int(torch.isnan(S).sum())
    assert (0 < n_nan < nc) if field == "nan" else n_nan == 0
    assert float(torch.nan_to_num(S).abs().max()) > 0 and len(G) == len(les["gradients"]) == nd
    for j in range(nd):
        assert G[j].shape == (nc, nd) and same(G[j], les["gradients"][j]), j
    if field != "view":
        return
    vp, _, ldv = B._field(vel, nc)
    assert vp.data_ptr() == P.data_ptr() + 8 * nc and ldv == nc     # no copy was made
    ldg = nc + 19
    pad = torch.full((2, nd * nd + 2, ldg), -7.25, dtype=torch.float32, device=P.device)    # row r = column r of a parent
    out = [B.colmajor_empty(nc), B.colmajor_empty(nc)]
    B._stream()
    B.call("ibh_shear_rate_of_velocity_grad", c.dpart.handle, B._ptr(vp), ldv, B._ptr(out[0]), C.c_void_p(pad[0, 1].data_ptr()), ldg)
    B.call("ibh_les_of", c.dpart.handle, B._ptr(vp), ldv, None, 0, C.c_float(0.0), None, None, None, B._ptr(out[1]),
           C.c_void_p(pad[1, 1].data_ptr()), ldg)
    assert torch.equal(P, P0) and same(out[0], S) and same(out[1], S) and torch.equal(pad[0], pad[1])
    assert bool((pad[:, 0] == -7.25).all() and (pad[:, -1] == -7.25).all() and (pad[:, :, nc:] == -7.25).all())
    for j in range(nd):
        assert same(pad[0, 1 + nd * j:1 + nd * (j + 1), :nc].T, G[j]), j


# ---------------------------------------------------------------------------------------------------------------------
# (d): linear velocity fields against the table answers
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", ["octree", "bs4 2d", "bs4 3d"])
def test_linear_fields_give_the_table_answers(cases, mesh):
    """u = A x for a shear, a dilatation and a rotation, on the cells whose 2-ring is same-level with no mirror face: every
    output within 4 x the Float32 oracle composition's own deviation from the table answers on this mesh
    (``les_model.bounds``: per output, the maximum over the three fields and the selected cells).  The single 8^3 block is
    left to the bit-for-bit test: this mask keeps 64 of its 512 cells."""
    c = cases[mesh]
    sel = lm.interior(c.part)
    assert 2 * sel.sum() >= sel.size                              # the mask cannot hide the kernel
    bound, _ = lm.bounds(mesh, c.part, oracle_view(c.part))
    worst = {}
    for name, make in lm.FIELDS:
        A = make(c.nd)
        vel = ibamd.hip(lm.linear_field(c.part, A))
        ans = lm.answers(A, c.Delta_h)
        got = T.les_closure_of(c.dpart, vel, c.Delta, model="smagorinsky", Cs=float(lm.CS), ducros=True, shock=True, shear=True)
        out = dict(S=got["S"], ducros=got["ducros"], shock=got["shock"], smagorinsky=got["nusgs"])
        if c.nd == 3:
            out["wale"] = T.les_closure_of(c.dpart, vel, c.Delta, model="wale", Cw=float(lm.CW))["nusgs"]
        for k, v in out.items():
            e = float(np.abs(ibamd.to_host(v).astype(f64) - ans[k])[sel].max())
            worst[k] = max(worst.get(k, 0.0), e)
    for k in sorted(worst):
        MEASURED[mesh, k] = (worst[k], bound[k])
        print(f"{mesh} | {k}: device {worst[k]:.3e}, bound {bound[k]:.3e}")
    for k in sorted(worst):
        assert worst[k] <= bound[k], (mesh, k, worst[k], bound[k])


# ---------------------------------------------------------------------------------------------------------------------
# (e), (f), (g), (i)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", ["octree", "bs4 2d"])
def test_state_view_and_padded_gradient_buffer(cases, mesh):
    """``vel = P[:, 2:]`` read in place, ``G`` inside a wider buffer with ``ldg > nc``: the written columns are the
    composition's, everything else in both parents keeps its bits."""
    c = cases[mesh]
    nd, nc = c.nd, c.nc
    rng = np.random.default_rng(5)
    P = ibamd.hip(np.concatenate([rng.uniform(1, 2, (nc, 2)).astype(f32), c.wavy(9)], axis=1))
    P0 = P.clone()
    vel = P[:, 2:]
    comp = composition(c.dpart, vel, c.Delta)
    v, nv, ldv = B._field(vel, nc)
    assert v.data_ptr() == P.data_ptr() + 8 * nc and ldv == nc     # no copy was made
    got = T.les_closure_of(c.dpart, vel, c.Delta, model="smagorinsky", shear=True)
    assert torch.equal(got["S"], comp["S"]) and torch.equal(got["nusgs"], comp["smagorinsky"])
    ldg = nc + 37
    pad = torch.full((nd * nd + 2, ldg), -7.25, dtype=torch.float32, device=P.device)    # row r = column r of the parent
    pad0 = pad.clone()
    duc = B.colmajor_empty(nc)
    B._stream()
    B.call("ibh_les_of", c.dpart.handle, B._ptr(v), ldv, None, 0, C.c_float(0.0), None, B._ptr(duc), None, None,
           C.c_void_p(pad.data_ptr() + 4 * ldg), ldg)
    assert torch.equal(P, P0)
    assert torch.equal(duc, comp["ducros"])
    assert torch.equal(pad[0], pad0[0]) and torch.equal(pad[-1], pad0[-1]) and torch.equal(pad[:, nc:], pad0[:, nc:])
    for j in range(nd):
        for i in range(nd):
            assert torch.equal(pad[1 + nd * j + i, :nc], comp["g"][i][j]), (i, j)


@pytest.mark.parametrize("mesh", ["octree", "bs4 2d", "bs4 3d"])
def test_nan_velocity_has_the_compositions_pattern(cases, mesh):
    c = cases[mesh]
    v = c.wavy(4)
    v[c.nc // 2, 0] = np.nan
    comp = assert_is_the_composition(c, ibamd.hip(v), f"{mesh} NaN")
    n_nan = int(torch.isnan(comp["S"]).sum())
    assert 0 < n_nan <= 1 + 2 * c.nd * 2 ** (c.nd - 1)             # the cell and its face neighbours


def test_past_the_grid_cap():
    """A face-list partition of just over 4096 * 256 cells: the launch is capped at 4096 workgroups, so some threads take a
    second cell (``k_jst3`` and ``k_shock`` once had no loop: their last elements were never written)."""
    c = cc.grid_cap_case(Case)
    vel = ibamd.hip(c.wavy(2))
    comp = composition(c.dpart, vel, c.Delta)
    got = T.les_closure_of(c.dpart, vel, ducros=True, shear=True)
    assert torch.equal(got["S"], comp["S"]) and torch.equal(got["ducros"], comp["ducros"])
    assert float(got["S"][-1]) == float(comp["S"][-1]) != 0.0 and float(got["ducros"][-1]) == float(comp["ducros"][-1])


@pytest.mark.parametrize("mesh", ["octree", "bs4 2d"])
def test_graph_replay(cases, mesh):
    c = cases[mesh]
    vel = ibamd.hip(c.wavy(1))
    kw = dict(model="wale" if c.nd == 3 else "smagorinsky", ducros=True, shock=True, shear=True, gradients=True)
    g = ibamd.GraphedClosure(lambda p, v, D: T.les_closure_of(p, v, D, **kw), c.dpart, vel, c.Delta)
    vel.copy_(ibamd.hip(c.wavy(77)))
    out = g()
    torch.cuda.synchronize()
    eager = T.les_closure_of(c.dpart, vel, c.Delta, **kw)
    for k in ("nusgs", "ducros", "shock", "S"):
        assert torch.equal(out[k], eager[k]), k
    for j in range(c.nd):
        assert torch.equal(out["gradients"][j], eager["gradients"][j]), j
    first = T.les_closure_of(c.dpart, ibamd.hip(c.wavy(1)), c.Delta, **kw)
    assert not torch.equal(first["S"], eager["S"])                # the replay saw the new input


# ---------------------------------------------------------------------------------------------------------------------
# (h): the closure that uses it
# ---------------------------------------------------------------------------------------------------------------------
def _operator_form(dpart, P, Delta, fluid, model, euler_flags):
    """``navier_stokes_les_residual`` operator by operator: nothing fused but (with ``euler_flags`` 0) the Euler sweep."""
    from ibamd.hiparray import HipArray
    nd = dpart.nd
    r = ibamd.residual_euler_sensor(dpart, P, fluid=fluid, flags=euler_flags)
    g = [list(ibamd.cell_gradient(dpart, P[:, 2 + i].contiguous())) for i in range(nd)]
    nusgs = T.WALE_nuSGS(Delta, g) if model == "wale" else T.Smagorinsky_nuSGS(Delta, T.shear_rate(g))
    mut = (HipArray(P[:, 0]) / (HipArray(P[:, 1]) * fluid.R) * HipArray(nusgs)).t
    gP = ibamd.cell_gradient(dpart, P)
    for d in range(1, nd + 1):
        Fv = cfd.viscous_fluxes(fluid, ibamd.at_faces(dpart, P, d), ibamd.face_gradient(dpart, P, gP, d), d,
                                mu_t=ibamd.at_faces(dpart, mut.contiguous(), d))
        r += ibamd.green_gauss(dpart, Fv, d)
    return r


@pytest.mark.parametrize("mesh,model", [("octree", "wale"), ("2d adv", "smagorinsky")])
def test_navier_stokes_les_residual(cases, adv_mesh, mesh, model):
    """Everything behind the Euler sweep is the operator-by-operator form bit for bit; the tuned sweep's Euler rows are held
    to ``percell.BOUND_CLOSURE`` per cell against the literal form.  The 2-D mesh has 8^2 blocks: the composed path."""
    import euler_sensor_model as esm
    c = cases[mesh] if mesh == "octree" else cc.adv2d_case(Case, adv_mesh)
    fluid = cfd.Fluid()
    Ph = euler_field(c.part.centers)
    Ph[:, 2:] = 30 * c.wavy(6)
    P = ibamd.hip(Ph)
    got = closures.navier_stokes_les_residual(c.dpart, P, c.Delta, fluid=fluid, model=model)
    assert got.shape == (c.nc, c.nd + 2)
    tuned = _operator_form(c.dpart, P, c.Delta, fluid, model, 0)
    assert torch.equal(got, tuned)
    euler = ibamd.residual_euler_sensor(c.dpart, P, fluid=fluid)
    assert float((got - euler)[:, 1:].abs().max()) > 0            # the viscous sum is there
    literal = ibamd.to_host(_operator_form(c.dpart, P, c.Delta, fluid, model, ibamd.IBH_FORCE_GENERAL))
    scale = esm.sensor_scale(c.part, Ph, literal)
    e = float(pc.percell_error(ibamd.to_host(got), literal, scale).max())
    print(f"navier_stokes_les_residual [{mesh}, {model}]: tuned Euler sweep against the literal form, per cell {e:.3e}")
    assert e <= pc.BOUND_CLOSURE
    out = B.colmajor_empty(c.nc, c.nd + 2)
    assert closures.navier_stokes_les_residual(c.dpart, P, c.Delta, fluid=fluid, model=model, out=out) is out
    assert torch.equal(out, got)

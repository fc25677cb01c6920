"""``k_epsilon_rhs`` / ``ibh_k_epsilon_rhs`` -- both right-hand sides of the standard k-epsilon model, the eddy viscosity, the
shear rate and the velocity gradients in ONE launch --, ``navier_stokes_k_epsilon_residual`` and
``k_epsilon_boundary_conditions`` on the device.

Every output is held to the device composition (``shear_rate_of_velocity``, ``standard_k_epsilon``, two
``scalar_transport``) bit for bit: on 3-D partitions of complete 8^3 blocks (wave per block), on face-list partitions in 2-D
and 3-D (thread per cell), with ``rk`` / ``reps`` alone (a NULL pointer for each of the others), on views into a wider state
and residual and a padded gradient buffer, with a NaN velocity and a NaN ``k``, past the grid cap, and replayed from a
graph.  The composition's own kernels answer to the oracle in tests/test_turbulence.py, tests/test_gpu_pointwise.py and
tests/test_gpu_percell_closures.py; here the fused form also answers to known answers that come from neither -- the closed
forms of tests/kepsilon_model.py on linear velocity fields -- and, per cell, to the Float64 oracle composition, both with
bounds from the Float32 oracle's own deviation (tests/test_kepsilon_model.py prints them).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import ibamd
import kepsilon_model as km
import les_model as lm
import closure_cases as cc
from closure_cases import same
from conftest import euler_field, oracle_view
from ibamd import _lib, cfd, closures
from ibamd import backend as B
from ibamd import turbulence as T

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
NU = float(km.NU)
MEASURED = {}


@pytest.fixture(scope="module", autouse=True)
def _print_measured():
    yield
    if MEASURED:
        print("\nk_epsilon_rhs, device maxima (check | mesh | output): measured / bound")
        for k in sorted(MEASURED):
            print(f"  {k[0]} | {k[1]} | {k[2]}: {MEASURED[k][0]:.3e} / {MEASURED[k][1]:.3e}")


class Case(cc.Case):
    def fields(self, seed=21):
        """(vel, k, eps) on the host: the wavy velocity, k in [0.5, 2], eps in [1, 4]."""
        k, eps = km.k_eps_fields(self.part, seed + 1)
        return self.wavy(seed), k, eps

    def device_fields(self, seed=21):
        return tuple(ibamd.hip(a) for a in self.fields(seed))


@pytest.fixture(scope="module")
def cases():
    return cc.make_cases(Case)


def composition(dpart, vel, k, eps, nu=NU):
    """The device composition: the four calls ``ibh_k_epsilon_rhs`` replaces."""
    S, gV = T.shear_rate_of_velocity(dpart, vel, gradients=True)
    ke = T.standard_k_epsilon(k, eps, S)
    rk = T.scalar_transport(dpart, k, ke["nuk"], vel, nu, ke["Sk"])
    reps = T.scalar_transport(dpart, eps, ke["nueps"], vel, nu, ke["Seps"])
    return dict(rk=rk, reps=reps, nut=ke["nut"], S=S, gradients=gV)


def check(c, got, comp, keys, what):
    assert set(got) == set(keys), (what, sorted(got))
    for k in keys:
        if k == "gradients":
            assert len(got[k]) == c.nd
            for j in range(c.nd):
                assert got[k][j].shape == (c.nc, c.nd)
                assert same(got[k][j], comp[k][j]), (what, "gradient block", j)
        else:
            assert got[k].shape == (c.nc,)
            assert same(got[k], comp[k]), (what, k)


def assert_is_the_composition(c, vel, k, eps, what=""):
    """Every optional output together, and ``rk`` / ``reps`` alone with NULL for the rest (the C entry: the wrapper always
    asks for nut)."""
    comp = composition(c.dpart, vel, k, eps)
    assert float(torch.nan_to_num(comp["rk"]).abs().max()) > 0 and float(torch.nan_to_num(comp["reps"]).abs().max()) > 0
    check(c, T.k_epsilon_rhs(c.dpart, vel, k, eps, NU, shear=True, gradients=True), comp,
          ("rk", "reps", "nut", "S", "gradients"), f"{what}: all")
    check(c, T.k_epsilon_rhs(c.dpart, vel, k, eps, NU), comp, ("rk", "reps", "nut"), f"{what}: no optional output")
    if T.fused_closures_apply(c.dpart):
        rk, reps = B.colmajor_empty(c.nc), B.colmajor_empty(c.nc)
        v, nd, ldv = B._field(vel, c.nc)
        par = (C.c_float * 5)(0.09, 1.0, 1.3, 1.44, 1.92)
        B._stream()
        B.call("ibh_k_epsilon_rhs", c.dpart.handle, B._ptr(v), ldv, B._ptr(k), B._ptr(eps), C.c_float(NU),
               C.cast(par, B.c_vp), B._ptr(rk), B._ptr(reps), None, None, None, 0)
        check(c, dict(rk=rk, reps=reps), comp, ("rk", "reps"), f"{what}: rk, reps alone")
    return comp


# ---------------------------------------------------------------------------------------------------------------------
# the composition, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", ["octree", "single"])
def test_all_block_partitions_are_the_composition(cases, mesh):
    """Wave per 8^3 block (``k_k_epsilon_rhs3``): the octree has SAME, MIRROR, COARSE and FINE sides and a block count that
    is no multiple of the four waves of a workgroup; the single block has six mirror sides."""
    c = cases[mesh]
    cc.assert_block_case(c, mesh)
    assert_is_the_composition(c, *c.device_fields(), mesh)


@pytest.mark.parametrize("nd", [2, 3])
def test_face_list_partitions_are_the_composition(cases, nd):
    """Thread per cell over the side table (``k_k_epsilon_rhs_cells``), the CSR walk at 2:1 interfaces."""
    c = cases[f"bs4 {nd}d"]
    assert_is_the_composition(c, *c.device_fields(33), f"bs4 {nd}d")


@pytest.mark.parametrize("mesh", ["octree", "bs4 2d", "bs4 3d"])
@pytest.mark.parametrize("where", ["velocity", "k"])
def test_nan_has_the_compositions_pattern(cases, mesh, where):
    c = cases[mesh]
    vel, k, eps = c.fields(4)
    if where == "velocity":
        vel[c.nc // 2, 0] = np.nan
    else:
        k[c.nc // 2] = np.nan
    comp = assert_is_the_composition(c, ibamd.hip(vel), ibamd.hip(k), ibamd.hip(eps), f"{mesh} NaN {where}")
    for o in ("rk", "reps"):
        n_nan = int(torch.isnan(comp[o]).sum())
        # the cell and its face neighbours; a NaN velocity also reaches the neighbours' neighbours through S
        assert 0 < n_nan <= (1 + 2 * c.nd * 2 ** (c.nd - 1)) ** 2, (o, n_nan)


def test_past_the_grid_cap():
    """A face-list partition of just over 4096 * 256 cells (the mesh of tests/test_gpu_les.py): the launch is capped at 4096
    workgroups, so some threads take a second cell."""
    c = cc.grid_cap_case(Case)
    vel, k, eps = c.device_fields(2)
    comp = composition(c.dpart, vel, k, eps)
    got = T.k_epsilon_rhs(c.dpart, vel, k, eps, NU, shear=True)
    for o in ("rk", "reps", "nut", "S"):
        assert torch.equal(got[o], comp[o]), o
        assert float(got[o][-1]) == float(comp[o][-1]) != 0.0, o


@pytest.mark.parametrize("mesh", ["octree", "bs4 2d"])
def test_graph_replay(cases, mesh):
    c = cases[mesh]
    vel, k, eps = c.device_fields(1)
    kw = dict(shear=True, gradients=True)
    g = ibamd.GraphedClosure(lambda p, v, kk, ee: T.k_epsilon_rhs(p, v, kk, ee, NU, **kw), c.dpart, vel, k, eps)
    new = c.device_fields(77)
    for dst, src in zip((vel, k, eps), new):
        dst.copy_(src)
    out = g()
    torch.cuda.synchronize()
    eager = T.k_epsilon_rhs(c.dpart, vel, k, eps, NU, **kw)
    for o in ("rk", "reps", "nut", "S"):
        assert torch.equal(out[o], eager[o]), o
    for j in range(c.nd):
        assert torch.equal(out["gradients"][j], eager["gradients"][j]), j
    first = T.k_epsilon_rhs(c.dpart, *c.device_fields(1), NU, **kw)
    assert not torch.equal(first["rk"], eager["rk"])              # the replay saw the new input


def test_partition_with_skirt_fragments_composes():
    """Two partitions of the octree: blocks and skirt fragments, not all-block.  The wrapper composes; the C entry says so."""
    c = cc.skirt_case(Case)
    vel, k, eps = c.device_fields()
    assert_is_the_composition(c, vel, k, eps, "two partitions")
    rk, reps = B.colmajor_empty(c.nc), B.colmajor_empty(c.nc)
    par = (C.c_float * 5)(0.09, 1.0, 1.3, 1.44, 1.92)
    B._stream()
    lib = _lib.load()
    rc = lib.ibh_k_epsilon_rhs(c.dpart.handle, B._ptr(vel), c.nc, B._ptr(k), B._ptr(eps), NU, C.cast(par, B.c_vp), B._ptr(rk),
                               B._ptr(reps), None, None, None, 0)
    assert rc != 0 and b"compose" in lib.ibh_last_error(), lib.ibh_last_error()


def test_misuse_raises_value_error(cases):
    c = cases["bs4 3d"]
    vel, k, eps = c.device_fields()
    with pytest.raises(ValueError):
        T.k_epsilon_rhs(c.dpart, vel[:, :2], k, eps, NU)                           # wrong vel width
    with pytest.raises(ValueError):
        T.k_epsilon_rhs(c.dpart, vel, k[:-1].contiguous(), eps, NU)                # a short k
    with pytest.raises(ValueError):
        T.k_epsilon_rhs(c.dpart, vel, k, eps[:-1].contiguous(), NU)
    with pytest.raises(ValueError):
        T.k_epsilon_rhs(c.dpart, vel, k, eps, NU, out_k=B.colmajor_empty(c.nc, 2))  # an out_k that is not a vector
    with pytest.raises(ValueError):
        T.k_epsilon_rhs(c.dpart, vel, k, eps, NU, out_eps=B.colmajor_empty(c.nc - 1))
    with pytest.raises(ValueError):
        T.k_epsilon_rhs(c.dpart, ibamd.to_host(vel), k, eps, NU)                   # a host array: no CPU path


# ---------------------------------------------------------------------------------------------------------------------
# answers that come from neither the fused form nor the composition
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", ["octree", "bs4 2d", "bs4 3d"])
def test_linear_fields_give_the_closed_forms(cases, mesh):
    """u = A x for a shear, a dilatation and a rotation with constant k0, eps0, on the cells whose 2-ring is same-level with
    no mirror face: rk = nut S^2 - eps0 - k0 tr(A), reps = C1 nut S^2 eps0 / k0 - C2 eps0^2 / k0 - eps0 tr(A); every output
    within 4 x the Float32 oracle composition's own deviation from the same answers on this mesh
    (``kepsilon_model.bounds``: per output, the maximum over the three fields and the selected cells).

    """
    c = cases[mesh]
    sel = lm.interior(c.part)
    assert 2 * sel.sum() >= sel.size                              # the mask cannot hide the kernel
    bound, _ = km.bounds(mesh, c.part, oracle_view(c.part))
    k = ibamd.hip(np.full(c.nc, km.K0, f32))
    eps = ibamd.hip(np.full(c.nc, km.EPS0, f32))
    worst = {}
    for name, make in lm.FIELDS:
        A = make(c.nd)
        vel = ibamd.hip(lm.linear_field(c.part, A))
        ans = km.closed_form(A, c.nc)
        got = T.k_epsilon_rhs(c.dpart, vel, k, eps, NU, shear=True)
        for o in km.OUTPUTS:
            e = float(np.abs(ibamd.to_host(got[o]).astype(f64) - ans[o])[sel].max())
            worst[o] = max(worst.get(o, 0.0), e)
    for o in km.OUTPUTS:
        MEASURED["linear", mesh, o] = (worst[o], bound[o])
        print(f"{mesh} | {o}: device {worst[o]:.3e}, bound {bound[o]:.3e}")
    for o in km.OUTPUTS:
        assert worst[o] <= bound[o], (mesh, o, worst[o], bound[o])


@pytest.mark.parametrize("mesh", ["octree", "bs4 2d"])
def test_wavy_fields_against_the_float64_oracle_per_cell(cases, mesh):
    """Every cell of the partition against the Float64 oracle composition of the same Float32 fields, the error of each cell
    over the cell's own scale (|source| + sum_d unsigned_green_gauss(|face flux|): what the sum's rounding is relative to;
    nut over its own magnitude): the device maximum within 4 x the Float32 oracle composition's own maximum."""
    c = cases[mesh]
    (vel, k, eps), ref, scale, dev = km.wavy_reference(mesh, c.part, oracle_view(c.part))
    got = T.k_epsilon_rhs(c.dpart, ibamd.hip(vel), ibamd.hip(k), ibamd.hip(eps), NU)
    worst = {o: float((np.abs(ibamd.to_host(got[o]).astype(f64) - ref[o]) / scale[o]).max()) for o in km.WAVY_OUTPUTS}
    for o in km.WAVY_OUTPUTS:
        MEASURED["wavy", mesh, o] = (worst[o], 4.0 * dev[o])
        print(f"{mesh} | {o}: device {worst[o]:.3e}, Float32 oracle {dev[o]:.3e}")
    for o in km.WAVY_OUTPUTS:
        assert worst[o] <= 4.0 * dev[o], (mesh, o, worst[o], dev[o])


# ---------------------------------------------------------------------------------------------------------------------
# views and padding
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", ["octree", "bs4 2d"])
def test_state_views_residual_columns_and_padded_gradient_buffer(cases, mesh):
    """``Q = [p T u v (w) k eps]`` read in place, ``rk`` / ``reps`` written into the last two columns of a wider residual,
    ``G`` inside a wider buffer with ``ldg > nc``: the written columns are the composition's, everything else in all parents
    keeps its bits."""
    c = cases[mesh]
    nd, nc = c.nd, c.nc
    rng = np.random.default_rng(5)
    vel_h, k_h, eps_h = c.fields(9)
    Q = ibamd.hip(np.concatenate([rng.uniform(1, 2, (nc, 2)).astype(f32), vel_h, k_h[:, None], eps_h[:, None]], axis=1))
    Q0 = Q.clone()
    vel, k, eps = Q[:, 2:2 + nd], Q[:, nd + 2], Q[:, nd + 3]
    comp = composition(c.dpart, vel, k, eps)
    v, nv, ldv = B._field(vel, nc)
    assert v.data_ptr() == Q.data_ptr() + 8 * nc and ldv == nc     # no copy was made
    assert T._vec(k, nc).data_ptr() == Q.data_ptr() + 4 * nc * (nd + 2)
    assert T._vec(eps, nc).data_ptr() == Q.data_ptr() + 4 * nc * (nd + 3)
    r = ibamd.hip(np.full((nc, nd + 4), -3.5, f32))
    r0 = r.clone()
    got = T.k_epsilon_rhs(c.dpart, vel, k, eps, NU, out_k=r[:, nd + 2], out_eps=r[:, nd + 3], shear=True)
    assert got["rk"].data_ptr() == r.data_ptr() + 4 * nc * (nd + 2) and got["reps"].data_ptr() == r.data_ptr() + 4 * nc * (nd + 3)
    assert torch.equal(r[:, nd + 2], comp["rk"]) and torch.equal(r[:, nd + 3], comp["reps"])
    assert torch.equal(r[:, :nd + 2], r0[:, :nd + 2])
    assert torch.equal(got["nut"], comp["nut"]) and torch.equal(got["S"], comp["S"])
    assert torch.equal(Q, Q0)
    # the C entry: G into a padded buffer, rk / reps into the residual's columns again
    ldg = nc + 37
    pad = torch.full((nd * nd + 2, ldg), -7.25, dtype=torch.float32, device=Q.device)    # row r = column r of the parent
    pad0 = pad.clone()
    r.copy_(r0)
    par = (C.c_float * 5)(0.09, 1.0, 1.3, 1.44, 1.92)
    B._stream()
    B.call("ibh_k_epsilon_rhs", c.dpart.handle, B._ptr(v), ldv, B._ptr(k), B._ptr(eps), C.c_float(NU), C.cast(par, B.c_vp),
           C.c_void_p(r.data_ptr() + 4 * nc * (nd + 2)), C.c_void_p(r.data_ptr() + 4 * nc * (nd + 3)), None, None,
           C.c_void_p(pad.data_ptr() + 4 * ldg), ldg)
    assert torch.equal(Q, Q0)
    assert torch.equal(r[:, nd + 2], comp["rk"]) and torch.equal(r[:, nd + 3], comp["reps"])
    assert torch.equal(r[:, :nd + 2], r0[:, :nd + 2])
    assert torch.equal(pad[0], pad0[0]) and torch.equal(pad[-1], pad0[-1]) and torch.equal(pad[:, nc:], pad0[:, nc:])
    for j in range(nd):
        for i in range(nd):
            assert torch.equal(pad[1 + nd * j + i, :nc], comp["gradients"][j][:, i]), (i, j)


# ---------------------------------------------------------------------------------------------------------------------
# the closure that uses it, and its boundary conditions
# ---------------------------------------------------------------------------------------------------------------------
def _operator_form(dpart, Q, nu, fluid):
    """``navier_stokes_k_epsilon_residual`` operator by operator: nothing fused but the Euler sweep."""
    from ibamd.hiparray import HipArray
    nd = dpart.nd
    nvp = nd + 2
    P = Q[:, :nvp]
    r = B.colmajor_empty(Q.shape[0], nvp + 2)
    r[:, :nvp] = ibamd.residual_euler_hll(dpart, P)
    g = [list(ibamd.cell_gradient(dpart, Q[:, 2 + i].contiguous())) for i in range(nd)]
    ke = T.standard_k_epsilon(Q[:, nvp].contiguous(), Q[:, nvp + 1].contiguous(), T.shear_rate(g))
    for col, nuR, src in ((nvp, ke["nuk"], ke["Sk"]), (nvp + 1, ke["nueps"], ke["Seps"])):
        R = Q[:, col].contiguous()
        rt = src.clone()
        for d in range(nd):
            conv = ibamd.at_faces(dpart, Q[:, 2 + d].contiguous() * R, d + 1)
            diff = ibamd.at_faces(dpart, float(nu) + nuR, d + 1) * ibamd.face_gradient(dpart, R, d + 1)
            rt += ibamd.green_gauss(dpart, diff - conv, d + 1)
        r[:, col] = rt
    mut = (HipArray(Q[:, 0]) / (HipArray(Q[:, 1]) * fluid.R) * HipArray(ke["nut"])).t
    gP = ibamd.cell_gradient(dpart, P)
    for d in range(1, nd + 1):
        Fv = cfd.viscous_fluxes(fluid, ibamd.at_faces(dpart, P, d), ibamd.face_gradient(dpart, P, gP, d), d,
                                mu_t=ibamd.at_faces(dpart, mut.contiguous(), d))
        r[:, :nvp] += ibamd.green_gauss(dpart, Fv, d)
    return r


@pytest.mark.parametrize("mesh", ["octree", "2d adv"])
def test_navier_stokes_k_epsilon_residual(cases, adv_mesh, mesh):
    """Everything behind the Euler sweep is the operator-by-operator form bit for bit.  The 2-D mesh has 8^2 blocks: the
    composed path."""
    c = cases[mesh] if mesh == "octree" else cc.adv2d_case(Case, adv_mesh)
    fluid = cfd.Fluid()
    vel_h, k_h, eps_h = c.fields(6)
    Ph = euler_field(c.part.centers)
    Ph[:, 2:] = 30 * vel_h
    Q = ibamd.hip(np.concatenate([Ph, k_h[:, None], eps_h[:, None]], axis=1))
    Q0 = Q.clone()
    got = closures.navier_stokes_k_epsilon_residual(c.dpart, Q, nu=NU, fluid=fluid)
    assert got.shape == (c.nc, c.nd + 4) and torch.equal(Q, Q0)
    ref = _operator_form(c.dpart, Q, NU, fluid)
    assert torch.equal(got, ref)
    euler = ibamd.residual_euler_hll(c.dpart, Q[:, :c.nd + 2])
    assert float((got[:, :c.nd + 2] - euler)[:, 1:].abs().max()) > 0      # the viscous sum is there
    assert float(got[:, c.nd + 2].abs().max()) > 0 and float(got[:, c.nd + 3].abs().max()) > 0
    out = B.colmajor_empty(c.nc, c.nd + 4)
    assert closures.navier_stokes_k_epsilon_residual(c.dpart, Q, nu=NU, fluid=fluid, out=out) is out
    assert torch.equal(out, got)
    with pytest.raises(ValueError):
        closures.navier_stokes_k_epsilon_residual(c.dpart, Q[:, :c.nd + 3], nu=NU, fluid=fluid)


def test_boundary_conditions_fused_against_composed():
    """``k_epsilon_boundary_conditions`` on a small sphere in a box (4^3 blocks, h = 0.4): the fused form -- one launch per
    boundary partition -- writes the ghost cells the composed ``impose_bc`` form writes, difference 0, and no other cell."""
    import bench
    import flow_bc_model as fm
    from ibamd.mesher import Mesh
    msh = Mesh(f32([-4, -4, -4]), f32([8, 8, 8]), ("sphere", bench.icosphere(subdiv=2), f32(0.4)), block_size=4)
    fam = [("farfield", [(d, sd) for d in (1, 2, 3) for sd in (False, True)])]
    dom = ibamd.Domain(msh, hypercube_families=fam, max_partition_size=10 ** 9)
    nd, n = dom.ndims, len(dom)
    ghosts = np.zeros(n, bool)
    for name in ("sphere", "farfield"):
        for b in dom.boundaries[name].values():
            ghosts[b.ghost_indices] = True
    assert ghosts.sum() >= 500
    rng = np.random.default_rng(3)
    Q0 = np.empty((n, nd + 4), f32)
    Q0[:, :nd + 2] = fm.image_point_family(n, nd, seed=3)[0]
    Q0[:, nd + 2] = rng.uniform(0.5, 2, n)
    Q0[:, nd + 3] = rng.uniform(1, 4, n)
    res = {}
    for fused in (True, False):
        Q = ibamd.hip(Q0)
        closures.k_epsilon_boundary_conditions(dom, Q, fm.FAR3, fused=fused)
        res[fused] = ibamd.to_host(Q)
    assert np.array_equal(res[True], res[False], equal_nan=True)
    assert np.array_equal(res[True][~ghosts], Q0[~ghosts])
    assert ((res[True][ghosts] != Q0[ghosts]).any(axis=1)).all()
    # the defaults are the free-stream values of standard_kϵ's docstring: k = 3 (U Tu)^2 / 2, eps = Cmu k^2 / (3 nu), Tu = 0.10
    k_inf = 1.5 * (100.0 * 0.10) ** 2
    rho = fm.FAR3[0] / (cfd.Fluid().R * fm.FAR3[1])
    mu = float(cfd.dynamic_viscosity(cfd.Fluid(), ibamd.hip(np.array([fm.FAR3[1]], f32)))[0])
    Q = ibamd.hip(Q0)
    closures.k_epsilon_boundary_conditions(dom, Q, fm.FAR3, k_inf=k_inf, eps_inf=0.09 * k_inf ** 2 / (3 * mu / rho), fused=True)
    assert np.allclose(ibamd.to_host(Q), res[True], rtol=1e-6, atol=0, equal_nan=True)
    Q = ibamd.hip(Q0)
    closures.k_epsilon_boundary_conditions(dom, Q, fm.FAR3, k_inf=2 * k_inf, fused=True)
    assert not np.allclose(ibamd.to_host(Q), res[True], rtol=1e-6, atol=0, equal_nan=True)
    with pytest.raises(ValueError):
        closures.k_epsilon_boundary_conditions(dom, ibamd.hip(Q0[:, :nd + 3]), fm.FAR3, fused=True)

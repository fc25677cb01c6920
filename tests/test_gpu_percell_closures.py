"""The operators, the viscous sum and the turbulence closure of BASELINE.json configs[4], per cell, against one float64
evaluation of the oracle per partition (tests/percell.py: references, scales, bounds; tests/test_percell_closures.py
calibrates them on the CPU).

Before this module these kernels were compared with the device composition of the face-list operators (bit for bit) and
the operators themselves norm-wise on one mesh: an operator wrong on a coarse / fine side would have been copied into the
reference.  Here every form answers to float64 per cell, on 2-D and 3-D partitions with level jumps, skirts, coarse
multigrid levels and the viscous kernel's tails; ``dpart.info`` pins what each partition is there for.  The inputs
(``percell.closure_field``) reach the closures' branches: T below, at and just above 10 K, mu_t = 0, S = 0 exactly, the
source's 10 R, velocities that cross zero.  ``test_pointwise_edges`` pins the pointwise physics per element, NaN / Inf
included, against the oracle (Julia's clamp / min / max propagate NaN).  The operator, viscous and turbulence kernels
run with one NaN temperature on two partitions, so does the closures' R row; their Euler rows and ``inviscid_fluxes`` are
strict expected failures: the fused sweeps do not propagate NaN, which measured 7-10 % of their speed.

``ibh_cell_gradient_all`` runs through the tuple ``cell_gradient`` on the partitions without 8^n blocks (2-D RAE2822 coarse
level, ``block_size=4``, 3-D coarse levels): ``ibh_cell_gradient_nd`` hands them to it.
"""
import numpy as np
import pytest
import torch

import ibamd
import percell as pc
from conftest import ADV_FAMILIES, RAE_FAMILIES, oracle_view
from ibamd import _lib
from ibamd import cfd, closures
from ibamd import turbulence as T
from oracle import cfd as ocfd
from oracle import domain as od
from oracle import turbulence as ot

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
NU = f32(1.5e-5)
VISC_WG, VISC_CAP = 512, 128          # csrc/ibh_cfd.hip: cells per workgroup, left-face tasks per direction in LDS
MEASURED = {}


def _record(form, err):
    MEASURED[form] = max(MEASURED.get(form, 0.0), err)


@pytest.fixture(scope="module", autouse=True)
def _print_measured():
    yield
    if MEASURED:
        print("\nper-cell maxima against float64:")
        for k in sorted(MEASURED):
            print(f"  {k}: {MEASURED[k]:.3e}")


def _tuned(key, value, default, fn):
    try:
        _lib.call("ibh_set_tuning", key.encode(), int(value))
        return fn()
    finally:
        _lib.call("ibh_set_tuning", key.encode(), int(default))


def _h(t):
    return ibamd.to_host(t)


def visc_tasks(part):
    """Per 512-cell chunk and direction: the left faces that ibh_viscous_residual's shared kernel cannot take from LDS (no
    single left neighbour inside the chunk), counted from the face lists."""
    nc = part.spacing.shape[0]
    out = []
    for d in range(1, part.ndims + 1):
        o, nb = part.face_owners_neighbors[d]
        nleft = np.bincount(nb, minlength=nc)
        left = np.full(nc, -1, np.int64)
        left[nb] = o
        c = np.arange(nc)
        ok = (nleft == 1) & (left // VISC_WG == c // VISC_WG)
        out.append(np.bincount(c[~ok] // VISC_WG, minlength=-(-nc // VISC_WG)))
    return np.stack(out, axis=1)


class Case:
    def __init__(self, part, nan_cell=False):
        self.part = part
        self.dpart = ibamd.to_backend(part, ibamd.hip)
        self.info = self.dpart.info
        self.classes = pc.cell_classes(part)
        self.op = oracle_view(part)
        self.nd = part.ndims
        self.nvp = self.nd + 2
        self.nc = part.spacing.shape[0]
        self.Q = pc.closure_field(part.centers)
        if nan_cell:   # one NaN temperature in the middle of the partition
            self.Q[self.nc // 2, 1] = np.nan
        self._ref = {}

    def ref(self, key, fn):
        if key not in self._ref:
            self._ref[key] = fn()
        return self._ref[key]

    def check(self, form, got, ref, scale, bound, faces_dim=None):
        if faces_dim:
            e = pc.check_faces(got, ref, scale, bound, self.part, faces_dim, classes=self.classes, what=form)
        else:
            e = pc.check(got, ref, scale, bound, self.part, classes=self.classes, what=form)
        _record(form, e)


def _dom(msh, fam=None, **kw):
    return ibamd.Domain(msh, hypercube_families=fam or [], boundaries=False, **kw)


@pytest.fixture(scope="module")
def cases(adv_mesh, rae_mesh_small):
    import bench
    from ibamd.mesher import Ball, Mesh
    out = {}
    (p,) = _dom(adv_mesh, ADV_FAMILIES, max_partition_size=10 ** 9).partitions.values()
    out["2d adv"] = Case(p)
    dom = _dom(rae_mesh_small, RAE_FAMILIES, max_partition_size=10 ** 9)
    (p,) = dom.partitions.values()
    out["2d rae"] = Case(p)
    for k, p in _dom(rae_mesh_small, RAE_FAMILIES, max_partition_size=16384).partitions.items():
        out[f"2d rae16k_{k}"] = Case(p)
    cds, _, _ = ibamd.multigrid(dom, max_levels=1)
    (p,) = cds[0].partitions.values()
    out["2d rae coarse"] = Case(p)
    msh4 = Mesh(f32([-1, -1]), f32([2, 2]), block_size=4,
                refinement_regions=[(Ball(np.array([0.3, 0.3]), 0.05), f32(0.02))])
    (p,) = _dom(msh4, max_partition_size=10 ** 9).partitions.values()
    out["2d bs4"] = Case(p)
    msh = Mesh(f32([-2, -2, -2]), f32([4, 4, 4]), block_size=8,
               refinement_regions=[(Ball(np.array([-2.0, -2.0, -2.0]), 0.1), f32(0.1))])
    d = _dom(msh, max_partition_size=10 ** 9)
    (p,) = d.partitions.values()
    out["3d corner"] = Case(p)
    n = len(msh)
    for k, p in _dom(msh, max_partition_size=-(-(n // 2) // 512) * 512 + 512).partitions.items():
        out[f"3d corner2_{k}"] = Case(p)
    cds, _, _ = ibamd.multigrid(d, max_levels=1)
    (p,) = cds[0].partitions.values()
    out["3d corner coarse"] = Case(p)
    msh = Mesh(f32([-2, -2, -2]), f32([4, 4, 4]), block_size=8,
               refinement_regions=[(Ball(np.array([1.2, 1.2, 1.2]), 0.1), f32(0.1))])
    (p,) = _dom(msh, max_partition_size=10 ** 9).partitions.values()
    out["3d ball"] = Case(p, nan_cell=True)
    msh = Mesh(f32([-4, -4, -4]), f32([8, 8, 8]), ("sphere", bench.icosphere(subdiv=2), f32(0.2)), block_size=8)
    msh.distance_fields = {}
    n = len(msh)
    for k, p in _dom(msh, max_partition_size=-(-(-(-n // 4)) // 512) * 512, only=[1]).partitions.items():
        out[f"3d sphere_{k}"] = Case(p)
    # a small partition (nc < 512) and one with nc % 512 != 0: the viscous kernel's tails
    msh = Mesh(f32([-1, -1, -1]), f32([2, 2, 2]), block_size=4)
    (p,) = _dom(msh, max_partition_size=10 ** 9).partitions.values()
    out["3d tiny"] = Case(p)
    return out


@pytest.fixture(scope="module")
def hierarchy():
    """A reduced configs[4] hierarchy: multigrid(max_levels=2) of a sphere octree (8^3, 4^3 and 2^3 blocks)."""
    import bench
    from ibamd.mesher import Mesh
    msh = Mesh(f32([-4, -4, -4]), f32([8, 8, 8]), ("sphere", bench.icosphere(subdiv=1), f32(0.4)), block_size=8)
    msh.distance_fields = {}
    dom = _dom(msh, max_partition_size=10 ** 9)
    cds, _, _ = ibamd.multigrid(dom, max_levels=2)
    out = {}
    for lvl, d in enumerate([dom] + cds):
        (p,) = d.partitions.values()
        out[f"3d level{lvl}"] = Case(p, nan_cell=(lvl == 1))
    return out


def test_coverage(cases, hierarchy):
    c = cases
    for n in ("2d adv", "2d rae"):
        assert c[n].info["full_blocks"] > 0 and c[n].info["irregular_cells"] == 0, n
    skirts = [v for k, v in c.items() if k.startswith("2d rae16k")]
    assert skirts and all(v.info["full_blocks"] > 0 and v.info["irregular_cells"] > 0 for v in skirts)
    for n in ("2d rae coarse", "2d bs4"):
        i = c[n].info
        assert i["full_blocks"] == 0 and 0 < i["direct_sides"] < 2 * 2 * c[n].nc, (n, i)   # the _cells kernels
    for n in ("3d corner", "3d ball"):
        assert T.all_blocks(c[n].dpart), n
        for key in ("sides_same", "sides_mirror", "sides_coarse", "sides_fine"):
            assert c[n].info[key] > 0, (n, key)
    assert sum(k.startswith("3d corner2") for k in c) == 2
    sph = [v for k, v in c.items() if k.startswith("3d sphere")]
    assert sph and all(v.info["full_blocks"] > 0 and v.info["irregular_cells"] > 0 for v in sph)
    assert c["3d corner coarse"].info["full_blocks"] == 0
    nc = {k: v.nc for k, v in c.items()}
    assert any(n < VISC_WG for n in nc.values()) and any(n % VISC_WG for n in nc.values() if n > VISC_WG), nc
    over = {k: int(visc_tasks(v.part).max()) for k, v in c.items()}
    assert max(over.values()) > VISC_CAP, over                 # the overflow path (tasks evaluated in place) runs
    for k, v in hierarchy.items():
        assert v.nc > 0, k
    h0, h1, h2 = (hierarchy[f"3d level{k}"] for k in range(3))
    assert T.all_blocks(h0.dpart) and h0.info["full_blocks"] * 512 == h0.nc      # 8^3 blocks: the fused block kernels
    assert h0.nc == 8 * h1.nc == 64 * h2.nc                                      # 4^3 and 2^3 blocks of the same tree
    for h in (h1, h2):   # no 8^3 block: the face-list sweep, the _cells operators and the fused face-list closures
        assert h.info["full_blocks"] == 0 and T.fused_closures_apply(h.dpart)
    for n in ("2d rae coarse", "2d bs4", "3d corner coarse", "3d tiny"):
        assert c[n].info["full_blocks"] == 0, n       # the tuple cell_gradient goes through ibh_cell_gradient_all


# ---------------------------------------------------------------------------------------------------------------------
# operators
# ---------------------------------------------------------------------------------------------------------------------
def test_operators(cases):
    for name, c in cases.items():
        op = c.op
        P = np.ascontiguousarray(c.Q[:, :c.nvp])
        u = np.ascontiguousarray(c.Q[:, 2])
        p = np.ascontiguousarray(c.Q[:, 0])
        P64, u64, p64 = pc.to64(P, u, p)
        dP, du, dp = ibamd.hip(P), ibamd.hip(u), ibamd.hip(p)
        tup = ibamd.cell_gradient(c.dpart, du)
        tupP = ibamd.cell_gradient(c.dpart, dP)
        D = od.JST_sensor(op, p)
        for d in range(1, c.nd + 1):
            gref = od.cell_gradient(op, u64, d)
            gs = pc.abs_cell_gradient(op, u64, d) + np.abs(gref)
            c.check("cell_gradient per dim", _h(ibamd.cell_gradient(c.dpart, du, d)), gref, gs, pc.BOUND_OPS)
            c.check("cell_gradient tuple (nd)", _h(tup[d - 1]), gref, gs, pc.BOUND_OPS)
            gP = od.cell_gradient(op, P64, d)
            gPs = pc.abs_cell_gradient(op, P64, d) + np.abs(gP)
            c.check("cell_gradient tuple (fields)", _h(tupP[d - 1]), gP, gPs, pc.BOUND_OPS)
            r = od.at_faces(op, P64, d)
            c.check("at_faces", _h(ibamd.at_faces(c.dpart, dP, d)), r, pc.abs_at_faces(op, P64, d) + np.abs(r),
                    pc.BOUND_OPS, faces_dim=d)
            r = od.face_gradient(op, P64, d)
            fgs = pc.abs_face_gradient(op, P64, d) + np.abs(r)
            c.check("face_gradient", _h(ibamd.face_gradient(c.dpart, dP, d)), r, fgs, pc.BOUND_OPS, faces_dim=d)
            gP32 = tuple(od.cell_gradient(op, P, k) for k in range(1, c.nd + 1))
            fg = ibamd.face_gradient(c.dpart, dP, tuple(ibamd.hip(g) for g in gP32), d)
            rr = od.face_gradient(op, P64, tuple(g.astype(f64) for g in gP32), d)
            for k in range(c.nd):
                sc = fgs if k == d - 1 else pc.abs_at_faces(op, gP32[k].astype(f64), d) + np.abs(rr[k])
                c.check("face_gradient (gradient form)", _h(fg[k]), rr[k], sc, pc.BOUND_OPS, faces_dim=d)
            uf = od.at_faces(op, P, d)                           # float32 face values, exact inputs
            r = od.green_gauss(op, uf.astype(f64), d)
            c.check("green_gauss", _h(ibamd.green_gauss(c.dpart, ibamd.hip(uf), d)), r,
                    pc.abs_green_gauss(op, uf.astype(f64), d) + np.abs(r), pc.BOUND_OPS)
            r = od.JST_sensor(op, p64, d)
            c.check("JST_sensor per dim", _h(ibamd.JST_sensor(c.dpart, dp, d)), r, 1 + np.abs(r), pc.BOUND_OPS)
            gu32 = od.cell_gradient(op, P, d)
            for withD, ho in ((False, False), (True, False), (True, True)):
                Dx = D if withD else None
                rL, rR = od.MUSCL(op, P64, gu32.astype(f64), d, D=None if Dx is None else Dx.astype(f64), high_order=ho)
                gL, gR = ibamd.MUSCL(c.dpart, dP, ibamd.hip(gu32), d, D=None if Dx is None else ibamd.hip(Dx),
                                     high_order=ho)
                sc = pc.muscl_scale(op, P, gu32, d, D=Dx, high_order=ho)
                form = f"MUSCL D={withD} high_order={ho}"
                c.check(form, _h(gL), rL, sc + np.abs(rL), pc.BOUND_OPS, faces_dim=d)
                c.check(form, _h(gR), rR, sc + np.abs(rR), pc.BOUND_OPS, faces_dim=d)
        ufs = [od.at_faces(op, P, d) for d in range(1, c.nd + 1)]
        r = od.divergent(op, [x.astype(f64) for x in ufs])
        s = sum(pc.abs_green_gauss(op, x.astype(f64), d + 1) for d, x in enumerate(ufs)) + np.abs(r)
        c.check("divergent", _h(ibamd.divergent(c.dpart, [ibamd.hip(x) for x in ufs])), r, s, pc.BOUND_OPS)
        r = od.JST_sensor(op, p64)
        c.check("JST_sensor", _h(ibamd.JST_sensor(c.dpart, dp)), r, 1 + np.abs(r), pc.BOUND_OPS)


# ---------------------------------------------------------------------------------------------------------------------
# viscous sum, transport, shear rate, Wray-Agarwal
# ---------------------------------------------------------------------------------------------------------------------
def _strided(a):
    """A column-major device copy of ``a`` whose leading dimension exceeds the row count (a column slice)."""
    n, nv = a.shape
    buf = torch.full((nv + 1, n + 13), float("nan"), dtype=torch.float32, device="cuda").T
    v = buf[:n, :nv]
    v.copy_(ibamd.hip(np.ascontiguousarray(a)))
    return v


def test_viscous_residual(cases):
    fluid = ocfd.Fluid()
    for name, c in cases.items():
        P = np.ascontiguousarray(c.Q[:, :c.nvp])
        R = np.ascontiguousarray(c.Q[:, c.nvp])
        mut = ((c.Q[:, 0] / (fluid.R * c.Q[:, 1])) * R).astype(f32)
        R0 = (np.random.default_rng(1).uniform(-1, 1, P.shape) * 1e-3).astype(f32)
        ref = c.ref("visc", lambda: pc.oracle_viscous_sum(c.op, *pc.to64(P, mut, R0)))
        scale = c.ref("visc_s", lambda: pc.viscous_scale(c.part, P, mut, ref, R0))
        dP = _strided(P)
        assert dP.stride(1) > c.nc
        gfull = ibamd.cell_gradient(c.dpart, ibamd.hip(P))
        gvel = ibamd.cell_gradient(c.dpart, ibamd.hip(np.ascontiguousarray(P[:, 2:])))
        for per_cell in (0, 1):
            for vonly, g in ((False, gfull), (True, gvel)):
                out = _strided(R0)

                def run():
                    cfd.viscous_residual(c.dpart, cfd.Fluid(), dP, g, ibamd.hip(mut), out, velocity_gradients_only=vonly)
                    return _h(out)
                got = _tuned("viscous_per_cell", per_cell, 0, run)
                c.check(f"viscous_residual per_cell={per_cell} velocity_gradients_only={vonly}", got, ref, scale,
                        pc.BOUND_VISCOUS)


def test_turbulence(cases):
    for name, c in cases.items():
        vel = np.ascontiguousarray(c.Q[:, 2:c.nvp])
        R = np.ascontiguousarray(c.Q[:, c.nvp])
        dvel = ibamd.hip(vel)
        S64 = ot.shear_rate(pc.oracle_velocity_gradients(c.op, vel.astype(f64)))
        Ss = pc.shear_scale(c.op, vel, S64)
        S = _h(T.shear_rate_of_velocity(c.dpart, dvel))
        c.check("shear_rate_of_velocity", S, S64, Ss, pc.BOUND_TURB)
        S2, G = T.shear_rate_of_velocity(c.dpart, dvel, gradients=True)
        c.check("shear_rate_of_velocity gradients=True", _h(S2), S64, Ss, pc.BOUND_TURB)
        for d in range(c.nd):
            r = od.cell_gradient(c.op, vel.astype(f64), d + 1)
            c.check("shear_rate_of_velocity gradients", _h(G[d]), r,
                    pc.abs_cell_gradient(c.op, vel.astype(f64), d + 1) + np.abs(r), pc.BOUND_OPS)
        # Wray-Agarwal on the device's float32 S (the kernel in isolation)
        wa64 = pc.oracle_wray_agarwal_of(c.op, *pc.to64(R, S))
        was = pc.wray_agarwal_scale(c.op, R, S)
        wa = T.Wray_Agarwal_of(c.dpart, ibamd.hip(R), ibamd.hip(S))
        for k in ("nut", "nuR", "S"):
            c.check(f"Wray_Agarwal_of {k}", _h(wa[k]), wa64[k], was[k], pc.BOUND_TURB)
        # transport on the float32 nuR / S of the oracle (inputs exact)
        wa32 = pc.oracle_wray_agarwal_of(c.op, R, S)
        nuR, Sw = wa32["nuR"], wa32["S"]
        t64 = pc.oracle_transport(c.op, *pc.to64(R, nuR, vel), NU, Sw.astype(f64))
        ts = pc.transport_scale(c.op, R, nuR, vel, NU, Sw, t64)
        for blocks in (1, 0):
            got = _tuned("transport_blocks", blocks, 1, lambda: _h(T.scalar_transport(
                c.dpart, ibamd.hip(R), ibamd.hip(nuR), dvel, float(NU), ibamd.hip(Sw))))
            c.check(f"scalar_transport transport_blocks={blocks}", got, t64, ts, pc.BOUND_TRANSPORT)


# ---------------------------------------------------------------------------------------------------------------------
# whole closures
# ---------------------------------------------------------------------------------------------------------------------
def _closures(c, tag, finite=False):
    """Both closures against float64; ``finite``: on the field without its NaN cell (the fused sweeps' deviation)."""
    Q = c.Q.copy()
    if finite:
        Q[np.isnan(Q)] = f32(288.15)
    Q64 = Q.astype(f64)
    for visc in (True, False):
        ref = c.ref(f"cl{visc}{finite}", lambda: pc.oracle_wa_residual(c.op, Q64, NU, viscous=visc))
        sc = c.ref(f"cls{visc}{finite}", lambda: pc.closure_scale(c.op, Q, ref, NU, viscous=visc))
        dQ = ibamd.hip(Q)
        if visc:
            for fused in (True, False):
                got = _h(closures.navier_stokes_wray_agarwal_residual(c.dpart, dQ, nu=float(NU), fused_viscous=fused))
                c.check(f"{tag} navier_stokes_wray_agarwal fused_viscous={fused}", got, ref, sc, pc.BOUND_CLOSURE)
        else:
            got = _h(closures.euler_wray_agarwal_residual(c.dpart, dQ, nu=float(NU)))
            c.check(f"{tag} euler_wray_agarwal", got, ref, sc, pc.BOUND_CLOSURE)


def test_closures(cases):
    for name, c in cases.items():
        _closures(c, "closure", finite=True)


def test_closures_hierarchy(hierarchy):
    for name, c in hierarchy.items():
        _closures(c, f"closure {name}", finite=True)


SWEEP_NAN = ("the fused sweeps (ibh_flux.h and the block / quad / column kernels) keep fmaxf / fminf in the JST sensor, "
             "the MUSCL minmod and the temperature clamp, so around a NaN cell their residual is finite where Julia's is "
             "NaN: the NaN-propagating form measured 7-10 % slower (bench.py medians of 3 alternating runs per build: "
             "advection 2-D 147.4 k -> 133.0 k, --residual euler 2-D 67.7 k -> 61.6 k, sphere3d_4.6M 45.6 k -> 42.2 k "
             "Mcells*iters/s; DESIGN section 5)")


def _closure_forms(c):
    """(form, device residual, float64 reference) of both closures on the case's field, NaN cell included."""
    Q64 = c.Q.astype(f64)
    for visc, fused in ((True, True), (True, False), (False, None)):
        ref = c.ref(f"nan{visc}", lambda: pc.oracle_wa_residual(c.op, Q64, NU, viscous=visc))
        dQ = ibamd.hip(c.Q)
        got = _h(closures.navier_stokes_wray_agarwal_residual(c.dpart, dQ, nu=float(NU), fused_viscous=fused) if visc
                 else closures.euler_wray_agarwal_residual(c.dpart, dQ, nu=float(NU)))
        yield f"navier_stokes fused_viscous={fused}" if visc else "euler", got, ref, visc


def _nan_cases(cases, hierarchy):
    out = [cases["3d ball"], hierarchy["3d level1"]]
    assert all(np.isnan(c.Q).any() for c in out)
    return out


def test_closures_nan_cell_turbulence_row(cases, hierarchy):
    """The R row of both closures around a NaN temperature: Julia's NaN pattern exactly, the bound elsewhere."""
    for c in _nan_cases(cases, hierarchy):
        for form, got, ref, visc in _closure_forms(c):
            sc = c.ref(f"nans{visc}", lambda: pc.closure_scale(c.op, c.Q, ref, NU, viscous=visc))
            c.check(f"closure (NaN cell) {form}: R row", got[:, c.nvp], ref[:, c.nvp], sc[:, c.nvp], pc.BOUND_CLOSURE)


@pytest.mark.xfail(strict=True, raises=AssertionError, reason=SWEEP_NAN)
def test_closures_nan_cell_euler_rows(cases, hierarchy):
    """The Euler rows around a NaN temperature: finite where the reference is NaN (never the other way round), on every
    closure form.  Anything else is a real failure (RuntimeError), not the expected one."""
    seen = []
    for c in _nan_cases(cases, hierarchy):
        for form, got, ref, visc in _closure_forms(c):
            g, r = got[:, :c.nvp], ref[:, :c.nvp]
            if (np.isnan(g) & ~np.isnan(r)).any():
                raise RuntimeError(f"{form}: NaN in the Euler rows where the reference has none")
            seen.append(int((np.isnan(r) & ~np.isnan(g)).sum()))
    assert min(seen) == 0, f"finite where Julia has NaN on every form: {seen} entries"


@pytest.mark.xfail(strict=True, raises=AssertionError, reason="inviscid_fluxes shares ibh_flux.h with the sweeps: " + SWEEP_NAN)
def test_inviscid_fluxes_nan_temperature():
    """HLL and sensor forms with NaN / -Inf temperatures: Julia's NaN pattern (the clamp in ibh_flux.h loses the NaN)."""
    fl, ofl = cfd.Fluid(), ocfd.Fluid()
    rng = np.random.default_rng(4)
    n = 64
    P = np.stack([1e5 * (1 + 0.05 * rng.uniform(-1, 1, n)), 288 * (1 + 0.05 * rng.uniform(-1, 1, n)),
                  30 * rng.uniform(-1, 1, n), 30 * rng.uniform(-1, 1, n)], axis=1).astype(f32)
    P[:4, 1] = [np.nan, -np.inf, np.nan, 5.0]
    PR = P[::-1].copy()
    nuL, nuR = rng.uniform(0, 1, n).astype(f32), rng.uniform(0, 1, n).astype(f32)
    bad = {}
    with np.errstate(all="ignore"):
        for d in (1, 2):
            got = _h(cfd.inviscid_fluxes(fl, ibamd.hip(P), ibamd.hip(PR), d))
            ref = ocfd.inviscid_fluxes(ofl, P.astype(f64), PR.astype(f64), d)
            bad[f"hll {d}"] = int((np.isnan(got) != np.isnan(ref)).sum())
            got = _h(cfd.inviscid_fluxes(fl, ibamd.hip(P), ibamd.hip(PR), ibamd.hip(nuL), ibamd.hip(nuR), d))
            ref = ocfd.inviscid_fluxes_sensor(ofl, P.astype(f64), PR.astype(f64), nuL.astype(f64), nuR.astype(f64), d)
            bad[f"sensor {d}"] = int((np.isnan(got) != np.isnan(ref)).sum())
    assert not any(bad.values()), bad


# ---------------------------------------------------------------------------------------------------------------------
# pointwise physics: edges and NaN semantics
# ---------------------------------------------------------------------------------------------------------------------
T_EDGES = f32([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-30, 9.999999, 10.0, 10.000001, 1.0, 50.0, 150.0, 288.15, 1000.0,
               3000.0, 1e4, 3e4, 1e5])


def _ulps(got, ref):
    from ew_model import ulp_distance
    g, r = np.asarray(got, f32), np.asarray(np.asarray(ref, f64).astype(f32))
    assert np.array_equal(np.isnan(g), np.isnan(r)), (g, r)
    return int(ulp_distance(g, r).max())


def test_inviscid_fluxes_wave_speed_edges():
    """Pointwise ``inviscid_fluxes`` where the clamps of SR = min(uR - aR, 0) and SL = max(uL + aL, 0) bind or nearly do:
    both sides supersonic to the right (F = FL) and to the left (F = FR), uR - aR and uL + aL one Float32 step either side
    of 0 (the flux is continuous there, so the device's own rounding of a may fall on either side), both sides at rest,
    and the clear 0 / 0 (uL = -3 a, uR = +3 a: SL = SR = 0), NaN in every variable in the float64 oracle and on the
    device alike.  Magnitude scale and bound of ``test_pointwise_edges``."""
    fl, ofl = cfd.Fluid(), ocfd.Fluid()
    TL, TR, pL, pR = f32(300.0), f32(280.0), f32(1.1e5), f32(0.9e5)
    aL, aR = (f32(np.sqrt(f64(ofl.gamma) * f64(ofl.R) * f64(T))) for T in (TL, TR))
    up, dn = (lambda v: np.nextafter(f32(v), f32(np.inf))), (lambda v: np.nextafter(f32(v), f32(-np.inf)))
    # (uL, uR) along the flux direction; the other component is 20 / -15
    rows = {"supersonic right": (2 * aL, 3 * aR), "supersonic left": (-3 * aL, -2 * aR),
            "uR - aR = +1 step": (f32(50.0), up(aR)), "uR - aR = 0": (f32(50.0), aR), "uR - aR = -1 step": (f32(50.0), dn(aR)),
            "uL + aL = +1 step": (up(-aL), f32(-50.0)), "uL + aL = 0": (-aL, f32(-50.0)),
            "uL + aL = -1 step": (dn(-aL), f32(-50.0)), "at rest": (f32(0.0), f32(0.0)), "0/0": (-3 * aL, 3 * aR)}
    names = list(rows)
    for d in (1, 2):
        PL = np.array([[pL, TL, 20.0, -15.0]] * len(rows), f32)
        PR = np.array([[pR, TR, 20.0, -15.0]] * len(rows), f32)
        PL[:, 1 + d] = [rows[k][0] for k in names]
        PR[:, 1 + d] = [rows[k][1] for k in names]
        PL[names.index("at rest"), 2:] = 0
        PR[names.index("at rest"), 2:] = 0
        got = _h(cfd.inviscid_fluxes(fl, ibamd.hip(PL), ibamd.hip(PR), d))
        L, Rr = PL.astype(f64), PR.astype(f64)
        with np.errstate(all="ignore"):
            ref = ocfd.inviscid_fluxes(ofl, L, Rr, d)
        nan = names.index("0/0")
        assert np.isnan(ref[nan]).all() and np.isfinite(np.delete(ref, nan, axis=0)).all()
        assert np.allclose(ref[0], ocfd.inviscid_fluxes(ofl, L[:1], L[:1], d)[0], rtol=1e-14, atol=0)        # F = FL
        assert np.allclose(ref[1], ocfd.inviscid_fluxes(ofl, Rr[1:2], Rr[1:2], d)[0], rtol=1e-14, atol=0)    # F = FR
        assert np.array_equal(np.isnan(got), np.isnan(ref)), (d, got, ref)
        sc = np.abs(ref)
        for X in (L, Rr):
            sc = sc + np.abs(ocfd.inviscid_fluxes(ofl, X, X, d)) + \
                ((ocfd.speed_of_sound(ofl, X[:, 1]) + np.abs(X[:, 1 + d]))[:, None] * np.abs(ocfd.primitive2state(ofl, X)))
        fin = np.arange(len(rows)) != nan
        # at rest the transverse momentum row has scale 0: the flux must be exactly 0 there (percell_error: 0, else inf)
        err = pc.percell_error(got[fin], ref[fin], sc[fin])
        worst = int(np.argmax(err.max(axis=1)))
        e = float(err.max())
        _record("pointwise inviscid_fluxes, wave-speed edges (per-element, magnitude scale)", e)
        assert e <= pc.BOUND_EULER, (d, np.array(names)[fin][worst], e, got[fin][worst], ref[fin][worst])


def test_pointwise_edges():
    """Per element against the float64 oracle: finite values within a few ulps, NaN exactly where Julia has NaN."""
    fl, ofl = cfd.Fluid(), ocfd.Fluid()
    rng = np.random.default_rng(3)
    Tv = np.concatenate([T_EDGES, np.linspace(10, 1e5, 4000, dtype=f32), rng.uniform(10, 400, 4000).astype(f32)])
    dT = ibamd.hip(Tv)
    T64 = Tv.astype(f64)
    u = {}
    with np.errstate(all="ignore"):
        u["speed_of_sound"] = _ulps(_h(cfd.speed_of_sound(fl, dT)), ocfd.speed_of_sound(ofl, T64))
        u["dynamic_viscosity"] = _ulps(_h(cfd.dynamic_viscosity(fl, dT)), ocfd.dynamic_viscosity(ofl, T64))
        u["heat_conductivity"] = _ulps(_h(cfd.heat_conductivity(fl, dT)), ocfd.heat_conductivity(ofl, T64))
        n = Tv.size
        P = np.stack([1e5 * (1 + 0.05 * rng.uniform(-1, 1, n)), Tv, 30 * rng.uniform(-1, 1, n),
                      30 * rng.uniform(-1, 1, n)], axis=1).astype(f32)
        P[:3, 0] = [np.nan, np.inf, 0.0]
        u["primitive2state"] = _ulps(_h(cfd.primitive2state(fl, ibamd.hip(P))), ocfd.primitive2state(ofl, P.astype(f64)))
        Qs = ocfd.primitive2state(ofl, np.where(np.isfinite(P), P, 300).astype(f32))
        Qs[:4, 1] = [np.nan, -1.0, 0.0, np.inf]
        u["state2primitive"] = _ulps(_h(cfd.state2primitive(fl, ibamd.hip(Qs))), ocfd.state2primitive(ofl, Qs.astype(f64)))
        PR = P[::-1].copy()
        for d in (1, 2):
            got = _h(cfd.inviscid_fluxes(fl, ibamd.hip(P), ibamd.hip(PR), d))
            fin = np.isfinite(P).all(axis=1) & np.isfinite(PR).all(axis=1)
            L, Rr = P[fin].astype(f64), PR[fin].astype(f64)
            ref = ocfd.inviscid_fluxes(ofl, L, Rr, d)
            # HLL cancels: per element on the magnitudes it combines, |F(P)| + (a + |u|) |U(P)| of both sides
            sc = np.abs(ref)
            for X in (L, Rr):
                sc = sc + np.abs(ocfd.inviscid_fluxes(ofl, X, X, d)) + \
                    ((ocfd.speed_of_sound(ofl, X[:, 1]) + np.abs(X[:, 1 + d]))[:, None] * np.abs(ocfd.primitive2state(ofl, X)))
            assert np.isfinite(got[fin]).all()
            e = float((np.abs(got[fin] - ref) / sc).max())
            _record("pointwise inviscid_fluxes (per-element, magnitude scale)", e)
            assert e <= pc.BOUND_EULER, e
        G = [rng.uniform(-100, 100, P.shape).astype(f32) for _ in range(2)]
        mt = np.abs(rng.uniform(0, 1e-4, n)).astype(f32)
        mt[:50] = 0
        for d in (1, 2):
            got = _h(cfd.viscous_fluxes(fl, ibamd.hip(P), tuple(ibamd.hip(g) for g in G), d, mu_t=ibamd.hip(mt)))
            ref = ocfd.viscous_fluxes(ofl, P.astype(f64), [g.astype(f64) for g in G], d, mu_t=mt.astype(f64))
            assert np.array_equal(np.isnan(got), np.isnan(ref)), d
            sc = pc.abs_viscous_fluxes(ofl, np.abs(P.astype(f64)), [np.abs(g.astype(f64)) for g in G], d,
                                       mt.astype(f64)) + np.abs(ref)
            fin = np.isfinite(ref)
            e = float((np.abs(got[fin] - ref[fin]) / np.where(sc[fin] > 0, sc[fin], 1)).max())
            _record("pointwise viscous_fluxes (per-element, magnitude scale)", e)
            assert e <= pc.BOUND_VISCOUS, e
        # wall function and Wray-Agarwal
        y = rng.uniform(1e-5, 1e-2, n).astype(f32)
        uu = rng.uniform(0, 100, n).astype(f32)
        nu = rng.uniform(1e-5, 2e-5, n).astype(f32)
        uu[:4] = [np.nan, np.inf, 0.0, -5.0]
        wg = T.wall_function(ibamd.hip(y), ibamd.hip(uu), ibamd.hip(nu))
        wr = ot.wall_function(y.astype(f64), uu.astype(f64), nu.astype(f64))
        for k in ("nut", "du_dn"):
            g, r = _h(wg[k]), np.asarray(wr[k])
            assert np.array_equal(np.isnan(g), np.isnan(r)), (k, g[:4], r[:4])
            u[f"wall_function {k}"] = _ulps(g[4:], r[4:])
        Rw = rng.uniform(0, 1e-4, n).astype(f32)
        Sw = rng.uniform(0, 1e3, n).astype(f32)
        gR = rng.uniform(-1, 1, (n, 2)).astype(f32)
        gS = rng.uniform(-1, 1, (n, 2)).astype(f32)
        Rw[:3] = [np.nan, 1e-5, 1e-5]
        Sw[:3] = [1.0, np.nan, np.inf]
        wag = T.Wray_Agarwal(ibamd.hip(Rw), ibamd.hip(Sw), ibamd.hip(gR), ibamd.hip(gS))
        war = ot.Wray_Agarwal(Rw.astype(f64), Sw.astype(f64), gR.astype(f64), gS.astype(f64))
        for k in ("nut", "nuR"):
            u[f"Wray_Agarwal {k}"] = _ulps(_h(wag[k]), war[k])
        g, r = _h(wag["S"]), war["S"]
        assert np.array_equal(np.isnan(g), np.isnan(r)), "Wray_Agarwal S"
        # the source cancels in grad R . grad S: per element on the magnitudes it sums
        R64, S64 = Rw.astype(f64), Sw.astype(f64)
        C1, C2 = f64(f32(0.0829)), f64(f32(0.72) + f32(0.0829) / f32(0.41) ** 2)
        with np.errstate(all="ignore"):
            sc = np.abs(r) + C1 * np.abs(R64) * np.abs(S64) + \
                C2 * (np.abs(gR) * np.abs(gS)).sum(axis=1) * np.abs(R64) / (np.abs(S64) + f64(ot.EPS)) + 10 * np.abs(R64)
        fin = np.isfinite(r) & np.isfinite(sc)
        assert np.array_equal(g[~np.isfinite(r) & ~np.isnan(r)], r[~np.isfinite(r) & ~np.isnan(r)])
        e = float((np.abs(g[fin] - r[fin]) / sc[fin]).max())
        _record("pointwise Wray_Agarwal S (per-element, magnitude scale)", e)
        assert e <= pc.BOUND_TURB, e
        # FlowBC: NaN / Inf temperature (NaN Mach number: pb = 0) and pressure at the image point
        nrm = np.tile(f32([[1.0, 0.0]]), (n, 1))
        for bc, obc in ((cfd.FlowBC(fl, [1e5, 288.15, 100.0, 0.0]), ocfd.FlowBC(ofl, f32([1e5, 288.15, 100.0, 0.0]))),
                        (cfd.FlowBC(fl, [1e5, 288.15, 0.0], normal_flow=True),
                         ocfd.FlowBC(ofl, f32([1e5, 288.15, 0.0]), normal_flow=True))):
            # every row, NaN / Inf temperatures and pressures included: the kernel's Bool weights are Julia's strong zeros
            g = _h(bc(ibamd.hip(P), ibamd.hip(nrm)))
            r = np.asarray(obc(P.astype(f64), nrm.astype(f64)))
            u["FlowBC"] = max(u.get("FlowBC", 0), _ulps(g, r))
    print("\npointwise: max ulps against float64", u)
    for k, v in u.items():
        _record(f"pointwise {k} (ulps)", float(v))
    assert u["speed_of_sound"] <= 2 and u["heat_conductivity"] <= 4
    assert u["dynamic_viscosity"] <= 16          # the exp2 / log2 power over T in [10, 1e5] K (csrc/ibh_cfd.hip)
    assert u["primitive2state"] <= 8 and u["state2primitive"] <= 64
    assert all(v <= 64 for k, v in u.items() if k.startswith(("wall_function", "FlowBC")))
    assert u["Wray_Agarwal nut"] == 0 and u["Wray_Agarwal nuR"] <= 1

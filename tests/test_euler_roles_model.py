"""Cell roles in the Euler march without a device: ``ibamd.cell_roles`` against the numpy model (tests/euler_roles_model.py)
and against the geometry of the bodies, the masked transfers of the model against ``euler_mg_model``'s, the convergence of
the cycle with roles in the model -- the rehearsal of tests/test_gpu_euler_roles.py -- the exports, and every argument check
that comes before a launch.  No GPU."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

import euler_mg_model as mg
import euler_roles_model as rm
import ibamd
import regimes as rg
from abi import assert_bound, header_text
from conftest import ADV_FAMILIES, GOLDEN, RAE_FAMILIES, oracle_boundaries_view, oracle_view
from ibamd import _lib
from ibamd import backend as B
from ibamd import solver
from ibamd.solver import DualTimeMarch, EulerMarch, MultigridMarch, rk_stages
from oracle import cfd as ocfd
from oracle import domain as od
from test_euler_mg_model import Args as TransferArgs
from test_euler_mg_model import conv_far
from test_julia_binding import header_prototypes, julia_ccalls

f32, f64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ibh_restrict_euler_roles", "ibh_forcing_roles", "ibh_sumsq_roles")
RAE_COUNTS = [(33374, 1976, 1770), (8034, 958, 288), (1859, 457, 4)]      # (fluid, ghost, solid) per level


@pytest.fixture(scope="module")
def rae(rae_mesh_small):
    return mg.hierarchy(rae_mesh_small, 2, hypercube_families=RAE_FAMILIES)


@pytest.fixture(scope="module")
def rae_roles(rae):
    return [ibamd.cell_roles(d) for d in rae[0]]


@pytest.fixture(scope="module")
def adv(adv_mesh_coarse):
    return mg.hierarchy(adv_mesh_coarse, 2, hypercube_families=ADV_FAMILIES)


def inside_polygon(poly, X):
    """Ray casting: is ``X[i]`` inside the closed polygon ``poly`` (``(m, 2)``, last vertex joined to the first)?  A ray
    towards +x crosses an edge whose ends lie on either side of the point's y, left of the crossing."""
    x, y = X[:, 0].astype(f64)[:, None], X[:, 1].astype(f64)[:, None]
    x0, y0 = poly[:, 0][None, :], poly[:, 1][None, :]
    x1, y1 = np.roll(poly[:, 0], -1)[None, :], np.roll(poly[:, 1], -1)[None, :]
    straddle = (y0 > y) != (y1 > y)
    with np.errstate(all="ignore"):
        xc = x0 + (y - y0) * (x1 - x0) / (y1 - y0)
    return (np.count_nonzero(straddle & (x < xc), axis=1) % 2) == 1


# ---------------------------------------------------------------------------------------------------------------------
# the roles
# ---------------------------------------------------------------------------------------------------------------------
def test_role_counts_on_the_airfoil(rae, rae_roles):
    """The three levels of ``rae_mesh_small``: the counts of the flood fill, the product's labels equal to the model's frontier
    sweeps, ghost rows exactly the boundaries', and the partition-local form."""
    doms = rae[0]
    assert [len(d) for d in doms] == [37120, 9280, 2320]
    for dom, roles, counts in zip(doms, rae_roles, RAE_COUNTS):
        assert roles.dtype == np.uint8 and roles.shape == (len(dom),)
        assert tuple(np.bincount(roles, minlength=3)) == counts
        assert np.array_equal(roles, rm.cell_roles(dom))
        ghosts = np.unique(np.concatenate([b.ghost_indices for parts in dom.boundaries.values() for b in parts.values()]))
        assert np.array_equal(np.nonzero(roles == ibamd.ROLE_GHOST)[0], ghosts)
        part = mg.part_of(dom)
        assert np.array_equal(roles[part.domain], roles)            # one partition, in global order
    assert (ibamd.ROLE_FLUID, ibamd.ROLE_GHOST, ibamd.ROLE_SOLID) == (0, 1, 2) == (rm.FLUID, rm.GHOST, rm.SOLID)


def test_solid_rows_lie_inside_the_airfoil(rae, rae_roles):
    """On every level no fluid centre lies inside the polygon of tests/golden/rae2822.dat and no solid centre outside it."""
    poly = np.loadtxt(os.path.join(GOLDEN, "rae2822.dat"), dtype=f64)
    for dom, roles in zip(rae[0], rae_roles):
        inside = inside_polygon(poly, dom.global_centers())
        assert not inside[roles == ibamd.ROLE_FLUID].any()
        assert inside[roles == ibamd.ROLE_SOLID].all()
        assert inside.sum() > (roles == ibamd.ROLE_SOLID).sum()      # (ghost rows lie on both sides of the wall)


def test_seed_and_partitions(rae, rae_roles, rae_domains):
    """A seed in the far field gives the default; a seed inside the airfoil makes that pocket the fluid; a ghost seed and a
    seed out of range raise.  The same mesh in three partitions gives the same roles: the graph is every partition's."""
    dom, roles = rae[0][0], rae_roles[0]
    fluid, solid, ghost = (int(np.nonzero(roles == k)[0][0]) for k in (0, 2, 1))
    assert np.array_equal(ibamd.cell_roles(dom, fluid_seed=fluid), roles)
    assert np.array_equal(rm.cell_roles(dom, fluid_seed=fluid), roles)
    swapped = ibamd.cell_roles(dom, fluid_seed=solid)
    assert swapped[solid] == 0 and swapped[fluid] == 2 and np.array_equal(swapped == 1, roles == 1)
    assert 0 < (swapped == 0).sum() <= RAE_COUNTS[0][2]
    assert np.array_equal(swapped, rm.cell_roles(dom, fluid_seed=solid))
    with pytest.raises(ValueError, match="ghost"):
        ibamd.cell_roles(dom, fluid_seed=ghost)
    with pytest.raises(ValueError, match="fluid_seed"):
        ibamd.cell_roles(dom, fluid_seed=len(dom))
    split = rae_domains[0]
    assert len(split.partitions) == 3
    assert np.array_equal(ibamd.cell_roles(split), roles)


def test_open_walls_have_no_solid_rows(adv):
    """``adv_mesh_coarse`` has only open walls -- nothing is cut off from the fluid -- so every level has zero solid rows."""
    for dom in adv[0]:
        roles = ibamd.cell_roles(dom)
        assert (roles == ibamd.ROLE_SOLID).sum() == 0 and (roles == ibamd.ROLE_GHOST).sum() > 0
        assert np.array_equal(roles, rm.cell_roles(dom))


def test_a_sphere_in_three_dimensions():
    """The immersed sphere of tests/test_3d.py (radius 1, 4 096 cells, blocks of 4^3): every solid centre lies inside the
    sphere and every fluid centre outside it; product and model agree."""
    from ibamd.mesher import Mesh
    from test_3d import icosphere
    msh = Mesh(f32([-2, -2, -2]), f32([4, 4, 4]), ("sphere", icosphere(1.0, subdiv=2), f32(0.25)), block_size=4)
    dom = ibamd.Domain(msh, max_partition_size=10 ** 9)
    roles = ibamd.cell_roles(dom)
    r = np.linalg.norm(dom.global_centers().astype(f64), axis=1)
    counts = np.bincount(roles, minlength=3)
    print(f"sphere: (fluid, ghost, solid) = {tuple(counts)}; solid r <= {r[roles == 2].max():.3f}, fluid r >= {r[roles == 0].min():.3f}")
    assert counts.sum() == len(dom) == 4096 and (counts > 0).all()
    assert (r[roles == ibamd.ROLE_SOLID] < 1.0).all() and (r[roles == ibamd.ROLE_FLUID] > 1.0).all()
    assert np.array_equal(roles, rm.cell_roles(dom))


# ---------------------------------------------------------------------------------------------------------------------
# the masked transfers of the model
# ---------------------------------------------------------------------------------------------------------------------
def test_all_fluid_roles_are_the_plain_transfers(adv):
    """With every row fluid the model's masked restriction and forcing equal ``euler_mg_model``'s bit for bit."""
    doms, coarseners, _ = adv
    fine = mg.part_of(doms[0])
    P = rg.euler_regime(fine, "transonic")
    rng = np.random.default_rng(3)
    R, S = (rng.normal(size=P.shape).astype(f32) for _ in range(2))
    nf, nk = coarseners[0].n_input, coarseners[0].n_output
    for Sx in (S, None):
        ref_P, ref_D = mg.restrict(coarseners[0], P, R, Sx)
        got_P, got_D = rm.restrict(coarseners[0], P, R, Sx, np.zeros(nf, np.uint8))
        assert got_P.tobytes() == ref_P.tobytes() and got_D.tobytes() == ref_D.tobytes()
    Rc = rng.normal(size=ref_D.shape).astype(f32)
    assert rm.forcing(ref_D, Rc, np.zeros(nk, np.uint8)).tobytes() == (ref_D - Rc).tobytes()


def test_masked_rows_never_reach_the_defect(adv):
    """NaN in the ghost and solid rows of ``R`` and ``S``: the masked defect is that of the arrays with zeros there, ``P_c`` is
    the plain one, the forcing is zero outside the coarse fluid rows, and the norm takes the fluid rows alone."""
    doms, coarseners, _ = adv
    P = rg.euler_regime(mg.part_of(doms[0]), "transonic")
    rng = np.random.default_rng(4)
    nf, nk = coarseners[0].n_input, coarseners[0].n_output
    roles, roles_c = rng.integers(0, 3, nf).astype(np.uint8), rng.integers(0, 3, nk).astype(np.uint8)
    R, S = (rng.normal(size=P.shape).astype(f32) for _ in range(2))
    Rn, Sn = R.copy(), S.copy()
    Rn[roles != 0] = np.nan
    Sn[roles == 2] = np.nan
    got_P, got_D = rm.restrict(coarseners[0], P, Rn, Sn, roles)
    ref_P, ref_D = mg.restrict(coarseners[0], P, np.where((roles == 0)[:, None], R + S, f32(0)), None)
    assert got_P.tobytes() == ref_P.tobytes() == mg.restrict(coarseners[0], P, R, S)[0].tobytes()
    assert got_D.tobytes() == ref_D.tobytes() and np.isfinite(got_D).all()
    Rc = rng.normal(size=got_D.shape).astype(f32)
    Rc[roles_c != 0] = np.nan
    Sc = rm.forcing(got_D, Rc, roles_c)
    assert np.isfinite(Sc).all() and not Sc[roles_c != 0].any() and not np.signbit(Sc[roles_c != 0]).any()
    assert np.array_equal(Sc[roles_c == 0], (got_D - Rc)[roles_c == 0])
    assert np.array_equal(rm.sumsq(Rn, roles), (R[roles == 0].astype(f64) ** 2).sum(axis=0))
    assert np.array_equal(rm.sumsq(Rn, np.full(nf, 2, np.uint8)), np.zeros(4))


# ---------------------------------------------------------------------------------------------------------------------
# convergence: the rehearsal of tests/test_gpu_euler_roles.py::test_convergence
# ---------------------------------------------------------------------------------------------------------------------
CONV = dict(scale=0.3, cycles=40, stages=3, pre=1, post=1, n_coarsest=2, mach=0.5, ratio=0.9)


def conv_single_grid_steps():
    """The whole single-grid steps within the cycles' fine sweeps: 40 cycles of ``(pre + post) stages + 1 = 7`` sweeps are
    280 sweeps, 93 steps of 3 (the single grid's norm is still climbing there: the 94th step would raise it)."""
    return CONV["cycles"] * ((CONV["pre"] + CONV["post"]) * CONV["stages"] + 1) // CONV["stages"]


def test_convergence_in_the_model(rae, rae_roles):
    """``rae_mesh_small`` as one partition at Mach 0.5 and zero incidence from the free stream, far field and slip wall on every
    level, ``rk_stages(3)``, per-cell time steps at ``scale`` 0.3, ``pre = post = 1``, ``n_coarsest = 2``: 40 V-cycles with roles
    (solid rows held at the free stream) against the single grid's 280 fine sweeps (93 whole steps).  Both end finite and
    the cycles' ``||R_rho||_2`` over the fluid rows is at most 0.9 times the single grid's.

    Float32 model: cycles 4.763e4 (history peak 5.85e4), single grid 5.942e4 (5.953e4 after 94 steps): ratio 0.80.  The
    single grid with the same blanking gives 5.944e4 (5.955e4 after 94 steps): blanking alone does not change its stall.
    The plain cycles of ``euler_mg_model`` -- no roles -- are non-finite from cycle 22 on (recorded, not asserted: 25 s more)."""
    doms, coarseners, prolongators = rae
    fl, far = ocfd.Fluid(), conv_far()
    free, wall = ocfd.FlowBC(fl, far), ocfd.FlowBC(fl, f32([far[0], far[1], 0.0]), normal_flow=True)

    def bcs_of(dom):
        view = oracle_boundaries_view(dom)

        def bcs(P):
            od.impose_bc(lambda b, Pi: free(Pi, b.normals), view, "farfield", P)
            od.impose_bc(lambda b, Pi: wall(Pi, b.normals), view, "wall", P)
        return bcs
    levels = [rm.level(oracle_view(mg.part_of(d)), bcs_of(d), r, far) for d, r in zip(doms, rae_roles)]
    single = mg.level(levels[0].op, bcs_of(doms[0]))
    stages = rk_stages(CONV["stages"])
    start = np.tile(far, (len(doms[0]), 1))
    single.bcs(start)
    P, hist = start.copy(), []
    levels[0].bcs(P)
    for _ in range(CONV["cycles"]):
        P = rm.cycle(levels, coarseners, prolongators, P, stages=stages, scale=CONV["scale"], pre=CONV["pre"],
                     post=CONV["post"], n_coarsest=CONV["n_coarsest"], dtype=f32, history=hist)
    Ps = start
    for _ in range(conv_single_grid_steps()):
        Ps = mg.smooth(single, Ps, None, 0.0, stages, CONV["scale"], f32)

    def norm(X):
        return float(np.sqrt(rm.sumsq(mg.residual(single, X, f32), rae_roles[0])[0]))
    n_mg, n_sg = norm(P), norm(Ps)
    print(f"{CONV['cycles']} cycles with roles: fluid-row ||R_rho|| {n_mg:.4g} (history peak {np.sqrt(max(h[0] for h in hist)):.4g}), "
          f"single grid after {conv_single_grid_steps()} steps {n_sg:.4g}: ratio {n_mg / n_sg:.3f}")
    assert conv_single_grid_steps() == 93 and len(hist) == CONV["cycles"] and hist[0].shape == (4,)
    assert np.isfinite(P).all() and np.isfinite(Ps).all()
    assert (P[rae_roles[0] == 2] == far).all()
    assert n_mg <= CONV["ratio"] * n_sg


# ---------------------------------------------------------------------------------------------------------------------
# exports and the checks before any launch
# ---------------------------------------------------------------------------------------------------------------------
def test_exported_bound_and_named_by_the_julia_binding():
    assert_bound(NAMES)
    hdr = header_text()
    protos, calls = header_prototypes(), {c[0]: c for c in julia_ccalls()}
    for name in NAMES:
        assert name in calls, f"julia/IBHip.jl does not ccall {name}"
        assert calls[name][1] == protos[name][0] and calls[name][2] == protos[name][1], name
    assert protos["ibh_restrict_euler_roles"][1] == protos["ibh_restrict_euler"][1][:9] + ["ptr"] + protos["ibh_restrict_euler"][1][9:]
    assert protos["ibh_forcing_roles"][1] == ["i64", "i32", "ptr", "i64", "ptr", "i64", "ptr"]
    assert protos["ibh_sumsq_roles"][1] == ["i64", "i32", "ptr", "i64", "ptr", "ptr"]
    assert [int(re.search(rf"#define IBH_ROLE_{k}\s+(\d+)", hdr).group(1)) for k in ("FLUID", "GHOST", "SOLID")] == [0, 1, 2]
    src = open(os.path.join(ROOT, "julia", "IBHip.jl")).read()
    for fn in ("restrict_euler_roles!", "forcing_roles!", "sumsq_roles!"):
        assert re.search(r"^function " + re.escape(fn) + r"\(", src, re.M), fn
    from ibamd import cfd
    for name in ("forcing_roles", "sumsq_roles", "restrict_euler"):
        assert getattr(ibamd, name) is getattr(B, name) is getattr(cfd, name)
    from ibamd import domain
    assert ibamd.cell_roles is domain.cell_roles and ibamd.Roles is B.Roles


class Args(TransferArgs):
    """``test_euler_mg_model.Args`` with a role byte per fine row and the argument lists of the three entries."""

    def __init__(self):
        super().__init__()
        self.bufs["roles"] = (C.c_float * 1024)()
        self.bufs["out"] = (C.c_float * 1024)()

    def restrict_roles(self, **o):
        d = dict(acc=C.addressof(self.coa), f=C.pointer(self.fluid), nd=2, P=self.addr("P"), ldp=self.NF, R=self.addr("R"),
                 ldr=self.NF, S=self.addr("S"), lds=self.NF, roles=self.addr("roles"), Pc=self.addr("Pc"), ldpc=self.NK,
                 D=self.addr("D"), ldd=self.NK)
        return list({**d, **self.resolve(o)}.values())

    def forcing(self, **o):
        d = dict(n=self.NK, nv=4, D=self.addr("D"), ldd=self.NK, R=self.addr("R"), ldr=self.NK, roles=self.addr("roles"))
        return list({**d, **self.resolve(o)}.values())

    def sumsq(self, **o):
        d = dict(n=self.NF, nv=4, x=self.addr("R"), ldx=self.NF, roles=self.addr("roles"), out=self.addr("out"))
        return list({**d, **self.resolve(o)}.values())


RESTRICT = ([(dict([(k, None)]), b"null") for k in ("acc", "f", "P", "R", "roles", "Pc", "D")]
            + [(dict(nd=1), b"nd must be 2 or 3"), (dict(nd=4), b"nd must be 2 or 3")]
            + [(dict([(k, 39)]), b"leading dimension") for k in ("ldp", "ldr", "lds")]
            + [(dict([(k, 9)]), b"leading dimension") for k in ("ldpc", "ldd")]
            + [(dict(D="Pc"), b"D_c may not alias P_c"), (dict(D=("Pc", 39)), b"D_c may not alias P_c")]
            + [(dict([(k, v)]), b"may not alias P_f, R_f or S_f") for k in ("Pc", "D") for v in ("P", "R", "S", ("P", 159))]
            + [(dict([(k, v)]), b"may not alias roles_f") for k in ("Pc", "D") for v in ("roles", ("roles", 9))])
FORCING = ([(dict([(k, None)]), b"null") for k in ("D", "R", "roles")]
           + [(dict(nv=0), b"nv in 1 .. 8"), (dict(nv=9), b"nv in 1 .. 8"), (dict(n=-1), b"n must be >= 0")]
           + [(dict(ldd=9), b"leading dimension"), (dict(ldr=9), b"leading dimension")]
           + [(dict(R="D"), b"may not alias"), (dict(R=("D", 39)), b"may not alias"), (dict(roles="D"), b"may not alias"),
              (dict(roles=("D", 9)), b"may not alias")])
SUMSQ = ([(dict([(k, None)]), b"null") for k in ("x", "roles", "out")]
         + [(dict(nv=0), b"nv in 1 .. 8"), (dict(nv=9), b"nv in 1 .. 8"), (dict(n=-1), b"n must be >= 0")]
         + [(dict(ldx=39), b"leading dimension")]
         + [(dict(out="R"), b"may not alias"), (dict(out=("R", 159)), b"may not alias"), (dict(out="roles"), b"may not alias"),
            (dict(out=("roles", 9)), b"may not alias")])


def _ids(cases):
    return ["_".join(f"{k}-{v}" for k, v in c.items()).replace(" ", "").replace("'", "") + f"_{i}" for i, (c, _) in enumerate(cases)]


def _misuse(entry, method, over, what):
    lib = _lib.load()
    a = Args()               # (alive across the call: the argument list holds addresses into it)
    rc = getattr(lib, entry)(*getattr(a, method)(**over))
    assert rc != 0 and what in lib.ibh_last_error() and entry.encode() + b":" in lib.ibh_last_error(), lib.ibh_last_error()


@pytest.mark.parametrize("over,what", RESTRICT, ids=_ids(RESTRICT))
def test_restrict_euler_roles_misuse(over, what):
    _misuse("ibh_restrict_euler_roles", "restrict_roles", over, what)


@pytest.mark.parametrize("over,what", FORCING, ids=_ids(FORCING))
def test_forcing_roles_misuse(over, what):
    _misuse("ibh_forcing_roles", "forcing", over, what)


@pytest.mark.parametrize("over,what", SUMSQ, ids=_ids(SUMSQ))
def test_sumsq_roles_misuse(over, what):
    _misuse("ibh_sumsq_roles", "sumsq", over, what)


def test_nothing_to_do_is_no_error():
    """Zero rows: valid arguments, nothing launched -- no device is needed to return."""
    lib = _lib.load()
    a = Args()
    a.coa.n_out = 0
    assert lib.ibh_restrict_euler_roles(*a.restrict_roles()) == 0
    assert lib.ibh_restrict_euler_roles(*a.restrict_roles(S=None, lds=0)) == 0
    assert lib.ibh_forcing_roles(*a.forcing(n=0)) == 0
    assert lib.ibh_sumsq_roles(*a.sumsq(n=0)) == 0


def test_roles_are_refused_before_the_device(monkeypatch):
    """Every refused argument raises before a partition, an array or a launch is asked for."""
    monkeypatch.setattr(B, "call", lambda name, *a: pytest.fail(f"{name} was called: the argument check did not stop it"))
    monkeypatch.setattr(B, "to_backend", lambda *a: pytest.fail("a partition was asked for before the arguments were checked"))
    monkeypatch.setattr(B, "_part", lambda *a: pytest.fail("a partition was asked for before the arguments were checked"))
    monkeypatch.setattr(B, "_dev", lambda *a: pytest.fail("the device was asked for before the arguments were checked"))
    part = types.SimpleNamespace(ndims=2, nc=10)
    far = [1e5, 288.15, 170.0, 0.0]
    with pytest.raises(ValueError, match=r"one value per cell of the partition, \(10,\)"):
        B.Roles(part, np.zeros(9, np.uint8), far)
    with pytest.raises(ValueError, match="one value per cell"):
        B.Roles(part, np.zeros((10, 1), np.uint8), far)
    with pytest.raises(ValueError, match="ROLE_FLUID"):
        B.Roles(part, np.full(10, 3, np.uint8), far)
    for bad in (far[:3], far + [0.0], [far]):
        with pytest.raises(ValueError, match="solid_state must be the nd \\+ 2 = 4 primitives"):
            B.Roles(part, np.zeros(10, np.uint8), bad)
    with pytest.raises(ValueError, match="solid_state must be the nd \\+ 2 = 5 primitives"):
        B.Roles(types.SimpleNamespace(ndims=3, nc=10), np.zeros(10, np.uint8), far)
    parts = [object(), object()]
    stand_in = object.__new__(B.Roles)
    with pytest.raises(ValueError, match="one Roles per level: 2 levels, 1 roles"):
        MultigridMarch(parts, [None], [None], roles=[stand_in])
    with pytest.raises(ValueError, match="one Roles per level: 2 levels, 3 roles"):
        MultigridMarch(parts, [None], [None], roles=[stand_in] * 3)
    with pytest.raises(ValueError, match="must be a backend.Roles"):
        MultigridMarch(parts, [None], [None], roles=[stand_in, None])
    with pytest.raises(ValueError, match="must be a backend.Roles"):
        MultigridMarch(parts, [None], [None], roles=[np.zeros(10, np.uint8)] * 2)
    for march in (lambda **kw: EulerMarch(object(), **kw), lambda **kw: DualTimeMarch(object(), 1e-3, 4, **kw)):
        with pytest.raises(ValueError, match="roles must be a backend.Roles"):
            march(roles=np.zeros(10, np.uint8))


def test_marches_without_roles_keep_their_signatures():
    """``roles`` is the last argument of every march and defaults to None: a call written before it reads as it did."""
    import inspect
    for cls in (EulerMarch, DualTimeMarch, MultigridMarch):
        params = list(inspect.signature(cls.__init__).parameters.values())
        assert params[-1].name == "roles" and params[-1].default is None
    assert list(inspect.signature(B.restrict_euler).parameters)[-1] == "roles"
    assert solver.EulerMarch.residual_norms is not None

"""The numpy model of multigrid for the Euler march (tests/euler_mg_model.py) and what can be said of ``ibh_restrict_euler``,
``ibh_prolong_euler`` and ``solver.MultigridMarch`` without a device: the algebra of the coarse forcing, the structure of the
coarseners the restriction rests on, its conservation, the fixed point and the convergence of the cycle in the model -- the
rehearsal of tests/test_gpu_euler_mg.py's cases -- the exports, and the argument checks that come before any launch.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import euler_mg_model as mg
import euler_step_model as em
import regimes as rg
from abi import assert_bound
from conftest import ADV_FAMILIES, RAE_FAMILIES, oracle_boundaries_view, oracle_view
from ibamd import _lib
from ibamd import backend as B
from ibamd import solver
from ibamd.solver import MultigridMarch, rk_stages, ssp_stages
from oracle import cfd as ocfd
from oracle import domain as od
from test_julia_binding import header_prototypes, julia_ccalls

f32, f64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ibh_restrict_euler", "ibh_prolong_euler")


@pytest.fixture(scope="module")
def adv(adv_mesh_coarse):
    return mg.hierarchy(adv_mesh_coarse, 2, hypercube_families=ADV_FAMILIES)


@pytest.fixture(scope="module")
def corner():
    return mg.hierarchy(mg.corner_mesh(), 1)


# ---------------------------------------------------------------------------------------------------------------------
# the operators and the algebra
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", ["adv", "corner"])
def test_coarsener_rows_are_the_children(mesh, adv, corner):
    """Every coarsener row of ``multigrid()`` has exactly 2^nd entries of weight 2^-nd and every fine cell appears exactly
    once: the restriction of a conserved variable is the volume average over the children.  Every row of both operators
    starts on a 16-byte boundary (the rows off it are the synthetic operator's of the GPU tests)."""
    doms, coarseners, prolongators = adv if mesh == "adv" else corner
    nd = doms[0].ndims
    for l, (c, p) in enumerate(zip(coarseners, prolongators)):
        assert (c.n_input, c.n_output) == (len(doms[l]), len(doms[l + 1])) == (p.n_output, p.n_input)
        assert (c.lengths == 2 ** nd).all() and (c.w == f32(0.5 ** nd)).all()
        assert np.array_equal(np.sort(c.idx), np.arange(c.n_input))
        assert (c.off[:-1] % 4 == 0).all() and (p.off[:-1] % 4 == 0).all()
        assert (p.lengths >= 1).all() and p.idx.max() < p.n_input
        fine, coarse = mg.part_of(doms[l]), mg.part_of(doms[l + 1])
        assert np.array_equal(fine.domain, np.arange(c.n_input)) and len(fine.image) == c.n_input   # one partition, in order
        vf, vc = fine.spacing.astype(f64).prod(axis=1), coarse.spacing.astype(f64).prod(axis=1)
        kids = c.idx.reshape(-1, 2 ** nd)
        assert np.array_equal(vf[kids].sum(axis=1), vc)                     # the children tile their parent


@pytest.mark.parametrize("mesh", ["adv", "corner"])
def test_restriction_conserves(mesh, adv, corner):
    """In float64 the restricted conserved state times the parent's volume is the sum over the children, row by row and so
    in total, and the restricted primitives are the primitives of that state."""
    doms, coarseners, _ = adv if mesh == "adv" else corner
    nd = doms[0].ndims
    fl = em.fluid_of(f64)
    fine, coarse = mg.part_of(doms[0]), mg.part_of(doms[1])
    P = rg.euler_regime(fine, "transonic").astype(f64)
    R = np.random.default_rng(3).normal(size=P.shape)
    Pc, D = mg.restrict(coarseners[0], P, R, None, f64)
    Q, Qc = ocfd.primitive2state(fl, P), ocfd.primitive2state(fl, Pc)
    kids = coarseners[0].idx.reshape(-1, 2 ** nd)
    for got, src in ((Qc, Q), (D, R)):
        assert np.allclose(got * 2 ** nd, src[kids].sum(axis=1), rtol=1e-13, atol=1e-13 * np.abs(src).max())
    vf, vc = fine.spacing.astype(f64).prod(axis=1), coarse.spacing.astype(f64).prod(axis=1)
    assert np.allclose((Qc * vc[:, None]).sum(axis=0), (Q * vf[:, None]).sum(axis=0), rtol=1e-12)


def test_forcing_algebra(adv):
    """``I(R_f + S_f - g Q_f) - (R_c - g Q_c) = D_c - R_c`` with ``Q_c = I Q_f``, to float64 rounding: ``g`` cancels."""
    doms, coarseners, _ = adv
    rng = np.random.default_rng(1)
    n, nc = coarseners[0].n_input, coarseners[0].n_output
    Rf, Sf, Qf, Rc = (rng.normal(size=(k, 4)) for k in (n, n, n, nc))
    g = 1.5 / 3e-4
    Qc = mg.apply(coarseners[0], Qf, f64)
    lhs = mg.apply(coarseners[0], Rf + Sf - g * Qf, f64) - (Rc - g * Qc)
    rhs = mg.apply(coarseners[0], Rf + Sf, f64) - Rc
    assert np.abs(lhs - rhs).max() <= 1e-15 * g * 8       # rounding of terms of size g |Q|
    assert np.abs(rhs).max() > 1.0


def test_float32_transfers_follow_the_float64_ones(adv):
    """The Float32 model of the two transfers stays within a few Float32 epsilons of the float64 one on each column's scale."""
    doms, coarseners, prolongators = adv
    fine, coarse = mg.part_of(doms[0]), mg.part_of(doms[1])
    P, Pn, Po = rg.euler_regime(fine, "transonic"), rg.euler_regime(coarse, "transonic"), rg.euler_regime(coarse, "transonic", 9)
    R = np.random.default_rng(3).normal(size=P.shape).astype(f32)
    for a, b in zip(mg.restrict(coarseners[0], P, R, R, f32) + (mg.prolong(prolongators[0], P, Pn, Po, f32),),
                    mg.restrict(coarseners[0], P, R, R, f64) + (mg.prolong(prolongators[0], P, Pn, Po, f64),)):
        assert a.dtype == f32 and b.dtype == f64
        assert (np.abs(a - b).max(axis=0) <= 32 * em.EPS32 * np.abs(b).max(axis=0)).all()


# ---------------------------------------------------------------------------------------------------------------------
# the cycle in the model: the rehearsal of the GPU cases
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stages,pre,post", [(1, 1, 1), (3, 1, 1), (1, 2, 0)], ids=["euler", "rk3", "pre2"])
def test_fixed_point_in_the_model(adv, stages, pre, post):
    """tests/test_gpu_euler_mg.py::test_fixed_point in the Float32 model: with ``S = -R(P)`` a cycle moves the transonic state
    by less than ``n e_v``, with ``S = 0`` by more."""
    doms, coarseners, prolongators = adv
    levels = [mg.level(oracle_view(mg.part_of(d))) for d in doms]
    P = rg.euler_regime(mg.part_of(doms[0]), "transonic")
    R = mg.residual(levels[0], P, f32)
    e, n = mg.round_trip_error(P), mg.round_trips(3, stages, pre, post, 2)
    kw = dict(stages=rk_stages(stages), scale=0.75, pre=pre, post=post, n_coarsest=2, dtype=f32)
    fixed = mg.cycle(levels, coarseners, prolongators, P, -R, 0.0, **kw)
    free = mg.cycle(levels, coarseners, prolongators, P, np.zeros_like(R), 0.0, **kw)
    moved, moved0 = (np.abs(x.astype(f64) - P).max(axis=0) for x in (fixed, free))
    print(f"stages={stages} pre={pre} post={post}: n = {n}, moved {moved / (n * e)} x n e_v with S = -R, {moved0 / (n * e)} with S = 0")
    assert (moved <= n * e).all() and (moved0 > n * e).all()


def test_one_level_cycle_is_the_plain_steps(adv):
    doms, _, _ = adv
    lv = mg.level(oracle_view(mg.part_of(doms[2])))
    P = rg.euler_regime(mg.part_of(doms[2]), "transonic")
    ref = P
    for _ in range(2):
        ref = mg.smooth(lv, ref, None, 0.0, rk_stages(3), 0.75, f32)
    assert np.array_equal(mg.cycle([lv], [], [], P, stages=rk_stages(3), n_coarsest=2), ref)


# ---------------------------------------------------------------------------------------------------------------------
# exports and the checks before any launch
# ---------------------------------------------------------------------------------------------------------------------
def test_exported_bound_and_named_by_the_julia_binding():
    assert_bound(NAMES)
    protos, calls = header_prototypes(), {c[0]: c for c in julia_ccalls()}
    for name in NAMES:
        assert name in calls and calls[name][1] == protos[name][0] and calls[name][2] == protos[name][1], name
    assert protos["ibh_restrict_euler"][1].count("ptr") == 7 and len(protos["ibh_restrict_euler"][1]) == 13
    assert protos["ibh_prolong_euler"][1].count("ptr") == 7 and len(protos["ibh_prolong_euler"][1]) == 11
    src = open(os.path.join(ROOT, "julia", "IBHip.jl")).read()
    assert re.search(r"^function restrict_euler!\(", src, re.M) and re.search(r"^function prolong_euler!\(", src, re.M)
    import ibamd
    from ibamd import cfd
    for name in ("restrict_euler", "prolong_euler"):
        assert getattr(ibamd, name) is getattr(B, name) is getattr(cfd, name)
    assert ibamd.MultigridMarch is solver.MultigridMarch


class Acc(C.Structure):
    """The leading fields of ``ibh_acc`` (ibh_common.h): a stand-in operator with no stencils -- no check reads them."""
    _fields_ = [("n_out", C.c_int32), ("n_in", C.c_int32), ("off", C.c_void_p), ("idx", C.c_void_p), ("w", C.c_void_p),
                ("packed", C.c_void_p)]


class Args:
    """Well-formed argument lists over host buffers: nothing is dereferenced before the checks, and every case below returns
    from them."""
    NF, NK = 40, 10

    def __init__(self):
        self.bufs = {k: (C.c_float * 1024)() for k in ("P", "R", "S", "Pc", "D", "Pn", "Po", "out", "pack")}
        self.coa, self.pro = Acc(self.NK, self.NF), Acc(self.NF, self.NK)
        self.fluid = _lib.ibh_fluid(283.0, 1.4, 1.716e-5, 273.15, 110.4, 2, (C.c_float * 4)(0.00646, 6.468e-5, 0, 0))

    def addr(self, k, off=0):
        return (C.addressof(self.bufs[k]) + 31) // 32 * 32 + 4 * off          # (32-byte aligned: the pack must be)

    def restrict(self, **o):
        d = dict(acc=C.addressof(self.coa), f=C.pointer(self.fluid), nd=2, P=self.addr("P"), ldp=self.NF, R=self.addr("R"),
                 ldr=self.NF, S=self.addr("S"), lds=self.NF, Pc=self.addr("Pc"), ldpc=self.NK, D=self.addr("D"), ldd=self.NK)
        return list({**d, **self.resolve(o)}.values())

    def prolong(self, **o):
        d = dict(acc=C.addressof(self.pro), f=C.pointer(self.fluid), nd=2, Pn=self.addr("Pn"), Po=self.addr("Po"), ldc=self.NK,
                 pack=self.addr("pack"), P=self.addr("P"), ldp=self.NF, out=self.addr("out"), ldo=self.NF)
        return list({**d, **self.resolve(o)}.values())

    def resolve(self, o):
        return {k: (self.addr(*v) if isinstance(v, tuple) else self.addr(v) if isinstance(v, str) else v) for k, v in o.items()}


RESTRICT = ([(dict([(k, None)]), b"null") for k in ("acc", "f", "P", "R", "Pc", "D")]
            + [(dict(nd=1), b"nd must be 2 or 3"), (dict(nd=4), b"nd must be 2 or 3")]
            + [(dict([(k, 39)]), b"leading dimension") for k in ("ldp", "ldr", "lds")]
            + [(dict([(k, 9)]), b"leading dimension") for k in ("ldpc", "ldd")]
            + [(dict(D="Pc"), b"D_c may not alias P_c"), (dict(D=("Pc", 39)), b"D_c may not alias P_c")]
            + [(dict([(k, v)]), b"may not alias P_f, R_f or S_f") for k in ("Pc", "D") for v in ("P", "R", "S", ("P", 159))])
PROLONG = ([(dict([(k, None)]), b"null") for k in ("acc", "f", "Pn", "Po", "P", "out")]
           + [(dict(nd=1), b"nd must be 2 or 3"), (dict(nd=5), b"nd must be 2 or 3")]
           + [(dict(pack=None), b"pack is missing"), (dict(pack=("pack", 1)), b"32-byte aligned"),
              (dict(pack=("pack", 4)), b"32-byte aligned")]
           + [(dict(ldc=9), b"leading dimension"), (dict(ldp=39), b"leading dimension"), (dict(ldo=39), b"leading dimension")]
           + [(dict(out="Pn"), b"P_out may not alias Pc_new or Pc_old"), (dict(out="Po"), b"P_out may not alias Pc_new or Pc_old"),
              (dict(pack="Pn"), b"pack may not alias"), (dict(pack="P"), b"pack may not alias"), (dict(pack="out"), b"pack may not alias"),
              (dict(out=("P", 8)), b"may not overlap it otherwise"), (dict(out="P", ldo=48), b"may not overlap it otherwise")])


def _ids(cases):
    return ["_".join(f"{k}-{v}" for k, v in c.items()).replace(" ", "").replace("'", "") + f"_{i}" for i, (c, _) in enumerate(cases)]


@pytest.mark.parametrize("over,what", RESTRICT, ids=_ids(RESTRICT))
def test_restrict_euler_misuse(over, what):
    lib = _lib.load()
    a = Args()               # (alive across the call: the argument list holds addresses into it)
    rc = lib.ibh_restrict_euler(*a.restrict(**over))
    assert rc != 0 and what in lib.ibh_last_error() and b"ibh_restrict_euler" in lib.ibh_last_error(), lib.ibh_last_error()


@pytest.mark.parametrize("over,what", PROLONG, ids=_ids(PROLONG))
def test_prolong_euler_misuse(over, what):
    lib = _lib.load()
    a = Args()
    rc = lib.ibh_prolong_euler(*a.prolong(**over))
    assert rc != 0 and what in lib.ibh_last_error() and b"ibh_prolong_euler" in lib.ibh_last_error(), lib.ibh_last_error()


def test_nothing_to_do_is_no_error():
    """An operator without output rows: valid arguments, nothing launched; so is the in-place prolongation's argument list up
    to the launch -- ``S_f`` may be NULL and ``P_out`` may be ``P_f``."""
    lib = _lib.load()
    a = Args()
    a.coa.n_out = 0
    assert lib.ibh_restrict_euler(*a.restrict()) == 0
    assert lib.ibh_restrict_euler(*a.restrict(S=None, lds=0)) == 0
    a.pro.n_out = 0
    assert lib.ibh_prolong_euler(*a.prolong()) == 0
    assert lib.ibh_prolong_euler(*a.prolong(out="P")) == 0


def test_multigrid_march_rejects_misuse_before_the_device(monkeypatch):
    """Every refused argument raises before the march asks for a partition, an array or a launch."""
    monkeypatch.setattr(B, "call", lambda name, *a: pytest.fail(f"{name} was called: the argument check did not stop it"))
    monkeypatch.setattr(B, "to_backend", lambda *a: pytest.fail("a partition was asked for before the arguments were checked"))
    parts = [object(), object()]
    with pytest.raises(ValueError, match="smoothing.*no source row"):
        MultigridMarch(parts, [None], [None], smoothing=(0.5, 2))
    with pytest.raises(ValueError, match="Shu-Osher"):
        MultigridMarch(parts, [None], [None], stages=ssp_stages(3))
    with pytest.raises(ValueError, match="residual callable"):
        MultigridMarch(parts, [None], [None], residual=lambda *a: None)
    with pytest.raises(ValueError, match="TimeAverage"):
        MultigridMarch(parts, [None], [None], average=object())
    for flags in (B.IBH_IMAGE_ONLY, B.IBH_PHASE_INTERIOR, B.IBH_PHASE_BOUNDARY, B.IBH_PASS_A_ONLY, B.IBH_PASS_B_ONLY):
        with pytest.raises(ValueError, match="IBH_IMAGE_ONLY, the overlap phases and the single-pass flags"):
            MultigridMarch(parts, [None], [None], flags=flags)


# ---------------------------------------------------------------------------------------------------------------------
# convergence: the rehearsal of tests/test_gpu_euler_mg.py::test_convergence
# ---------------------------------------------------------------------------------------------------------------------
CONV = dict(scale=0.3, cycles=3, stages=3, pre=1, post=1, n_coarsest=2, mach=0.5)


def conv_far():
    a = float(np.sqrt(1.4 * 283.0 * 288.15))
    return f32([1e5, 288.15, CONV["mach"] * a, 0.0])


def test_convergence_in_the_model(rae_mesh_small):
    """``rae_mesh_small`` as one partition, Mach 0.5 at zero incidence from the free stream, far field and slip wall on every
    level: 3 V-cycles on 3 levels against 7 single-grid steps, both ``rk_stages(3)`` with per-cell time steps at ``scale``
    0.3 -- 21 fine-level sweeps each, the cycle's sweep before the restriction counted.  Both end finite and the cycles end
    with the smaller ``||R_rho||_2`` (Float32 model: 1.44e5 against 1.77e5, from 1.89e5).

    What the model shows beyond that, and why the case is this short: the norm runs over every row, and on this mesh it is
    carried by the ghost cells of the immersed wall, whose residual no march drives to zero -- the boundary condition
    overwrites them -- and which feed on each other at the thin trailing edge.  It falls for about 30 sweeps and then grows in
    both marches: at ``scale`` 0.75 both marches end non-finite (single grid after ~120 sweeps), at 0.3 the single grid stays
    finite past 480 sweeps and the cycles until ~150.  The cycles lead up to ~50 sweeps (1.64e5 against 1.75e5 at 42) and
    trail from ~80 (2.35e5 against 2.00e5 at 84); over the fluid cells alone the two stay within 3 % of each other from 42
    sweeps on.  Fewer levels do not change that (2 levels: 3.23e5 against 2.56e5 at 140 sweeps)."""
    doms, coarseners, prolongators = mg.hierarchy(rae_mesh_small, 2, hypercube_families=RAE_FAMILIES)
    fl, far = ocfd.Fluid(), conv_far()
    free, wall = ocfd.FlowBC(fl, far), ocfd.FlowBC(fl, f32([far[0], far[1], 0.0]), normal_flow=True)

    def bcs_of(dom):
        view = oracle_boundaries_view(dom)

        def bcs(P):
            od.impose_bc(lambda b, Pi: free(Pi, b.normals), view, "farfield", P)
            od.impose_bc(lambda b, Pi: wall(Pi, b.normals), view, "wall", P)
        return bcs
    levels = [mg.level(oracle_view(mg.part_of(d)), bcs_of(d)) for d in doms]
    stages = rk_stages(CONV["stages"])
    start = np.tile(far, (len(doms[0]), 1))
    levels[0].bcs(start)
    count = dict(sweeps=0)
    P = start
    for _ in range(CONV["cycles"]):
        P = mg.cycle(levels, coarseners, prolongators, P, stages=stages, scale=CONV["scale"], pre=CONV["pre"], post=CONV["post"],
                     n_coarsest=CONV["n_coarsest"], dtype=f32, count=count)
    fine_sweeps = CONV["cycles"] * ((CONV["pre"] + CONV["post"]) * len(stages) + 1)
    assert fine_sweeps % len(stages) == 0
    Ps = start
    for _ in range(fine_sweeps // len(stages)):
        Ps = mg.smooth(levels[0], Ps, None, 0.0, stages, CONV["scale"], f32)

    def norm(X):
        return float(np.sqrt((mg.residual(levels[0], X, f32)[:, 0].astype(f64) ** 2).sum()))
    n0, n_mg, n_sg = norm(start), norm(P), norm(Ps)
    print(f"{fine_sweeps} fine sweeps ({count['sweeps'] / len(doms[0]):.2f} work units in the cycles): ||R_rho|| {n0:.4g} -> "
          f"multigrid {n_mg:.4g}, single grid {n_sg:.4g}")
    assert np.isfinite(P).all() and np.isfinite(Ps).all()
    assert n_mg < n_sg

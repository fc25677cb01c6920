"""The battery the Euler step tests share (tests/test_gpu_euler_{step,stage,ssp,dual,smooth}.py): helpers, the fixtures, the
compositions of the library's own launches that define each form of the update, one table of the forms -- step, stage, ssp,
dual -- and the checks that take a record of it.  Not a test module.

Every check is the union of what the four modules asserted on their own form; a sub-check that cannot apply to a form is
switched off in its record, with the reason beside the switch.  The table is written for the tests: which call, which
arguments, which composition, which float64 model.  Nothing in it is read from the library.
"""
import types

import numpy as np
import pytest
import torch

import euler_dual_model as dm
import euler_ssp_model as sp
import euler_stage_model as sm
import euler_step_model as em
import ibamd
import regimes as rg
from conftest import ADV_FAMILIES
from ibamd import _lib, cfd
from ibamd import backend as B
from ibamd.hiparray import HipArray as H
from ibamd.solver import bdf_coefficients
from test_gpu_percell_regimes import MESHES, meshes  # noqa: F401  (the module-scoped fixture of the four meshes)

f32 = np.float32
FLUID = cfd.Fluid()
SCALE = 0.75
TAU = f32(1e-3)
NAN = float("nan")
THIRD = float(f32(1.0) / f32(3.0))
QUARTER = (0.75, 0.25, 0.25)
THIRDS = (1.0 / 3.0, 2.0 / 3.0, 2.0 / 3.0)
HALVES = (0.5, 0.5, 0.5)
GENERAL, NO_FUSE, NO_QUAD = B.IBH_FORCE_GENERAL, B.IBH_NO_FUSE, B.IBH_NO_QUAD
STEP_CASES = [("adv", 0), ("adv", NO_QUAD), ("adv", GENERAL), ("adv", NO_FUSE), ("rae6k_2", 0), ("rae6k_2", GENERAL),
              ("rae6k_2", NO_FUSE), ("corner", 0), ("corner", GENERAL), ("corner", NO_FUSE), ("sphere_1", 0),
              ("sphere_1", GENERAL), ("sphere_1", NO_FUSE)]
ONE_LAUNCH = {("adv", 0), ("adv", NO_QUAD)}


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


def residual(dpart, Pd, scheme, flags):
    fn = ibamd.residual_euler_hll if scheme == "hll" else ibamd.residual_euler_sensor
    return fn(dpart, Pd, flags=flags, fluid=FLUID)


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


# ---------------------------------------------------------------------------------------------------------------------
# the compositions that define the bits
# ---------------------------------------------------------------------------------------------------------------------
def col(A, v):
    return A[:, v].contiguous()


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


def stage_dt(dtd, alpha):
    """dt .* alpha by the broadcast layer, alpha a Float32 scalar."""
    return (H(dtd) * float(f32(alpha))).t


def composed_stage(P0d, Rd, dtd, alpha):
    return ibamd.update_euler(P0d, Rd, stage_dt(dtd, alpha), FLUID)


def composed_ssp(P0d, Pd, Rd, dtd, a, b, c):
    n, nv = P0d.shape
    a, b, c = (float(f32(x)) for x in (a, b, c))
    Q0, Q = cfd.primitive2state(FLUID, P0d), cfd.primitive2state(FLUID, Pd)
    dts = (H(dtd) * c).t
    Q2 = B.colmajor_empty(n, nv)
    for v in range(nv):
        T = (H(Q0[:, v].contiguous()) * a + H(Q[:, v].contiguous()) * b).t
        if dtd.numel() == 1:
            B._stream()
            _lib.call("ibh_update_dev", n, B._ptr(dts), B._ptr(T), B._ptr(Rd[:, v].contiguous()), B._ptr(Q2[:, v]))
        else:
            t = (H(Rd[:, v].contiguous()) * H(dts)).t
            Q2[:, v] = (H(T) + H(t)).t
    return cfd.state2primitive(FLUID, Q2)


def composed_dual(P0d, Rd, Sd, dtd, alpha, g):
    n, nv = P0d.shape
    alpha, g = float(f32(alpha)), float(f32(g))
    Q0 = cfd.primitive2state(FLUID, P0d)
    h = (H(dtd) * alpha).t
    den = (H(h) * g + 1.0).t
    per_cell = dtd.numel() != 1
    den1 = None if per_cell else float(den.item())       # (one element does not broadcast against n rows: the same Float32)
    Q2 = B.colmajor_empty(n, nv)
    num = B.colmajor_empty(n)
    for v in range(nv):
        RS = (H(col(Rd, v)) + H(col(Sd, v))).t
        if per_cell:
            t = (H(RS) * H(h)).t
            num = (H(col(Q0, v)) + H(t)).t
            Q2[:, v] = (H(num) / H(den)).t
        else:
            B._stream()
            _lib.call("ibh_update_dev", n, B._ptr(h), B._ptr(col(Q0, v)), B._ptr(RS), B._ptr(num))
            Q2[:, v] = (H(num) / den1).t
    return cfd.state2primitive(FLUID, Q2)


# ---------------------------------------------------------------------------------------------------------------------
# the special rows a form plants: a NaN row, a NaN temperature, p = 0 with R = 0, a NaN residual, rho -> 0, p = 0
# ---------------------------------------------------------------------------------------------------------------------
def _rho(P, i):
    return P[i, 0] / (f32(283.0) * P[i, 1])


def _plant(X, R, o, R_rho):
    """The six rows in the state ``X`` from row ``o``; ``R_rho``: the density residual that takes row 31 to rho = 0."""
    X[7 + o] = np.nan
    X[11 + o, 1] = np.nan
    X[19 + o, 0] = 0.0
    R[19 + o] = 0.0
    R[23 + o, 0] = np.nan
    R[31 + o, 0] = R_rho
    X[40 + o, 0] = 0.0
    return [7 + o, 11 + o, 19 + o, 23 + o, 31 + o, 40 + o]


def _plant_step(h, coef):
    return _plant(h.P, h.R, 0, -_rho(h.P, 31) / h.dt), [7], [19]


def _plant_stage(h, coef):
    return _plant(h.P0, h.R, 0, -_rho(h.P0, 31) / (f32(h.dt) * f32(coef[0]))), [7], [19]


def _plant_ssp(h, coef):
    """In P0 (rows 7 .. 40) and in P (rows 107 .. 140).  No row is asked to be non-finite: p = 0 in one of the two states is
    blended with the other state's finite row."""
    a, b, c = (f32(x) for x in coef)
    special = []
    for X, o in ((h.P0, 0), (h.P, 100)):
        special += _plant(X, h.R, o, -(a * _rho(h.P0, 31 + o) + b * _rho(h.P, 31 + o)) / (f32(h.dt) * c))
    return special, [7, 107], []


def _plant_dual(h, coef):
    """And a NaN in the source; (R + S) h = -rho."""
    h.S[19] = 0.0
    special = _plant(h.P0, h.R, 0, -_rho(h.P0, 31) / (f32(h.dt) * f32(coef[0])) - h.S[31, 0])
    h.S[47, 1] = np.nan
    return special + [47], [7], [19, 47]


# ---------------------------------------------------------------------------------------------------------------------
# the table of forms
# ---------------------------------------------------------------------------------------------------------------------
def arrays(**kw):
    """The arrays of one call by role -- P0, P, R, S, dt -- and g; host or device.  A role a form does not have is None."""
    return types.SimpleNamespace(**{**dict(P0=None, P=None, R=None, S=None, dt=None, g=None), **kw})


def with_(a, **kw):
    return types.SimpleNamespace(**{**vars(a), **kw})


def _dual_host_rows(n, nd, per_cell=False):
    P0, R, S, dt, g = dm.dual_rows(n, nd, per_cell)
    return arrays(P0=P0, R=R, S=S, dt=dt, g=float(g))


class Form:
    """One form of the update and of the sweep-plus-update.

    ``update`` / ``stage``: the library calls.  ``args(a, coef)``: the leading arguments of ``update`` from the arrays ``a``
    -- also those of the composition, of the host model and, after ``got``, of its deviation function.  ``stage_args``: what
    ``stage`` takes between the partition and ``out``.  ``inputs``: the roles the update reads, with the padding the padded
    call gives each.  ``aliases``: (role, label) of every input that ``out`` may be.  ``coefs``: the coefficient sets the
    update test is parametrised over, by id.  ``f64_cases(h)``: the (coef, g) the float64 check runs.  ``plant(h, coef)``:
    plants the special rows, returns (planted rows, rows that must be all NaN, rows that must not be finite)."""

    def __init__(self, name, **kw):
        self.name = name
        self.has_P0 = True               # (the step has no base state beside the swept one)
        self.per_cell_one_launch = True  # (step_euler takes a per-cell dt in two launches)
        self.in_place = " out is P"
        self.__dict__.update(kw)

    def call_update(self, a, coef, out=None):
        return self.update(*self.args(a, coef), FLUID, out=out)

    def call_stage(self, dpart, a, coef, out, scheme, flags, work=None):
        return self.stage(dpart, *self.stage_args(a, coef), out, FLUID, scheme, work=work, flags=flags)


STEP = Form(
    "step", update=ibamd.update_euler, stage=ibamd.step_euler, update_name="update_euler",
    args=lambda a, c: (a.P, a.R, a.dt), stage_args=lambda a, c: (a.P, a.dt), composed=composed_update,
    host_rows=lambda n, nd, pc=False: arrays(**dict(zip(("P", "R", "dt"), em.synthetic_rows(n, nd, per_cell=pc)))),
    model=em.update, deviation=em.update_deviation, bound=lambda nd, model: 4 * em.MODEL_DEVIATION_EPS[nd], bound_fmt=".1f",
    inputs=(("P", 13), ("R", 5)), aliases=(("P", "in place"),), coefs={"": ()}, f64_cases=lambda h: [((), None)],
    f64_tag=lambda c, g: "", stage_coefs=((),), stage_tag=lambda dname, c: "" if dname == "global dt" else " " + dname,
    special_coef=(), plant=_plant_step,
    has_P0=False,                        # "out is P0", in the update and in the step: there is no P0
    per_cell_one_launch=False,           # "without work", "padded out", "left work alone" with a per-cell dt: two launches
    in_place=" in place")
STAGE = Form(
    "stage", update=ibamd.update_euler_stage, stage=ibamd.stage_euler, update_name="update_euler_stage",
    args=lambda a, c: (a.P0, a.R, a.dt, *c), stage_args=lambda a, c: (a.P, a.P0, a.dt, *c), composed=composed_stage,
    host_rows=lambda n, nd, pc=False: arrays(**dict(zip(("P0", "R", "dt"), em.synthetic_rows(n, nd, per_cell=pc)))),
    model=sm.update_stage, deviation=sm.update_stage_deviation, bound=lambda nd, model: 4 * em.MODEL_DEVIATION_EPS[nd],
    bound_fmt=".1f", inputs=(("P0", 13), ("R", 5)), aliases=(("P0", "out is P0"),),
    coefs={"one": (1.0,), "third": (THIRD,), "quarter": (0.25,)}, f64_cases=lambda h: [((THIRD,), None)],
    f64_tag=lambda c, g: "", stage_coefs=((THIRD,),), stage_tag=lambda dname, c: " " + dname,
    special_coef=(THIRD,), plant=_plant_stage)
SSP = Form(
    "ssp", update=ibamd.update_euler_ssp, stage=ibamd.stage_euler_ssp, update_name="update_euler_ssp",
    args=lambda a, c: (a.P0, a.P, a.R, a.dt, *c), stage_args=lambda a, c: (a.P, a.P0, a.dt, *c), composed=composed_ssp,
    host_rows=lambda n, nd, pc=False: arrays(**dict(zip(("P0", "P", "R", "dt"), sp.second_rows(n, nd, pc)))),
    model=sp.update_ssp, deviation=sp.update_ssp_deviation, bound=lambda nd, model: 4 * model, bound_fmt=".3f",
    inputs=(("P0", 7), ("P", 13), ("R", 5)), aliases=(("P0", "out is P0"), ("P", "out is P")),
    coefs={"quarter": QUARTER, "thirds": THIRDS, "halves": HALVES}, f64_cases=lambda h: [(QUARTER, None), (THIRDS, None)],
    f64_tag=lambda c, g: f" a={c[0]:.3f}", stage_coefs=(QUARTER, THIRDS),
    stage_tag=lambda dname, c: f" {dname} a={c[0]:.2f}", special_coef=QUARTER, plant=_plant_ssp)
DUAL = Form(
    "dual", update=ibamd.update_euler_dual, stage=ibamd.stage_euler_dual, update_name="update_euler_dual",
    args=lambda a, c: (a.P0, a.R, a.S, a.dt, *c, a.g), stage_args=lambda a, c: (a.P, a.P0, a.S, a.dt, *c, a.g),
    composed=composed_dual, host_rows=_dual_host_rows, model=dm.update_dual, deviation=dm.update_dual_deviation,
    bound=lambda nd, model: 4 * dm.MODEL_DEVIATION_EPS[nd], bound_fmt=".1f",
    inputs=(("P0", 7), ("R", 5), ("S", 13)), aliases=(("P0", "out is P0"),), coefs={"one": (1.0,), "third": (THIRD,)},
    f64_cases=lambda h: [((alpha,), g) for alpha in (1.0, THIRD) for g in (0.0, h.g)],
    f64_tag=lambda c, g: f" alpha={c[0]:.3f} g={g:.1f}", stage_coefs=((1.0,), (THIRD,)),
    stage_tag=lambda dname, c: f" {dname} alpha={c[0]:.2f}", special_coef=(THIRD,), plant=_plant_dual)
FORMS = {f.name: f for f in (STEP, STAGE, SSP, DUAL)}


# ---------------------------------------------------------------------------------------------------------------------
# rows for the updates alone
# ---------------------------------------------------------------------------------------------------------------------
def to_device(h):
    """The device arrays of the host rows ``h``; a global dt as a one-element tensor."""
    d = {k: ibamd.hip(v) for k, v in vars(h).items() if k in ("P0", "P", "R", "S") and v is not None}
    dtd = ibamd.hip(h.dt) if np.ndim(h.dt) else torch.tensor([float(h.dt)], dtype=torch.float32, device="cuda")
    return arrays(dt=dtd, g=h.g, **d)


_rows = {}


def rows(form, n, nd, per_cell):
    """(host rows, device rows, {(coef, g): composition}) of the form's host row generator, computed once."""
    key = (form.name, n, nd, per_cell)
    if key not in _rows:
        h = form.host_rows(n, nd, per_cell)
        _rows[key] = (h, to_device(h), {})
    return _rows[key]


# ---------------------------------------------------------------------------------------------------------------------
# the checks
# ---------------------------------------------------------------------------------------------------------------------
def check_update_bit_for_bit(form, n, nd, per_cell, coef=(), g=None):
    """The update against its composition: into a given array, allocated, into every input it may alias, with padded
    leading dimensions and nothing written past row n, with a per-cell dt off the 16-byte grid.  ``g``: in place of the
    rows' own.  Returns (the device rows, the composition)."""
    _, a, refs = rows(form, n, nd, per_cell)
    if g is not None:
        a = with_(a, g=g)
    if (coef, a.g) not in refs:
        refs[coef, a.g] = form.composed(*form.args(a, coef))
    ref = refs[coef, a.g]
    out = B.colmajor_empty(n, nd + 2)
    out.fill_(NAN)
    assert form.call_update(a, coef, out=out) is out
    same_bits(out, ref, "out of place")
    assert np.isfinite(ibamd.to_host(out)).all()
    same_bits(form.call_update(a, coef), ref, "allocated")
    for role, label in form.aliases:
        inplace = getattr(a, role).clone()
        form.call_update(with_(a, **{role: inplace}), coef, out=inplace)
        same_bits(inplace, ref, label)
    base = torch.full((nd + 2, n + 29), NAN, dtype=torch.float32, device="cuda")
    pads = {role: padded(n, nd + 2, pad) for role, pad in form.inputs}
    for role, p in pads.items():
        p.copy_(getattr(a, role))
    Op = base.T[:n]
    form.call_update(with_(a, **pads), coef, out=Op)
    same_bits(Op, ref, "padded")
    assert torch.isnan(base[:, n:]).all()                                       # nothing written past row n
    if per_cell:                                     # a per-cell dt that starts one element into a larger array
        big = torch.full((n + 3,), NAN, dtype=torch.float32, device="cuda")
        view = big[1:n + 1]
        view.copy_(a.dt)
        assert view.data_ptr() % 16 == 4
        same_bits(form.call_update(with_(a, dt=view), coef), ref, "per-cell dt off the 16-byte grid")
    return a, ref


def check_update_special_rows(form, nd):
    """A NaN row, a NaN temperature, p = 0, a NaN residual and rho -> 0 (dt R_rho = -rho), with the form's time step and in
    every state it reads: the NaN / Inf pattern of the composition."""
    h = form.host_rows(300, nd)
    coef = form.special_coef
    special, all_nan, not_finite = form.plant(h, coef)
    a = to_device(h)
    ref = form.composed(*form.args(a, coef))
    got = form.call_update(a, coef)
    same_bits(got, ref, "special rows")
    g, r = ibamd.to_host(got), ibamd.to_host(ref)
    assert np.array_equal(np.isinf(g), np.isinf(r)) and np.array_equal(np.signbit(g)[np.isinf(r)], np.signbit(r)[np.isinf(r)])
    assert all(np.isnan(g[i]).all() for i in all_nan) and not any(np.isfinite(g[i]).all() for i in not_finite)
    ok = np.setdiff1d(np.arange(300), special)
    assert np.isfinite(g[ok]).all()


def check_update_against_float64(form, nd, per_cell):
    """Per element against the form's float64 model on the update's own scale, at the form's bound: 4 x the Float32 numpy
    model's own deviation -- the margin for rounding order inside a sum -- as a measured constant of the model module or, for
    ssp, computed here on the same rows."""
    h, a, _ = rows(form, 20000, nd, per_cell)
    for coef, g in form.f64_cases(h):
        hg, ag = (h, a) if g is None else (with_(h, g=g), with_(a, g=g))
        got = ibamd.to_host(form.call_update(ag, coef))
        dev = form.deviation(got, *form.args(hg, coef))
        model = form.deviation(form.model(*form.args(hg, coef), f32), *form.args(hg, coef))
        bound = form.bound(nd, model)
        print(f"{form.update_name} nd={nd} per_cell={per_cell}{form.f64_tag(coef, g)}: device {dev:.3f} eps, Float32 model "
              f"{model:.3f} eps, bound {bound:{form.bound_fmt}} eps")
        assert dev <= bound


def check_stage_bit_for_bit(form, meshes, mesh, flags, scheme):
    """The sweep-plus-update against the update of the residual, on the transonic and the cold state, with the global and a
    per-cell dt and every stage coefficient set of the form.  The base state P0 is the regime's state and the swept state P
    one step from it (the step sweeps the regime's state itself)."""
    c = meshes[mesh]
    n, nv = c.part.spacing.shape[0], c.nd + 2
    for regime in ("transonic", "cold"):
        base = ibamd.hip(rg.euler_regime(c.part, regime))
        dt1 = ibamd.timestep_euler(c.dpart, base, FLUID, SCALE)
        cells = ibamd.timestep_euler(c.dpart, base, FLUID, SCALE, out=False, cells=B.colmajor_empty(n))
        work, out = B.colmajor_empty(n, nv), B.colmajor_empty(n, nv)
        a = arrays(P=base)
        if form.has_P0:
            a.P0, a.P = base, B.colmajor_empty(n, nv)
            ibamd.step_euler(c.dpart, base, dt1, a.P, FLUID, scheme, work=work, flags=flags)   # P: one step from P0
            assert not torch.equal(a.P, base)
        if "S" in dict(form.inputs):                 # the BDF2 source and g of a physical step of 8 x the time step
            cn, cm, a.g = bdf_coefficients(2, 8 * float(dt1.item()))
            a.S = ibamd.dual_source(a.P0, a.P, cn, cm, FLUID)
        a.R = residual(c.dpart, a.P, scheme, flags)
        finite_R = np.isfinite(ibamd.to_host(a.R)).all(axis=1)
        swept = torch.from_numpy(finite_R).to(work.device)
        for dt, dname in ((dt1, "global dt"), (cells, "per-cell dt")):
            a.dt = dt
            one_launch = (mesh, flags) in ONE_LAUNCH and (form.per_cell_one_launch or a.dt is dt1)
            for coef in form.stage_coefs:
                def stage(arr, o, work=None):
                    return form.call_stage(c.dpart, arr, coef, o, scheme, flags, work)

                what = f"{mesh} flags={flags} {scheme} {regime}" + form.stage_tag(dname, coef)
                ref = form.call_update(a, coef)
                work.fill_(NAN)                              # a row the sweep or the update leaves unwritten shows
                out.fill_(NAN)
                assert stage(a, out, work) is out
                same_bits(out, ref, what)
                assert finite_R.any() and np.isfinite(ibamd.to_host(out)[finite_R]).all(), what
                if one_launch:                               # the sweep stores the update itself: no work array
                    assert torch.isnan(work).all(), what + ": the one-launch form left work alone"
                    out.fill_(NAN)
                    stage(a, out)
                    same_bits(out, ref, what + " without work")
                    po = padded(n, nv, 19, fill=NAN)
                    stage(a, po)
                    same_bits(po, ref, what + " padded out")
                    if form.has_P0:
                        b0 = a.P0.clone()
                        stage(with_(a, P0=b0), b0)
                        same_bits(b0, ref, what + " out is P0")
                else:
                    assert not torch.isnan(work[swept]).any(), what + ": swept into work"
                    same_bits(work, a.R, what + ": work holds the residual")
                    with pytest.raises(_lib.IbhError, match="work must be"):
                        stage(a, out)
                # out is P: the two-launch form everywhere
                inplace = a.P.clone()
                work.fill_(NAN)
                stage(with_(a, P=inplace), inplace, work)
                same_bits(inplace, ref, what + form.in_place)
                assert not torch.isnan(work[swept]).any(), what + ": swept into work"
                inplace.copy_(a.P)
                with pytest.raises(_lib.IbhError, match="work must be"):
                    stage(with_(a, P=inplace), inplace)
                if form.has_P0:                              # out is P0 (P0 is not P) with a work array, and a padded S
                    b0, Sp = a.P0.clone(), a.S
                    if Sp is not None:
                        Sp = padded(n, nv, 11)
                        Sp.copy_(a.S)
                    stage(with_(a, P0=b0, S=Sp), b0, work)
                    same_bits(b0, ref, what + (" out is P0, with work" if Sp is None else " out is P0, padded S"))


def replayed_march(make_march, P0, nsteps, warmup=2, onward=False):
    """``nsteps`` steps of a fresh march captured once and replayed -- no host read-back, no allocation in a step -- after
    ``warmup`` eager steps from ``P0`` (workspaces are allocated on first use).  The captured steps start from ``P0`` again
    or, ``onward``, from the warm-up's result, which is restored before the replay.  Returns the replay's last array, filled
    with NaN between capture and replay."""
    m = make_march()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        Pw = P0
        for _ in range(warmup):
            Pw = m.step(Pw)
        first = Pw.clone() if onward else None
        stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            Pg = Pw if onward else P0
            for _ in range(nsteps):
                Pg = m.step(Pg)
        Pg.fill_(NAN)
        if onward:
            Pw.copy_(first)              # (a march may return the array the captured steps started from)
        graph.replay()
    stream.synchronize()
    B._stream()
    return Pg

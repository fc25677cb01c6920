"""Implicit residual smoothing on the device -- ``smooth_residual``, ``update_euler_smoothed``,
``EulerMarch(smoothing=(eps, n_iter))`` -- bit for bit against the float32 model of tests/smooth_model.py and against the
composition of the library's own launches.  Meshes, states and helpers: those of tests/euler_forms.py; the four
meshes hold one-face, multi-face and no-face sides, mirror faces and skirt cells, in 2-D and 3-D."""
import numpy as np
import pytest
import torch

import ibamd
import regimes as rg
import smooth_model as sm
from ibamd import _lib, cfd
from ibamd import backend as B
from ibamd.solver import EulerMarch, rk_stages, ssp_stages
from euler_forms import FLUID, FORMS, SCALE, TAU, arrays, march_dom, meshes, residual, same_bits  # noqa: F401

pytestmark = pytest.mark.gpu
f32 = np.float32
NAN = float("nan")
MESHES = ("adv", "rae6k_2", "corner", "sphere_1")
_tables = {}


def table(c):
    if c.name not in _tables:
        _tables[c.name] = sm.face_table(c.part)
    return _tables[c.name]


def padded_nan(n, nv, pad):
    """(the whole (nv, n + pad) allocation filled with NaN, its (n, nv) view with leading dimension n + pad)"""
    base = torch.full((nv, n + pad), NAN, dtype=torch.float32, device="cuda")
    return base, base.T[:n]


def host(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def side_classes(part):
    """{"none", "one", "many"}: the face counts the sides of the partition's cells have; and its number of mirror faces."""
    seen, mirror = set(), 0
    for d in range(part.ndims):
        own, nei = (np.asarray(a) for a in part.face_owners_neighbors[d + 1])
        mirror += int((own == nei).sum())
        for right in (False, True):
            cnt = np.diff(np.asarray(part.face_accumulators[(d + 1, right)].off))
            seen |= {k for k, m in (("none", cnt == 0), ("one", cnt == 1), ("many", cnt > 1)) if m.any()}
    return seen, mirror


def pruned(part):
    """A copy of the partition's face lists with sides emptied: every cell loses the faces of one side in turn, every 97th
    cell all of them (n = 0).  The meshes themselves give every cell a face on every side -- a mirror face at the domain's
    edge -- so the no-face entries of the side table are reached only here.  Without block structure: face lists alone."""
    import copy

    from ibamd.accumulator import Accumulator
    q = copy.copy(part)
    q.block_size = 0
    q.face_accumulators = dict(part.face_accumulators)
    nc = part.spacing.shape[0]
    cells = np.arange(nc)
    for d in range(part.ndims):
        for right in (False, True):
            acc = part.face_accumulators[(d + 1, right)]
            off, idx = np.asarray(acc.off, dtype=np.int64), np.asarray(acc.idx)
            cnt = np.diff(off)
            cnt[(cells % (2 * part.ndims + 1) == 2 * d + right) | (cells % 97 == 0)] = 0
            keep = np.repeat(cnt > 0, np.diff(off))
            q.face_accumulators[(d + 1, right)] = Accumulator(csr=(np.concatenate([[0], np.cumsum(cnt)]), idx[keep], None),
                                                              n_input=acc.n_input)
    return q


def test_meshes_hold_every_side_class(meshes):
    for name in MESHES:
        c = meshes[name]
        seen, mirror = side_classes(c.part)
        assert seen == {"one", "many"} and mirror > 0, name
        assert 0 < c.dpart.info["direct_sides"] < 2 * c.nd * c.part.spacing.shape[0]
    assert meshes["rae6k_2"].partial and meshes["sphere_1"].partial           # skirt cells
    for name in ("rae6k_2", "corner"):
        q = pruned(meshes[name].part)
        assert side_classes(q)[0] == {"none", "one", "many"} and sm.face_table(q)[1].min() == 0


@pytest.mark.parametrize("mesh", ["rae6k_2", "corner"])
def test_smooth_residual_no_face_sides(meshes, mesh):
    """Sides without a face contribute nothing, and a cell without faces keeps ``R + eps * 0``."""
    q = pruned(meshes[mesh].part)
    dq = B.DevicePartition(q)
    T, n = sm.face_table(q)
    nc, nv = q.spacing.shape[0], q.ndims + 2
    rng = np.random.default_rng(5)
    R = (rng.standard_normal((nc, nv)) * (10.0 ** rng.integers(-3, 6, size=nv))).astype(f32)
    Rd = ibamd.hip(R)
    for eps in (0.0, 0.5, 2.0):
        ref = R
        for n_iter in (1, 2, 3):
            ref = sm.iterate(T, n, R, ref, eps, f32)
            same_bits(ibamd.smooth_residual(dq, Rd, eps, n_iter), host(ref), f"{mesh} pruned eps={eps} n_iter={n_iter}")
    assert np.array_equal(ref[n == 0], R[n == 0])


@pytest.mark.parametrize("nvk", ["one", "euler", "eight"])
@pytest.mark.parametrize("mesh", MESHES)
def test_smooth_residual_bit_for_bit(meshes, mesh, nvk):
    c = meshes[mesh]
    nc = c.part.spacing.shape[0]
    nv = {"one": 1, "euler": c.nd + 2, "eight": 8}[nvk]
    if nvk == "euler":   # a real sweep residual
        R = ibamd.to_host(residual(c.dpart, ibamd.hip(rg.euler_regime(c.part, "transonic")), "hll", 0)).copy()
        assert np.isfinite(R).mean() > 0.99 and (np.nanmax(np.abs(R), axis=0) > 0).all()
    else:
        rng = np.random.default_rng(11 + nv)
        R = (rng.standard_normal((nc, nv)) * (10.0 ** rng.integers(-3, 6, size=nv))).astype(f32)
    R[nc // 3] = NAN                                   # the model's NaN pattern: a NaN and an Inf row spread to their
    R[(2 * nc) // 3] = np.inf                          # neighbours, one ring per iteration
    R[(2 * nc) // 3 + 1] = -np.inf
    if nv == 1:
        R = R[:, 0].copy()
        Rd, (Sb, S), (Tb, T) = ibamd.hip(R), (None, B.colmajor_empty(nc)), (None, B.colmajor_empty(nc))
    else:
        (Rb, Rd), (Sb, S), (Tb, T) = padded_nan(nc, nv, 13), padded_nan(nc, nv, 5), padded_nan(nc, nv, 29)
        Rd.copy_(ibamd.hip(R))
    for eps in (0.0, 0.5, 2.0):
        ref = R
        for n_iter in (1, 2, 3):
            ref = sm.iterate(*table(c), R, ref, eps, f32)
            what = f"{mesh} nv={nv} eps={eps} n_iter={n_iter}"
            S.fill_(NAN)
            T.fill_(NAN)
            got = ibamd.smooth_residual(c.dpart, Rd, eps, n_iter, out=S, tmp=T if n_iter >= 2 else None)
            assert got is S
            same_bits(S, host(ref), what)
            assert np.isnan(ref).any() and np.isfinite(ref).sum() > 0.9 * ref.size, what
            if Sb is not None:                         # nothing past row nc, nothing in the padding, R left alone
                assert torch.isnan(Sb[:, nc:]).all() and torch.isnan(Tb[:, nc:]).all() and torch.isnan(Rb[:, nc:]).all()
                same_bits(Rd, host(R), what + ": R")
    if nv > 1:   # without out / tmp: allocated, same bits
        same_bits(ibamd.smooth_residual(c.dpart, Rd, 2.0, 3), host(ref), f"{mesh} nv={nv} allocated")


def composed(form, P0, P, S, dt, coef):
    """The defining composition of the form's update, on the smoothed residual ``S``."""
    f = FORMS[form]
    return f.composed(*f.args(arrays(P0=P0, P=P, R=S, dt=dt), coef))


@pytest.mark.parametrize("form", ["stage", "ssp"])
@pytest.mark.parametrize("mesh", ["adv", "rae6k_2", "corner"])
def test_update_smoothed_bit_for_bit(meshes, mesh, form):
    c = meshes[mesh]
    nc, nv = c.part.spacing.shape[0], c.nd + 2
    P = ibamd.hip(rg.euler_regime(c.part, "transonic"))
    P0 = ibamd.hip(rg.euler_regime(c.part, "crossing"))
    R = residual(c.dpart, P, "hll", 0)
    dts = {"global": ibamd.timestep_euler(c.dpart, P, FLUID, SCALE),
           "per_cell": ibamd.timestep_euler(c.dpart, P, FLUID, SCALE, out=False, cells=B.colmajor_empty(nc))}
    coef = (0.25,) if form == "stage" else (0.75, 0.25, 0.25)
    eps = 0.5
    for n_iter in (1, 3):
        S = ibamd.smooth_residual(c.dpart, R, eps, n_iter)
        prev = R if n_iter == 1 else ibamd.smooth_residual(c.dpart, R, eps, n_iter - 1)
        for dtk, dt in dts.items():
            ref = composed(form, P0, P, S, dt, coef)
            what = f"{mesh} {form} {dtk} n_iter={n_iter}"
            assert np.isfinite(ibamd.to_host(ref)).mean() > 0.99, what
            Pin = P if form == "ssp" else None
            base, out = padded_nan(nc, nv, 7)
            got = ibamd.update_euler_smoothed(c.dpart, P0, Pin, R, prev, eps, dt, coef, FLUID, out=out)
            assert got is out
            same_bits(out, ref, what + " fresh")
            assert torch.isnan(base[:, nc:]).all(), what
            same_bits(ibamd.update_euler_smoothed(c.dpart, P0, Pin, R, prev, eps, dt, coef, FLUID), ref, what + " allocated")
            q = P0.clone()
            ibamd.update_euler_smoothed(c.dpart, q, Pin, R, prev, eps, dt, coef, FLUID, out=q)
            same_bits(q, ref, what + " out = P0")
            q = P.clone()                              # (the stage form ignores P: the swept state as destination)
            ibamd.update_euler_smoothed(c.dpart, P0, q, R, prev, eps, dt, coef, FLUID, out=q)
            same_bits(q, ref, what + " out = P")
    # a forward-Euler step is the stage on the step's own input with c = 1
    same_bits(ibamd.update_euler_smoothed(c.dpart, P, None, R, R, eps, dts["global"], (1.0,), FLUID),
              ibamd.update_euler(P, ibamd.smooth_residual(c.dpart, R, eps, 1), dts["global"], FLUID), f"{mesh} step")


EPS, N_ITER, NSTEPS = 0.5, 2, 5
STAGES = {"euler": 1, "rk3": 3, "ssprk3": ssp_stages(3)}


def composed_march(dpart, P, stages, local, bcs):
    """The smoothed march from public calls: time step, then per stage the sweep, ``smooth_residual(n_iter)`` as launches of
    its own and the unsmoothed update of the stage's form."""
    nc = P.shape[0]
    for _ in range(NSTEPS):
        if local:
            dt = ibamd.timestep_euler(dpart, P, FLUID, SCALE, out=False, cells=B.colmajor_empty(nc))
        else:
            dt = ibamd.timestep_euler(dpart, P, FLUID, SCALE)
        P0 = src = P
        if stages == 1:
            kinds = [("step",)]
        elif isinstance(stages, int):
            kinds = [("stage", a) for a in rk_stages(stages)]
        else:
            kinds = [("ssp",) + tuple(t) for t in stages]
        for k in kinds:
            S = ibamd.smooth_residual(dpart, residual(dpart, src, "hll", 0), EPS, N_ITER)
            if k[0] == "step":
                out = ibamd.update_euler(src, S, dt, FLUID)
            elif k[0] == "stage":
                out = ibamd.update_euler_stage(P0, S, dt, k[1], FLUID)
            elif k[1:3] == (0.0, 1.0):
                out = ibamd.update_euler_stage(src, S, dt, k[3], FLUID)
            else:
                out = ibamd.update_euler_ssp(P0, src, S, dt, *k[1:], FLUID)
            bcs(out)
            src = out
        P = src
    return P


@pytest.mark.parametrize("local", [False, True], ids=["global_dt", "local_dt"])
@pytest.mark.parametrize("stages", list(STAGES))
def test_march_smoothed(march_dom, stages, local):
    dom, part, dpart, bcs = march_dom
    P0 = ibamd.hip(rg.euler_regime(part, "transonic"))
    start = P0.clone()
    ref = composed_march(dpart, P0, STAGES[stages], local, bcs)
    assert np.isfinite(ibamd.to_host(ref)).all()
    m = EulerMarch(dpart, FLUID, scale=SCALE, bcs=bcs, local_dt=local, stages=STAGES[stages], smoothing=(EPS, N_ITER))
    assert len(m._smooth) == 1
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    P = P0
    for _ in range(NSTEPS):
        P = m.step(P)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before, "the march allocated after construction"
    same_bits(P, ref, f"smoothed march {stages} local={local}")
    same_bits(P0, start, "the initial array is left alone")


def test_march_smoothed_forms(march_dom):
    """``residual=`` and the number of smoothing arrays: none for one iteration, one for two, two from three."""
    dom, part, dpart, bcs = march_dom
    P0 = ibamd.hip(rg.euler_regime(part, "transonic"))
    kw = dict(scale=SCALE, bcs=bcs, local_dt=True, stages=3)
    for n_iter, narr in ((1, 0), (2, 1), (3, 2), (4, 2)):
        m = EulerMarch(dpart, FLUID, smoothing=(EPS, n_iter), **kw)
        assert len(m._smooth) == narr
        r = EulerMarch(dpart, FLUID, smoothing=(EPS, n_iter),
                       residual=lambda p, P, out: ibamd.residual_euler_hll(p, P, out=out, fluid=FLUID), **kw)
        a = m.step(m.step(P0))
        same_bits(r.step(r.step(P0)), a, f"residual= n_iter={n_iter}")
        # by hand: the stage of the low-storage family on smooth_residual(n_iter)
        P = P0
        for _ in range(2):
            dt = ibamd.timestep_euler(dpart, P, FLUID, SCALE, out=False, cells=B.colmajor_empty(P.shape[0]))
            src = P
            for alpha in rk_stages(3):
                S = ibamd.smooth_residual(dpart, residual(dpart, src, "hll", 0), EPS, n_iter)
                src = ibamd.update_euler_stage(P, S, dt, alpha, FLUID)
                bcs(src)
            P = src
        same_bits(a, P, f"n_iter={n_iter}")


@pytest.mark.parametrize("stages", list(STAGES))
def test_march_without_smoothing_is_the_unsmoothed_march(march_dom, stages):
    """``smoothing=None``, the default: the step / stage calls of the march as it was, bit for bit."""
    dom, part, dpart, bcs = march_dom
    P0 = ibamd.hip(rg.euler_regime(part, "transonic"))
    nc, nv = P0.shape
    m = EulerMarch(dpart, FLUID, scale=SCALE, bcs=bcs, stages=STAGES[stages], smoothing=None)
    assert m.smoothing is None and m._smooth == ()
    d = EulerMarch(dpart, FLUID, scale=SCALE, bcs=bcs, stages=STAGES[stages])
    P = Pd = Pr = P0
    work = B.colmajor_empty(nc, nv)
    for _ in range(3):
        P, Pd = m.step(P), d.step(Pd)
        dt = ibamd.timestep_euler(dpart, Pr, FLUID, SCALE)
        base = src = Pr
        if stages == "euler":
            src = ibamd.step_euler(dpart, src, dt, B.colmajor_empty(nc, nv), FLUID, work=work)
            bcs(src)
        elif stages == "rk3":
            for alpha in rk_stages(3):
                src = ibamd.stage_euler(dpart, src, base, dt, alpha, B.colmajor_empty(nc, nv), FLUID, work=work)
                bcs(src)
        else:
            for a, b, c_ in ssp_stages(3):
                out = B.colmajor_empty(nc, nv)
                if (a, b) == (0.0, 1.0):
                    ibamd.stage_euler(dpart, src, src, dt, c_, out, FLUID, work=work)
                else:
                    ibamd.stage_euler_ssp(dpart, src, base, dt, a, b, c_, out, FLUID, work=work)
                bcs(out)
                src = out
        Pr = src
    same_bits(P, Pr, f"smoothing=None {stages}")
    same_bits(P, Pd, f"default {stages}")


def test_python_layer_rejects_misuse(meshes, march_dom):
    dom, part, dpart, bcs = march_dom
    with pytest.raises(ValueError, match="time average"):
        EulerMarch(dpart, FLUID, smoothing=(0.5, 2), average=cfd.TimeAverage(TAU))
    for bad in ((0.5, 0), (0.5, -1), (0.5, 1.5), (-0.5, 2), (NAN, 2), (float("inf"), 2), (0.5,), 0.5):
        with pytest.raises((ValueError, TypeError)):
            EulerMarch(dpart, FLUID, smoothing=bad)
    for flag in (B.IBH_IMAGE_ONLY, B.IBH_PHASE_INTERIOR, B.IBH_PHASE_BOUNDARY):
        with pytest.raises(ValueError, match="not taken"):
            EulerMarch(dpart, FLUID, smoothing=(0.5, 2), flags=flag)
    c = meshes["adv"]
    nc, nv = c.part.spacing.shape[0], c.nd + 2
    R, S = B.colmajor_empty(nc, nv).fill_(1.0), B.colmajor_empty(nc, nv)
    for eps, n_iter in ((-0.5, 1), (NAN, 1), (0.5, 0), (0.5, 2.5)):
        with pytest.raises(ValueError):
            ibamd.smooth_residual(c.dpart, R, eps, n_iter)
    with pytest.raises(_lib.IbhError, match="alias"):
        ibamd.smooth_residual(c.dpart, R, 0.5, 1, out=R)
    with pytest.raises(_lib.IbhError, match="alias"):
        ibamd.smooth_residual(c.dpart, R, 0.5, 2, out=S, tmp=S)
    with pytest.raises(ValueError):
        ibamd.smooth_residual(c.dpart, torch.zeros((9, nc), device="cuda").T, 0.5, 1)          # nv > 8
    with pytest.raises(ValueError):
        ibamd.smooth_residual(c.dpart, R[:-1], 0.5, 1)
    P = ibamd.hip(rg.euler_regime(c.part, "transonic"))
    dt = ibamd.timestep_euler(c.dpart, P, FLUID, SCALE)
    with pytest.raises(ValueError):
        ibamd.update_euler_smoothed(c.dpart, P, P, R, R, 0.5, dt, (0.5, 0.5), FLUID)
    with pytest.raises(ValueError):
        ibamd.update_euler_smoothed(c.dpart, P, None, R, R, -1.0, dt, (1.0,), FLUID)
    with pytest.raises(_lib.IbhError, match="may not alias"):
        ibamd.update_euler_smoothed(c.dpart, P, None, R, S, 0.5, dt, (1.0,), FLUID, out=S)
    with pytest.raises(_lib.IbhError, match="may not alias"):
        ibamd.update_euler_smoothed(c.dpart, P, None, R, R, 0.5, dt, (1.0,), FLUID, out=R)

"""Shu-Osher (strong-stability-preserving) Runge-Kutta stages on the device -- ``update_euler_ssp``, ``stage_euler_ssp``,
``EulerMarch(stages=ssp_stages(order))`` -- bit for bit against the composition of the library's own launches that defines
them, and against the float64 model of tests/euler_ssp_model.py.  Meshes, states and helpers: those of
tests/test_gpu_euler_step.py.

The composition (six kinds of launch): ``primitive2state`` of ``P0`` and of ``P``; ``dts = dt .* c`` and, per column,
``T = Q0 .* a .+ Q .* b`` by the broadcast layer with Float32 scalars; per column ``ibh_update_dev(dts, T, R)`` (a per-cell
``dt``: the broadcasts ``R .* dts`` and ``T .+ ...``); ``state2primitive``.
"""

import numpy as np
import pytest
import torch

import euler_ssp_model as sp
import euler_step_model as em
import ibamd
import regimes as rg
from ibamd import _lib, cfd
from ibamd import backend as B
from ibamd.hiparray import HipArray as H
from ibamd.solver import EulerMarch, ssp_stages
from test_gpu_euler_step import (FLUID, NO_FUSE, ONE_LAUNCH, SCALE, STEP_CASES, TAU, march_dom, meshes, padded,  # noqa: F401
                                 residual, same_bits)

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
QUARTER = (0.75, 0.25, 0.25)
THIRDS = (1.0 / 3.0, 2.0 / 3.0, 2.0 / 3.0)
HALVES = (0.5, 0.5, 0.5)
NAN = float("nan")


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


# ---------------------------------------------------------------------------------------------------------------------
# update
# ---------------------------------------------------------------------------------------------------------------------
_rows = {}


def rows(n, nd, per_cell):
    """Host and device (P0, P, R, dt) of ``euler_ssp_model.second_rows``, and the compositions computed so far."""
    if (n, nd, per_cell) not in _rows:
        P0, P, R, dt = sp.second_rows(n, nd, per_cell)
        dtd = ibamd.hip(dt) if per_cell else torch.tensor([float(dt)], dtype=torch.float32, device="cuda")
        _rows[n, nd, per_cell] = (P0, P, R, dt, ibamd.hip(P0), ibamd.hip(P), ibamd.hip(R), dtd, {})
    return _rows[n, nd, per_cell]


@pytest.mark.parametrize("abc", [QUARTER, THIRDS, HALVES], ids=["quarter", "thirds", "halves"])
@pytest.mark.parametrize("per_cell", [False, True], ids=["global_dt", "per_cell_dt"])
@pytest.mark.parametrize("nd", [2, 3])
@pytest.mark.parametrize("n", [1, 77, 2048 * 256 + 77])
def test_update_ssp_bit_for_bit(n, nd, per_cell, abc):
    """One row, less than a workgroup, and past the grid cap of 2 048 workgroups of 256 (the grid-stride loop)."""
    _, _, _, _, P0d, Pd, Rd, dtd, refs = rows(n, nd, per_cell)
    assert not torch.equal(P0d, Pd)
    if abc not in refs:
        refs[abc] = composed_ssp(P0d, Pd, Rd, dtd, *abc)
    ref = refs[abc]
    out = B.colmajor_empty(n, nd + 2)
    out.fill_(NAN)
    assert ibamd.update_euler_ssp(P0d, Pd, Rd, dtd, *abc, FLUID, out=out) is out
    same_bits(out, ref, "out of place")
    assert np.isfinite(ibamd.to_host(out)).all()
    same_bits(ibamd.update_euler_ssp(P0d, Pd, Rd, dtd, *abc, FLUID), ref, "allocated")
    inplace = P0d.clone()
    ibamd.update_euler_ssp(inplace, Pd, Rd, dtd, *abc, FLUID, out=inplace)
    same_bits(inplace, ref, "out is P0")
    inplace = Pd.clone()
    ibamd.update_euler_ssp(P0d, inplace, Rd, dtd, *abc, FLUID, out=inplace)
    same_bits(inplace, ref, "out is P")
    same_bits(ibamd.update_euler_ssp(Pd, Pd, Rd, dtd, *abc, FLUID), composed_ssp(Pd, Pd, Rd, dtd, *abc), "P0 is P")
    base = torch.full((nd + 2, n + 29), NAN, dtype=torch.float32, device="cuda")
    Bp, Pp, Rp, Op = padded(n, nd + 2, 7), padded(n, nd + 2, 13), padded(n, nd + 2, 5), base.T[:n]
    Bp.copy_(P0d)
    Pp.copy_(Pd)
    Rp.copy_(Rd)
    ibamd.update_euler_ssp(Bp, Pp, Rp, dtd, *abc, FLUID, out=Op)
    same_bits(Op, ref, "padded")
    assert torch.isnan(base[:, n:]).all()                                       # nothing written past row n
    if per_cell:                                     # a per-cell dt that starts one element into a larger array
        big = torch.full((n + 3,), NAN, dtype=torch.float32, device="cuda")
        view = big[1:n + 1]
        view.copy_(dtd)
        assert view.data_ptr() % 16 == 4
        same_bits(ibamd.update_euler_ssp(P0d, Pd, Rd, view, *abc, FLUID), ref, "per-cell dt off the 16-byte grid")


@pytest.mark.parametrize("nd", [2, 3])
def test_update_ssp_nan_and_vacuum_rows(nd):
    """The rows of test_update_stage_nan_and_vacuum_rows -- a NaN row, a NaN temperature, p = 0, a NaN residual, rho -> 0 --
    placed in P0 (rows 7 .. 40) and in P (rows 107 .. 140): the NaN / Inf pattern of the composition."""
    a, b, c = (f32(x) for x in QUARTER)
    P0, P, R, dt = sp.second_rows(300, nd)
    h = f32(dt) * c
    special = []
    for X, o in ((P0, 0), (P, 100)):
        X[7 + o] = np.nan
        X[11 + o, 1] = np.nan
        X[19 + o, 0] = 0.0
        R[19 + o] = 0.0
        R[23 + o, 0] = np.nan
        rho = a * (P0[31 + o, 0] / (f32(283.0) * P0[31 + o, 1])) + b * (P[31 + o, 0] / (f32(283.0) * P[31 + o, 1]))
        R[31 + o, 0] = -rho / h
        X[40 + o, 0] = 0.0
        special += [7 + o, 11 + o, 19 + o, 23 + o, 31 + o, 40 + o]
    P0d, Pd, Rd = ibamd.hip(P0), ibamd.hip(P), ibamd.hip(R)
    dtd = torch.tensor([float(dt)], dtype=torch.float32, device="cuda")
    ref = composed_ssp(P0d, Pd, Rd, dtd, *QUARTER)
    got = ibamd.update_euler_ssp(P0d, Pd, Rd, dtd, *QUARTER, FLUID)
    same_bits(got, ref, "special rows")
    g, r = ibamd.to_host(got), ibamd.to_host(ref)
    assert np.array_equal(np.isinf(g), np.isinf(r)) and np.array_equal(np.signbit(g)[np.isinf(r)], np.signbit(r)[np.isinf(r)])
    assert np.isnan(g[7]).all() and np.isnan(g[107]).all()
    ok = np.setdiff1d(np.arange(300), special)
    assert np.isfinite(g[ok]).all()


@pytest.mark.parametrize("per_cell", [False, True], ids=["global_dt", "per_cell_dt"])
@pytest.mark.parametrize("nd", [2, 3])
def test_update_ssp_against_float64(nd, per_cell):
    """Per element against the float64 model on the update's own scale (``euler_ssp_model.update_ssp_scale``:
    ``euler_step_model.update_scale`` with the blend as the base state): at most 4 x the deviation of the Float32 numpy model
    on the same rows, computed here -- the margin ``update_euler`` and ``update_euler_stage`` are held to, for rounding order
    inside a sum."""
    P0, P, R, dt, P0d, Pd, Rd, dtd, _ = rows(20000, nd, per_cell)
    for abc in (QUARTER, THIRDS):
        got = ibamd.to_host(ibamd.update_euler_ssp(P0d, Pd, Rd, dtd, *abc, FLUID))
        dev = sp.update_ssp_deviation(got, P0, P, R, dt, *abc)
        model = sp.update_ssp_deviation(sp.update_ssp(P0, P, R, dt, *abc, f32), P0, P, R, dt, *abc)
        print(f"update_euler_ssp nd={nd} per_cell={per_cell} a={abc[0]:.3f}: device {dev:.3f} eps, Float32 model {model:.3f} "
              f"eps, bound {4 * model:.3f} eps")
        assert dev <= 4 * model


# ---------------------------------------------------------------------------------------------------------------------
# stage
# ---------------------------------------------------------------------------------------------------------------------
# (every SSP instantiation of both 2-D sweeps kept its sibling's occupancy without scratch and its timing range lies below the
# two-launch form's, profiles/euler_ssp: the one-launch set is that of step_euler and stage_euler)
@pytest.mark.parametrize("scheme", ["hll", "sensor"])
@pytest.mark.parametrize("mesh,flags", STEP_CASES, ids=[f"{m}-{f}" for m, f in STEP_CASES])
def test_stage_ssp_bit_for_bit(meshes, mesh, flags, scheme):
    c = meshes[mesh]
    n, nv = c.part.spacing.shape[0], c.nd + 2
    one_launch = (mesh, flags) in ONE_LAUNCH
    for regime in ("transonic", "cold"):
        P0 = ibamd.hip(rg.euler_regime(c.part, regime))
        dt1 = ibamd.timestep_euler(c.dpart, P0, FLUID, SCALE)
        cells = ibamd.timestep_euler(c.dpart, P0, FLUID, SCALE, out=False, cells=B.colmajor_empty(n))
        work, out = B.colmajor_empty(n, nv), B.colmajor_empty(n, nv)
        Pd = B.colmajor_empty(n, nv)
        ibamd.step_euler(c.dpart, P0, dt1, Pd, FLUID, scheme, work=work, flags=flags)      # P: one step from P0
        assert not torch.equal(Pd, P0)
        R = residual(c.dpart, Pd, scheme, flags)
        finite_R = np.isfinite(ibamd.to_host(R)).all(axis=1)
        for dt, dname in ((dt1, "global dt"), (cells, "per-cell dt")):
            for abc in (QUARTER, THIRDS):
                what = f"{mesh} flags={flags} {scheme} {regime} {dname} a={abc[0]:.2f}"
                ref = ibamd.update_euler_ssp(P0, Pd, R, dt, *abc, FLUID)
                work.fill_(NAN)                              # a row the sweep or the update leaves unwritten shows
                out.fill_(NAN)
                assert ibamd.stage_euler_ssp(c.dpart, Pd, P0, dt, *abc, out, FLUID, scheme, work=work, flags=flags) is out
                same_bits(out, ref, what)
                assert finite_R.any() and np.isfinite(ibamd.to_host(out)[finite_R]).all(), what
                if one_launch:                               # the sweep stores the update itself: no work array
                    assert torch.isnan(work).all(), what + ": the one-launch form left work alone"
                    out.fill_(NAN)
                    ibamd.stage_euler_ssp(c.dpart, Pd, P0, dt, *abc, out, FLUID, scheme, flags=flags)
                    same_bits(out, ref, what + " without work")
                    po = padded(n, nv, 19, fill=NAN)
                    ibamd.stage_euler_ssp(c.dpart, Pd, P0, dt, *abc, po, FLUID, scheme, flags=flags)
                    same_bits(po, ref, what + " padded out")
                    base = P0.clone()
                    ibamd.stage_euler_ssp(c.dpart, Pd, base, dt, *abc, base, FLUID, scheme, flags=flags)
                    same_bits(base, ref, what + " out is P0")
                else:
                    with pytest.raises(_lib.IbhError, match="work must be"):
                        ibamd.stage_euler_ssp(c.dpart, Pd, P0, dt, *abc, out, FLUID, scheme, flags=flags)
                # out is P: the two-launch form everywhere
                inplace = Pd.clone()
                work.fill_(NAN)
                ibamd.stage_euler_ssp(c.dpart, inplace, P0, dt, *abc, inplace, FLUID, scheme, work=work, flags=flags)
                same_bits(inplace, ref, what + " out is P")
                assert not torch.isnan(work[torch.from_numpy(finite_R).to(work.device)]).any(), what + ": swept into work"
                inplace.copy_(Pd)
                with pytest.raises(_lib.IbhError, match="work must be"):
                    ibamd.stage_euler_ssp(c.dpart, inplace, P0, dt, *abc, inplace, FLUID, scheme, flags=flags)


def test_python_layer_rejects_misuse(meshes):
    c = meshes["corner"]
    Pd = ibamd.hip(rg.euler_regime(c.part, "rest"))
    dt = torch.ones(1, dtype=torch.float32, device="cuda")
    out = torch.empty_like(Pd.T).T
    work = torch.empty_like(Pd.T).T
    with pytest.raises(_lib.IbhError, match="work must be"):
        ibamd.stage_euler_ssp(c.dpart, Pd, Pd, dt, *QUARTER, out)                   # 3-D: two launches, needs work
    with pytest.raises(_lib.IbhError, match="may not alias"):
        ibamd.update_euler_ssp(Pd, Pd, out, dt, *QUARTER, out=out)
    with pytest.raises(_lib.IbhError, match="work may not alias"):
        ibamd.stage_euler_ssp(c.dpart, Pd, out, dt, *QUARTER, work, work=out)
    with pytest.raises(_lib.IbhError, match="IBH_IMAGE_ONLY"):
        ibamd.stage_euler_ssp(c.dpart, Pd, Pd, dt, *QUARTER, out, work=work, flags=B.IBH_IMAGE_ONLY)
    with pytest.raises(TypeError):
        ibamd.update_euler_ssp(Pd, Pd, out, 1e-3, *QUARTER)                         # a host dt
    with pytest.raises(ValueError):
        ibamd.update_euler_ssp(Pd, Pd[:, :4], out, dt, *QUARTER)                    # P of another shape
    with pytest.raises(ValueError):
        ibamd.stage_euler_ssp(c.dpart, Pd, Pd, dt, *QUARTER, out, scheme="roe")
    with pytest.raises(TypeError):
        ibamd.stage_euler_ssp(c.dpart, Pd, Pd, dt, *QUARTER)                        # out is required
    with pytest.raises(ValueError):
        EulerMarch(c.dpart, FLUID, stages=((0.0, 1.0, 1.0), 0.5))                   # triples and plain coefficients mixed
    with pytest.raises(ValueError):
        EulerMarch(c.dpart, FLUID, stages=((0.0, 1.0),))


# ---------------------------------------------------------------------------------------------------------------------
# march
# ---------------------------------------------------------------------------------------------------------------------
NSTEPS = 5


def composed_march(dpart, P0, scheme, bcs, avg, stages, nsteps, flags=0):
    """The march written out: the time step from the step's input; stage 1 (no blend) through ``update_euler_stage``, the
    others through the six-launch composition; boundary conditions after every stage; one push per step with the full dt.
    ``flags``: those of the residual sweep."""
    P = P0
    for _ in range(nsteps):
        dt = ibamd.timestep_euler(dpart, P, FLUID, SCALE)
        Pk = P
        for k, (a, b, c) in enumerate(stages):
            R = residual(dpart, Pk, scheme, flags)
            if k == 0:
                assert (a, b) == (0.0, 1.0)
                Pk = ibamd.update_euler_stage(Pk, R, dt, c, FLUID)
            else:
                Pk = composed_ssp(P, Pk, R, dt, a, b, c)
            if bcs is not None:
                bcs(Pk)
        if avg is not None:
            avg.push(Pk, dt)
        P = Pk
    return P


@pytest.mark.parametrize("scheme", ["hll", "sensor"])
def test_march_ssp3(march_dom, scheme):
    dom, part, dpart, bcs = march_dom
    P0 = ibamd.hip(rg.euler_regime(part, "transonic"))
    start = P0.clone()
    avg_ref = cfd.TimeAverage(TAU)
    ref = composed_march(dpart, P0, scheme, bcs, avg_ref, ssp_stages(3), NSTEPS)
    assert np.isfinite(ibamd.to_host(ref)).all()

    avg = cfd.TimeAverage(TAU)
    m = EulerMarch(dpart, FLUID, scheme=scheme, scale=SCALE, bcs=bcs, average=avg, stages=ssp_stages(3))
    assert m.stages == ssp_stages(3) and len(m._buf) == 3
    P = P0
    for _ in range(NSTEPS):
        P = m.step(P)
    same_bits(P, ref, f"march {scheme}, ssp3")
    same_bits(avg.mu, avg_ref.mu, "mean")
    same_bits(avg.sigma, avg_ref.sigma, "sigma")
    same_bits(P0, start, "the initial array is left alone")

    # the other two forms of a stage.  A residual callable and the update: the sweep of the one-launch form into ``work``, so
    # the same bits.  ``flags=NO_FUSE``: the sweep into ``work`` and the update, but IBH_NO_FUSE asks for the two-kernel form
    # of the sweep itself, whose residual rounds differently from the single-kernel form's: its bits
    # are those of the composition over that sweep.
    res = (lambda p, Pin, o: ibamd.residual_euler_hll(p, Pin, out=o, fluid=FLUID)) if scheme == "hll" else \
          (lambda p, Pin, o: ibamd.residual_euler_sensor(p, Pin, out=o, fluid=FLUID))
    ref_two = composed_march(dpart, P0, scheme, bcs, None, ssp_stages(3), NSTEPS, flags=NO_FUSE)
    for name, kw, want in (("NO_FUSE", dict(flags=NO_FUSE), ref_two), ("residual=", dict(residual=res), ref)):
        other = EulerMarch(dpart, FLUID, scheme=scheme, scale=SCALE, bcs=bcs, stages=ssp_stages(3), **kw)
        Po = P0
        for _ in range(NSTEPS):
            Po = other.step(Po)
        same_bits(Po, want, f"march {scheme}, ssp3, {name}")
    same_bits(P0, start, "the initial array is left alone by every form")

    # the same steps captured once and replayed: no host read-back, no allocation in a step
    g_m = EulerMarch(dpart, FLUID, scheme=scheme, scale=SCALE, bcs=bcs, stages=ssp_stages(3))
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
        Pg.fill_(NAN)
        graph.replay()
    stream.synchronize()
    B._stream()
    same_bits(Pg, ref, f"march {scheme}, ssp3, graph replay")
    same_bits(P0, start, "the initial array is left alone by the replay")
    del Pw


def test_march_ssp2(march_dom):
    dom, part, dpart, bcs = march_dom
    P0 = ibamd.hip(rg.euler_regime(part, "transonic"))
    m = EulerMarch(dpart, FLUID, scale=SCALE, bcs=bcs, stages=ssp_stages(2))
    P = P0
    for _ in range(2):
        P = m.step(P)
    same_bits(P, composed_march(dpart, P0, "hll", bcs, None, ssp_stages(2), 2), "march hll, ssp2")

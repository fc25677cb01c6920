"""Multi-stage (Runge-Kutta) Euler steps on the device -- ``update_euler_stage``, ``stage_euler``, ``EulerMarch(stages=m)`` --
bit for bit against the compositions of the library's own launches that define them, and against the float64 model of
tests/euler_stage_model.py.  Meshes, states and helpers: those of tests/test_gpu_euler_step.py (``adv``: the one-launch
stage; ``rae6k_2``: skirts and face-list cells; ``corner`` and ``sphere_1``: 3-D).

A stage is defined by two launches the library already has: ``dts = dt .* alpha`` by the broadcast layer with ``alpha`` a
Float32 scalar, then ``update_euler(P0, R, dts)``.
"""

import numpy as np
import pytest
import torch

import euler_stage_model as sm
import euler_step_model as em
import ibamd
import regimes as rg
from ibamd import _lib, cfd
from ibamd import backend as B
from ibamd.hiparray import HipArray as H
from ibamd.solver import EulerMarch, rk_stages
from test_gpu_euler_step import (FLUID, ONE_LAUNCH, SCALE, STEP_CASES, TAU, march_dom, meshes, padded, residual, rows,  # noqa: F401
                                 same_bits)

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
THIRD = float(f32(1.0) / f32(3.0))
ALPHAS = [1.0, THIRD, 0.25]
NAN = float("nan")


def stage_dt(dtd, alpha):
    """dt .* alpha by the broadcast layer, alpha a Float32 scalar."""
    return (H(dtd) * float(f32(alpha))).t


def composed_stage(P0d, Rd, dtd, alpha):
    return ibamd.update_euler(P0d, Rd, stage_dt(dtd, alpha), FLUID)


# ---------------------------------------------------------------------------------------------------------------------
# update
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", ALPHAS, ids=["one", "third", "quarter"])
@pytest.mark.parametrize("per_cell", [False, True], ids=["global_dt", "per_cell_dt"])
@pytest.mark.parametrize("nd", [2, 3])
@pytest.mark.parametrize("n", [1, 77, 2048 * 256 + 77])
def test_update_stage_bit_for_bit(n, nd, per_cell, alpha):
    """One row, less than a workgroup, and past the grid cap of 2 048 workgroups of 256 (the grid-stride loop)."""
    P, R, dt, Pd, Rd, dtd, ref_step = rows(n, nd, per_cell)
    ref = composed_stage(Pd, Rd, dtd, alpha)
    if alpha == 1.0:
        same_bits(ref, ref_step, "alpha = 1: the composition is update_euler's")
        same_bits(ref, ibamd.update_euler(Pd, Rd, dtd, FLUID), "alpha = 1: update_euler")
    out = B.colmajor_empty(n, nd + 2)
    out.fill_(NAN)
    assert ibamd.update_euler_stage(Pd, Rd, dtd, alpha, FLUID, out=out) is out
    same_bits(out, ref, "out of place")
    assert np.isfinite(ibamd.to_host(out)).all()
    same_bits(ibamd.update_euler_stage(Pd, Rd, dtd, alpha, FLUID), ref, "allocated")
    inplace = Pd.clone()
    ibamd.update_euler_stage(inplace, Rd, dtd, alpha, FLUID, out=inplace)
    same_bits(inplace, ref, "out is P0")
    base = torch.full((nd + 2, n + 29), NAN, dtype=torch.float32, device="cuda")
    Pp, Rp, Op = padded(n, nd + 2, 13), padded(n, nd + 2, 5), base.T[:n]
    Pp.copy_(Pd)
    Rp.copy_(Rd)
    ibamd.update_euler_stage(Pp, Rp, dtd, alpha, FLUID, out=Op)
    same_bits(Op, ref, "padded")
    assert torch.isnan(base[:, n:]).all()                                       # nothing written past row n
    if per_cell:                                     # a per-cell dt that starts one element into a larger array
        big = torch.full((n + 3,), NAN, dtype=torch.float32, device="cuda")
        view = big[1:n + 1]
        view.copy_(dtd)
        assert view.data_ptr() % 16 == 4
        same_bits(ibamd.update_euler_stage(Pd, Rd, view, alpha, FLUID), ref, "per-cell dt off the 16-byte grid")


@pytest.mark.parametrize("nd", [2, 3])
def test_update_stage_nan_and_vacuum_rows(nd):
    """The rows of test_update_nan_and_vacuum_rows -- a NaN row and rows with rho -> 0 -- with the stage's time step: the
    NaN / Inf pattern of the composition."""
    P, R, dt = em.synthetic_rows(300, nd)
    h = f32(dt) * f32(THIRD)                               # the time step the stage uses
    P[7] = np.nan
    P[11, 1] = np.nan
    P[19, 0] = 0.0
    R[19] = 0.0
    R[23, 0] = np.nan
    rho = P[31, 0] / (f32(283.0) * P[31, 1])
    R[31, 0] = -rho / h
    P[40, 0] = 0.0
    Pd, Rd = ibamd.hip(P), ibamd.hip(R)
    dtd = torch.tensor([float(dt)], dtype=torch.float32, device="cuda")
    ref = composed_stage(Pd, Rd, dtd, THIRD)
    got = ibamd.update_euler_stage(Pd, Rd, dtd, THIRD, FLUID)
    same_bits(got, ref, "special rows")
    g, r = ibamd.to_host(got), ibamd.to_host(ref)
    assert np.array_equal(np.isinf(g), np.isinf(r)) and np.array_equal(np.signbit(g)[np.isinf(r)], np.signbit(r)[np.isinf(r)])
    assert np.isnan(g[7]).all() and not np.isfinite(g[19]).all()
    ok = np.setdiff1d(np.arange(300), [7, 11, 19, 23, 31, 40])
    assert np.isfinite(g[ok]).all()


@pytest.mark.parametrize("per_cell", [False, True], ids=["global_dt", "per_cell_dt"])
@pytest.mark.parametrize("nd", [2, 3])
def test_update_stage_against_float64(nd, per_cell):
    """Per element against the float64 model: 4 x the Float32 step model's own deviation (euler_step_model.
    MODEL_DEVIATION_EPS), the margin ``update_euler`` is held to."""
    P, R, dt, Pd, Rd, dtd, _ = rows(20000, nd, per_cell)
    got = ibamd.to_host(ibamd.update_euler_stage(Pd, Rd, dtd, THIRD, FLUID))
    dev = sm.update_stage_deviation(got, P, R, dt, THIRD)
    model = sm.update_stage_deviation(sm.update_stage(P, R, dt, THIRD, f32), P, R, dt, THIRD)
    print(f"update_euler_stage nd={nd} per_cell={per_cell}: device {dev:.3f} eps, Float32 model {model:.3f} eps, "
          f"bound {4 * em.MODEL_DEVIATION_EPS[nd]:.1f} eps")
    assert dev <= 4 * em.MODEL_DEVIATION_EPS[nd]


# ---------------------------------------------------------------------------------------------------------------------
# stage
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", ["hll", "sensor"])
@pytest.mark.parametrize("mesh,flags", STEP_CASES, ids=[f"{m}-{f}" for m, f in STEP_CASES])
def test_stage_bit_for_bit(meshes, mesh, flags, scheme):
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
        for dt, dname in ((dt1, "global dt"), (cells, "per-cell dt")):
            what = f"{mesh} flags={flags} {scheme} {regime} {dname}"
            ref = ibamd.update_euler_stage(P0, R, dt, THIRD, FLUID)
            work.fill_(NAN)                                  # a row the sweep or the update leaves unwritten shows
            out.fill_(NAN)
            assert ibamd.stage_euler(c.dpart, Pd, P0, dt, THIRD, out, FLUID, scheme, work=work, flags=flags) is out
            same_bits(out, ref, what)
            finite_R = np.isfinite(ibamd.to_host(R)).all(axis=1)
            assert finite_R.any() and np.isfinite(ibamd.to_host(out)[finite_R]).all(), what
            if one_launch:                                   # the sweep stores the update itself: no work array
                assert torch.isnan(work).all(), what + ": the one-launch form left work alone"
                out.fill_(NAN)
                ibamd.stage_euler(c.dpart, Pd, P0, dt, THIRD, out, FLUID, scheme, flags=flags)
                same_bits(out, ref, what + " without work")
                po = padded(n, nv, 19, fill=NAN)
                ibamd.stage_euler(c.dpart, Pd, P0, dt, THIRD, po, FLUID, scheme, flags=flags)
                same_bits(po, ref, what + " padded out")
                base = P0.clone()
                ibamd.stage_euler(c.dpart, Pd, base, dt, THIRD, base, FLUID, scheme, flags=flags)
                same_bits(base, ref, what + " out is P0")
            else:
                with pytest.raises(_lib.IbhError, match="work must be"):
                    ibamd.stage_euler(c.dpart, Pd, P0, dt, THIRD, out, FLUID, scheme, flags=flags)
            # out is P: the two-launch form everywhere
            inplace = Pd.clone()
            work.fill_(NAN)
            ibamd.stage_euler(c.dpart, inplace, P0, dt, THIRD, inplace, FLUID, scheme, work=work, flags=flags)
            same_bits(inplace, ref, what + " out is P")
            inplace.copy_(Pd)
            with pytest.raises(_lib.IbhError, match="work must be"):
                ibamd.stage_euler(c.dpart, inplace, P0, dt, THIRD, inplace, FLUID, scheme, flags=flags)
        if regime == "transonic":
            # alpha = 1 on the step's own state: the bits of step_euler
            ref1 = B.colmajor_empty(n, nv)
            ibamd.step_euler(c.dpart, P0, dt1, ref1, FLUID, scheme, work=work, flags=flags)
            out.fill_(NAN)
            ibamd.stage_euler(c.dpart, P0, P0, dt1, 1.0, out, FLUID, scheme, work=work, flags=flags)
            same_bits(out, ref1, f"{mesh} flags={flags} {scheme}: alpha = 1, P0 = P")


def test_python_layer_rejects_misuse(meshes):
    c = meshes["corner"]
    Pd = ibamd.hip(rg.euler_regime(c.part, "rest"))
    dt = torch.ones(1, dtype=torch.float32, device="cuda")
    out = torch.empty_like(Pd.T).T
    work = torch.empty_like(Pd.T).T
    with pytest.raises(_lib.IbhError, match="work must be"):
        ibamd.stage_euler(c.dpart, Pd, Pd, dt, 0.5, out)                            # 3-D: two launches, needs work
    with pytest.raises(_lib.IbhError, match="may not alias"):
        ibamd.update_euler_stage(Pd, out, dt, 0.5, out=out)
    with pytest.raises(_lib.IbhError, match="work may not alias"):
        ibamd.stage_euler(c.dpart, Pd, out, dt, 0.5, work, work=out)
    with pytest.raises(_lib.IbhError, match="IBH_IMAGE_ONLY"):
        ibamd.stage_euler(c.dpart, Pd, Pd, dt, 0.5, out, work=work, flags=B.IBH_IMAGE_ONLY)
    with pytest.raises(TypeError):
        ibamd.update_euler_stage(Pd, out, 1e-3, 0.5)                                # a host dt
    with pytest.raises(ValueError):
        ibamd.stage_euler(c.dpart, Pd, Pd, dt, 0.5, out, scheme="roe")
    with pytest.raises(ValueError):
        EulerMarch(c.dpart, FLUID, stages=0)
    with pytest.raises(ValueError):
        EulerMarch(c.dpart, FLUID, stages=())


# ---------------------------------------------------------------------------------------------------------------------
# march
# ---------------------------------------------------------------------------------------------------------------------
NSTEPS = 5


def composed_march(dpart, P0, scheme, bcs, avg, alphas, nsteps, local_dt=False):
    """The march written out: time step from the step's input, per stage the sweep of the previous stage and the update of
    the input, boundary conditions after every stage, one push per step with the full dt."""
    P = P0
    for _ in range(nsteps):
        if local_dt:
            dt = ibamd.timestep_euler(dpart, P, FLUID, SCALE, out=False, cells=B.colmajor_empty(P.shape[0]))
        else:
            dt = ibamd.timestep_euler(dpart, P, FLUID, SCALE)
        Pk = P
        for a in alphas:
            Pk = ibamd.update_euler_stage(P, residual(dpart, Pk, scheme, 0), dt, a, FLUID)
            if bcs is not None:
                bcs(Pk)
        if avg is not None:
            avg.push(Pk, dt)
        P = Pk
    return P


@pytest.mark.parametrize("scheme", ["hll", "sensor"])
def test_march_four_stages(march_dom, scheme):
    dom, part, dpart, bcs = march_dom
    P0 = ibamd.hip(rg.euler_regime(part, "transonic"))
    start = P0.clone()
    avg_ref = cfd.TimeAverage(TAU)
    ref = composed_march(dpart, P0, scheme, bcs, avg_ref, rk_stages(4), NSTEPS)
    assert np.isfinite(ibamd.to_host(ref)).all()

    avg = cfd.TimeAverage(TAU)
    m = EulerMarch(dpart, FLUID, scheme=scheme, scale=SCALE, bcs=bcs, average=avg, stages=4)
    assert m.stages == rk_stages(4)
    P = P0
    for _ in range(NSTEPS):
        P = m.step(P)
    same_bits(P, ref, f"march {scheme}, 4 stages")
    same_bits(avg.mu, avg_ref.mu, "mean")
    same_bits(avg.sigma, avg_ref.sigma, "sigma")
    same_bits(P0, start, "the initial array is left alone")

    # the same steps captured once and replayed: no host read-back, no allocation in a step
    g_m = EulerMarch(dpart, FLUID, scheme=scheme, scale=SCALE, bcs=bcs, stages=4)
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
    same_bits(Pg, ref, f"march {scheme}, 4 stages, graph replay")
    same_bits(P0, start, "the initial array is left alone by the replay")
    del Pw


def test_march_stage_forms(march_dom):
    """``local_dt`` with three stages and ``residual=`` with two against their compositions; one stage against today's
    march."""
    dom, part, dpart, bcs = march_dom
    P0 = ibamd.hip(rg.euler_regime(part, "transonic"))
    local = EulerMarch(dpart, FLUID, scale=SCALE, bcs=bcs, local_dt=True, stages=3)
    P = P0
    for _ in range(2):
        P = local.step(P)
    same_bits(P, composed_march(dpart, P0, "hll", bcs, None, rk_stages(3), 2, local_dt=True), "local_dt, 3 stages")

    m = EulerMarch(dpart, FLUID, scale=SCALE, stages=2,
                   residual=lambda p, P, out: ibamd.residual_euler_hll(p, P, out=out, fluid=FLUID))
    plain = EulerMarch(dpart, FLUID, scale=SCALE, stages=2)
    same_bits(m.step(m.step(P0)), plain.step(plain.step(P0)), "residual=, 2 stages")
    same_bits(plain.step(plain.step(P0)), composed_march(dpart, P0, "hll", None, None, rk_stages(2), 2), "2 stages")

    today = EulerMarch(dpart, FLUID, scale=SCALE, bcs=bcs)
    Pt = P0
    for _ in range(3):
        Pt = today.step(Pt)
    for stages in ((1.0,), 1):
        one = EulerMarch(dpart, FLUID, scale=SCALE, bcs=bcs, stages=stages)
        assert len(one._buf) == 2
        Po = P0
        for _ in range(3):
            Po = one.step(Po)
        same_bits(Po, Pt, f"stages={stages!r} is today's march")
    with pytest.raises(ValueError):
        EulerMarch(dpart, FLUID, local_dt=True, average=cfd.TimeAverage(TAU), stages=3)

"""Multi-stage (Runge-Kutta) Euler steps on the device -- ``update_euler_stage``, ``stage_euler``, ``EulerMarch(stages=m)`` --
bit for bit against the compositions of the library's own launches that define them, and against the float64 model of
tests/euler_stage_model.py.  Meshes, states and helpers: those of tests/euler_forms.py (``adv``: the one-launch
stage; ``rae6k_2``: skirts and face-list cells; ``corner`` and ``sphere_1``: 3-D).

A stage is defined by two launches the library already has: ``dts = dt .* alpha`` by the broadcast layer with ``alpha`` a
Float32 scalar, then ``update_euler(P0, R, dts)``.
"""

import numpy as np
import pytest
import torch

import euler_forms as ef
import ibamd
import regimes as rg
from euler_forms import FLUID, NAN, SCALE, STEP_CASES, TAU, march_dom, meshes, residual, same_bits  # noqa: F401
from ibamd import _lib, cfd
from ibamd import backend as B
from ibamd.solver import EulerMarch, rk_stages

pytestmark = pytest.mark.gpu
ALPHAS = ef.STAGE.coefs


# ---------------------------------------------------------------------------------------------------------------------
# update
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", list(ALPHAS.values()), ids=list(ALPHAS))
@pytest.mark.parametrize("per_cell", [False, True], ids=["global_dt", "per_cell_dt"])
@pytest.mark.parametrize("nd", [2, 3])
@pytest.mark.parametrize("n", [1, 77, 2048 * 256 + 77])
def test_update_stage_bit_for_bit(n, nd, per_cell, alpha):
    """One row, less than a workgroup, and past the grid cap of 2 048 workgroups of 256 (the grid-stride loop)."""
    a, ref = ef.check_update_bit_for_bit(ef.STAGE, n, nd, per_cell, alpha)
    if alpha == (1.0,):
        s, refs = ef.rows(ef.STEP, n, nd, per_cell)[1:]
        if ((), None) not in refs:
            refs[(), None] = ef.composed_update(s.P, s.R, s.dt)
        same_bits(ref, refs[(), None], "alpha = 1: the composition is update_euler's")
        same_bits(ref, ibamd.update_euler(a.P0, a.R, a.dt, FLUID), "alpha = 1: update_euler")


@pytest.mark.parametrize("nd", [2, 3])
def test_update_stage_nan_and_vacuum_rows(nd):
    """The rows of test_update_nan_and_vacuum_rows -- a NaN row and rows with rho -> 0 -- with the stage's time step: the
    NaN / Inf pattern of the composition."""
    ef.check_update_special_rows(ef.STAGE, nd)


@pytest.mark.parametrize("per_cell", [False, True], ids=["global_dt", "per_cell_dt"])
@pytest.mark.parametrize("nd", [2, 3])
def test_update_stage_against_float64(nd, per_cell):
    """Per element against the float64 model: 4 x the Float32 step model's own deviation (euler_step_model.
    MODEL_DEVIATION_EPS), the margin ``update_euler`` is held to."""
    ef.check_update_against_float64(ef.STAGE, nd, per_cell)


# ---------------------------------------------------------------------------------------------------------------------
# stage
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", ["hll", "sensor"])
@pytest.mark.parametrize("mesh,flags", STEP_CASES, ids=[f"{m}-{f}" for m, f in STEP_CASES])
def test_stage_bit_for_bit(meshes, mesh, flags, scheme):
    ef.check_stage_bit_for_bit(ef.STAGE, meshes, mesh, flags, scheme)
    # alpha = 1 on the step's own state: the bits of step_euler
    c = meshes[mesh]
    n, nv = c.part.spacing.shape[0], c.nd + 2
    P0 = ibamd.hip(rg.euler_regime(c.part, "transonic"))
    dt1 = ibamd.timestep_euler(c.dpart, P0, FLUID, SCALE)
    work, out, ref1 = (B.colmajor_empty(n, nv) for _ in range(3))
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
    Pg = ef.replayed_march(lambda: EulerMarch(dpart, FLUID, scheme=scheme, scale=SCALE, bcs=bcs, stages=4), P0, NSTEPS)
    same_bits(Pg, ref, f"march {scheme}, 4 stages, graph replay")
    same_bits(P0, start, "the initial array is left alone by the replay")


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

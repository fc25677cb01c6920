"""Shu-Osher (strong-stability-preserving) Runge-Kutta stages on the device -- ``update_euler_ssp``, ``stage_euler_ssp``,
``EulerMarch(stages=ssp_stages(order))`` -- bit for bit against the composition of the library's own launches that defines
them, and against the float64 model of tests/euler_ssp_model.py.  Meshes, states and helpers: those of
tests/euler_forms.py.

The composition (six kinds of launch): ``primitive2state`` of ``P0`` and of ``P``; ``dts = dt .* c`` and, per column,
``T = Q0 .* a .+ Q .* b`` by the broadcast layer with Float32 scalars; per column ``ibh_update_dev(dts, T, R)`` (a per-cell
``dt``: the broadcasts ``R .* dts`` and ``T .+ ...``); ``state2primitive``.
"""

import numpy as np
import pytest
import torch

import euler_forms as ef
import ibamd
import regimes as rg
from euler_forms import (FLUID, NO_FUSE, QUARTER, SCALE, STEP_CASES, TAU, composed_ssp, march_dom, meshes,  # noqa: F401
                         residual, same_bits)
from ibamd import _lib, cfd
from ibamd import backend as B
from ibamd.solver import EulerMarch, ssp_stages

pytestmark = pytest.mark.gpu
ABCS = ef.SSP.coefs


# ---------------------------------------------------------------------------------------------------------------------
# update
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("abc", list(ABCS.values()), ids=list(ABCS))
@pytest.mark.parametrize("per_cell", [False, True], ids=["global_dt", "per_cell_dt"])
@pytest.mark.parametrize("nd", [2, 3])
@pytest.mark.parametrize("n", [1, 77, 2048 * 256 + 77])
def test_update_ssp_bit_for_bit(n, nd, per_cell, abc):
    """One row, less than a workgroup, and past the grid cap of 2 048 workgroups of 256 (the grid-stride loop)."""
    a, _ = ef.check_update_bit_for_bit(ef.SSP, n, nd, per_cell, abc)
    assert not torch.equal(a.P0, a.P)
    same_bits(ibamd.update_euler_ssp(a.P, a.P, a.R, a.dt, *abc, FLUID), composed_ssp(a.P, a.P, a.R, a.dt, *abc), "P0 is P")


@pytest.mark.parametrize("nd", [2, 3])
def test_update_ssp_nan_and_vacuum_rows(nd):
    """The rows of test_update_stage_nan_and_vacuum_rows -- a NaN row, a NaN temperature, p = 0, a NaN residual, rho -> 0 --
    placed in P0 (rows 7 .. 40) and in P (rows 107 .. 140): the NaN / Inf pattern of the composition."""
    ef.check_update_special_rows(ef.SSP, nd)


@pytest.mark.parametrize("per_cell", [False, True], ids=["global_dt", "per_cell_dt"])
@pytest.mark.parametrize("nd", [2, 3])
def test_update_ssp_against_float64(nd, per_cell):
    """Per element against the float64 model on the update's own scale (``euler_ssp_model.update_ssp_scale``:
    ``euler_step_model.update_scale`` with the blend as the base state): at most 4 x the deviation of the Float32 numpy model
    on the same rows, computed here -- the margin ``update_euler`` and ``update_euler_stage`` are held to, for rounding order
    inside a sum."""
    ef.check_update_against_float64(ef.SSP, nd, per_cell)


# ---------------------------------------------------------------------------------------------------------------------
# stage
# ---------------------------------------------------------------------------------------------------------------------
# (every SSP instantiation of both 2-D sweeps kept its sibling's occupancy without scratch and its timing range lies below the
# two-launch form's, profiles/euler_ssp: the one-launch set is that of step_euler and stage_euler)
@pytest.mark.parametrize("scheme", ["hll", "sensor"])
@pytest.mark.parametrize("mesh,flags", STEP_CASES, ids=[f"{m}-{f}" for m, f in STEP_CASES])
def test_stage_ssp_bit_for_bit(meshes, mesh, flags, scheme):
    ef.check_stage_bit_for_bit(ef.SSP, meshes, mesh, flags, scheme)


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
    Pg = ef.replayed_march(lambda: EulerMarch(dpart, FLUID, scheme=scheme, scale=SCALE, bcs=bcs, stages=ssp_stages(3)), P0,
                           NSTEPS)
    same_bits(Pg, ref, f"march {scheme}, ssp3, graph replay")
    same_bits(P0, start, "the initial array is left alone by the replay")


def test_march_ssp2(march_dom):
    dom, part, dpart, bcs = march_dom
    P0 = ibamd.hip(rg.euler_regime(part, "transonic"))
    m = EulerMarch(dpart, FLUID, scale=SCALE, bcs=bcs, stages=ssp_stages(2))
    P = P0
    for _ in range(2):
        P = m.step(P)
    same_bits(P, composed_march(dpart, P0, "hll", bcs, None, ssp_stages(2), 2), "march hll, ssp2")

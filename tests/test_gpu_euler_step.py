"""The explicit Euler step on the device -- ``timestep_euler``, ``update_euler``, ``step_euler``, ``EulerMarch`` -- bit for bit
against the compositions of the library's own launches that they replace, and against the float64 models of
tests/euler_step_model.py.  Meshes: the four of tests/test_gpu_percell_regimes.py (``adv``: every block in quads, pairs or
singles, the one-launch step; ``rae6k_2``: skirts and face-list cells; ``corner`` and ``sphere_1``: 3-D); states:
``regimes.euler_regime``.
"""

import numpy as np
import pytest
import torch

import euler_forms as ef
import euler_step_model as em
import ibamd
import percell_steps as ps
import regimes as rg
from euler_forms import (FLUID, MESHES, SCALE, STEP_CASES, TAU, composed_update, march_dom, meshes, padded,  # noqa: F401
                         residual, same_bits)
from ibamd import _lib, cfd
from ibamd import backend as B
from ibamd.hiparray import HipArray as H
from ibamd.solver import EulerMarch

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
DT_REGIMES = ("transonic", "crossing", "rest", "cold")


# ---------------------------------------------------------------------------------------------------------------------
# time step
# ---------------------------------------------------------------------------------------------------------------------
def materialised_C(Pd):
    """C_d = abs.(u_d) .+ speed_of_sound(fluid, T) by the IEEE path: ibh_cfd_speed_of_sound, then HipArray abs and +."""
    n, nd = Pd.shape[0], Pd.shape[1] - 2
    a = cfd.speed_of_sound(FLUID, Pd[:, 1].contiguous())
    Cd = B.colmajor_empty(n, nd)
    for d in range(nd):
        Cd[:, d] = (abs(H(Pd[:, 2 + d].contiguous())) + H(a)).t
    return Cd


def composed_dt_cells(dpart, Cd, scale):
    per = None
    for d in range(Cd.shape[1]):
        g = ibamd.unsigned_green_gauss(dpart, ibamd.at_faces(dpart, Cd[:, d].contiguous(), d + 1), d + 1)
        per = g if per is None else H(per).maximum_with(H(g)).t
    return ((0.5 / H(per)) * scale).t


@pytest.mark.parametrize("regime", DT_REGIMES)
@pytest.mark.parametrize("mesh", MESHES)
def test_timestep_bit_for_bit_and_against_float64(meshes, mesh, regime):
    c = meshes[mesh]
    P = rg.euler_regime(c.part, regime)
    if regime == "cold":
        assert (P[:, 1] < 10).any()
    Pd = ibamd.hip(P)
    Cd = materialised_C(Pd)
    ref_dt = ibamd.timestep_advection(c.dpart, Cd, scale=SCALE)
    cells = B.colmajor_empty(P.shape[0])
    cells.fill_(float("nan"))
    dt = ibamd.timestep_euler(c.dpart, Pd, FLUID, SCALE, cells=cells)
    same_bits(dt, ref_dt, f"{mesh} {regime} dt")
    same_bits(cells, composed_dt_cells(c.dpart, Cd, SCALE), f"{mesh} {regime} dt_cells")
    assert float(dt.item()) == float(ibamd.to_host(cells).min())
    # each output alone: the same values (dt_cells alone is one launch)
    same_bits(ibamd.timestep_euler(c.dpart, Pd, FLUID, SCALE), ref_dt, "dt alone")
    only = torch.full_like(cells, float("nan"))
    assert ibamd.timestep_euler(c.dpart, Pd, FLUID, SCALE, out=False, cells=only) is only
    same_bits(only, cells, "dt_cells alone")
    # padded leading dimension
    Pp = padded(P.shape[0], P.shape[1])
    Pp.copy_(Pd)
    same_bits(ibamd.timestep_euler(c.dpart, Pp, FLUID, SCALE), ref_dt, "padded P")
    # float64 model, at the bound the advection time step is held to
    ref64, _ = em.timestep(c.op, P, SCALE, f64)
    err = ps.check_dt(dt.item(), ref64, f"{mesh} {regime}")
    print(f"timestep_euler {mesh} {regime}: dt {dt.item():.6e}, {err / ps.ULP:.2f} ulp from float64")


# ---------------------------------------------------------------------------------------------------------------------
# update
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_cell", [False, True], ids=["global_dt", "per_cell_dt"])
@pytest.mark.parametrize("nd", [2, 3])
@pytest.mark.parametrize("n", [1, 77, 2048 * 256 + 77])
def test_update_bit_for_bit(n, nd, per_cell):
    """One row, less than a workgroup, and past the grid cap of 2 048 workgroups of 256 (the grid-stride loop)."""
    ef.check_update_bit_for_bit(ef.STEP, n, nd, per_cell)


@pytest.mark.parametrize("nd", [2, 3])
def test_update_nan_and_vacuum_rows(nd):
    """A NaN row and rows with rho -> 0 (p = 0; dt R_rho = -rho): the NaN / Inf pattern of the composition."""
    ef.check_update_special_rows(ef.STEP, nd)


@pytest.mark.parametrize("per_cell", [False, True], ids=["global_dt", "per_cell_dt"])
@pytest.mark.parametrize("nd", [2, 3])
def test_update_against_float64(nd, per_cell):
    """Per element against the float64 model: 4 x the Float32 model's own deviation (euler_step_model.MODEL_DEVIATION_EPS,
    measured in tests/test_euler_step_model.py) -- the margin for rounding order inside a sum."""
    ef.check_update_against_float64(ef.STEP, nd, per_cell)


def test_python_layer_rejects_misuse(meshes):
    c = meshes["corner"]
    Pd = ibamd.hip(rg.euler_regime(c.part, "rest"))
    dt = torch.ones(1, dtype=torch.float32, device="cuda")
    out = torch.empty_like(Pd.T).T
    with pytest.raises(_lib.IbhError, match="work must be"):
        ibamd.step_euler(c.dpart, Pd, dt, out)                                   # 3-D: two launches, needs work
    with pytest.raises(_lib.IbhError, match="may not alias"):
        ibamd.update_euler(Pd, out, dt, out=out)
    with pytest.raises(_lib.IbhError, match="IBH_IMAGE_ONLY"):
        ibamd.step_euler(c.dpart, Pd, dt, out, work=torch.empty_like(out.T).T, flags=B.IBH_IMAGE_ONLY)
    with pytest.raises(TypeError):
        ibamd.update_euler(Pd, out, 1e-3)                                        # a host dt
    with pytest.raises(ValueError):
        ibamd.update_euler(Pd, out, torch.ones(3, dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError):
        ibamd.step_euler(c.dpart, Pd, dt, out, scheme="roe")
    with pytest.raises(TypeError):
        ibamd.step_euler(c.dpart, Pd, dt, torch.empty((Pd.shape[0], Pd.shape[1]), dtype=torch.float32, device="cuda"))
    # a work that aliases P or out is rejected on the one-launch path too, where it would not be used: nothing is launched
    a = meshes["adv"]
    Pa = ibamd.hip(rg.euler_regime(a.part, "rest"))
    oa = B.colmajor_empty(*Pa.shape)
    oa.fill_(float("nan"))
    for work in (Pa, oa):
        with pytest.raises(_lib.IbhError, match="work may not alias"):
            ibamd.step_euler(a.dpart, Pa, dt, oa, FLUID, "hll", work=work, flags=0)
        assert torch.isnan(oa).all()


# ---------------------------------------------------------------------------------------------------------------------
# step
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", ["hll", "sensor"])
@pytest.mark.parametrize("mesh,flags", STEP_CASES, ids=[f"{m}-{f}" for m, f in STEP_CASES])
def test_step_bit_for_bit(meshes, mesh, flags, scheme):
    ef.check_stage_bit_for_bit(ef.STEP, meshes, mesh, flags, scheme)


# ---------------------------------------------------------------------------------------------------------------------
# march
# ---------------------------------------------------------------------------------------------------------------------
NSTEPS = 20


def composed_march(dpart, P0, scheme, bcs, avg):
    P = P0
    for _ in range(NSTEPS):
        dt = ibamd.timestep_advection(dpart, materialised_C(P), scale=SCALE)
        P = composed_update(P, residual(dpart, P, scheme, 0), dt)
        bcs(P)
        avg.push(P, dt)
    return P


@pytest.mark.parametrize("scheme", ["hll", "sensor"])
def test_march(march_dom, scheme):
    dom, part, dpart, bcs = march_dom
    assert dpart.info["fusable_blocks"] == dpart.info["full_blocks"] > 0 and dpart.info["irregular_cells"] == 0
    assert sum(b.ghost_indices.size for name in ("outlet", "lower", "upper") for b in dom.boundaries[name].values()) > 0
    P0 = ibamd.hip(rg.euler_regime(part, "transonic"))
    start = P0.clone()
    avg_ref = cfd.TimeAverage(TAU)
    ref = composed_march(dpart, P0, scheme, bcs, avg_ref)
    assert np.isfinite(ibamd.to_host(ref)).all()

    avg = cfd.TimeAverage(TAU)
    m = EulerMarch(dpart, FLUID, scheme=scheme, scale=SCALE, bcs=bcs, average=avg)
    P = P0
    for _ in range(NSTEPS):
        P = m.step(P)
    same_bits(P, ref, f"march {scheme}")
    same_bits(avg.mu, avg_ref.mu, "mean")
    same_bits(avg.sigma, avg_ref.sigma, "sigma")
    same_bits(P0, start, "the initial array is left alone")

    # the same steps captured once and replayed: no host read-back, no allocation in a step
    Pg = ef.replayed_march(lambda: EulerMarch(dpart, FLUID, scheme=scheme, scale=SCALE, bcs=bcs), P0, NSTEPS)
    same_bits(Pg, ref, f"march {scheme}, graph replay")
    same_bits(P0, start, "the initial array is left alone by the replay")


def test_march_forms(march_dom):
    """``residual=`` (a callable followed by update_euler), ``dt_every`` and ``local_dt`` against their compositions."""
    dom, part, dpart, bcs = march_dom
    P0 = ibamd.hip(rg.euler_regime(part, "transonic"))
    m = EulerMarch(dpart, FLUID, scale=SCALE, residual=lambda p, P, out: ibamd.residual_euler_hll(p, P, out=out, fluid=FLUID))
    plain = EulerMarch(dpart, FLUID, scale=SCALE)
    same_bits(m.step(m.step(P0)), plain.step(plain.step(P0)), "residual=")
    every = EulerMarch(dpart, FLUID, scale=SCALE, dt_every=2)
    dt0 = ibamd.timestep_euler(dpart, P0, FLUID, SCALE)
    P1 = ibamd.update_euler(P0, residual(dpart, P0, "hll", 0), dt0, FLUID)
    P2 = ibamd.update_euler(P1, residual(dpart, P1, "hll", 0), dt0, FLUID)
    same_bits(every.step(every.step(P0)), P2, "dt_every=2 keeps the time step for two steps")
    local = EulerMarch(dpart, FLUID, scale=SCALE, local_dt=True)
    cells = ibamd.timestep_euler(dpart, P0, FLUID, SCALE, out=False, cells=B.colmajor_empty(P0.shape[0]))
    same_bits(local.step(P0), ibamd.update_euler(P0, residual(dpart, P0, "hll", 0), cells, FLUID), "local_dt")
    with pytest.raises(ValueError):
        EulerMarch(dpart, FLUID, local_dt=True, average=cfd.TimeAverage(TAU))

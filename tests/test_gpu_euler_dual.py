"""Dual time stepping on the device -- ``dual_source``, ``update_euler_dual``, ``stage_euler_dual``, ``DualTimeMarch`` -- bit
for bit against the composition of the library's own launches that defines them, against the float64 model of
tests/euler_dual_model.py, and the contraction of the inner iteration on the residual of the backward-difference equation.
Meshes, states and helpers: those of tests/euler_forms.py.

The composition: ``primitive2state`` of ``P0``; ``h = dt .* alpha`` and ``den = h .* g .+ 1`` by the broadcast layer with
Float32 scalars; per column ``RS = R .+ S``, ``ibh_update_dev(h, Q0, RS)`` (a per-cell ``dt``: the broadcasts ``RS .* h`` and
``Q0 .+ ...``) and ``./ den``; ``state2primitive``.  The source: ``primitive2state`` twice and ``Qn .* cn .+ Qm .* cm``.
"""

import numpy as np
import pytest
import torch

import euler_dual_model as dm
import euler_forms as ef
import euler_step_model as em
import ibamd
import regimes as rg
from euler_forms import FLUID, NAN, SCALE, STEP_CASES, THIRD, col, meshes, padded, same_bits  # noqa: F401
from ibamd import _lib, cfd
from ibamd import backend as B
from ibamd.hiparray import HipArray as H
from ibamd.solver import DualTimeMarch, bdf_coefficients, rk_stages

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
ALPHAS = ef.DUAL.coefs


def composed_source(Pnd, Pmd, cn, cm):
    n, nv = Pnd.shape
    cn, cm = float(f32(cn)), float(f32(cm))
    Qn = cfd.primitive2state(FLUID, Pnd)
    Qm = cfd.primitive2state(FLUID, Pmd) if Pmd is not None else None
    S = B.colmajor_empty(n, nv)
    for v in range(nv):
        S[:, v] = ((H(col(Qn, v)) * cn + H(col(Qm, v)) * cm) if Qm is not None else (H(col(Qn, v)) * cn)).t
    return S


# ---------------------------------------------------------------------------------------------------------------------
# source and update
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nd", [2, 3])
@pytest.mark.parametrize("n", [1, 77, 2048 * 256 + 77])
def test_dual_source_bit_for_bit(n, nd):
    Pn, _, _ = em.synthetic_rows(n, nd, seed=11)
    Pm, _, _ = em.synthetic_rows(n, nd)
    Pnd, Pmd = ibamd.hip(Pn), ibamd.hip(Pm)
    cn, cm, _ = bdf_coefficients(2, 8 * dm.DT0)
    for second in (Pmd, None):
        what = "BDF2" if second is not None else "BDF1"
        ref = composed_source(Pnd, second, cn, cm)
        out = B.colmajor_empty(n, nd + 2)
        out.fill_(NAN)
        assert ibamd.dual_source(Pnd, second, cn, cm, FLUID, out=out) is out
        same_bits(out, ref, what)
        assert np.isfinite(ibamd.to_host(out)).all()
        same_bits(ibamd.dual_source(Pnd, second, cn, cm, FLUID), ref, what + " allocated")
        base = torch.full((nd + 2, n + 29), NAN, dtype=torch.float32, device="cuda")
        Np, Mp, Op = padded(n, nd + 2, 7), padded(n, nd + 2, 13), base.T[:n]
        Np.copy_(Pnd)
        Mp.copy_(Pmd)
        ibamd.dual_source(Np, Mp if second is not None else None, cn, cm, FLUID, out=Op)
        same_bits(Op, ref, what + " padded")
        assert torch.isnan(base[:, n:]).all()                                   # nothing written past row n
    same_bits(ibamd.dual_source(Pnd, Pnd, cn, cm, FLUID), composed_source(Pnd, Pnd, cn, cm), "Pm is Pn")


@pytest.mark.parametrize("bdf2_g", [False, True], ids=["g0", "gbdf2"])
@pytest.mark.parametrize("alpha", list(ALPHAS.values()), ids=list(ALPHAS))
@pytest.mark.parametrize("per_cell", [False, True], ids=["global_dt", "per_cell_dt"])
@pytest.mark.parametrize("nd", [2, 3])
@pytest.mark.parametrize("n", [1, 77, 2048 * 256 + 77])
def test_update_dual_bit_for_bit(n, nd, per_cell, alpha, bdf2_g):
    """One row, less than a workgroup, and past the grid cap of 2 048 workgroups of 256 (the grid-stride loop); g = 0 and
    the BDF2 value of a physical step of 8 x the rows' time step."""
    ef.check_update_bit_for_bit(ef.DUAL, n, nd, per_cell, alpha, g=None if bdf2_g else 0.0)


@pytest.mark.parametrize("nd", [2, 3])
def test_update_dual_nan_and_vacuum_rows(nd):
    """The rows of test_update_stage_nan_and_vacuum_rows -- a NaN row, a NaN temperature, p = 0, a NaN residual, rho -> 0 --
    and a NaN in the source: the NaN / Inf pattern of the composition."""
    ef.check_update_special_rows(ef.DUAL, nd)


@pytest.mark.parametrize("per_cell", [False, True], ids=["global_dt", "per_cell_dt"])
@pytest.mark.parametrize("nd", [2, 3])
def test_zero_g_and_zero_source_is_the_stage(nd, per_cell):
    a = ef.rows(ef.DUAL, 20000, nd, per_cell)[1]
    Z = torch.zeros_like(a.R.T).T
    for alpha in (1.0, THIRD):
        got = ibamd.to_host(ibamd.update_euler_dual(a.P0, a.R, Z, a.dt, alpha, 0.0, FLUID))
        ref = ibamd.to_host(ibamd.update_euler_stage(a.P0, a.R, a.dt, alpha, FLUID))
        assert np.isfinite(ref).all() and np.array_equal(got, ref)


@pytest.mark.parametrize("per_cell", [False, True], ids=["global_dt", "per_cell_dt"])
@pytest.mark.parametrize("nd", [2, 3])
def test_update_dual_against_float64(nd, per_cell):
    """Per element against the float64 model on the update's own scale (``euler_dual_model.update_dual_scale``): at most 4 x
    the Float32 numpy model's own deviation (``euler_dual_model.MODEL_DEVIATION_EPS``, measured in
    tests/test_euler_dual_model.py) -- the margin ``update_euler`` and ``update_euler_stage`` are held to."""
    ef.check_update_against_float64(ef.DUAL, nd, per_cell)


# ---------------------------------------------------------------------------------------------------------------------
# stage
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", ["hll", "sensor"])
@pytest.mark.parametrize("mesh,flags", STEP_CASES, ids=[f"{m}-{f}" for m, f in STEP_CASES])
def test_stage_dual_bit_for_bit(meshes, mesh, flags, scheme):
    ef.check_stage_bit_for_bit(ef.DUAL, meshes, mesh, flags, scheme)


def test_rejections(meshes):
    """Each misuse is an error before any launch: ``out`` and ``work`` stay as they were."""
    for mesh in ("adv", "corner"):
        c = meshes[mesh]
        Pd = ibamd.hip(rg.euler_regime(c.part, "rest"))
        P0 = Pd.clone()
        dt = torch.ones(1, dtype=torch.float32, device="cuda")
        out, work, S = (torch.full_like(Pd.T, NAN).T for _ in range(3))
        args = dict(fluid=FLUID, scheme="hll")
        with pytest.raises(ValueError, match="S may not be out"):
            ibamd.stage_euler_dual(c.dpart, Pd, P0, out, dt, 1.0, 1.0, out, work=work, **args)
        with pytest.raises(ValueError, match="S may not be work"):
            ibamd.stage_euler_dual(c.dpart, Pd, P0, work, dt, 1.0, 1.0, out, work=work, **args)
        with pytest.raises(_lib.IbhError, match="work may not alias"):
            ibamd.stage_euler_dual(c.dpart, Pd, P0, S, dt, 1.0, 1.0, out, work=Pd, **args)
        with pytest.raises(_lib.IbhError, match="ibh_stage_euler_dual: IBH_IMAGE_ONLY"):
            ibamd.stage_euler_dual(c.dpart, Pd, P0, S, dt, 1.0, 1.0, out, work=work, flags=B.IBH_IMAGE_ONLY, **args)
        for g in (-1.0, float("inf"), NAN):
            with pytest.raises(ValueError, match="g must be"):
                ibamd.stage_euler_dual(c.dpart, Pd, P0, S, dt, 1.0, g, out, work=work, **args)
            with pytest.raises(ValueError, match="g must be"):
                ibamd.update_euler_dual(P0, work, S, dt, 1.0, g, FLUID, out=out)
        with pytest.raises(ValueError, match="S may not be out"):
            ibamd.update_euler_dual(P0, work, out, dt, 1.0, 1.0, FLUID, out=out)
        with pytest.raises(ValueError, match="out may not be"):
            ibamd.dual_source(Pd, P0, 1.0, -0.5, FLUID, out=P0)
        assert torch.isnan(out).all() and torch.isnan(work).all() and torch.equal(Pd, P0)
        # the library's own checks, past the Python layer: error codes, nothing launched
        f = B._cfluid(FLUID)
        n, nv = Pd.shape
        import ctypes as C
        p = B._ptr
        B._stream()
        for S_, g_, w_, msg in ((out, 1.0, work, "S may not alias P_out"), (work, 1.0, work, "work may not alias"),
                                (S, -1.0, work, "g must be"), (S, float("inf"), work, "g must be")):
            with pytest.raises(_lib.IbhError, match=msg):
                _lib.call("ibh_stage_euler_dual", c.dpart.handle, C.byref(f), 0, p(Pd), n, p(P0), n, p(S_), n, p(out), n, p(dt), 0,
                          C.c_float(1.0), C.c_float(g_), p(w_), n, 0)
        with pytest.raises(_lib.IbhError, match="g must be"):
            _lib.call("ibh_update_euler_dual", C.byref(f), nv - 2, n, p(P0), n, p(work), n, p(S), n, p(dt), 0, C.c_float(1.0),
                      C.c_float(-1.0), p(out), n)
        assert torch.isnan(out).all() and torch.isnan(work).all()


# ---------------------------------------------------------------------------------------------------------------------
# march
# ---------------------------------------------------------------------------------------------------------------------
NPHYS, N_INNER = 3, 4


class Pushes:
    """What a ``TimeAverage`` is handed."""

    def __init__(self):
        self.seen = []

    def push(self, P, dt):
        self.seen.append((P.data_ptr(), dt))


def composed_dual_march(c, P, dt_real, local_dt, nphys=NPHYS, n_inner=N_INNER, stages=rk_stages(3), calls=None):
    """The march written out with the public calls: the source from the two latest states (BDF1 on the first step), then the
    pseudo-steps -- the pseudo-time step from the pseudo-step's input, the stages on that input as base state."""
    n, nv = P.shape
    work = B.colmajor_empty(n, nv)
    prev = None
    for _ in range(nphys):
        cn, cm, g = bdf_coefficients(1 if prev is None else 2, dt_real)
        S = ibamd.dual_source(P, prev, cn, cm, FLUID)
        Pk = P
        for _ in range(n_inner):
            if local_dt:
                dtau = ibamd.timestep_euler(c.dpart, Pk, FLUID, SCALE, out=False, cells=B.colmajor_empty(n))
            else:
                dtau = ibamd.timestep_euler(c.dpart, Pk, FLUID, SCALE)
            base = Pk
            for alpha in stages:
                Pk = ibamd.stage_euler_dual(c.dpart, Pk, base, S, dtau, alpha, g, B.colmajor_empty(n, nv), FLUID, "hll",
                                            work=work)
                if calls is not None:
                    calls.append(Pk.data_ptr())
        prev, P = P, Pk
    return P


@pytest.mark.parametrize("local_dt", [True, False], ids=["local_dt", "global_dt"])
@pytest.mark.parametrize("mesh", ["adv", "corner"])
def test_dual_time_march(meshes, mesh, local_dt):
    c = meshes[mesh]
    P0 = ibamd.hip(rg.euler_regime(c.part, "transonic"))
    start = P0.clone()
    dt_real = 4.0 * float(ibamd.timestep_euler(c.dpart, P0, FLUID, SCALE).item())
    ref = composed_dual_march(c, P0, dt_real, local_dt)
    assert np.isfinite(ibamd.to_host(ref)).all() and not torch.equal(ref, P0)

    seen, avg = [], Pushes()
    m = DualTimeMarch(c.dpart, dt_real, N_INNER, fluid=FLUID, scale=SCALE, local_dt=local_dt, stages=3, average=avg,
                      bcs=lambda P: seen.append(P.data_ptr()))
    P, returned = P0, []
    for _ in range(NPHYS):
        P = m.step(P)
        assert P.data_ptr() not in [r.data_ptr() for r in returned[-1:]] + [P0.data_ptr()]
        returned.append(P)
    same_bits(P, ref, f"dual march {mesh}")
    same_bits(P0, start, "the caller's array is left alone")
    assert len(seen) == NPHYS * N_INNER * 3                                     # bcs after every stage
    assert [dt for _, dt in avg.seen] == [dt_real] * NPHYS and [p for p, _ in avg.seen] == [r.data_ptr() for r in returned]
    assert m.nsteps == NPHYS

    # a returned array stays valid during the next step: the second step's result, read after the third step
    m2 = DualTimeMarch(c.dpart, dt_real, N_INNER, fluid=FLUID, scale=SCALE, local_dt=local_dt, stages=3)
    P2 = m2.step(m2.step(P0))
    snap = P2.clone()
    P3 = m2.step(P2)
    same_bits(P2, snap, "the array returned by step 2 after step 3")
    same_bits(P3, ref, "a second march")

    # residual=: the callable into work, then update_euler_dual -- the same sweep, the same bits
    other = DualTimeMarch(c.dpart, dt_real, N_INNER, fluid=FLUID, scale=SCALE, local_dt=local_dt, stages=3,
                          residual=lambda p, Pin, o: ibamd.residual_euler_hll(p, Pin, out=o, fluid=FLUID))
    Po = P0
    for _ in range(NPHYS):
        Po = other.step(Po)
    same_bits(Po, ref, f"dual march {mesh}, residual=")

    # the same three steps captured after one warm-up step and replayed: steps 2 .. 4 of an eager march
    ref4 = m.step(P)
    Pg = ef.replayed_march(lambda: DualTimeMarch(c.dpart, dt_real, N_INNER, fluid=FLUID, scale=SCALE, local_dt=local_dt, stages=3),
                           P0, NPHYS, warmup=1, onward=True)
    same_bits(Pg, ref4, f"dual march {mesh}, graph replay")
    same_bits(P0, start, "the caller's array is left alone by the replay")


@pytest.mark.parametrize("mesh", ["adv", "corner"])
def test_uniform_state_is_kept(meshes, mesh):
    """A uniform stream at rest is a solution of every backward-difference equation (R = 0, S = g Q): after two physical
    steps -- 8 pseudo-steps of 3 stages -- every element is within the float64-model bound of it, on the update's scale.
    The velocities' scale: ``update_dual_scale`` takes the residual as given, and the momentum residual of this state is a
    sum of 2 nd face terms p / dx that cancel to zero; what enters u before that cancellation is h (2 nd p / dx) / rho with
    h <= scale dx / (2 a), i.e. scale nd p / (rho a) = scale nd a / gamma (a: the speed of sound) -- the rounding of a
    pressure that differs between neighbours in its last bit reaches the velocity on that scale."""
    c = meshes[mesh]
    n, nv = c.part.spacing.shape[0], c.nd + 2
    P = np.zeros((n, nv), f32)
    P[:, 0], P[:, 1] = 1e5, 288.15
    Pd = ibamd.hip(P)
    dt_real = 4.0 * float(ibamd.timestep_euler(c.dpart, Pd, FLUID, SCALE).item())
    m = DualTimeMarch(c.dpart, dt_real, N_INNER, fluid=FLUID, scale=SCALE, stages=3)
    got = ibamd.to_host(m.step(m.step(Pd)))
    cn, cm, g = bdf_coefficients(2, dt_real)
    S = dm.dual_source(P, P, cn, cm, f64)
    dtau = ibamd.to_host(m.dt)
    scale = dm.update_dual_scale(P, np.zeros_like(P), S, dtau, 1.0, g)
    a = np.sqrt(f64(FLUID.gamma) * f64(FLUID.R) * 288.15)
    scale[:, 2:] = SCALE * c.nd * a / f64(FLUID.gamma)
    err = np.abs(got.astype(f64) - P.astype(f64)) / scale / em.EPS32
    print(f"{mesh}: a uniform state after two physical steps: p {err[:, 0].max():.3f}, T {err[:, 1].max():.3f}, velocities "
          f"{err[:, 2:].max():.3f} eps (max |u| {np.abs(got[:, 2:]).max():.3e}), bound {4 * dm.MODEL_DEVIATION_EPS[c.nd]:.1f} eps")
    assert np.isfinite(got).all()
    assert err.max() <= 4 * dm.MODEL_DEVIATION_EPS[c.nd]


# ---------------------------------------------------------------------------------------------------------------------
# the inner iteration
# ---------------------------------------------------------------------------------------------------------------------
def bdf_residual_norm(c, Pd, S, g):
    """|| R(P) + S - g primitive2state(P) ||_2 over all cells and variables, from the sweep and primitive2state, in float64."""
    R = ibamd.to_host(ibamd.residual_euler_hll(c.dpart, Pd, fluid=FLUID)).astype(f64)
    Q = ibamd.to_host(cfd.primitive2state(FLUID, Pd)).astype(f64)
    return float(np.sqrt(((R + ibamd.to_host(S).astype(f64) - g * Q) ** 2).sum()))


def test_inner_iterations_contract(meshes):
    """``adv`` without boundary conditions (the mirror faces close the box), "transonic", one stage, a global pseudo-time step,
    dt_real = 2 x the explicit step at scale 0.75: the residual of the BDF2 equation after 20 pseudo-steps is below 1/10 of
    its value before the first.  A pseudo-step multiplies every linear mode by at most 1 / (1 + h g) = 1 / 1.75 once the
    explicit part is within its CFL limit: 20 steps give 1.4e-5, 1/10 leaves four decades.  A wrong sign of g or S grows."""
    c = meshes["adv"]
    n, nv = c.part.spacing.shape[0], c.nd + 2
    Pm = ibamd.hip(rg.euler_regime(c.part, "transonic"))
    dt = ibamd.timestep_euler(c.dpart, Pm, FLUID, SCALE)
    Pn = ibamd.step_euler(c.dpart, Pm, dt, B.colmajor_empty(n, nv), FLUID, "hll")       # the history: one explicit step
    dt_real = 2.0 * float(dt.item())
    cn, cm, g = bdf_coefficients(2, dt_real)
    S = ibamd.dual_source(Pn, Pm, cn, cm, FLUID)
    before = bdf_residual_norm(c, Pn, S, g)
    P = Pn
    for _ in range(20):
        dtau = ibamd.timestep_euler(c.dpart, P, FLUID, SCALE)
        P = ibamd.stage_euler_dual(c.dpart, P, P, S, dtau, 1.0, g, B.colmajor_empty(n, nv), FLUID, "hll")
    after = bdf_residual_norm(c, P, S, g)
    print(f"BDF2 residual norm {before:.4e} -> {after:.4e} after 20 pseudo-steps: a factor {after / before:.3e}")
    assert np.isfinite(after) and after < 0.1 * before

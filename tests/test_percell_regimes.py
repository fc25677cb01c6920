"""The per-cell checker across flow regimes, on the CPU: calibration, the scales' reach, sensitivity.

tests/regimes.py holds the fields; ``percell.euler_scale_waves`` / ``percell.scalar_scale_c`` the scales under which correct
Float32 arithmetic passes in every regime, ``percell.BOUND_EULER_REGIMES`` / ``percell.BOUND_SCALAR_REGIMES`` the bounds the
GPU tests use with them (tests/test_gpu_percell_regimes.py).

- Calibration: the Float32 numpy oracle and the C restatement against float64, every regime on the RAE2822 and advection
  partitions and the golden octree: at most half of the regime bounds.
- Scales: under the present ``euler_scale`` the Float32 oracle itself exceeds ``BOUND_EULER`` at rest and near stagnation,
  under ``stencil_scale`` it exceeds ``BOUND`` for |C| ~ 50 -- the present scales hold only for |C| ~ 1 and a Mach number
  away from 0.
- Sensitivity: a planted error in a copy of the oracle's arithmetic fails the regime check on the regime that reaches it.
"""
import os

import numpy as np
import pytest

import ibamd
import percell as pc
import regimes as rg
from conftest import ADV_FAMILIES, GOLDEN, RAE_FAMILIES, advection_mesh, oracle_view, rae_mesh
from oracle import cfd as ocfd
from oracle import domain as od
from oracle import residual_c as rc

f32, f64 = np.float32, np.float64


@pytest.fixture(scope="module")
def cases():
    """(name, product partition, oracle view, C part) of the cases of tests/test_percell.py::test_calibration."""
    from test_golden import _partition
    out = []
    for name, msh, fam, mps in (("rae", rae_mesh(), RAE_FAMILIES, 16384), ("adv", advection_mesh(), ADV_FAMILIES, 4096)):
        dom = ibamd.Domain(msh, hypercube_families=fam, max_partition_size=mps)
        out += [(f"{name}{k}", p) for k, p in dom.partitions.items()]
    out.append(("octree", _partition(dict(np.load(os.path.join(GOLDEN, "octree_partition.npz"))))))
    return [(name, p, oracle_view(p), rc.CPart(p)) for name, p in out]


@pytest.fixture(scope="module")
def euler_refs(cases):
    """{(case, regime): (P, float64 reference, Float32 oracle)}, computed once."""
    out = {}
    fluid = ocfd.Fluid()
    for name, part, op, cp in cases:
        for reg in rg.EULER_REGIMES:
            P = rg.euler_regime(part, reg)
            out[name, reg] = (P, pc.ref64_euler(op, P), pc.oracle_euler_residual(op, P, fluid))
    return out


def _max(err):
    assert np.isfinite(err).all()
    return float(err.max())


def test_regimes_reach_their_branches(cases):
    """The fields, not the kernels, guarantee the coverage: each Euler regime reaches its branch on every case, no face
    is near SL = SR = 0, and the crossing C changes sign inside blocks."""
    for name, part, op, cp in cases:
        for reg in rg.EULER_REGIMES:
            rg.assert_euler_coverage(op, rg.euler_regime(part, reg), reg, what=name)
        both, _ = rg.cf_signs_in_blocks(op, rg.c_regime(part, "crossing"))
        assert both >= 1, name


def test_calibration(cases, euler_refs):
    """Float32 oracle and C restatement against float64 under the regime scales: at most half the regime bounds."""
    eu, sc = {}, {}
    for name, part, op, cp in cases:
        for reg in rg.EULER_REGIMES:
            P, r64, r32 = euler_refs[name, reg]
            s = pc.euler_scale_waves(part, P, r64)
            e = max(_max(pc.percell_error(r32, r64, s)), _max(pc.percell_error(cp.residual_euler(P), r64, s)))
            eu[reg] = max(eu.get(reg, 0.0), e)
        for creg in rg.C_REGIMES:
            C = rg.c_regime(part, creg)
            for kind in rg.U_KINDS:
                u = rg.u_kind(part, kind)
                r64 = pc.ref64_advection(op, u, C)
                r32, rcc = pc.oracle_advection_residual(op, u, C), cp.residual_advection(u, C)
                if creg == "zero":
                    assert not r64.any() and not r32.any() and not rcc.any(), (name, kind)
                    continue
                s = pc.scalar_scale_c(part, u, C, r64)
                e = max(_max(pc.percell_error(r32, r64, s)), _max(pc.percell_error(rcc, r64, s)))
                sc[creg, kind] = max(sc.get((creg, kind), 0.0), e)
    print("\nregime calibration, Float32 oracle / C restatement against float64 (max over the cases):")
    for k, v in eu.items():
        print(f"  euler {k}: {v:.2e}")
    for k, v in sc.items():
        print(f"  scalar C {k[0]}, u {k[1]}: {v:.2e}")
    print(f"  worst: euler {max(eu.values()):.2e}, scalar {max(sc.values()):.2e}")
    assert max(eu.values()) <= pc.BOUND_EULER_REGIMES / 2, eu
    assert max(sc.values()) <= pc.BOUND_SCALAR_REGIMES / 2, sc
    assert pc.BOUND_EULER_REGIMES <= pc.BOUND_EULER and pc.BOUND_SCALAR_REGIMES <= pc.BOUND


def test_present_scales_hold_for_the_present_states_only(cases, euler_refs):
    """Why the regimes need scales of their own: correct Float32 arithmetic fails the present bounds under the present
    scales at rest and near stagnation (``euler_scale`` vanishes with the velocity, the HLL dissipation a dQ does not)
    and for |C| ~ 50 (``stencil_scale`` carries no |C|), and for |C| ~ 1e-3 the present scalar scale lets through an
    error a thousand times rounding."""
    name, part, op, cp = next(c for c in cases if c[0] == "adv1")
    seen = {}
    for reg in rg.EULER_REGIMES:
        P, r64, r32 = euler_refs[name, reg]
        seen[reg] = (_max(pc.percell_error(r32, r64, pc.euler_scale(part, P, r64))),
                     _max(pc.percell_error(r32, r64, pc.euler_scale_waves(part, P, r64))))
    print("\nFloat32 oracle on partition 1 of the advection domain, euler_scale / euler_scale_waves:")
    for k, (a, b) in seen.items():
        print(f"  {k}: {a:.2e} / {b:.2e}")
    assert seen["rest"][0] > pc.BOUND_EULER and seen["stagnation"][0] > pc.BOUND_EULER, seen
    assert all(b <= pc.BOUND_EULER_REGIMES / 2 for a, b in seen.values()), seen
    u = rg.u_kind(part, "noisy")
    sc = {}
    for creg in ("big", "tiny", "crossing"):
        C = rg.c_regime(part, creg)
        r64 = pc.ref64_advection(op, u, C)
        r32 = pc.oracle_advection_residual(op, u, C)
        sc[creg] = (_max(pc.percell_error(r32, r64, pc.scalar_scale(part, u, r64))),
                    _max(pc.percell_error(r32, r64, pc.scalar_scale_c(part, u, C, r64))))
    print("Float32 oracle, stencil_scale / scalar_scale_c:", {k: (f"{a:.1e}", f"{b:.1e}") for k, (a, b) in sc.items()})
    assert sc["big"][0] > pc.BOUND, sc
    assert sc["tiny"][0] < 1e-3 * pc.BOUND * 5, sc           # ~ |C| times rounding: no check at all
    assert all(b <= pc.BOUND_SCALAR_REGIMES / 2 for a, b in sc.values()), sc


# ---------------------------------------------------------------------------------------------------------------------
# sensitivity: a copy of the oracle's arithmetic with one error planted
# ---------------------------------------------------------------------------------------------------------------------
def _hll(fluid, PL, PR, dim, clamp_SR=True, clamp_SL=True, clamp_a=True):
    """oracle.cfd.inviscid_fluxes, with switches for the planted errors."""
    def sound(T):
        return ocfd.speed_of_sound(fluid, T) if clamp_a else np.sqrt(fluid.gamma * fluid.R * T)
    QL, FL, uL, _ = ocfd._side_flux(fluid, PL, dim)
    QR, FR, uR, _ = ocfd._side_flux(fluid, PR, dim)
    aL, aR = sound(PL[:, 1]), sound(PR[:, 1])
    SR = (uR - aR).astype(f64)
    SL = (uL + aL).astype(f64)
    if clamp_SR:
        SR = np.minimum(SR, 0.0)
    if clamp_SL:
        SL = np.maximum(SL, 0.0)
    SR, SL = SR[:, None], SL[:, None]
    return (SL * FL - SR * FR + SR * SL * (QR - QL)) / (SL - SR)


def _sensor(part, p, floor):
    nu = np.full_like(p, floor)
    for d in range(1, part.ndims + 1):
        nu = np.maximum(nu, od.JST_sensor(part, p, d))
    return nu


def _euler(part, P, floor=f32(1e-7), **kw):
    """percell.oracle_euler_residual, with the planted errors of ``_hll`` and the sensor's floor."""
    fluid = ocfd.Fluid()
    R = np.zeros_like(P)
    D = _sensor(part, np.ascontiguousarray(P[:, 0]), floor)
    for dim in range(1, part.ndims + 1):
        PL, PR = od.MUSCL(part, P, od.cell_gradient(part, P, dim), dim, D=D, high_order=True)
        R -= od.green_gauss(part, _hll(fluid, PL, PR, dim, **kw), dim)
    return R


def _advection(part, u, C, abs_cf=True):
    ud = np.zeros_like(u)
    D = od.JST_sensor(part, u)
    for dim in range(1, part.ndims + 1):
        Cf = od.at_faces(part, np.ascontiguousarray(C[:, dim - 1]), dim)
        uL, uR = od.MUSCL(part, u, od.cell_gradient(part, u, dim), dim, D=D, high_order=True)
        ud -= od.green_gauss(part, (uL + uR) * Cf / f32(2) + (np.abs(Cf) if abs_cf else Cf) * (uL - uR) / f32(2), dim)
    return ud


PLANTED = [("supersonic+", dict(clamp_SR=False)), ("supersonic-", dict(clamp_SL=False)), ("cold", dict(clamp_a=False))]


@pytest.mark.parametrize("regime,planted", PLANTED, ids=[p[0] for p in PLANTED])
def test_sensitivity_euler(cases, euler_refs, regime, planted):
    """A clamp left out of the copy fails the regime check on every case; the unbroken copy is the oracle bit for bit."""
    for name, part, op, cp in cases:
        P, r64, r32 = euler_refs[name, regime]
        s = pc.euler_scale_waves(part, P, r64)
        assert np.array_equal(_euler(op, P), r32), name
        assert pc.check(r32, r64, s, pc.BOUND_EULER_REGIMES, part, what=name) <= pc.BOUND_EULER_REGIMES
        with np.errstate(all="ignore"):
            bad = _euler(op, P, **planted)
        with pytest.raises(AssertionError, match="per-cell error|NaN pattern"):
            pc.check(bad, r64, s, pc.BOUND_EULER_REGIMES, part, what=f"{name} {regime}")


def test_sensor_floor_is_below_the_bound(cases, euler_refs):
    """The sensor's floor 1e-7 replaced by 0 (in ``JST_sensor``; MUSCL's own max(D, 1e-7) stays) is NOT a probe: on the
    floor regime it moves the blend weight from 1e-7 to ~1e-10 of the difference between the limited and the central
    face value, below rounding.  Asserted, so that the missing probe is a measured statement."""
    worst = 0.0
    for name, part, op, cp in cases:
        P, r64, r32 = euler_refs[name, "floor"]
        s = pc.euler_scale_waves(part, P, r64)
        worst = max(worst, _max(pc.percell_error(_euler(op, P, floor=f32(0.0)), r32, s)))
    print(f"\nsensor floor 0 against 1e-7 on the floor regime, Float32 oracle copies: {worst:.2e}")
    assert worst < pc.BOUND_EULER_REGIMES / 10


def test_sensitivity_scalar(cases):
    """|Cf| replaced by Cf fails on the crossing C; a 1e-4 relative error on all cells of the tiny-C case fails under
    ``scalar_scale_c`` and passes under ``stencil_scale`` (which reads it as 1e-7)."""
    for name, part, op, cp in cases:
        u = rg.u_kind(part, "noisy")
        C = rg.c_regime(part, "crossing")
        r64 = pc.ref64_advection(op, u, C)
        s = pc.scalar_scale_c(part, u, C, r64)
        assert np.array_equal(_advection(op, u, C), pc.oracle_advection_residual(op, u, C)), name
        assert pc.check(_advection(op, u, C), r64, s, pc.BOUND_SCALAR_REGIMES, part, what=name) <= pc.BOUND_SCALAR_REGIMES
        with pytest.raises(AssertionError, match="per-cell error"):
            pc.check(_advection(op, u, C, abs_cf=False), r64, s, pc.BOUND_SCALAR_REGIMES, part, what=f"{name} crossing")
        C = rg.c_regime(part, "tiny")
        r64 = pc.ref64_advection(op, u, C)
        bad = pc.oracle_advection_residual(op, u, C) * f32(1 + 1e-4)
        with pytest.raises(AssertionError, match="per-cell error"):
            pc.check(bad, r64, pc.scalar_scale_c(part, u, C, r64), pc.BOUND_SCALAR_REGIMES, part, what=f"{name} tiny")
        assert pc.check(bad, r64, pc.scalar_scale(part, u, r64), pc.BOUND, part, what=name) <= pc.BOUND

"""The per-cell checker of the operators, the viscous sum and the turbulence closure (tests/percell.py), on the CPU.

Calibration: the Float32 oracle stays at or below half of each family's bound against the float64 evaluation.
Sensitivity: a 1e-4 relative error on the coarsest level, and one FINE side with the wrong neighbour, fail the per-cell
check of the viscous sum and of the transport residual; on the ten-level RAE2822 partitions the first passes the
norm-wise check.  NaN rule: a NaN where the reference has none (or none where it has one) fails before any bound.
"""
import numpy as np
import pytest

import percell as pc
from conftest import oracle_view, rel_inf
from oracle import cfd as ocfd
from oracle import domain as od
from oracle import turbulence as ot
from test_percell import cases  # noqa: F401  (module fixture: RAE2822 / advection partitions, 3-D octree)

f32, f64 = np.float32, np.float64
NU = f32(1.5e-5)


def _inputs(part):
    Q = pc.closure_field(part.centers)
    nvp = part.ndims + 2
    P = np.ascontiguousarray(Q[:, :nvp])
    R = np.ascontiguousarray(Q[:, nvp])
    mut = (Q[:, 0] / (ocfd.Fluid().R * Q[:, 1])) * R
    R0 = (np.random.default_rng(1).uniform(-1, 1, P.shape) * 1e-3).astype(f32)
    return Q, P, R, mut, R0


def test_the_closure_oracle_is_dtype_generic(cases):  # noqa: F811
    name, part = cases[0]
    op = oracle_view(part)
    Q, P, R, mut, R0 = _inputs(part)
    vel = Q[:, 2:part.ndims + 2]
    S = ot.shear_rate(pc.oracle_velocity_gradients(op, vel))
    for dt, args in ((f32, (Q, P, R, mut, R0, vel, S)), (f64, pc.to64(Q, P, R, mut, R0, vel, S))):
        q, p, r, m, r0, v, s = args
        assert pc.oracle_viscous_sum(op, p, m, r0).dtype == dt
        assert pc.oracle_transport(op, r, r * f32(0.72), v, NU, s).dtype == dt
        assert ot.shear_rate(pc.oracle_velocity_gradients(op, v)).dtype == dt
        assert all(a.dtype == dt for a in pc.oracle_wray_agarwal_of(op, r, s).values())
        for visc in (True, False):
            assert pc.oracle_wa_residual(op, q, NU, viscous=visc).dtype == dt


def _families(part):
    """{family: (float32 oracle, float64 reference, scale, bound)} on the closure field."""
    op = oracle_view(part)
    Q, P, R, mut, R0 = _inputs(part)
    vel = Q[:, 2:part.ndims + 2]
    out = {}
    r64 = pc.oracle_viscous_sum(op, *pc.to64(P, mut, R0))
    out["viscous"] = (pc.oracle_viscous_sum(op, P, mut, R0), r64, pc.viscous_scale(part, P, mut, r64, R0), pc.BOUND_VISCOUS)
    S32 = ot.shear_rate(pc.oracle_velocity_gradients(op, vel))
    S64 = ot.shear_rate(pc.oracle_velocity_gradients(op, vel.astype(f64)))
    out["shear"] = (S32, S64, pc.shear_scale(part, vel, S64), pc.BOUND_TURB)
    wa32 = pc.oracle_wray_agarwal_of(op, R, S32)
    wa64 = pc.oracle_wray_agarwal_of(op, *pc.to64(R, S32))
    was = pc.wray_agarwal_scale(part, R, S32)
    for k in ("nut", "nuR", "S"):
        out["wray_agarwal_" + k] = (wa32[k], wa64[k], was[k], pc.BOUND_TURB)
    nuR, Sw = wa32["nuR"], wa32["S"]
    t64 = pc.oracle_transport(op, *pc.to64(R, nuR, vel), NU, Sw.astype(f64))
    out["transport"] = (pc.oracle_transport(op, R, nuR, vel, NU, Sw), t64,
                        pc.transport_scale(part, R, nuR, vel, NU, Sw, t64), pc.BOUND_TRANSPORT)
    # operators (BOUND_OPS), on the primitive state: cell_gradient, at_faces, face_gradient, green_gauss, JST_sensor, MUSCL
    P64 = P.astype(f64)
    p0 = np.ascontiguousarray(P[:, 0])
    for d in range(1, part.ndims + 1):
        r = od.cell_gradient(op, P64, d)
        out[f"cell_gradient {d}"] = (od.cell_gradient(op, P, d), r, pc.abs_cell_gradient(op, P64, d) + np.abs(r), pc.BOUND_OPS)
        fo = {}
        r = od.at_faces(op, P64, d)
        fo["at_faces"] = (od.at_faces(op, P, d), r, pc.abs_at_faces(op, P64, d) + np.abs(r))
        r = od.face_gradient(op, P64, d)
        fo["face_gradient"] = (od.face_gradient(op, P, d), r, pc.abs_face_gradient(op, P64, d) + np.abs(r))
        uf = od.at_faces(op, P, d)
        r = od.green_gauss(op, uf.astype(f64), d)
        out[f"green_gauss {d}"] = (od.green_gauss(op, uf, d), r, pc.abs_green_gauss(op, uf.astype(f64), d) + np.abs(r),
                                   pc.BOUND_OPS)
        r = od.JST_sensor(op, p0.astype(f64), d)
        out[f"JST_sensor {d}"] = (od.JST_sensor(op, p0, d), r, 1 + np.abs(r), pc.BOUND_OPS)
        g32 = od.cell_gradient(op, P, d)
        D = od.JST_sensor(op, p0)
        rL, _ = od.MUSCL(op, P64, g32.astype(f64), d, D=D.astype(f64), high_order=True)
        gL, _ = od.MUSCL(op, P, g32, d, D=D, high_order=True)
        fo["MUSCL"] = (gL, rL, pc.muscl_scale(op, P, g32, d, D=D, high_order=True) + np.abs(rL))
        for k, (g, r, sc) in fo.items():   # face arrays: per face, folded onto the cells
            out[f"{k} {d}"] = (pc.faces_to_cells(part, d, pc.percell_error(g, r, sc)), None, None, pc.BOUND_OPS)
    for visc in (True, False):
        c64 = pc.oracle_wa_residual(op, Q.astype(f64), NU, viscous=visc)
        out[f"closure viscous={visc}"] = (pc.oracle_wa_residual(op, Q, NU, viscous=visc), c64,
                                          pc.closure_scale(part, Q, c64, NU, viscous=visc), pc.BOUND_CLOSURE)
    return out


def test_calibration(cases):  # noqa: F811
    """The Float32 oracle against float64: at most half of each family's bound, on every case."""
    worst = {}
    for name, part in cases:
        fam = _families(part)
        nvp = part.ndims + 2
        Q = pc.closure_field(part.centers)
        wa = fam["wray_agarwal_S"][1]
        assert (wa == 10 * Q[:, nvp].astype(f64)).sum() > 0 and (wa < 10 * Q[:, nvp].astype(f64)).sum() > 0, name
        assert (fam["shear"][1] == 0).any() and (Q[:, nvp] == 0).any() and (Q[:, 1] < 10).any(), name
        for k, (g, r, s, b) in fam.items():
            if r is None:      # face operators: g holds the per-cell maxima of the per-face error already
                e = float(g.max())
                assert e <= b / 2, (name, k, e)
            else:
                e = pc.check(g, r, s, b / 2, part, classes={}, what=f"{name} {k}")
            k = k.rstrip(" 123")
            worst[k] = max(worst.get(k, 0.0), e)
    print("\ncalibration (per-cell error of the Float32 oracle against float64):",
          {k: f"{v:.2e}" for k, v in worst.items()})


def _fine_side_views(part, x, k=8):
    """Oracle views of ``part`` in which one face on a FINE side (a coarse owner, a finer neighbour) names the wrong
    neighbour: the finer cell of the next face of the same owner along the same dimension."""
    sp = np.asarray(part.spacing)
    for d in range(1, part.ndims + 1):
        o, nb = part.face_owners_neighbors[d]
        fine = np.nonzero((sp[nb, d - 1] < sp[o, d - 1]) & (o != nb))[0]
        for f in fine[:k]:   # (k None: all of them)
            g = [j for j in fine if o[j] == o[f] and nb[j] != nb[f]]
            if not g:
                continue
            view = oracle_view(part)
            fon = dict(view.face_owners_neighbors)
            nb2 = nb.copy()
            nb2[f] = nb[g[0]]
            fon[d] = (o, nb2)
            view.face_owners_neighbors = fon
            yield view


@pytest.mark.parametrize("which", ["viscous", "transport"])
def test_sensitivity(cases, which):  # noqa: F811
    gap = fine_gap = 0
    for name, part in cases:
        Q, P, R, mut, R0 = _inputs(part)
        vel = Q[:, 2:part.ndims + 2]
        op = oracle_view(part)
        if which == "viscous":
            res = lambda view: pc.oracle_viscous_sum(view, P, mut, R0)  # noqa: E731
            r64 = pc.oracle_viscous_sum(op, *pc.to64(P, mut, R0))
            s = pc.viscous_scale(part, P, mut, r64, R0)
            bound = pc.BOUND_VISCOUS
            r0 = R0
        else:
            wa = pc.oracle_wray_agarwal_of(op, R, ot.shear_rate(pc.oracle_velocity_gradients(op, vel)))
            res = lambda view: pc.oracle_transport(view, R, wa["nuR"], vel, NU, wa["S"])  # noqa: E731
            r64 = pc.oracle_transport(op, *pc.to64(R, wa["nuR"], vel), NU, wa["S"].astype(f64))
            s = pc.transport_scale(part, R, wa["nuR"], vel, NU, wa["S"], r64)
            bound = pc.BOUND_TRANSPORT
            r0 = wa["S"]
        r32 = res(op)
        assert pc.check(r32, r64, s, bound, part, what=name) <= bound
        lev = pc.levels(part)
        # (1) a 1e-4 relative error on the coarsest level alone (of the operator sum, not of the R0 / S it starts from)
        bad = r32 + (r32 - r0) * f32(1e-4) * (lev == lev.max()).reshape((-1,) + (1,) * (r32.ndim - 1))
        with pytest.raises(AssertionError, match="per-cell error"):
            pc.check(bad, r64, s, bound, part, what=name)
        if lev.max() >= 2:
            assert rel_inf(bad, r64) <= 1e-5, name
            gap += 1
        # (2) one FINE side with the wrong neighbour
        # (the least conspicuous norm-wise of all FINE-side faces whose wrong id the per-cell check sees at all)
        seen = [b for b in (res(v) for v in _fine_side_views(part, P, k=None)) if pc.percell_error(b, r64, s).max() > bound]
        if seen:
            bad = min(seen, key=lambda b: rel_inf(b, r64))
            with pytest.raises(AssertionError, match="per-cell error"):
                pc.check(bad, r64, s, bound, part, what=name)
            if lev.max() >= 2 and which == "viscous":   # (the transport's R is noisy on every level: there the least
                assert rel_inf(bad, r64) <= 1e-5, (name, rel_inf(bad, r64))   # visible wrong id reads 6.7e-5 norm-wise)
                fine_gap += 1
    assert gap >= 3 and (fine_gap >= 2 or which != "viscous")   # (two of the three RAE2822 partitions have a FINE side a wrong id shows on)


def test_nan_pattern_rule(cases):  # noqa: F811
    """A NaN the reference does not have -- or a finite value where it has NaN -- fails before any bound; NaN where the
    reference has NaN, and equal infinities, are exact."""
    name, part = cases[0]
    fam = _families(part)
    g, r, s, b = fam["viscous"]
    r = r.copy()
    r[5, 1] = np.nan
    r[7, 2] = np.inf
    got = g.copy()
    with pytest.raises(AssertionError, match="NaN pattern"):
        pc.check(got, r, s, b, part, what="finite where the reference is NaN")
    got[5, 1] = np.nan
    got[7, 2] = np.inf
    assert pc.check(got, r, s, b, part, what="same pattern") <= b
    got[9, 3] = np.nan
    with pytest.raises(AssertionError, match="NaN pattern"):
        pc.check(got, r, s, b, part, what="an extra NaN")
    got[9, 3] = g[9, 3]
    got[7, 2] = -np.inf
    with pytest.raises(AssertionError, match="per-cell error"):
        pc.check(got, r, s, b, part, what="opposite infinity")
    # a NaN outside the checked cells is not looked at (image-only sweeps leave the skirt untouched)
    got[7, 2] = np.inf
    got[11, 0] = np.nan
    cells = np.setdiff1d(np.arange(got.shape[0]), [11])
    assert pc.check(got, r, s, b, part, cells=cells, what="outside") <= b

"""The right-hand sides of the standard k-epsilon model as the numpy oracle composes them, their closed-form answers on
linear velocity fields, and the fields of the device checks.

Test infrastructure shared by tests/test_kepsilon_model.py (CPU) and tests/test_gpu_k_epsilon.py (GPU).

``oracle_rhs`` is the composition of the reference's docstring (turbulence.jl:150-194) from the oracle's grid operators on
``oracle_view(part)`` and ``oracle.turbulence`` -- nothing of libibhip is involved --, dtype-generic: Float32 inputs give the
Float32 oracle, Float64 inputs (the same Float32 values, widened) the reference every per-cell check is made against.

Closed forms: with ``u = A x``, constant ``k0`` and ``eps0``, every gradient of ``k`` and ``eps`` vanishes and
``div(u k0) = k0 tr(A)``, so on the cells of ``les_model.interior``

    rk   = nut S^2 - eps0 - k0 tr(A)
    reps = C1 nut S^2 eps0 / k0 - C2 eps0^2 / k0 - eps0 tr(A),      nut = Cmu k0^2 / eps0,  S = les_model.answers(A)["S"].

``bounds`` measures the Float32 oracle composition's own deviation from these answers per output over the three fields of
``les_model.FIELDS`` and the selected cells of a mesh; the device is held to 4 x it (``les_model.bounds``'s rule: Float32
operator rounding is the yardstick, x 4 allows for the device's different but legal operation order inside the block
kernel's gradients).
"""
import numpy as np

import les_model as lm
from oracle import domain as od
from oracle import turbulence as ot

f32, f64 = np.float32, np.float64
NU = f32(1.5e-5)
PARAMS = dict(Cmu=f32(0.09), sk=f32(1.0), se=f32(1.3), C1=f32(1.44), C2=f32(1.92))
K0, EPS0 = f32(1.3), f32(2.7)
OUTPUTS = ("rk", "reps", "nut", "S")
WAVY_OUTPUTS = ("rk", "reps", "nut")


# ---------------------------------------------------------------------------------------------------------------------
# fields: all positive, k in [0.5, 2], eps in [1, 4], smooth plus 5 % seeded noise
# ---------------------------------------------------------------------------------------------------------------------
def wavy_velocity(part, seed=21):
    """A velocity field with every gradient component alive, plus noise (``closure_cases.Case.wavy``)."""
    X, nd = part.centers, part.ndims
    rng = np.random.default_rng(seed)
    v = np.stack([np.sin(2 * X[:, (i + 1) % nd]) * np.cos(X[:, i]) + 0.3 * X[:, i] for i in range(nd)], axis=1)
    return (v + 0.05 * rng.standard_normal((X.shape[0], nd))).astype(f32)


def k_eps_fields(part, seed=3):
    """(k, eps): smooth in [0.6, 1.9] / [1.2, 3.8] times (1 + 5 % uniform noise), clipped to [0.5, 2] / [1, 4]."""
    X, nd = np.asarray(part.centers).astype(f64), part.ndims
    rng = np.random.default_rng(seed)
    n = X.shape[0]
    sk = 1.25 + 0.65 * np.sin(1.3 * X[:, 0] + 0.4) * np.cos(0.9 * X[:, nd - 1])
    se = 2.5 + 1.3 * np.cos(1.1 * X[:, 1 % nd] - 0.3) * np.sin(0.7 * X[:, 0] + 1.0)
    k = np.clip(sk * (1 + 0.05 * rng.uniform(-1, 1, n)), 0.5, 2.0).astype(f32)
    eps = np.clip(se * (1 + 0.05 * rng.uniform(-1, 1, n)), 1.0, 4.0).astype(f32)
    return k, eps


# ---------------------------------------------------------------------------------------------------------------------
# the oracle composition
# ---------------------------------------------------------------------------------------------------------------------
def transport(op, R, nuR, vel, nu, S):
    """S + sum_d green_gauss(at_faces(nu + nuR, d) .* face_gradient(R, d) .- at_faces(vel_d .* R, d), d), and the per-cell
    scale of its rounding: |S| + sum_d unsigned_green_gauss(|the face flux|, d)."""
    out, scale = S, np.abs(S)
    for d in range(1, op.ndims + 1):
        flux = od.at_faces(op, nu + nuR, d) * od.face_gradient(op, R, d) - od.at_faces(op, vel[:, d - 1] * R, d)
        out = out + od.green_gauss(op, flux, d)
        scale = scale + od.unsigned_green_gauss(op, np.abs(flux), d)
    return out, scale


def oracle_rhs(op, vel, k, eps, nu=NU, dtype=f32):
    """{rk, reps, nut, S} of the composition in ``dtype``, and {rk, reps}: the per-cell scales of the two sums."""
    vel, k, eps = (np.ascontiguousarray(np.asarray(a).astype(dtype)) for a in (vel, k, eps))
    nu = dtype(nu)
    g = [list(od.cell_gradient(op, np.ascontiguousarray(vel[:, i]))) for i in range(op.ndims)]
    S = ot.shear_rate(g)
    ke = ot.standard_k_epsilon(k, eps, S, **PARAMS)
    rk, sk = transport(op, k, ke["nuk"], vel, nu, ke["Sk"])
    reps, se = transport(op, eps, ke["nueps"], vel, nu, ke["Seps"])
    out = dict(rk=rk, reps=reps, nut=ke["nut"], S=S)
    for key, v in out.items():
        assert v.dtype == dtype, (key, v.dtype)
    return out, dict(rk=sk.astype(f64), reps=se.astype(f64))


# ---------------------------------------------------------------------------------------------------------------------
# closed forms on linear velocity fields
# ---------------------------------------------------------------------------------------------------------------------
def closed_form(A, n, k0=K0, eps0=EPS0):
    """The answers per cell (float64) for u = A x, k = k0, eps = eps0 (Float32 values, widened)."""
    k0, e0 = f64(k0), f64(eps0)
    P = {key: f64(v) for key, v in PARAMS.items()}
    S = lm.answers(A, np.ones(n, f32))["S"]
    tr = float(np.trace(A.astype(f64)))
    nut = P["Cmu"] * k0 ** 2 / e0
    rk = nut * S ** 2 - e0 - k0 * tr
    reps = P["C1"] * nut * S ** 2 * e0 / k0 - P["C2"] * e0 ** 2 / k0 - e0 * tr
    return dict(rk=rk, reps=reps, nut=np.full(n, nut, f64), S=S)


_BOUNDS = {}


def bounds(key, part, op):
    """{output: 4 x max over the three fields and the cells of ``les_model.interior(part)`` of |Float32 oracle composition -
    closed form|} for the mesh ``key`` (computed once), and the deviations themselves."""
    if key not in _BOUNDS:
        sel = lm.interior(part)
        n = sel.size
        k, eps = np.full(n, K0, f32), np.full(n, EPS0, f32)
        dev = {}
        for name, make in lm.FIELDS:
            A = make(part.ndims)
            got, _ = oracle_rhs(op, lm.linear_field(part, A), k, eps, dtype=f32)
            ans = closed_form(A, n)
            for o in OUTPUTS:
                dev[o] = max(dev.get(o, 0.0), float(np.abs(got[o].astype(f64) - ans[o])[sel].max()))
        _BOUNDS[key] = ({o: 4.0 * v for o, v in dev.items()}, dev)
    return _BOUNDS[key]


_WAVY = {}


def wavy_reference(key, part, op, seed=21):
    """(fields, Float64 oracle composition, scales, {output: max over the cells of |Float32 oracle - Float64 oracle| / scale})
    of the wavy fields on the mesh ``key`` (computed once), for rk, reps and nut (scaled by its own magnitude; S is held to
    its table answers on the linear fields)."""
    if key not in _WAVY:
        vel = wavy_velocity(part, seed)
        k, eps = k_eps_fields(part, seed + 1)
        ref, scale = oracle_rhs(op, vel, k, eps, dtype=f64)
        o32, _ = oracle_rhs(op, vel, k, eps, dtype=f32)
        scale["nut"] = np.abs(ref["nut"])
        dev = {o: float((np.abs(o32[o].astype(f64) - ref[o]) / scale[o]).max()) for o in WAVY_OUTPUTS}
        _WAVY[key] = ((vel, k, eps), ref, scale, dev)
    return _WAVY[key]

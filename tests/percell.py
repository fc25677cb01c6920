"""Per-cell error checks of the fused residual sweeps against a float64 evaluation of the oracle.

Test infrastructure.  A norm-wise check (``conftest.rel_inf``: max |got - exp| / max |exp|) cannot see a wrong coarse
block: for a noisy state the residual grows like 1/h, so the coarsest level sits ~700x below the finest one and a
0.1 % error on every coarsest-level cell passes 1e-5.  Here every cell is held to its own scale:

- scalar sweeps: ``conftest.stencil_scale`` = |ref| + max |u| over the cell and its face neighbours / h;
- Euler sweeps, per variable v: |ref_v| + max over the cell's two-deep face neighbourhood of sum_d |F_d,v(P)| / h, with
  F_d(P) = inviscid_fluxes(P, P, d) the physical flux (HLL consistency): the residual is a difference of such fluxes.

The reference is the numpy oracle evaluated in float64 (it is dtype-generic: Float32 inputs give the Float32 oracle
bit for bit, tests/test_golden.py).  ``check`` reports the worst cell of every class -- refinement level, image /
skirt, the side kinds of the cell's faces and, in 2-D, the block class of the partition tables (quad, pair, single,
face-list cell, deeper-cell table) -- so that a failure points at a class.
"""
import numpy as np

from oracle import cfd as ocfd
from oracle import domain as od

f32, f64 = np.float32, np.float64

# Per-cell bounds of the GPU sweeps against the float64 reference.  The Float32 oracle and its C restatement stay below
# half of them on every test case (tests/test_percell.py::test_calibration: 4.6e-7 scalar, 1.0e-6 Euler); a 1e-4 relative
# error on the coarsest level alone reads 3e-5 (tests/test_percell.py::test_sensitivity).
BOUND = 2e-6
BOUND_EULER = 2.5e-6
# Bounds across flow regimes (tests/regimes.py), with the scales ``scalar_scale_c`` / ``euler_scale_waves``: 4 x the worst
# Float32-oracle / C-restatement figure over every regime and case of tests/test_percell_regimes.py::test_calibration
# (scalar 4.3e-7 at the tiny C on the smooth u, Euler 3.9e-7 at rest), rounded up to one digit and capped at BOUND /
# BOUND_EULER.  4 x: the tuned device forms measure about 1 x the literal Float32 arithmetic under the present scales; the
# factor leaves room for their reciprocal and regrouped HLL combine without admitting a wrong term.
BOUND_SCALAR_REGIMES = 2e-6   # 4 x 4.3e-7 = 1.7e-6
BOUND_EULER_REGIMES = 2e-6    # 4 x 3.9e-7 = 1.6e-6
# Bounds per kernel family against the float64 references below, each with the scales of ``*_scale``: the Float32 oracle
# stays at or below half of each on every case of tests/test_percell_closures.py::test_calibration, which prints the
# measured maxima (2-D RAE2822 / advection partitions and the 3-D octree: operators 1.1e-7, viscous sum 6.1e-8, shear rate
# 3.6e-8, Wray-Agarwal 5.7e-8, transport 1.1e-7, whole closures 2.6e-7).  The device kernels follow the oracle's evaluation
# order except for the Sutherland power (exp2 / log2, a few ulps) and the Euler rows' HLL flux (BOUND_EULER's argument).
BOUND_OPS = 1e-6         # at_faces, face_gradient, green_gauss, divergent, cell_gradient, JST_sensor, MUSCL
BOUND_VISCOUS = 1e-6     # R0 + sum_d green_gauss(viscous_fluxes(...), d)
BOUND_TRANSPORT = 1e-6   # S + sum_d green_gauss(at_faces(nu + nuR) face_gradient(R) - at_faces(u_d R), d)
BOUND_TURB = 1e-6        # shear_rate of the cell gradients, Wray_Agarwal(R, S, grad R, grad S)
BOUND_CLOSURE = 2.5e-6   # navier_stokes / euler_wray_agarwal_residual: the Euler rows carry BOUND_EULER's HLL flux


def oracle_advection_residual(part, u, C):
    """test/advection.jl:67-83 with ud starting from zero, in the dtype of ``u`` and ``C``."""
    ud = np.zeros_like(u)
    D = od.JST_sensor(part, u)
    for dim in range(1, part.ndims + 1):
        Cf = od.at_faces(part, np.ascontiguousarray(C[:, dim - 1]), dim)
        gu = od.cell_gradient(part, u, dim)
        uL, uR = od.MUSCL(part, u, gu, dim, D=D, high_order=True)
        ud -= od.green_gauss(part, (uL + uR) * Cf / f32(2) + np.abs(Cf) * (uL - uR) / f32(2), dim)
    return ud


def oracle_euler_residual(part, P, fluid):
    """Euler HLL residual composed from the reference operators, in the dtype of ``P``."""
    R = np.zeros_like(P)
    D = od.JST_sensor(part, np.ascontiguousarray(P[:, 0]))
    for dim in range(1, part.ndims + 1):
        gP = od.cell_gradient(part, P, dim)
        PL, PR = od.MUSCL(part, P, gP, dim, D=D, high_order=True)
        F = ocfd.inviscid_fluxes(fluid, PL, PR, dim)
        R -= od.green_gauss(part, F, dim)  # Float64 flux, rounded on the in-place update
    return R


def ref64_advection(part, u, C):
    r = oracle_advection_residual(part, np.asarray(u).astype(f64), np.asarray(C).astype(f64))
    assert r.dtype == f64
    return r


def ref64_euler(part, P, fluid=None):
    r = oracle_euler_residual(part, np.asarray(P).astype(f64), fluid or ocfd.Fluid())
    assert r.dtype == f64
    return r


def _face_max(part, a):
    """max of ``a`` over each cell and its face neighbours (rows of a 1-D or 2-D array)."""
    m = a.copy()
    for d in range(1, part.ndims + 1):
        o, nb = part.face_owners_neighbors[d]
        np.maximum.at(m, o, a[nb])
        np.maximum.at(m, nb, a[o])
    return m


def scalar_scale(part, u, ref):
    from conftest import stencil_scale
    return stencil_scale(part, u, ref)


def euler_scale(part, P, ref, fluid=None):
    """(nc, nv) scale of the Euler residual: |ref_v| + max over the two-deep face neighbourhood of sum_d |F_d,v(P)| / h."""
    fluid = fluid or ocfd.Fluid()
    P64 = np.asarray(P).astype(f64)
    F = np.zeros_like(P64)
    for d in range(1, part.ndims + 1):
        F += np.abs(ocfd.inviscid_fluxes(fluid, P64, P64, d))
    m = _face_max(part, _face_max(part, F))
    h = np.asarray(part.spacing).min(axis=1).astype(f64)
    return np.abs(np.asarray(ref, dtype=f64)) + m / h[:, None]


def euler_scale_waves(part, P, ref, fluid=None):
    """(nc, nv) scale of the Euler residual that holds in every flow regime: |ref_v| + max over the two-deep face
    neighbourhood of sum_d [|Q_v| (|u_d| + a) + pressure terms] / h, with Q = primitive2state(P), a = speed_of_sound(T)
    and the pressure terms p in the momentum row of direction d and p |u_d| in the energy row -- the HLL flux with every
    difference turned into a sum.  ``euler_scale``'s physical flux vanishes with the velocity; the dissipation term
    SL SR (QR - QL) / (SL - SR) ~ a dQ does not."""
    fluid = fluid or ocfd.Fluid()
    P64 = np.asarray(P).astype(f64)
    Q = np.abs(ocfd.primitive2state(fluid, P64))
    a = ocfd.speed_of_sound(fluid, P64[:, 1]).astype(f64)
    p = np.abs(P64[:, 0])
    W = np.zeros_like(P64)
    for d in range(1, part.ndims + 1):
        ud = np.abs(P64[:, 1 + d])
        W += Q * (ud + a)[:, None]
        W[:, 1] += p * ud
        W[:, 1 + d] += p
    m = _face_max(part, _face_max(part, W))
    h = np.asarray(part.spacing).min(axis=1).astype(f64)
    return np.abs(np.asarray(ref, dtype=f64)) + m / h[:, None]


def scalar_scale_c(part, u, C, ref):
    """Scale of the advection residual that carries the advecting velocity: |ref| + (max over the cell and its face
    neighbours of sum_d |C_d|) (max over the same cells of |u|) / h.  ``scalar_scale`` is this with sum_d |C_d| = 1."""
    c = _face_max(part, np.abs(np.asarray(C).astype(f64)).sum(axis=1))
    m = _face_max(part, np.abs(np.asarray(u).astype(f64)))
    h = np.asarray(part.spacing).min(axis=1).astype(f64)
    return np.abs(np.asarray(ref, dtype=f64)) + c * m / h


def percell_error(got, ref, scale):
    """|got - ref| / scale per cell (and variable); 0 where both the difference and the scale are 0 (a product with a
    zero factor, e.g. R = 0 in the Wray-Agarwal source)."""
    d = np.abs(np.asarray(got, dtype=f64) - np.asarray(ref, dtype=f64))
    s = np.broadcast_to(np.asarray(scale, dtype=f64), d.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(s > 0, d / np.where(s > 0, s, 1.0), np.where(d == 0, 0.0, np.inf))


# ---------------------------------------------------------------------------------------------------------------------
# cell classes
# ---------------------------------------------------------------------------------------------------------------------
def levels(part):
    """Refinement level per cell: 0 = finest."""
    h = np.asarray(part.spacing).min(axis=1)
    hs = np.unique(h)
    return np.searchsorted(hs, h)


def _side_classes(part):
    """Per cell: has a face to a coarser cell / to finer cells / a mirror face / no face on some side."""
    nc = part.spacing.shape[0]
    sp = np.asarray(part.spacing)
    coarse = np.zeros(nc, bool)
    fine = np.zeros(nc, bool)
    mirror = np.zeros(nc, bool)
    edge = np.zeros(nc, bool)                    # no face at all on one side: the edge of a skirt
    for d in range(1, part.ndims + 1):
        o, nb = part.face_owners_neighbors[d]
        ho, hn = sp[o, d - 1], sp[nb, d - 1]
        coarse[o[hn > ho]] = True
        coarse[nb[ho > hn]] = True
        fine[o[hn < ho]] = True
        fine[nb[ho < hn]] = True
        mirror[o[o == nb]] = True                # a mirror face names the cell twice
        nleft = np.bincount(nb, minlength=nc)    # faces on the low side of the cell (the cell is the neighbour)
        nright = np.bincount(o, minlength=nc)
        edge |= (nleft == 0) | (nright == 0)
    return dict(side_coarse=coarse, side_fine=fine, side_mirror=mirror, side_open=edge,
                side_same=~(coarse | fine | mirror | edge))


def _block_classes_2d(part):
    """Block classes of the 2-D quad sweep from the library's host-side analysis (csrc/ibh_analyze.cpp)."""
    from ibamd import hostview
    A = hostview.analyze2(part)
    nc = part.spacing.shape[0]
    out = {}

    def cells(bases, n):
        m = np.zeros(nc, bool)
        if len(bases):
            m[(np.asarray(bases, np.int64)[:, None] + np.arange(n)).ravel()] = True
        return m
    blocks = A["blocks"]
    Q = A["quads_all"]
    out["quad"] = cells(Q["desc"]["base"], 256)
    out["pair"] = cells(Q["pair_desc"]["base"], 128)
    single = Q["singles2"] if len(Q["pair_desc"]) else Q["singles"]
    out["single"] = cells(blocks["base"][single], 64)
    out["deeper_table"] = cells(blocks["base"][blocks["dt"] >= 0], 64)
    out["face_list"] = ~cells(blocks["base"], 64)
    QI = A["quads_image"]
    out["image_quad"] = cells(QI["desc"]["base"], 256)
    out["image_single"] = cells(blocks["base"][QI["singles"]], 64) if len(QI["singles"]) else np.zeros(nc, bool)
    return out


def cell_classes(part, block_classes=True):
    """{class name: boolean mask over the partition's cells}."""
    nc = part.spacing.shape[0]
    out = {}
    lev = levels(part)
    for k in range(lev.max() + 1):
        out[f"level{k}"] = lev == k
    img = np.zeros(nc, bool)
    img[np.asarray(part.image_in_domain)] = True
    out["image"] = img
    out["skirt"] = ~img
    out.update(_side_classes(part))
    if block_classes and part.ndims == 2 and getattr(part, "block_size", 8) == 8:
        out.update(_block_classes_2d(part))
    return {k: v for k, v in out.items() if v.any()}


# ---------------------------------------------------------------------------------------------------------------------
# the check
# ---------------------------------------------------------------------------------------------------------------------
def report(err, classes, got=None, ref=None, scale=None):
    """One line per class: worst cell (and variable), its error, value, reference and scale."""
    e = err if err.ndim == 2 else err[:, None]
    lines = []
    for name, mask in classes.items():
        if not mask.any():
            continue
        sub = e[mask]
        i, v = np.unravel_index(int(np.argmax(sub)), sub.shape)
        c = int(np.nonzero(mask)[0][i])
        s = f"  {name:>14s} ({int(mask.sum()):6d} cells): max {sub[i, v]:.3e} at cell {c} var {v}"
        if got is not None:
            g = np.asarray(got, dtype=f64).reshape(e.shape[0], -1)
            r = np.asarray(ref, dtype=f64).reshape(e.shape[0], -1)
            sc = np.asarray(scale, dtype=f64).reshape(e.shape[0], -1)
            s += f" (got {g[c, v]:.7g}, ref {r[c, v]:.7g}, scale {sc[c, v]:.3g})"
        lines.append(s)
    return "\n".join(lines)


def nan_pattern_mismatch(got, ref64, sel=None):
    """Entries where exactly one of ``got`` and ``ref64`` is NaN (Julia's ``clamp`` / ``min`` / ``max`` propagate NaN, so the
    device must produce NaN exactly where the float64 oracle does), restricted to the rows of ``sel``."""
    g, r = np.asarray(got, dtype=f64), np.asarray(ref64, dtype=f64)
    bad = np.isnan(g) != np.isnan(r)
    if sel is not None:
        bad &= (sel if bad.ndim == 1 else sel[:, None])
    return bad


def check(got, ref64, scale, bound, part, cells=None, classes=None, what=""):
    """First: the NaN pattern of ``got`` equals the reference's exactly (over ``cells``, all cells by default).  Then:
    max(|got - ref64| / scale) <= bound over the other cells (equal infinities count as exact); return that maximum.  A
    failure lists the worst cell of every class."""
    g, r = np.asarray(got, dtype=f64), np.asarray(ref64, dtype=f64)
    n = g.shape[0]
    sel = np.ones(n, bool)
    if cells is not None:
        sel = np.zeros(n, bool)
        sel[np.asarray(cells)] = True
    bad = nan_pattern_mismatch(g, r, sel)
    if bad.any():
        rows = bad if bad.ndim == 1 else bad.any(axis=1)
        cls = classes if classes is not None else cell_classes(part)
        per = ", ".join(f"{k} {int((m & rows).sum())}" for k, m in cls.items() if (m & rows).any())
        c = int(np.nonzero(rows)[0][0])
        raise AssertionError(f"{what}: NaN pattern differs from the reference on {int(bad.sum())} entries "
                             f"({int((np.isnan(g) & bad).sum())} NaN only in got); first cell {c}: got "
                             f"{g[c]}, ref {r[c]}; cells per class: {per}")
    nanr = np.isnan(r)
    same_inf = np.isinf(r) & (g == r)
    err = np.where(nanr | same_inf, 0.0, percell_error(np.where(nanr, 0.0, g), np.where(nanr | same_inf, 0.0, r),
                                                       np.where(nanr, 1.0, scale)))
    e = np.where(sel if err.ndim == 1 else sel[:, None], err, 0.0)
    worst = float("nan") if np.isnan(e).any() else float(e.max())
    if not worst <= bound:
        cls = classes if classes is not None else cell_classes(part)
        cls = {k: m & sel for k, m in cls.items()}
        nan = np.isnan(e).any(axis=1) if e.ndim == 2 else np.isnan(e)
        msg = (f"{what}: per-cell error {worst:.3e} > bound {bound:.1e}; {int(nan.sum())} NaN cells; "
               f"worst cell per class:\n" + report(np.nan_to_num(e, nan=np.inf), cls, got, ref64, scale))
        raise AssertionError(msg)
    return worst


def faces_to_cells(part, dim, fe):
    """Per-face values -> per-cell maxima over the cell's faces along ``dim`` (owner and neighbour side), so that a face
    error is reported in the classes of the cells it touches."""
    o, nb = part.face_owners_neighbors[dim]
    fe = np.asarray(fe, dtype=f64)
    shape = (part.spacing.shape[0],) + fe.shape[1:]
    m = np.zeros(shape)
    np.maximum.at(m, o, fe)
    np.maximum.at(m, nb, fe)
    return m


def check_faces(got, ref64, scale, bound, part, dim, classes=None, what=""):
    """``check`` of a face array along ``dim``: NaN pattern per face first, then the per-face error folded onto the cells."""
    g, r = np.asarray(got, dtype=f64), np.asarray(ref64, dtype=f64)
    bad = nan_pattern_mismatch(g, r)
    if bad.any():
        o, nb = part.face_owners_neighbors[dim]
        rows = np.nonzero(bad if bad.ndim == 1 else bad.any(axis=1))[0]
        sp = np.asarray(part.spacing)[:, dim - 1]
        first = "; ".join(f"face {f} (owner {o[f]} h {sp[o[f]]:.3g}, neighbour {nb[f]} h {sp[nb[f]]:.3g}): got {g[f]}, "
                          f"ref {r[f]}" for f in rows[:3])
        raise AssertionError(f"{what}: NaN pattern differs from the reference on {int(bad.sum())} face entries: {first}")
    nanr = np.isnan(r)
    fe = np.where(nanr, 0.0, percell_error(np.where(nanr, 0.0, g), np.where(nanr, 0.0, r), np.where(nanr, 1.0, scale)))
    zero = np.zeros(part.spacing.shape[0] if fe.ndim == 1 else (part.spacing.shape[0], fe.shape[1]))
    return check(faces_to_cells(part, dim, fe), zero, np.ones_like(zero), bound, part, classes=classes, what=what)


# ---------------------------------------------------------------------------------------------------------------------
# operators, viscous fluxes and the turbulence closure of BASELINE.json configs[4]
# ---------------------------------------------------------------------------------------------------------------------

def _c(a):
    return np.ascontiguousarray(a)


def oracle_viscous_sum(part, P, mut, R0=None, fluid=None):
    """R0 + sum_d green_gauss(viscous_fluxes(at_faces(P), face_gradient(P, cell_gradient(P), d), d;
    mu_t = at_faces(mu_t)), d) (cfd.jl:664-736 over ImmersedBoundary.jl:899-1069), in the dtype of ``P``."""
    fluid = fluid or ocfd.Fluid()
    R = np.zeros_like(P) if R0 is None else np.array(R0, dtype=P.dtype)
    gP = od.cell_gradient(part, P)
    for d in range(1, part.ndims + 1):
        Fv = ocfd.viscous_fluxes(fluid, od.at_faces(part, P, d), od.face_gradient(part, P, gP, d), d,
                                 mu_t=od.at_faces(part, mut, d))
        R += od.green_gauss(part, Fv, d)
    return R


def oracle_transport(part, R, nuR, vel, nu, S):
    """S + sum_d green_gauss(at_faces(nu + nuR) .* face_gradient(R) .- at_faces(vel[:, d] .* R), d)."""
    rt = np.array(S, copy=True)
    for d in range(1, part.ndims + 1):
        conv = od.at_faces(part, _c(vel[:, d - 1]) * R, d)
        diff = od.at_faces(part, nu + nuR, d) * od.face_gradient(part, R, d)
        rt += od.green_gauss(part, diff - conv, d)
    return rt


def oracle_velocity_gradients(part, vel):
    """g[i][j] = cell_gradient(vel[:, i], j + 1)."""
    nd = part.ndims
    return [[od.cell_gradient(part, _c(vel[:, i]), j + 1) for j in range(nd)] for i in range(nd)]


def oracle_wray_agarwal_of(part, R, S):
    from oracle import turbulence as ot
    gR = np.stack([od.cell_gradient(part, R, d + 1) for d in range(part.ndims)], axis=1)
    gS = np.stack([od.cell_gradient(part, S, d + 1) for d in range(part.ndims)], axis=1)
    return ot.Wray_Agarwal(R, S, gR, gS)


def oracle_wa_residual(part, Q, nu, fluid=None, viscous=True):
    """``closures.navier_stokes_wray_agarwal_residual`` (``viscous``) / ``euler_wray_agarwal_residual`` without boundary
    conditions, ``Q = [p T u v (w) R]``, in the dtype of ``Q``."""
    from oracle import turbulence as ot
    fluid = fluid or ocfd.Fluid()
    nvp = part.ndims + 2
    r = np.zeros_like(Q)
    r[:, :nvp] = oracle_euler_residual(part, _c(Q[:, :nvp]), ocfd.Fluid())
    R = _c(Q[:, nvp])
    S = ot.shear_rate(oracle_velocity_gradients(part, Q[:, 2:nvp]))
    wa = oracle_wray_agarwal_of(part, R, S)
    r[:, nvp] = oracle_transport(part, R, wa["nuR"], Q[:, 2:nvp], nu, wa["S"])
    if viscous:
        mut = (Q[:, 0] / (fluid.R * Q[:, 1])) * wa["nut"]
        r[:, :nvp] = oracle_viscous_sum(part, _c(Q[:, :nvp]), mut, r[:, :nvp], fluid)
    return r


def to64(*a):
    return tuple(np.asarray(x).astype(f64) for x in a)


# Scales: |ref| plus the float64 chain evaluated on magnitudes, every difference turned into a sum (a forward error
# bound: a float32 evaluation of the chain errs by a few ulps of these magnitudes, whatever cancels in the value).
def _ov(part):
    """Oracle view of a partition (the operators on the host)."""
    from conftest import oracle_view
    return oracle_view(part)


def abs_at_faces(part, a, dim):
    return od.at_faces(part, np.abs(a), dim)            # positive weights


def abs_face_gradient(part, a, dim):
    """(|u_n| + |u_o|) / dist"""
    o, nb = part.face_owners_neighbors[dim]
    a = np.abs(a)
    s = a[nb] + a[o]
    dist = od.face_distance(part, dim).astype(f64)
    return s / (dist if s.ndim == 1 else dist[:, None])


def abs_green_gauss(part, af, dim):
    return od.unsigned_green_gauss(part, np.abs(af), dim)


def abs_cell_gradient(part, a, dim):
    return abs_green_gauss(part, abs_at_faces(part, a, dim), dim)


def abs_viscous_fluxes(fluid, Pa, Ga, dim, muta):
    """viscous_fluxes on magnitudes: mu(T) + mu_t, k(T) with |k_i|, every sum of gradient entries a sum of magnitudes."""
    T = Pa[:, 1]
    mu = ocfd.dynamic_viscosity(fluid, T) + muta
    k = sum(abs(ki) * T ** i for i, ki in enumerate(fluid.k))
    nd = Pa.shape[1] - 2

    def vg(i, j):
        return Ga[j - 1][:, 1 + i]
    divu = sum(vg(i, i) for i in range(1, nd + 1))

    def tau(i, j):
        return (vg(i, j) + vg(j, i) + (f64(2) / 3 * divu if i == j else 0.0)) * mu
    F = np.zeros_like(Pa)
    F[:, 1] = Ga[dim - 1][:, 1] * k
    for j in range(1, nd + 1):
        F[:, 1] += tau(dim, j) * Pa[:, 1 + j]
        F[:, 1 + j] = tau(dim, j)
    return F


def viscous_sum_abs(part, P, mut, fluid=None):
    """Magnitude chain of the viscous sum (without R0)."""
    part = _ov(part)
    fluid = fluid or ocfd.Fluid()
    Pa, ma = np.abs(np.asarray(P, f64)), np.abs(np.asarray(mut, f64))
    gPa = [abs_cell_gradient(part, Pa, d) for d in range(1, part.ndims + 1)]
    s = np.zeros_like(Pa)
    for d in range(1, part.ndims + 1):
        Ga = [abs_face_gradient(part, Pa, d) if i == d else abs_at_faces(part, gPa[i - 1], d)
              for i in range(1, part.ndims + 1)]
        s += abs_green_gauss(part, abs_viscous_fluxes(fluid, abs_at_faces(part, Pa, d), Ga, d, abs_at_faces(part, ma, d)), d)
    return s


def viscous_scale(part, P, mut, ref, R0=None, fluid=None):
    s = np.abs(np.asarray(ref, f64)) + viscous_sum_abs(part, P, mut, fluid)
    return s if R0 is None else s + np.abs(np.asarray(R0, f64))


def transport_scale(part, R, nuR, vel, nu, S, ref, S_scale=None):
    """|ref| + |S| (or the scale of S) + sum_d ugg(at_faces(nu + |nuR|) (|R_n| + |R_o|) / dist + at_faces(|u_d R|))."""
    part = _ov(part)
    R, nuR, vel, S = to64(R, nuR, vel, S)
    s = np.abs(np.asarray(ref, f64)) + (np.abs(S) if S_scale is None else S_scale)
    for d in range(1, part.ndims + 1):
        s += abs_green_gauss(part, abs_at_faces(part, abs(f64(nu)) + np.abs(nuR), d) * abs_face_gradient(part, R, d)
                             + abs_at_faces(part, vel[:, d - 1] * R, d), d)
    return s


def gradient_scales(part, vel):
    """gs[i][j]: magnitude chain of cell_gradient(vel[:, i], j + 1)."""
    part = _ov(part)
    vel = np.asarray(vel, f64)
    nd = part.ndims
    return [[abs_cell_gradient(part, vel[:, i], j + 1) for j in range(nd)] for i in range(nd)]


def shear_scale(part, vel, S):
    """shear_rate = sqrt(2 |sym g|_F^2) is sqrt(2)-Lipschitz in the gradient entries: |S| + sqrt(2) sum_ij gs_ij."""
    gs = gradient_scales(part, vel)
    return np.abs(np.asarray(S, f64)) + np.sqrt(2.0) * sum(g for row in gs for g in row)


def _min_scale(a, b, sa, sb):
    """Scale of min(a, b): the taken branch's, both where the two are within the rounding of each other."""
    tie = np.abs(a - b) <= 1e-4 * (sa + sb)
    return np.where(tie, sa + sb, np.where(a < b, sa, sb))


def wray_agarwal_scale(part, R, S, S_scale=None, sigmaR=f32(0.72), C1=f32(0.0829), kappa=f32(0.41)):
    """Scales of Wray_Agarwal(R, S, cell_gradient(R), cell_gradient(S)) with R exact and S exact (or of scale S_scale):
    {"nut", "nuR", "S"} for the source min(C1 R S + C2 (grad R . grad S) R / (S + eps), 10 R)."""
    part = _ov(part)
    from oracle import turbulence as ot
    R, S = to64(R, S)
    Ss = np.abs(S) if S_scale is None else np.asarray(S_scale, f64)
    C2 = f64(sigmaR + C1 / kappa ** 2)
    eps = f64(ot.EPS)
    gR = np.stack([od.cell_gradient(part, R, d) for d in range(1, part.ndims + 1)], axis=1)
    gS = np.stack([od.cell_gradient(part, S, d) for d in range(1, part.ndims + 1)], axis=1)
    gRa = np.stack([abs_cell_gradient(part, R, d) for d in range(1, part.ndims + 1)], axis=1)
    gSa = np.stack([abs_cell_gradient(part, Ss, d) for d in range(1, part.ndims + 1)], axis=1)
    dot = (gR * gS).sum(axis=1)
    den = S + eps
    src = f64(C1) * R * S + C2 * dot * (R / den)
    s_src = np.abs(src) + f64(C1) * np.abs(R) * Ss + C2 * (gRa * gSa).sum(axis=1) * np.abs(R) / den
    if S_scale is not None:   # S itself carries an error: d src / d S = C1 R - C2 dot R / (S + eps)^2
        s_src = s_src + np.abs(f64(C1) * R - C2 * dot * R / den ** 2) * Ss
    ten = 10.0 * R
    s = np.abs(np.minimum(src, ten)) + _min_scale(src, ten, s_src, np.abs(ten))
    return dict(nut=np.abs(R), nuR=np.abs(R) * f64(sigmaR), S=s)


def closure_scale(part, Q, ref, nu, fluid=None, viscous=True):
    """(nc, nd + 3) scale of ``oracle_wa_residual``: the Euler scale (+ the viscous chain) on [p T u ..], the transport
    scale with the Wray-Agarwal source's (S from the velocity gradients) on R."""
    part = _ov(part)
    from oracle import turbulence as ot
    fluid = fluid or ocfd.Fluid()
    nvp = part.ndims + 2
    Q64 = np.asarray(Q, f64)
    ref = np.asarray(ref, f64)
    s = np.empty_like(Q64)
    s[:, :nvp] = euler_scale(part, Q64[:, :nvp], ref[:, :nvp], fluid)
    # + the HLL dissipation's magnitude, (a + |u_d|) |U(P)|: euler_scale's physical flux alone vanishes where the
    # velocities cross zero
    P64 = Q64[:, :nvp]
    a = ocfd.speed_of_sound(fluid, P64[:, 1])
    U = np.abs(ocfd.primitive2state(fluid, P64))
    D = sum((a + np.abs(P64[:, 1 + d]))[:, None] * U for d in range(1, part.ndims + 1))
    s[:, :nvp] += _face_max(part, _face_max(part, D)) / np.asarray(part.spacing).min(axis=1).astype(f64)[:, None]
    vel = Q64[:, 2:nvp]
    S = ot.shear_rate(oracle_velocity_gradients(part, vel))
    Ssc = shear_scale(part, vel, S)
    R = Q64[:, nvp]
    was = wray_agarwal_scale(part, R, S, S_scale=Ssc)
    if viscous:
        mut = (Q64[:, 0] / (f64(fluid.R) * Q64[:, 1])) * R
        s[:, :nvp] += viscous_sum_abs(part, Q64[:, :nvp], mut, fluid)
    s[:, nvp] = transport_scale(part, R, R * f64(0.72), vel, nu, np.zeros_like(R), ref[:, nvp], S_scale=was["S"])
    return s


# operators: float64 references and scales
def muscl_scale(part, u, du, dim, D=None, high_order=False):
    """Magnitude chain of MUSCL's uL / uR (minmod is 1-Lipschitz in each argument)."""
    part = _ov(part)
    u, du = to64(u, du)
    o, nb = part.face_owners_neighbors[dim]
    do, dn = od.owner_distance(part, dim).astype(f64), od.neighbor_distance(part, dim).astype(f64)
    if u.ndim == 2:
        do, dn = do[:, None], dn[:, None]
    ua, una, duo, dun = np.abs(u[o]), np.abs(u[nb]), np.abs(du[o]), np.abs(du[nb])
    guf = (ua + una) / (do + dn)
    s = ua + una + (2 * duo + guf) * do + (2 * dun + guf) * dn
    if D is None:
        return s
    Df = np.maximum(np.maximum(np.asarray(D, f64)[o], np.asarray(D, f64)[nb]), 1e-7)
    if u.ndim == 2:
        Df = Df[:, None]
    uf = (ua * dn + una * do) / (do + dn)
    if high_order:
        uf = uf + (duo * do + dun * dn) / 8
    return s * Df + (1 + Df) * uf


def closure_field(x, seed=3, nu=f32(1.5e-5)):
    """Q = [p T u v (w) R] that reaches the closures' branches: velocities of +-30 that cross zero, a uniform-velocity
    region (x > 80 % of the box: S = 0 exactly and R / (S + eps) large at its edge), R = 0 (mu_t = 0) where y < 10 % of the
    box, where the Wray-Agarwal source takes 10 R on most cells, and a few cells with T below, at and just above 10 K."""
    rng = np.random.default_rng(seed)
    n, nd = x.shape
    Q = np.empty((n, nd + 3), f32)
    Q[:, 0] = 1e5 * (1 + 0.05 * rng.uniform(-1, 1, n))
    Q[:, 1] = 288.15 * (1 + 0.05 * rng.uniform(-1, 1, n))
    lo, hi = x.min(axis=0), x.max(axis=0)
    xi = (x - lo) / (hi - lo)
    for d in range(nd):
        Q[:, 2 + d] = 30 * np.sin(2 * np.pi * xi[:, (d + 1) % nd] + d) + 5 * rng.uniform(-1, 1, n)
    Q[xi[:, 0] > 0.8, 2:2 + nd] = f32(100.0)
    Q[:, nd + 2] = 3 * nu * (1 + 0.5 * rng.uniform(0, 1, n))
    Q[xi[:, 1] < 0.1, nd + 2] = 0
    cold = np.nonzero(xi[:, 1] > 0.9)[0][:8]
    Q[cold, 1] = f32([9.5, 9.999999, 10.0, 10.000001, 10.5, 11.0, 12.0, 20.0])[:cold.size]
    return Q

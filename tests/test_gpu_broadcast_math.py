"""The widened device broadcast (``ibh_ew_eval``'s extended opcodes) against the numpy model of tests/ew_model.py: every
opcode on the one-wide and four-wide interpreters, column and row vectors, tails; fused against node by node; the
reference's CFD / turbulence formulas written as generic ``HipArray`` broadcasts against the oracle and the dedicated
kernels; Bool arrays; a graph replay."""
import numpy as np
import pytest
import torch

import ibamd
from ibamd import _lib
from ibamd import cfd as dcfd
from ibamd import hiparray as H
from ibamd import turbulence as dturb
from conftest import rel_inf
from ew_model import ARITY, EXACT, ROUNDED, model, same_bits, ulp_distance
from oracle import cfd as ocfd
from oracle import turbulence as oturb

pytestmark = pytest.mark.gpu
f32 = np.float32
A = ibamd.HipArray
INF = float("inf")
SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-40, -1e-40, 1.0, -1.0, 2.0, -3.0], f32)
BOOL_FIRST = {H.AND: 2, H.OR: 2, H.NOT: 1, H.BMUL: 1, H.IFELSE: 1}   # how many leading operands are Bool


def _ranges(op, rng, n):
    """Seeded operands of op (each an (n,) float32 array), special values mixed in."""
    u = lambda lo, hi: rng.uniform(lo, hi, n).astype(f32)  # noqa: E731
    lg = lambda lo, hi: (10.0 ** rng.uniform(lo, hi, n)).astype(f32)  # noqa: E731
    if op == H.EXP:
        xs = [u(-90, 90)]
    elif op == H.EXP2:
        xs = [u(-130, 130)]
    elif op in (H.LOG, H.LOG2, H.LOG10):
        xs = [np.where(rng.random(n) < 0.05, -1, 1).astype(f32) * lg(-40, 38)]
    elif op in (H.SIN, H.COS):
        xs = [np.concatenate([u(-10, 10)[: n // 2], u(-1e4, 1e4)[: n - n // 2]])]
    elif op == H.TANH:
        xs = [u(-12, 12)]
    elif op == H.ATAN:
        xs = [u(-1e3, 1e3)]
    elif op == H.POW:
        base = lg(-3, 3)
        base[::7] *= -1
        e = u(-6, 6)
        e[::7] = np.round(e[::7])              # negative bases under integer exponents keep their sign
        xs = [base, e]
    elif op == H.ATAN2:
        xs = [u(-5, 5), u(-5, 5)]
    else:
        xs = [u(-4, 4) for _ in range(ARITY[op])]
    nb = BOOL_FIRST.get(op, 0)
    for k in range(nb):
        xs[k] = (rng.random(n) < 0.5).astype(f32)
    for k in range(nb, len(xs)):               # special values in every float operand, in all combinations
        m = len(SPECIAL)
        xs[k][: m * m] = np.tile(SPECIAL, m) if k % 2 == 0 else np.repeat(SPECIAL, m)
    return xs


ALL = sorted(ARITY)


def _dev(x, b):
    h = A(x)
    h._bool = b
    return h


@pytest.mark.parametrize("width", ["one", "four"])
@pytest.mark.parametrize("op", ALL)
def test_opcode_against_model(op, width):
    """Flat (n·nv not a multiple of 4: the four-wide path has a tail), column-vector and row-vector operands."""
    _lib.call("ibh_set_tuning", b"ew_scalar", 1 if width == "one" else 0)
    try:
        rng = np.random.default_rng(op)
        n, nv = 1001, 3
        flat = _ranges(op, rng, n * nv)
        nb = BOOL_FIRST.get(op, 0)
        cases = []
        # (a) every operand an (n, nv) field
        cases.append(([_dev(x.reshape(nv, n).T, k < nb) for k, x in enumerate(flat)],
                      [x.reshape(nv, n).T for x in flat]))
        # (b) the last operand a column vector (n,) over the columns
        col = flat[-1][:n]
        cases.append(([_dev(x.reshape(nv, n).T, k < nb) for k, x in enumerate(flat[:-1])] + [_dev(col, nb == len(flat))],
                      [x.reshape(nv, n).T for x in flat[:-1]] + [col[:, None]]))
        # (c) the last operand a host row vector (Julia's u∞'), when there is another operand to set the shape
        if len(flat) > 1 and nb < len(flat):
            row = flat[-1][:nv].copy()
            cases.append(([_dev(x.reshape(nv, n).T, k < nb) for k, x in enumerate(flat[:-1])] + [row],
                          [x.reshape(nv, n).T for x in flat[:-1]] + [row[None, :]]))
        for dev, host in cases:
            ops = tuple(H.HipArray._operand(d) for d in dev)
            first = next(d for d in ops if isinstance(d, A))
            got = first._node(op, ops, False).to_host()
            with np.errstate(all="ignore"):
                exp = model(op, *host)
                exp = np.broadcast_to(exp, (n, nv)) if got.ndim == 2 else exp.reshape(n)
            if op in EXACT:
                assert same_bits(got, exp), (op, np.argwhere(ulp_distance(got, exp) != 0)[:5])
            else:
                d = ulp_distance(got, exp)
                assert d.max() <= 2, (op, d.max(), np.argwhere(d > 2)[:5])
    finally:
        _lib.call("ibh_set_tuning", b"ew_scalar", 0)


def _big_tree(x, y, b):
    """Every new opcode in one expression tree (and old ones around them)."""
    t = H.clamp(x, -1.0, 1.5) + H.exp(y * 0.1) - H.exp2(x) * H.log(abs(y) + 1.0)
    t = t + H.log2(abs(x) + 2.0) * H.log10(abs(y) + 3.0) + H.sin(x) * H.cos(y) - H.tanh(x) + H.atan(y)
    t = t + H.atan(x, y) + H.sign(x) * H.copysign(y, x) + H.inv(y + 4.0) + x ** 0 + x ** 2 - x ** 3 + (y + 4.0) ** -2
    t = t + (abs(x) + 0.5) ** 0.6666667 + (abs(x) + 0.5) ** 5 + 2.0 ** y
    c = ((x < y) & (x <= 0.5)) | ~((x > y) | (x >= 0.25)) | H.eq(x, y) | H.ne(x, 0.1)
    return H.ifelse(c & b, t, x) + b * y - (x > 0.1) * t


def test_fused_equals_node_by_node():
    rng = np.random.default_rng(7)
    n = 4099
    x, y = rng.uniform(-3, 3, (n, 2)).astype(f32), rng.uniform(-3, 3, (n, 2)).astype(f32)
    x[:11, 0] = SPECIAL
    bm = rng.random((n, 2)) < 0.5
    small = lambda X, Y, Bb: H.clamp(X, -1.0, 1.0) * (Y < 0.5) + H.ifelse(Bb, X ** 2, H.exp(Y))  # noqa: E731
    res = {}
    for fuse in (True, False):
        H.HipArray.fuse = fuse
        try:
            X, Y, Bb = A(x), A(y), A(bm)
            res[fuse] = (_big_tree(X, Y, Bb).to_host(), small(X, Y, Bb).to_host())
        finally:
            H.HipArray.fuse = True
    for a, b in zip(res[True], res[False]):
        assert same_bits(a, b)


def test_reference_formulas_generic():
    rng = np.random.default_rng(3)
    n = 5003
    fl, of = dcfd.Fluid(), ocfd.Fluid()
    g, R, mu, Tr, S = (f32(v) for v in (fl.gamma, fl.R, fl.mu_ref, fl.Tref, fl.S))

    T = rng.uniform(-50, 3000, n).astype(f32)
    TH = A(T)
    # speed_of_sound (cfd.jl:62-64), dynamic_viscosity (:71-77)
    a = ((g * R) * H.clamp(TH, 10.0, INF)).sqrt().to_host()
    Tc = H.clamp(TH, 10.0, INF)
    mu_g = (mu * (Tc / Tr) ** (f32(2.0) / 3) * (Tr + S) / (Tc + S)).to_host()
    assert ulp_distance(a, ocfd.speed_of_sound(of, T)).max() <= 2
    assert ulp_distance(mu_g, ocfd.dynamic_viscosity(of, T)).max() <= 4
    assert rel_inf(a, ibamd.to_host(dcfd.speed_of_sound(fl, ibamd.hip(T)))) <= 1e-6
    assert rel_inf(mu_g, ibamd.to_host(dcfd.dynamic_viscosity(fl, ibamd.hip(T)))) <= 1e-6

    for nd in (2, 3):
        P = np.concatenate([rng.uniform(0.5e5, 2e5, (n, 1)), rng.uniform(5, 400, (n, 1)),
                            rng.uniform(-300, 300, (n, nd))], axis=1).astype(f32)
        PH = A(P)
        # primitive2state (:106-123)
        p, Tq, u = PH.col(1), H.clamp(PH.col(2), 10.0, INF), A(PH.t[:, 2:])
        k = (u ** 2).sum(dims=2) / 2
        rho = p / (R * Tq)
        E = rho * (R / (g - f32(1)) * Tq + k)
        Q = np.concatenate([rho.to_host()[:, None], E.to_host()[:, None], (rho * u).to_host()], axis=1)
        assert ulp_distance(Q, ocfd.primitive2state(of, P)).max() <= 4
        assert rel_inf(Q, ibamd.to_host(dcfd.primitive2state(fl, ibamd.hip(P)))) <= 1e-6
        # state2primitive (:137-151)
        QH = A(Q)
        rho, E, ru = QH.col(1), QH.col(2), A(QH.t[:, 2:])
        u = ru / rho
        k = (u ** 2).sum(dims=2) / 2
        pp = (g - f32(1)) * (E - rho * k)
        Tp = H.clamp(pp / (rho * R), 10.0, INF)
        P2 = np.concatenate([pp.to_host()[:, None], Tp.to_host()[:, None], u.to_host()], axis=1)
        assert ulp_distance(P2, ocfd.state2primitive(of, Q)).max() <= 4
        assert rel_inf(P2, ibamd.to_host(dcfd.state2primitive(fl, ibamd.hip(Q)))) <= 1e-6

        # FlowBC call (:243-300), both forms, with du!dn
        nrm = rng.standard_normal((n, nd)).astype(f32)
        nrm /= np.sqrt((nrm * nrm).sum(axis=1, dtype=f32))[:, None]
        imd, dudn = rng.uniform(1e-3, 1e-2, n).astype(f32), rng.uniform(-100, 100, n).astype(f32)
        NH = A(nrm)
        for normal_flow in (False, True):
            uinf = [f32(120.0)] if normal_flow else list(rng.uniform(-200, 200, nd).astype(f32))
            Pinf = [f32(1e5), f32(288.0)] + uinf
            p, T_, u = PH.col(1), PH.col(2), A(PH.t[:, 2:])
            un = float(uinf[0]) if normal_flow else (NH * uinf).sum(dims=2)
            cur = (u * NH).sum(dims=2)
            aa = ((g * R) * H.clamp(T_, 10.0, INF)).sqrt()
            if normal_flow:   # un is a host number: the comparisons are host Bools
                M = abs(f32(un)) / aa
                ge, lt, gt, le = un >= 0.0, un < 0.0, un > 0.0, un <= 0.0
            else:
                M = abs(un) / aa
                ge, lt, gt, le = un >= 0.0, un < 0.0, un > 0.0, un <= 0.0
            pb = ge * ((M > 1.0) * Pinf[0] + (M <= 1.0) * p) + lt * ((M > 1.0) * p + (M <= 1.0) * Pinf[0])
            Tb = gt * Pinf[1] + le * T_
            if normal_flow:
                ub = u + NH * (un - cur + 0.0)
            else:
                ub = lt * u + ge * uinf
            V = (ub * ub).sum(dims=2).sqrt() + float(np.finfo(f32).eps)
            ub = ub * ((V - A(dudn) * A(imd)) / V)
            got = np.concatenate([pb.to_host()[:, None], Tb.to_host()[:, None], ub.to_host()], axis=1)
            bc, obc = dcfd.FlowBC(fl, Pinf, normal_flow), ocfd.FlowBC(of, np.array(Pinf, f32), normal_flow)
            exp = obc(P, nrm, imd, dudn)
            assert rel_inf(got, exp) <= 1e-5, (nd, normal_flow)
            assert ulp_distance(got, exp).max() <= 4, (nd, normal_flow)   # every column, element by element
            ded = ibamd.to_host(bc(ibamd.hip(P), ibamd.hip(nrm), ibamd.hip(imd), ibamd.hip(dudn)))
            assert rel_inf(got, ded) <= 1e-6, (nd, normal_flow)

    # pressure_coefficient (:411-424): M∞ a host number (squared on the host, as the library's own form does) ...
    p = rng.uniform(0.5e5, 2e5, n).astype(f32)
    M_inf = f32(0.7)
    cp = (2.0 * (A(p) / f32(1e5) - 1.0) / (f32(M_inf * M_inf) * g)).to_host()
    assert same_bits(cp, ibamd.to_host(dcfd.pressure_coefficient(fl, ibamd.hip(p), 1e5, M_inf)))
    # ... and a per-cell Mach number on the device, so `M .^ 2` is the device literal power (M*M)
    Mc = rng.uniform(0.1, 2.0, n).astype(f32)
    cp = (2.0 * (A(p) / f32(1e5) - 1.0) / (A(Mc) ** 2 * g)).to_host()
    assert same_bits(cp, f32(2) * (p / f32(1e5) - f32(1)) / ((Mc * Mc) * g))


def test_wall_function_fixed_point_generic():
    """turbulence.jl:16 (von_Karman) and wall_function(Rey)'s 20-step fixed point (:27-70), written as broadcasts."""
    rng = np.random.default_rng(5)
    Rey_h = (10.0 ** rng.uniform(-2, 6, 20000)).astype(f32)
    kap, C, Aa, beta, bstar, D, Ap, om = (f32(v) for v in (0.41, 4.9, 19.0, 0.075, 0.09, 4.2, 360.0, 0.5))
    Rey = H.clamp(abs(A(Rey_h)), float(np.finfo(f32).eps), INF)
    Rey.t  # noqa: B018
    yp = Rey.sqrt()
    for _ in range(20):
        up = (H.log(yp.maximum_with(1.0)) / kap + C).minimum_with(yp)
        yp = om * (Rey / up) + (f32(1) - om) * yp
        yp.t  # noqa: B018 (`yp = @. ...` materialises)
    up = Rey / yp
    mup = kap * yp * (1.0 - H.exp(-yp / Aa)) ** 2
    dudy = 1.0 / (1.0 + mup)
    kp = (yp ** 2 / (f32(6.0) * bstar / beta - f32(2.0))).minimum_with(D * H.exp(-yp / Ap))
    got = dict(yplus=yp, uplus=up, muplus=mup, kplus=kp, duplus_dyplus=dudy)
    # the oracle's lines with the model's exp / log (Float32(f(Float64(x)))): `1 - exp(-yp / A)` cancels for small yp,
    # so an ulp of exp becomes hundreds of ulps of muplus -- per element, the generic form is held to the model
    mexp, mlog = ROUNDED[H.EXP], ROUNDED[H.LOG]
    r = np.clip(np.abs(Rey_h), np.finfo(f32).eps, f32(np.inf))
    y = np.sqrt(r)
    for _ in range(20):
        y = om * (r / np.minimum(mlog(np.maximum(y, f32(1))) / kap + C, y)) + (f32(1) - om) * y
    mu_ = kap * y * (f32(1) - mexp(-y / Aa)) ** 2
    model_wf = dict(yplus=y, uplus=r / y, muplus=mu_, duplus_dyplus=f32(1) / (f32(1) + mu_),
                    kplus=np.minimum(y ** 2 / (f32(6.0) * bstar / beta - f32(2.0)), D * mexp(-y / Ap)))
    exp = oturb.wall_function_rey(Rey_h)
    ded = dturb.wall_function(ibamd.hip(Rey_h))
    for key, v in got.items():
        v = v.to_host()
        assert ulp_distance(v, model_wf[key]).max() <= 2, key
        assert rel_inf(v, exp[key]) <= 1e-6, key
        assert rel_inf(v, ibamd.to_host(ded[key])) <= 1e-6, key


def test_bool_arrays():
    rng = np.random.default_rng(11)
    n, nd = 777, 3
    un, u = rng.standard_normal(n).astype(f32), rng.standard_normal((n, nd)).astype(f32)
    un[:4] = [0.0, -0.0, np.nan, -1.0]
    uinf = rng.standard_normal(nd).astype(f32)
    U, V = A(un), A(u)
    lt = U < 0
    assert lt.dtype == np.bool_
    h = lt.to_host()
    assert h.dtype == np.bool_ and np.array_equal(h, un < 0)
    again = A(h)                                        # pushed back: still Bool
    assert again.dtype == np.bool_ and np.array_equal((~again).to_host(), ~(un < 0))
    got = ((U < 0) * V + (U >= 0) * uinf).to_host()
    exp = np.where((un < 0)[:, None], u, np.copysign(f32(0), u)) + np.where((un >= 0)[:, None], uinf[None, :],
                                                                             np.copysign(f32(0), uinf)[None, :])
    assert same_bits(got, exp.astype(f32))
    with pytest.raises(TypeError):
        bool(lt)
    for bad in (lambda: lt + lt, lambda: lt * lt, lambda: lt.sqrt(), lambda: H.ifelse(U, U, V), lambda: ~U,
                lambda: U & lt):
        with pytest.raises(TypeError):
            bad()
    assert same_bits((lt * f32(np.nan)).to_host(), np.where(un < 0, np.nan, 0).astype(f32))
    # exact Float64 comparisons: x > 0.1 is not x > 0.1f0
    x = np.array([f32(0.1), np.nextafter(f32(0.1), f32(0)), 1e38, np.inf, -0.0, 0.0, np.nan], f32)
    X = A(x)
    for s in (0.1, 1e39, -0.0, float("nan")):
        for py, npop in ((lambda a: a > s, np.greater), (lambda a: a <= s, np.less_equal),
                         (lambda a: H.eq(a, s), np.equal), (lambda a: H.ne(a, s), np.not_equal)):
            assert np.array_equal(py(X).to_host(), npop(x.astype(np.float64), s)), s


def test_closure_with_new_opcodes_replays_in_a_graph():
    rng = np.random.default_rng(13)
    n = 10001
    T = A(rng.uniform(-20, 600, (n, 2)).astype(f32))
    out = A(np.zeros((n, 2), f32))

    def closure(T, out):
        Tc = H.clamp(T, 10.0, INF)
        out -= H.ifelse(T > 250.0, (Tc / 273.15) ** f32(2.0 / 3), H.exp(-Tc / 300.0)) + (T < 0) * T ** 2
        out += (Tc * [1.0, 2.0]).sum(dims=2) * H.log(Tc)

    ref = A(np.zeros((n, 2), f32))
    closure(T, ref)
    closure(T, ref)
    g = ibamd.GraphedClosure(closure, T, out)
    g()
    g()
    torch.cuda.synchronize()
    assert same_bits(out.to_host(), ref.to_host())

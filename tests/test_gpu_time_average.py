"""``TimeAverage.push`` (``ibh_time_average_push``, cfd.jl:738-802) and ``pressure_coefficient`` (:411-424) on the GPU,
bit for bit against the numpy restatement (tests/cfd_model.py): every dt form in both precisions, 1-D and (n, nv) fields,
tails, strided Q, the march composition of the advection script."""
import numpy as np
import pytest

import cfd_model as M
import ibamd
from ibamd import _lib
from ibamd import cfd

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64


def _bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def _dev_field(a, ld=None):
    """(n,) or (n, nv) host array -> column-major device tensor, leading dimension ld >= n."""
    import torch
    if a.ndim == 1 or ld is None:
        return ibamd.hip(a)
    n, nv = a.shape
    store = np.zeros((nv, ld), f32)
    store[:, :n] = a.T
    return torch.from_numpy(store).cuda()[:, :n].T


SHAPES = [(1, None, None), (3, None, None), (37, None, None), (63, None, None), (4099, None, None), (37, 1, None),
          (61, 5, None), (1001, 5, None), (4096, 5, None), (37, 5, 40), (1001, 5, 1024), (64, 1, 67)]


def _case_id(s):
    n, nv, ld = s
    return f"n{n}" + ("" if nv is None else f"x{nv}") + ("" if ld is None else f"_ld{ld}")


FORMS = ["host", "host_pyfloat", "host_int", "device", "per_var", "element"]


CASES = [pytest.param(s, p, f, id=f"{f}-{p}-{_case_id(s)}") for f in FORMS for p in ("Float32", "Float64") for s in SHAPES
         if not (f == "per_var" and s[1] is None)]   # a per-variable dt needs a 2-D Q


@pytest.mark.parametrize("shape,prec,form", CASES)
def test_push_bit_identical(shape, prec, form):
    """10 pushes with varying dt after the first registry, μ and σ compared as raw bits."""
    import torch
    n, nv, ld = shape
    rng = np.random.default_rng(n * 7 + (nv or 0))
    qshape = (n,) if nv is None else (n, nv)
    tau = f32(0.7) if prec == "Float32" else 0.7
    avg = cfd.TimeAverage(tau)
    Qs = [rng.standard_normal(qshape).astype(f32) * f32(3) for _ in range(11)]
    mu = sg = None
    for k, Qh in enumerate(Qs):
        Qd = _dev_field(Qh, ld)
        if k == 0:
            ret = avg.push(Qd)
            mu, sg = M.ta_first(Qh)
            assert ret is avg.mu
            continue
        if form == "host":
            dt, dt_type, dth = f32(0.03 * k), f32, f32(0.03 * k)
        elif form == "host_pyfloat":
            dt, dt_type, dth = 0.03 * k, f64, 0.03 * k
        elif form == "host_int":
            dt, dt_type, dth = 1, int, 1
            if prec == "Float32":
                avg.tau = tau = f32(7.0)
            else:
                avg.tau = tau = 7.0
        elif form == "device":
            dth = np.array([0.03 * k], f32)
            dt, dt_type = ibamd.hip(dth), f32
        elif form == "per_var":
            dth = rng.uniform(0.0, 0.5, nv).astype(f32)
            dt, dt_type = ibamd.hip(dth), f32
        else:
            dth = rng.uniform(0.0, 0.5, qshape).astype(f32)
            dt, dt_type = _dev_field(dth, ld), f32
        P = M.eta_type(tau, dt_type)
        assert P is (f32 if prec == "Float32" and form != "host_pyfloat" else f64)
        ret = avg.push(Qd, dt)
        assert ret is avg.mu
        mu, sg = M.ta_push(mu, sg, Qh, M.ta_eta(dth, tau, P), P)
    torch.cuda.synchronize()
    gm, gs = ibamd.to_host(avg.mu), ibamd.to_host(avg.sigma)
    assert gm.shape == qshape and gs.shape == qshape
    assert np.array_equal(_bits(gm), _bits(mu)), np.abs(gm - mu).max()
    assert np.array_equal(_bits(gs), _bits(sg)), np.abs(gs - sg).max()


def test_first_registry_sign_and_nan():
    Q = np.array([-1.5, 2.0, np.nan, np.inf, -np.inf, -0.0, 0.0, -3.0, 1.0], f32)
    avg = cfd.TimeAverage(f32(1))
    avg.push(ibamd.hip(Q))
    mu, sg = M.ta_first(Q)
    assert np.array_equal(_bits(ibamd.to_host(avg.mu)), _bits(mu))
    assert np.array_equal(_bits(ibamd.to_host(avg.sigma)), _bits(sg))


def test_push_returns_mu_updated_in_place():
    import torch
    rng = np.random.default_rng(3)
    Q0, Q1 = rng.standard_normal((100, 5)).astype(f32), rng.standard_normal((100, 5)).astype(f32)
    avg = cfd.TimeAverage(f32(2))
    held = avg.push(ibamd.hip(Q0))
    sigma, ptr = avg.sigma, held.data_ptr()
    again = avg.push(ibamd.hip(Q1), f32(0.5))
    assert again is held and avg.mu is held and avg.sigma is sigma and held.data_ptr() == ptr
    mu, sg = M.ta_first(Q0)
    mu, sg = M.ta_push(mu, sg, Q1, M.ta_eta(f32(0.5), f32(2), f32), f32)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(ibamd.to_host(held)), _bits(mu))
    assert np.array_equal(_bits(ibamd.to_host(sigma)), _bits(sg))


def test_push_hiparray():
    """With a HipArray, μ and σ are HipArrays; a pending broadcast that reads μ sees the value before the push."""
    rng = np.random.default_rng(4)
    Q0, Q1 = rng.standard_normal(300).astype(f32), rng.standard_normal(300).astype(f32)
    avg = cfd.TimeAverage(f32(2))
    mu_h = avg.push(ibamd.HipArray(Q0))
    assert isinstance(mu_h, ibamd.HipArray) and mu_h is avg.mu
    before = mu_h * 1.0                      # pending: evaluated before the push writes μ
    assert avg.push(ibamd.HipArray(Q1), f32(1)) is mu_h
    mu, sg = M.ta_first(Q0)
    mu, sg = M.ta_push(mu, sg, Q1, M.ta_eta(f32(1), f32(2), f32), f32)
    assert np.array_equal(_bits(before.to_host()), _bits(Q0))
    assert np.array_equal(_bits(mu_h.to_host()), _bits(mu))
    assert np.array_equal(_bits(avg.sigma.to_host()), _bits(sg))


def test_invalid_dt_raises_before_any_launch():
    import torch
    n, nv = 10, 3
    rng = np.random.default_rng(5)
    Q = ibamd.hip(rng.standard_normal((n, nv)).astype(f32))
    avg = cfd.TimeAverage(f32(2))
    avg.push(Q)
    mu0, sg0 = ibamd.to_host(avg.mu), ibamd.to_host(avg.sigma)
    bad = [ibamd.hip(np.ones(n, f32)),           # length n with a 2-D Q, n != nv: the reshape puts it along nv
           ibamd.hip(np.ones(2, f32)),
           ibamd.hip(np.ones((n, 1), f32)),
           ibamd.hip(np.ones((nv, n), f32))]
    for dt in bad:
        with pytest.raises(ValueError):
            avg.push(Q, dt)
    with pytest.raises(TypeError):
        avg.push(Q, np.ones(nv, f32))                    # host array
    with pytest.raises(TypeError):
        avg.push(Q, torch.ones(nv))                      # host tensor
    with pytest.raises(TypeError):
        avg.push(Q, ibamd.hip(np.ones(nv, f32)).double())
    with pytest.raises(ValueError):
        avg.push(ibamd.hip(np.ones((n, nv + 1), f32)), f32(1))   # Q changed shape
    v = cfd.TimeAverage(f32(2))
    v.push(ibamd.hip(np.ones(n, f32)))
    for dt in (ibamd.hip(np.ones(n + 1, f32)), ibamd.hip(np.ones((n, 1), f32))):   # a 1-D Q: one element or n
        with pytest.raises(ValueError):
            v.push(ibamd.hip(np.ones(n, f32)), dt)
    one = ibamd.hip(np.ones(nv, f32))
    with pytest.raises(_lib.IbhError):                   # the C entry checks the sizes itself
        _lib.call("ibh_time_average_push", n, nv, _lib.c_vp(Q.data_ptr()), n, _lib.c_vp(avg.mu.data_ptr()),
                  _lib.c_vp(avg.sigma.data_ptr()), 2, _lib.c_vp(one.data_ptr()), nv - 1, nv, 0.0, 2.0, 0)
    with pytest.raises(_lib.IbhError):
        _lib.call("ibh_time_average_push", n, nv, _lib.c_vp(Q.data_ptr()), n, _lib.c_vp(avg.mu.data_ptr()),
                  _lib.c_vp(avg.sigma.data_ptr()), 3, _lib.c_vp(one.data_ptr()), nv, n, 0.0, 2.0, 0)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(ibamd.to_host(avg.mu)), _bits(mu0))
    assert np.array_equal(_bits(ibamd.to_host(avg.sigma)), _bits(sg0))


def test_march_composition_advection_script():
    """test/advection.jl's loop (device dt every step, sweep + update, the BC set) for 200 steps with ``push(u, dt)``
    after each step on the device dt; the host copies of u and dt feed the restatement.  Float32 and Float64 τ."""
    import torch
    from conftest import ADV_FAMILIES, advection_mesh
    msh = advection_mesh()
    dp = ibamd.Domain(msh, hypercube_families=ADV_FAMILIES, max_partition_size=10 ** 9)
    (part,) = dp.partitions.values()
    dpart = ibamd.to_backend(part, ibamd.hip)
    n = len(dp)
    C = ibamd.hip(np.ones((n, 2), f32))
    bcs = ibamd.BCSet(dp, [("upper", 1.0), ("lower", 0.0), ("outlet", "copy")])
    ua, ub = ibamd.hip(np.zeros(n, f32)), torch.empty(n, dtype=torch.float32, device="cuda")
    dt = ibamd.timestep_advection(dpart, C, scale=0.75)
    a32, a64 = cfd.TimeAverage(f32(0.05)), cfd.TimeAverage(0.05)
    h32 = h64 = None
    for _ in range(200):
        ibamd.timestep_advection(dpart, C, scale=0.75, out=dt)
        ibamd.step_advection(dpart, ua, C, dt, bcs, out=ub)
        ua, ub = ub, ua
        a32.push(ua, dt)
        a64.push(ua, dt)
        u, dth = ibamd.to_host(ua), ibamd.to_host(dt)
        if h32 is None:
            h32, h64 = M.ta_first(u), M.ta_first(u)
        else:
            h32 = M.ta_push(*h32, u, M.ta_eta(dth[0], f32(0.05), f32), f32)
            h64 = M.ta_push(*h64, u, M.ta_eta(dth[0], 0.05, f64), f64)
    assert bcs.healthy()
    assert float(h32[1].max()) > 0.01                    # the average moved
    for avg, h in ((a32, h32), (a64, h64)):
        assert np.array_equal(_bits(ibamd.to_host(avg.mu)), _bits(h[0]))
        assert np.array_equal(_bits(ibamd.to_host(avg.sigma)), _bits(h[1]))
    assert not np.array_equal(_bits(h32[0]), _bits(h64[0]))   # the two precisions are distinguishable here


@pytest.mark.parametrize("nv", [None, 4])
def test_pressure_coefficient_bit_identical(nv):
    rng = np.random.default_rng(6)
    p = rng.uniform(5e4, 1.5e5, (777,) if nv is None else (777, nv)).astype(f32)
    fluid = cfd.Fluid()
    p_inf, M_inf = f32(101325.0), f32(0.7)
    got = ibamd.to_host(cfd.pressure_coefficient(fluid, ibamd.hip(p), p_inf, M_inf))
    exp = M.pressure_coefficient(f32(fluid.gamma), p, p_inf, M_inf)
    assert got.shape == p.shape
    assert np.array_equal(_bits(got), _bits(exp))
    h = cfd.pressure_coefficient(fluid, ibamd.HipArray(p), p_inf, M_inf)
    assert isinstance(h, ibamd.HipArray) and np.array_equal(_bits(h.to_host()), _bits(exp))

"""``(dom::Domain)(f, args...)`` (ImmersedBoundary.jl:820-864) on device-resident global arrays: no converters, every
argument a device array -> one gather launch, the closure per partition on workspace views, one scatter launch
(csrc/ibh_domain.hip).  Compared bit for bit with the host path (the same closures through ``conv_to_backend=hip``),
which runs the same kernels on the same local layouts."""
import numpy as np
import pytest
import torch

import ibamd
from conftest import euler_field, rel_inf, seeded_field
from oracle import domain as od

pytestmark = pytest.mark.gpu
f32 = np.float32
HOST = dict(conv_to_backend=ibamd.hip, conv_from_backend=ibamd.to_host)
HOST_H = dict(conv_to_backend=ibamd.HipArray, conv_from_backend=ibamd.to_host)


def _bits_equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def adv_closure(part, u, ud, Cl):
    """test/advection.jl:67-83 at operator granularity (torch arrays); returns max(D), a device scalar of the inputs
    alone (``ud`` is updated in place, so its skirt rows -- unlike its image rows -- depend on the partition order)."""
    D = ibamd.JST_sensor(part, u)
    for dim in (1, 2):
        Cf = ibamd.at_faces(part, Cl[:, dim - 1].contiguous(), dim)
        gu = ibamd.cell_gradient(part, u, dim)
        uL, uR = ibamd.MUSCL(part, u, gu, dim, D=D, high_order=True)
        ud -= ibamd.green_gauss(part, (uL + uR) * Cf / 2 + torch.abs(Cf) * (uL - uR) / 2, dim)
    return torch.max(D)


def adv_closure_h(part, u, ud, C):
    """The same lines on HipArrays (every operator between them an ibh_ew_* broadcast)."""
    D = ibamd.JST_sensor(part, u)
    for dim in (1, 2):
        Cf = ibamd.at_faces(part, C.col(dim), dim)
        gu = ibamd.cell_gradient(part, u, dim)
        uL, uR = ibamd.MUSCL(part, u, gu, dim, D=D, high_order=True)
        ud -= ibamd.green_gauss(part, (uL + uR) * Cf / 2 + abs(Cf) * (uL - uR) / 2, dim)
    assert isinstance(ud, ibamd.HipArray)
    return D.maximum()


def o_adv_closure(part, u, ud, Cl):
    D = od.JST_sensor(part, u)
    for dim in (1, 2):
        Cf = od.at_faces(part, np.ascontiguousarray(Cl[:, dim - 1]), dim)
        gu = od.cell_gradient(part, u, dim)
        uL, uR = od.MUSCL(part, u, gu, dim, D=D, high_order=True)
        ud -= od.green_gauss(part, (uL + uR) * Cf / f32(2) + np.abs(Cf) * (uL - uR) / f32(2), dim)


def _host_and_device(dom, f, arrays, hiparray=False):
    """The call through the host path and on device arrays; returns (host arrays, results) of both."""
    hs = [a.copy() for a in arrays]
    rh = dom(f, *hs, **(HOST_H if hiparray else HOST))
    ds = [ibamd.HipArray(a) if hiparray else ibamd.hip(a) for a in arrays]
    rd = dom(f, *ds)
    return (hs, rh), ([ibamd.to_host(d) for d in ds], rd)


def _scalar(r):
    return np.float32(float(r))


@pytest.mark.parametrize("hiparray", [False, True])
def test_advection_closure_bitwise_and_oracle(adv_domains, hiparray):
    dp, do = adv_domains
    assert len(dp.partitions) == 3
    n = len(dp)
    u = seeded_field(dp.global_centers(), kind="step")
    C = np.ones((n, 2), f32)
    C[:, 1] = f32(0.5)
    (hs, rh), (ds, rd) = _host_and_device(dp, adv_closure_h if hiparray else adv_closure,
                                          [u, np.zeros(n, f32), C], hiparray)
    for h, d in zip(hs, ds):
        assert _bits_equal(d, h)
    assert len(rd) == len(rh) == 3 and all(_bits_equal(_scalar(a), _scalar(b)) for a, b in zip(rd, rh))
    assert np.array_equal(ds[0], u) and np.abs(ds[1]).max() > 0
    uo, udo = u.copy(), np.zeros(n, f32)
    do(o_adv_closure, uo, udo, C)
    assert rel_inf(ds[1], udo) <= 1e-5


def test_euler_residual_bitwise(rae_domains):
    dp, _ = rae_domains
    assert len(dp.partitions) > 1
    P = euler_field(dp.global_centers())

    def f(part, P, R):
        ibamd.residual_euler_hll(part, P, out=R)

    (hs, _), (ds, _) = _host_and_device(dp, f, [P, np.zeros_like(P)])
    assert _bits_equal(ds[1], hs[1]) and np.abs(ds[1]).max() > 0
    assert _bits_equal(ds[0], P)


def test_fused_sweep_3d_skirted_partitions_bitwise():
    from ibamd.mesher import Ball, Mesh
    msh = Mesh(f32([-2, -2, -2]), f32([4, 4, 4]), block_size=4,
               refinement_regions=[(Ball(np.array([0.6, 0.6, 0.6]), 0.1), f32(0.2))])
    dp = ibamd.Domain(msh, hypercube_families=[("farfield", [(1, False), (1, True)])], max_partition_size=8192,
                      boundaries=False)
    assert dp.ndims == 3 and len(dp.partitions) == 2
    n = len(dp)
    X = dp.global_centers()
    u = (np.sin(2 * X[:, 0]) * np.cos(X[:, 1]) + 0.3 * X[:, 2]).astype(f32)
    C = np.ones((n, 3), f32)

    def f(part, u, ud, C):
        ibamd.residual_advection(part, u, C, out=ud)

    (hs, _), (ds, _) = _host_and_device(dp, f, [u, np.zeros(n, f32), C])
    assert _bits_equal(ds[1], hs[1]) and np.abs(ds[1]).max() > 0


def test_full_size_rae2822_default_partitions_bitwise():
    import bench
    msh = bench.build_mesh("rae2822_0.87M")
    dp = ibamd.Domain(msh, boundaries=False)          # the reference default, max_partition_size = 100_000
    assert len(dp) == 867904 and len(dp.partitions) == 9
    P = euler_field(dp.global_centers())

    def f(part, P, R):
        ibamd.residual_euler_hll(part, P, out=R)
        return part.nc

    (hs, rh), (ds, rd) = _host_and_device(dp, f, [P, np.zeros_like(P)])
    assert rd == rh == [dp.partitions[i].domain.size for i in dp.partitions]
    assert _bits_equal(ds[1], hs[1]) and np.abs(ds[1]).max() > 0


def test_advection_script_200_steps_resident(adv_domains):
    """test/advection.jl:30-93 for 200 steps on 3 partitions: u stays on the device (domain call + impose_bc on device
    arrays); dt from the zero-argument call with converters.  The same loop through the host path: same bits."""
    dp, _ = adv_domains
    n = len(dp)
    C = np.ones((n, 2), f32)

    def g_dt(part):
        one = torch.ones(part.nc, dtype=torch.float32, device=part.spacing.device)
        a = ibamd.unsigned_green_gauss(part, ibamd.at_faces(part, one, 1), 1)
        b = ibamd.unsigned_green_gauss(part, ibamd.at_faces(part, one, 2), 2)
        return f32(0.5) / float(torch.maximum(a, b).max())

    dt = min(dp(g_dt, **HOST)) * f32(0.75)

    def bcs(u, **kw):
        ibamd.impose_bc(lambda b, ui: 1.0, dp, "upper", u, **kw)
        ibamd.impose_bc(lambda b, ui: 0.0, dp, "lower", u, **kw)
        ibamd.impose_bc(lambda b, ui: ui.clone(), dp, "outlet", u, **kw)

    uh = np.zeros(n, f32)
    ud_dev, C_dev = ibamd.hip(uh), ibamd.hip(C)
    u_dev = ibamd.hip(uh)
    for _ in range(200):
        rh = np.zeros(n, f32)
        dp(adv_closure, uh, rh, C, **HOST)
        uh += rh * dt
        bcs(uh, **HOST)
        ud_dev.zero_()
        dp(adv_closure, u_dev, ud_dev, C_dev)
        u_dev += ud_dev * float(dt)
        bcs(u_dev)
    ug = ibamd.to_host(u_dev)
    assert _bits_equal(ug, uh)
    assert ug.max() > 0.5 and np.isfinite(ug).all()


def test_fas_with_device_domain_call(adv_mesh_coarse):
    """Solver.FAS! whose residual closure is a domain call on every level of a partitioned multigrid hierarchy:
    device arrays straight through the call vs a closure that round-trips through the host path."""
    fam = [("neumann", [(1, True), (2, True)])]
    dp = ibamd.Domain(adv_mesh_coarse, hypercube_families=fam, max_partition_size=512, boundaries=False)
    cds, prol, coar = ibamd.multigrid(dp, max_levels=2)
    levels = [dp] + cds
    assert len(dp.partitions) > 1 and len(cds[0].partitions) > 1

    def lap(part, Q, r):
        for dim in (1, 2):
            r += ibamd.green_gauss(part, ibamd.face_gradient(part, Q, dim), dim)

    omega = [f32(0.2) * f32(d.partitions[1].spacing[:, 0].min()) ** 2 for d in levels]

    def f_dev(l, Q):
        r = ibamd.colmajor_empty(Q.shape[0], Q.shape[1])
        r.zero_()
        levels[l](lap, Q, r)
        return r, omega[l]

    def f_host(l, Q):
        Qh, rh = ibamd.to_host(Q), np.zeros(tuple(Q.shape), f32)
        levels[l](lap, Qh, rh, **HOST)
        return ibamd.hip(rh), omega[l]

    Q0 = seeded_field(dp.global_centers(), nv=2)
    Qd, Qh = ibamd.hip(Q0), ibamd.hip(Q0)
    rd = ibamd.FAS(f_dev, Qd, coarseners=coar, prolongators=prol, n_iter=4, rtol=0.0, atol=0.0)
    rh = ibamd.FAS(f_host, Qh, coarseners=coar, prolongators=prol, n_iter=4, rtol=0.0, atol=0.0)
    assert _bits_equal(ibamd.to_host(Qd), ibamd.to_host(Qh))
    assert abs(rd - rh) <= 1e-9 * rh and not np.array_equal(ibamd.to_host(Qd), Q0)   # (norms: atomic sum order)


def test_snapshot_semantics_in_place_stencil(adv_domains):
    """An in-place closure that reads neighbours: every partition reads the arguments as they were before the call."""
    dp, _ = adv_domains
    u0 = seeded_field(dp.global_centers())

    def smooth(part, u):   # u <- (u_W + 2 u + u_E) / 4 on a uniform patch: a neighbour average
        g = ibamd.unsigned_green_gauss(part, ibamd.at_faces(part, u, 1), 1) * part.spacing[:, 0] / 2
        u.copy_(g)

    ud = ibamd.hip(u0)
    dp(smooth, ud)
    got = ibamd.to_host(ud)
    # numpy restatement: gather every partition from the snapshot, run the closure, then write back
    exp = u0.copy()
    for i in dp.partitions:
        part = dp.partitions[i]
        loc = ibamd.hip(np.array(u0[part.domain]))
        smooth(ibamd.to_backend(part, ibamd.hip), loc)
        exp[part.image] = ibamd.to_host(loc)[part.image_in_domain]
    assert _bits_equal(got, exp)
    seq = u0.copy()
    dp(smooth, seq, **HOST)      # the sequential host path: later partitions read earlier partitions' writes
    assert not np.array_equal(seq, exp)


def test_graphed_domain_call_replays_bitwise(adv_domains):
    dp, _ = adv_domains
    n = len(dp)
    u = ibamd.hip(seeded_field(dp.global_centers(), kind="step"))
    ud = ibamd.colmajor_empty(n)
    ud.zero_()
    C = ibamd.hip(np.ones((n, 2), f32))

    def call(u, ud, C):
        dp(adv_closure, u, ud, C)

    u_before = ibamd.to_host(u)
    g = ibamd.GraphedClosure(call, u, ud, C)
    assert _bits_equal(ibamd.to_host(u), u_before) and not ibamd.to_host(ud).any()
    call(u, ud, C)
    eager = ibamd.to_host(ud)
    ud.zero_()
    g()
    assert _bits_equal(ibamd.to_host(ud), eager) and np.abs(eager).max() > 0
    assert _bits_equal(ibamd.to_host(u), u_before)


def test_invalid_arguments_raise_before_any_launch(adv_domains):
    dp, _ = adv_domains
    n = len(dp)
    called = []

    def f(part, *args):
        called.append(part)
        for a in args:
            if isinstance(a, torch.Tensor) and a.dtype == torch.float32:
                a.fill_(7.0)

    good = ibamd.hip(seeded_field(dp.global_centers()))
    before = ibamd.to_host(good)
    bad_cases = [
        (ValueError, ibamd.hip(np.zeros(n - 1, f32))),                               # row count
        (ValueError, ibamd.HipArray(np.zeros(n + 1, f32))),
        (TypeError, torch.zeros(n, dtype=torch.float64, device=good.device)),         # Float64
        (TypeError, torch.zeros((n, 2), dtype=torch.float32, device=good.device)),    # row-major (n, 2)
        (TypeError, np.zeros(n, f32)),                                                # host array, no converters
    ]
    for exc, bad in bad_cases:
        with pytest.raises(exc):
            dp(f, good, bad)
        assert not called
        assert _bits_equal(ibamd.to_host(good), before)
        if isinstance(bad, torch.Tensor) and bad.dtype == torch.float32:
            assert not bad.any()

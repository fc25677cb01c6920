"""CFD utilities without a device: the restatement of ``TimeAverage`` (tests/cfd_model.py) by hand-computed answers, and
the host-scalar free-stream utilities of ``ibamd.cfd`` (``ISA_atmosphere``, ``streamwise_direction``,
``Reynolds_number``, ``adjust_Reynolds``: cfd.jl:302-436, 619-654) against the standard atmosphere and the restatement."""
import warnings

import numpy as np
import pytest

import cfd_model as M
from ibamd import cfd

f32, f64 = np.float32, np.float64


def _bits(a):
    return np.asarray(a, dtype=f32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------- TimeAverage
@pytest.mark.parametrize("tau", [f32(4.0), 4.0], ids=["Float32", "Float64"])
def test_time_average_three_pushes_by_hand(tau):
    """τ = 4; Q = 2, 6 (dt = 1: η = 1/4), -1 (dt = 2: η = 1/2) -- every value exact in both precisions:
    σ = sqrt(0 * 3/4 + 16 / 4) = 2, μ = 2 * 3/4 + 6 / 4 = 3, then σ = sqrt(4 / 2 + 16 / 2) = sqrt(10), μ = 3/2 - 1/2 = 1."""
    avg = cfd.TimeAverage(tau)
    assert avg.tau == tau and avg.mu is None and avg.sigma is None
    P = M.eta_type(tau, f32)
    assert P is (f32 if isinstance(tau, f32) else f64)
    mu, sg = M.ta_first(np.array([2.0], f32))
    assert mu[0] == 2 and sg[0] == 0 and not np.signbit(sg[0])
    mu, sg = M.ta_push(mu, sg, np.array([6.0], f32), M.ta_eta(f32(1), tau, P), P)
    assert mu[0] == 3 and sg[0] == 2
    mu, sg = M.ta_push(mu, sg, np.array([-1.0], f32), M.ta_eta(f32(2), tau, P), P)
    assert mu[0] == 1 and sg[0] == f32(np.sqrt(10.0))
    assert mu.dtype == f32 and sg.dtype == f32


def test_time_average_precision_by_hand():
    """τ = 3, dt = 1, Q = 1 then 0: μ = 1 - η.  Float32: η = f32(1/3) = 0x3eaaaaab and 1 - η = 0x3f2aaaaa exactly;
    Float64: 1 - 1/3 rounds to f32(2/3) = 0x3f2aaaab.  σ = sqrt(η): 0x3f13cd3a in both."""
    for tau, mu_bits in ((f32(3.0), 0x3F2AAAAA), (3.0, 0x3F2AAAAB), (3, 0x3F2AAAAB)):
        P = M.eta_type(tau, type(1))
        assert cfd.TimeAverage(tau).sigma is None
        mu, sg = M.ta_first(np.array([1.0], f32))
        mu, sg = M.ta_push(mu, sg, np.array([0.0], f32), M.ta_eta(1, tau, P), P)
        assert _bits(mu)[0] == mu_bits, (tau, hex(_bits(mu)[0]))
        assert _bits(sg)[0] == 0x3F13CD3A, (tau, hex(_bits(sg)[0]))


def test_time_average_first_registry_keeps_sign_and_nan():
    """``σ = μ .* 0``, not ``fill(0)``: -0.0 where Q < 0, NaN where Q is NaN or ±Inf."""
    assert cfd.TimeAverage(f32(1)).mu is None
    Q = np.array([-1.5, 2.0, np.nan, np.inf, -np.inf, -0.0, 0.0], f32)
    mu, sg = M.ta_first(Q)
    assert np.array_equal(_bits(mu), _bits(Q))
    assert np.signbit(sg[0]) and sg[0] == 0 and not np.signbit(sg[1]) and sg[1] == 0
    assert np.isnan(sg[2:5]).all()
    assert np.signbit(sg[5]) and not np.signbit(sg[6])


# ----------------------------------------------------------------------------------------------------- ISA_atmosphere
TABLE = [(0.0, 288.15, 101325.0), (11000.0, 216.65, 22632.0), (20000.0, 216.65, 5474.9), (32000.0, 228.65, 868.02),
         (47000.0, 270.65, 110.91), (51000.0, 270.65, 66.939)]


@pytest.mark.parametrize("h,T,p", TABLE)
def test_isa_layer_bases(h, T, p):
    fluid, P = cfd.ISA_atmosphere(h)
    assert isinstance(fluid, cfd.Fluid) and P.shape == (3,)
    assert abs(P[0] - p) <= 1e-4 * p and abs(P[1] - T) <= 1e-4 * T
    assert P[2] == 0                                     # Mach = 0
    ep, eT = M.isa(h)
    assert np.isclose(P[0], ep, rtol=1e-6) and np.isclose(P[1], eT, rtol=1e-6)


@pytest.mark.parametrize("h", [b[0] for b in TABLE[1:]])
def test_isa_continuous_across_layer_bases(h):
    """From below (the layer under the base) and from above, within the 5 digits of the table's pressures."""
    for d in (1e-3, 0.5):
        (lo, hi) = (cfd.ISA_atmosphere(h - d)[1], cfd.ISA_atmosphere(h + d)[1])
        base = cfd.ISA_atmosphere(h)[1]
        for side in (lo, hi):
            assert abs(side[0] - base[0]) <= 1e-3 * base[0], (h, d, side, base)
            assert abs(side[1] - base[1]) <= 1e-3 * base[1], (h, d, side, base)


def test_isa_75km_uses_the_51km_layer():
    """The reference's loop `1:length(layers)-1` never selects the 71 km layer."""
    _, P = cfd.ISA_atmosphere(75000.0)
    T51 = 270.65 - 2.8e-3 * (75000 - 51000)
    assert abs(P[1] - T51) <= 1e-4 * T51
    assert abs(P[1] - (214.65 - 2.0e-3 * 4000)) > 1.0
    ep, eT = M.isa(75000.0)
    assert np.isclose(P[0], ep, rtol=1e-6) and np.isclose(P[1], eT, rtol=1e-6)


def test_isa_negative_altitude_raises_and_high_altitude_warns():
    with pytest.raises(ValueError):
        cfd.ISA_atmosphere(-1.0)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        cfd.ISA_atmosphere(90000.0)
    assert any("86 km" in str(x.message) for x in w)


def test_isa_mach_velocity_and_direction():
    """u = Mach * a(T) with Fluid()'s R = 283 (not the ISA's 287.05287); V overrides Mach; û normalised with eps."""
    _, P = cfd.ISA_atmosphere(0.0, Mach=f32(0.5), u_hat=(f32(3.0), f32(4.0)))
    a = M.speed_of_sound(f32(288.15))
    assert P.shape == (4,)
    norm = f32(np.finfo(f32).eps) + f32(5.0)
    assert np.isclose(P[2], f32(0.5) * a * (f32(3.0) / norm), rtol=1e-6)
    assert np.isclose(P[3], f32(0.5) * a * (f32(4.0) / norm), rtol=1e-6)
    assert abs(a - np.sqrt(1.4 * 287.05287 * 288.15)) > 1.0                   # it is R = 283
    _, P = cfd.ISA_atmosphere(1000.0, Mach=f32(0.5), V=f32(10.0))
    assert np.isclose(P[2], 10.0, rtol=1e-6)
    _, P = cfd.ISA_atmosphere(0.0, dT=f32(10.0))
    assert np.isclose(P[1], 298.15, rtol=1e-6) and np.isclose(P[0], 101325.0, rtol=1e-6)


# ------------------------------------------------------------------------------------- streamwise_direction, Reynolds
def test_streamwise_direction():
    assert np.array_equal(cfd.streamwise_direction(0), [1.0, 0.0])
    assert np.allclose(cfd.streamwise_direction(90, 0), [0.0, 0.0, 1.0], atol=1e-12)
    d = cfd.streamwise_direction(30.0, 45.0)
    c = np.cos(np.radians(30.0))
    assert np.allclose(d, [c * np.cos(np.radians(45.0)), -c * np.sin(np.radians(45.0)), 0.5], rtol=1e-12)
    assert cfd.streamwise_direction(f32(10)).dtype == f32


def test_reynolds_number_and_adjust():
    f = cfd.Fluid()
    _, P = cfd.ISA_atmosphere(0.0, Mach=f32(0.3))
    Re = cfd.Reynolds_number(f, P, f32(1.0))
    assert np.isclose(Re, M.reynolds(P, f32(1.0)), rtol=1e-6)
    g = cfd.adjust_Reynolds(f, P, f32(1.0), 1e6)
    assert isinstance(g, cfd.Fluid) and g is not f and f.mu_ref == cfd.Fluid().mu_ref
    assert (g.R, g.gamma, g.k, g.Tref, g.S) == (f.R, f.gamma, f.k, f.Tref, f.S)
    assert abs(cfd.Reynolds_number(g, P, f32(1.0)) - 1e6) <= 1e-5 * 1e6

"""numpy restatement of the reference's CFD utilities that the port adds: ``TimeAverage`` (cfd.jl:738-802),
``pressure_coefficient`` (:411-424), ``ISA_atmosphere`` (:302-397), ``streamwise_direction`` (:399-436),
``Reynolds_number`` / ``adjust_Reynolds`` (:619-654).

Test infrastructure: written line by line from cfd.jl with Julia's promotions made explicit (``astype`` / the numpy
scalar type of every constant); it does not import the product.  Julia types map to numpy as Float32 -> np.float32,
Float64 (and a Python float, like a Julia literal ``1.0``) -> np.float64, Int -> Python int.
"""
import math
import warnings

import numpy as np

f32, f64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------------- TimeAverage
def jl_type(x):
    """Julia type of a host scalar: f32, f64 or int."""
    if isinstance(x, (bool, int, np.integer)):
        return int
    if isinstance(x, np.float32):
        return f32
    if isinstance(x, (float, np.float64)):
        return f64
    raise TypeError(type(x))


def eta_type(tau, dt_type):
    """typeof(dt / τ): Int / Int is Float64, otherwise the wider float."""
    a, b = jl_type(tau), dt_type
    if a is int and b is int:
        return f64
    return f64 if f64 in (a, b) else f32


def ta_first(Q):
    """cfd.jl:778-783: ``μ = copy(Q); σ = μ .* 0`` (Float32 * Int -> Float32: -0.0 for Q < 0, NaN for NaN / Inf)."""
    mu = np.array(Q, dtype=f32, copy=True)
    with np.errstate(invalid="ignore"):
        sigma = mu * f32(0)
    return mu, sigma


def ta_eta(dt, tau, P):
    """``η = @. dt / τ`` in the promoted type P (dt a host scalar or a Float32 array).  A 1-D dt with a 2-D Q lies along
    Q's last axis (cfd.jl:785-789): numpy broadcasting of an (nv,) array against (n, nv) does exactly that."""
    return np.asarray(dt).astype(P) / P(tau)


def ta_push(mu, sigma, Q, eta, P):
    """cfd.jl:791-797 (σ from the OLD μ): ``σ^2``, ``μ - Q``, ``(μ - Q)^2`` are Float32 ⊗ Float32; ``1.0f0 - η`` and every
    product with η are in P; the sums (and the sqrt) in P, rounded to Float32 by the in-place store."""
    one_m_eta = P(1.0) - eta
    s2 = sigma * sigma
    d = mu - Q
    d2 = d * d
    sigma_new = np.sqrt(s2.astype(P) * one_m_eta + d2.astype(P) * eta).astype(f32)
    mu_new = (mu.astype(P) * one_m_eta + Q.astype(P) * eta).astype(f32)
    return mu_new, sigma_new


# ------------------------------------------------------------------------------------------------ pressure_coefficient
def pressure_coefficient(gamma, p, p_inf, M_inf):
    """``@. 2 * (p / p∞ - 1.0f0) / (M∞ ^ 2 * γ)`` with Float32 scalars."""
    M, g, pinf = f32(M_inf), f32(gamma), f32(p_inf)
    s = (M * M) * g
    return (f32(2) * (p / pinf - f32(1.0))) / s


# ------------------------------------------------------------------------------------------------------ ISA atmosphere
ISA_LAYERS = [
    (f32(0.0), f32(288.15), f32(-6.5), f32(101325.0)),
    (f32(11000.0), f32(216.65), f32(0.0), f32(22632.0)),
    (f32(20000.0), f32(216.65), f32(1.0), f32(5474.9)),
    (f32(32000.0), f32(228.65), f32(2.8), f32(868.02)),
    (f32(47000.0), f32(270.65), f32(0.0), f32(110.91)),
    (f32(51000.0), f32(270.65), f32(-2.8), f32(66.939)),
    (f32(71000.0), f32(214.65), f32(-2.0), f32(3.9564)),
]


def isa(altitude_m, dT=f32(0.0)):
    """_ISA_atmosphere (cfd.jl:304-368) -> (P, T)."""
    R, g0 = f32(287.05287), f32(9.80665)
    if altitude_m < 0:
        raise ValueError("Altitude cannot be negative")
    if altitude_m > 86000:
        warnings.warn("Altitude above 86 km - model accuracy decreases")
    idx = 0
    for i in range(len(ISA_LAYERS) - 1):          # 1:length(layers)-1
        if altitude_m >= ISA_LAYERS[i][0]:
            idx = i
    h_base, T_base, lapse, P_base = ISA_LAYERS[idx]
    lapse_m = lapse / f32(1000.0)
    dh = altitude_m - h_base
    T = T_base + lapse_m * dh + dT
    if abs(lapse_m) < f32(1e-10):
        P = P_base * np.exp(-g0 * dh / (R * (T_base + dT)))
    else:
        expo = -g0 / (R * lapse_m)
        Tb = T_base + dT
        P = P_base * ((Tb + lapse_m * dh) / Tb) ** expo
    return P, T


def speed_of_sound(T, R=f32(283.0), gamma=f32(1.4)):
    """cfd.jl:62-64 with Fluid()'s defaults."""
    return np.sqrt(gamma * R * np.clip(T, f32(10.0), f32(np.inf)))


def dynamic_viscosity(T, mu_ref=f32(1.716e-5), Tref=f32(273.15), S=f32(110.4)):
    """cfd.jl:71-77, the reference's exponent 2/3 included."""
    T = np.clip(T, f32(10.0), f32(np.inf))
    return mu_ref * ((T / Tref) ** (f32(2.0) / 3)) * (Tref + S) / (T + S)


def reynolds(P, Lref, R=f32(283.0), mu_ref=f32(1.716e-5)):
    """cfd.jl:626-638."""
    P = np.asarray(P)
    V = math.sqrt(float(np.sum(P[2:].astype(f64) ** 2)))
    rho = P[0] / (R * P[1])
    return V * Lref * rho / dynamic_viscosity(P[1], mu_ref=mu_ref)

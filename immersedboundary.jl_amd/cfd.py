"""``CFD`` pointwise physics on device arrays (mirror of /root/reference/src/cfd.jl for the functions residual
closures call): ``Fluid``, ``speed_of_sound``, ``dynamic_viscosity``, ``heat_conductivity``,
``primitive2state``, ``state2primitive``, ``inviscid_fluxes`` (HLL and sensor/Rusanov methods),
``viscous_fluxes``, ``pressure_coefficient`` and ``TimeAverage``.  Same names and argument order; ``dim`` is the
1-based Cartesian direction (the matrix-normal form of the reference is a curvilinear extension outside this hot path).
Arithmetic runs in libibhip kernels (csrc/ibh_cfd.hip, csrc/ibh_stats.hip); device arrays only.

The free-stream utilities ``ISA_atmosphere``, ``streamwise_direction``, ``Reynolds_number`` and ``adjust_Reynolds``
(cfd.jl:302-436, 619-654) are host scalars: numpy, no device.
"""
from __future__ import annotations

import ctypes as C
import math
import numbers
import warnings

import numpy as np
import torch

from . import _lib
from . import backend as B
from ._header import constants


class Fluid:
    """cfd.jl:14-53 (defaults = air, Float32)."""

    def __init__(self, R=283.0, gamma=1.4, k=(0.00646, 6.468e-5), mu_ref=1.716e-5, Tref=273.15, S=110.4):
        self.R, self.gamma = float(R), float(gamma)
        self.k = [float(k)] if np.isscalar(k) else [float(x) for x in k]
        if len(self.k) > 4:
            raise ValueError("at most 4 heat-conductivity coefficients are supported")
        self.mu_ref, self.Tref, self.S = float(mu_ref), float(Tref), float(S)

    def _c(self):
        kk = (C.c_float * 4)(*(self.k + [0.0] * (4 - len(self.k))))
        return _lib.ibh_fluid(self.R, self.gamma, self.mu_ref, self.Tref, self.S, len(self.k), kk)


def _pointwise(name, fld, T):
    T, nv, _ = B._field(T)
    flat = T if T.ndim == 1 else T.T.contiguous().T
    out = B._like(flat, flat.shape[0])
    f = fld._c()
    B._stream()
    B.call(name, C.byref(f), int(flat.numel()), B._ptr(flat), B._ptr(out))
    return out


def speed_of_sound(fld, T):
    """cfd.jl:62-64"""
    return _pointwise("ibh_cfd_speed_of_sound", fld, T)


def dynamic_viscosity(fld, T):
    """cfd.jl:71-77"""
    return _pointwise("ibh_cfd_dynamic_viscosity", fld, T)


def JST_sensor(Pim1, Pi, Pip1):
    """``CFD.JST_sensor(Pim1, Pi, Pip1)`` (cfd.jl:563-573): the three-point form, elementwise."""
    a, _, _ = B._field(Pim1)
    b, _, _ = B._field(Pi)
    c, _, _ = B._field(Pip1)
    if not (a.shape == b.shape == c.shape):
        raise ValueError("JST_sensor: the three arrays must have one shape")
    a, b, c = (x if x.ndim == 1 or x.stride(1) == x.shape[0] else x.T.contiguous().T for x in (a, b, c))
    out = B._like(a, a.shape[0])
    B._stream()
    B.call("ibh_cfd_jst_sensor3", int(a.numel()), B._ptr(a), B._ptr(b), B._ptr(c), B._ptr(out))
    return out


def shock_sensor(velocity_gradients):
    """``CFD.shock_sensor`` (cfd.jl:575-617): ``velocity_gradients[i][j]`` = device array of d u_i / d x_j."""
    nd = len(velocity_gradients)
    arrs = [B._field(velocity_gradients[i][j])[0] for i in range(nd) for j in range(nd)]
    n = arrs[0].shape[0]
    if any(a.ndim != 1 or a.shape[0] != n for a in arrs):
        raise ValueError("shock_sensor: gradients are vectors of one length")
    ptrs = (B.c_vp * (nd * nd))(*[a.data_ptr() for a in arrs])
    out = B.colmajor_empty(n)
    B._stream()
    B.call("ibh_cfd_shock_sensor", nd, n, ptrs, B._ptr(out))
    return out


def heat_conductivity(fld, T):
    """cfd.jl:84-90"""
    return _pointwise("ibh_cfd_heat_conductivity", fld, T)


def _nd(P):
    nd = P.shape[1] - 2
    if P.ndim != 2 or nd not in (2, 3):
        raise ValueError("expected (n, nd+2) with nd = 2 or 3")
    return nd


def primitive2state(fluid, P):
    """cfd.jl:106-123"""
    P, _, ldp = B._field(P)
    nd = _nd(P)
    Q = B._like(P, P.shape[0])
    f = fluid._c()
    B._stream()
    B.call("ibh_cfd_primitive2state", C.byref(f), nd, P.shape[0], B._ptr(P), ldp, B._ptr(Q), P.shape[0])
    return Q


def state2primitive(fluid, Q):
    """cfd.jl:137-151"""
    Q, _, ldq = B._field(Q)
    nd = _nd(Q)
    P = B._like(Q, Q.shape[0])
    f = fluid._c()
    B._stream()
    B.call("ibh_cfd_state2primitive", C.byref(f), nd, Q.shape[0], B._ptr(Q), ldq, B._ptr(P), Q.shape[0])
    return P


# the explicit Euler step around the fused sweeps (ibh_timestep_euler / ibh_update_euler / ibh_step_euler): defined with the
# other fused entries in backend.py, reachable from here beside the pointwise functions they compose
timestep_euler = B.timestep_euler
update_euler = B.update_euler
step_euler = B.step_euler
update_euler_stage = B.update_euler_stage          # (ibh_update_euler_stage / ibh_stage_euler: a Runge-Kutta stage)
stage_euler = B.stage_euler
update_euler_ssp = B.update_euler_ssp              # (ibh_update_euler_ssp / ibh_stage_euler_ssp: a Shu-Osher stage)
stage_euler_ssp = B.stage_euler_ssp
smooth_residual = B.smooth_residual                # (ibh_smooth_residual / ibh_update_euler_smoothed: implicit residual smoothing)
update_euler_smoothed = B.update_euler_smoothed
restrict_euler = B.restrict_euler                  # (ibh_restrict_euler / ibh_prolong_euler: the transfers of a multigrid cycle)
prolong_euler = B.prolong_euler
forcing_roles = B.forcing_roles                    # (ibh_forcing_roles / ibh_sumsq_roles: the cycle and its norm on fluid rows)
sumsq_roles = B.sumsq_roles


def inviscid_fluxes(fluid, PL, PR, *args):
    """``inviscid_fluxes(fluid, PL, PR, dim)`` (HLL, cfd.jl:459-508) or
    ``inviscid_fluxes(fluid, PL, PR, nuL, nuR, dim)`` (sensor/Rusanov, cfd.jl:516-554)."""
    PL, _, ld = B._field(PL)
    PR, _, ld2 = B._field(PR)
    if PR.shape != PL.shape:   # the kernel takes PR's extent from PL
        raise ValueError(f"inviscid_fluxes: PR of shape {tuple(PR.shape)}, PL of shape {tuple(PL.shape)}")
    if ld2 != ld:
        PR = PR.T.contiguous().T
        PL = PL.T.contiguous().T
        ld = PL.shape[0]
    nd = _nd(PL)
    n = PL.shape[0]
    F = B._like(PL, n)
    f = fluid._c()
    B._stream()
    if len(args) == 1:
        B.call("ibh_cfd_inviscid_fluxes_hll", C.byref(f), nd, int(args[0]), n, B._ptr(PL), B._ptr(PR), ld, B._ptr(F), n)
    elif len(args) == 3:
        nuL, _, _ = B._field(args[0], n)
        nuR, _, _ = B._field(args[1], n)
        B.call("ibh_cfd_inviscid_fluxes_sensor", C.byref(f), nd, int(args[2]), n, B._ptr(PL), B._ptr(PR), ld,
               B._ptr(nuL), B._ptr(nuR), B._ptr(F), n)
    else:
        raise TypeError("inviscid_fluxes(fluid, PL, PR, dim) or inviscid_fluxes(fluid, PL, PR, nuL, nuR, dim)")
    return F


def _check_gradients(what, grads, nd, ncol):
    """The viscous kernels take the extent of every gradient array from ``nd``: one (n, ncol) array per dimension, or they
    would read past the allocation."""
    if len(grads) != nd:
        raise ValueError(f"{what}: Pgrad needs one array per dimension")
    for g in grads:
        if g.ndim != 2 or g.shape[1] != ncol:
            raise ValueError(f"{what}: every gradient array must be (n, {ncol}), got {tuple(g.shape)}"
                             + (" (gradients of the velocities alone need velocity_gradients_only=True)"
                                if g.ndim == 2 and g.shape[1] == nd and ncol == nd + 2 else ""))


def viscous_fluxes(fluid, P, Pgrad, dim, mu_t=0.0):
    """cfd.jl:664-736 (Cartesian ``dim``); ``Pgrad`` = tuple of the gradients of P along each axis."""
    P, _, ldp = B._field(P)
    nd = _nd(P)
    n = P.shape[0]
    grads = [B._field(g, n)[0] for g in Pgrad]
    _check_gradients("viscous_fluxes", grads, nd, nd + 2)
    grads = [g.T.contiguous().T for g in grads]
    ptrs = (B.c_vp * nd)(*[g.data_ptr() for g in grads])
    F = B._like(P, n)
    f = fluid._c()
    mt_arr, mt_const = None, 0.0
    if hasattr(mu_t, "data_ptr"):
        mt_arr, _, _ = B._field(mu_t, n)
    else:
        mt_const = float(mu_t)
    B._stream()
    B.call("ibh_cfd_viscous_fluxes", C.byref(f), nd, int(dim), n, B._ptr(P), ldp, ptrs, n, B._ptr(mt_arr),
           C.c_float(mt_const), B._ptr(F), n)
    return F


def viscous_residual(part, fluid, P, Pgrad, mu_t, R, velocity_gradients_only=False):
    """``R[:, 1:] .+= sum_d green_gauss(part, viscous_fluxes(fluid, at_faces(part, P, d), face_gradient(part, P, Pgrad, d), d;
    mu_t = at_faces(part, mu_t, d)), d)`` in ONE launch (``ibh_viscous_residual``), bit-identical to that composition
    (cfd.jl:664-736 over ImmersedBoundary.jl:899-926, 1039-1069).  ``Pgrad`` = the tuple ``cell_gradient(part, P)`` -- or, with
    ``velocity_gradients_only``, ``cell_gradient(part, P[:, 3:end])``: the viscous fluxes read the gradients of the velocities
    and the NORMAL derivative of T only, which is a ``face_gradient`` --, ``mu_t`` a cell array, ``R`` the (nc, nd + 2)
    residual updated in place."""
    part = B._part(part)
    P, _, ldp = B._field(P, part.nc)
    nd = _nd(P)
    if nd != part.nd:   # the kernel takes the column counts of P, Pgrad and R from the partition
        raise ValueError(f"viscous_residual: P must be (nc, nd + 2) with the partition's nd = {part.nd}")
    grads = [B._field(g, part.nc)[0] for g in Pgrad]
    _check_gradients("viscous_residual", grads, nd, nd if velocity_gradients_only else nd + 2)
    ldg = {g.stride(1) for g in grads}
    if len(ldg) != 1:
        grads = [g.T.contiguous().T for g in grads]
        ldg = {part.nc}
    ptrs = (B.c_vp * nd)(*[g.data_ptr() for g in grads])
    mt = B._field(mu_t, part.nc)[0]
    R, nvr, ldr = B._field_inplace(R, part.nc, "R")
    if nvr != nd + 2:
        raise ValueError("R must be (nc, nd + 2)")
    f = fluid._c()
    B._stream()
    B.call("ibh_viscous_residual", part.handle, C.byref(f), B._ptr(P), ldp, ptrs, int(ldg.pop()),
           0 if velocity_gradients_only else 2, B._ptr(mt), B._ptr(R), ldr)
    return R


class FlowBC:
    """cfd.jl:160-300 -- generic flow boundary condition, called on device arrays inside ``impose_bc`` closures:
    ``bc(P, bdry.normals)``, ``bc(P, bdry.normals, du_dn=..., image_distances=bdry.image_distances, transpiration=...)``.
    ``FlowBC(fluid, [p, T, u, v(, w)])`` is a Dirichlet state (inlet/outlet/no-slip wall), ``FlowBC(fluid, [p, T, un],
    normal_flow=True)`` imposes the normal velocity only (slip wall)."""

    def __init__(self, fluid, P, normal_flow=False):
        self.fluid = fluid
        self.p_inf, self.T_inf = float(P[0]), float(P[1])
        self.u_inf = np.ascontiguousarray(np.asarray(P[2:], dtype=np.float32))
        self.normal_flow = bool(normal_flow)

    def __call__(self, P, normals, image_distances=None, du_dn=None, transpiration=0.0):
        P, _, ldp = B._field(P)
        nd = _nd(P)
        n = P.shape[0]
        nrm, nnv, ldn = B._field(normals, n)
        if nnv != nd:
            raise ValueError("normals must be (n, nd)")
        if self.normal_flow:
            assert self.u_inf.size == 1, "Only 3 parcels in P (p, T and normal flow) allowed for normal_flow = true BC"
        elif self.u_inf.size != nd:
            raise ValueError("FlowBC needs one free-stream velocity component per dimension")
        if (du_dn is None) != (image_distances is None):
            raise ValueError("du!dn and image_distances must be passed together for BC imposition")
        imd = None if image_distances is None else B._field(image_distances, n)[0]
        dn = None if du_dn is None else B._field(du_dn, n)[0]
        tv, tc = None, 0.0
        if hasattr(transpiration, "data_ptr"):
            tv = B._field(transpiration, n)[0]
        else:
            tc = float(transpiration)
        out = B._like(P, n)
        f = self.fluid._c()
        B._stream()
        B.call("ibh_cfd_flow_bc", C.byref(f), nd, n, B._ptr(P), ldp, B._ptr(nrm), ldn, C.c_float(self.p_inf),
               C.c_float(self.T_inf), self.u_inf.ctypes.data_as(B.c_vp), int(self.normal_flow), B._ptr(imd), B._ptr(dn),
               C.c_float(tc), B._ptr(tv), B._ptr(out), n)
        return out


# ---------------------------------------------------------------------------------------------------------------------
# pressure coefficient and running statistics (device arrays)
# ---------------------------------------------------------------------------------------------------------------------
def pressure_coefficient(fluid, p, p_inf, M_inf):
    """``CFD.pressure_coefficient`` (cfd.jl:411-424): ``2 * (p / p∞ - 1) / (M∞^2 * γ)`` as one broadcast launch
    (``ibh_ew_eval``), in the reference's order with ``M∞^2 * γ`` folded on the host in Float32 (``M*M``, then ``*γ``).
    The result is Float32 with ``p∞`` and ``M∞`` rounded to Float32; the reference returns Float64 for Float64 scalars.
    Takes and returns a device tensor or a ``HipArray``."""
    from .hiparray import HipArray
    hit = isinstance(p, HipArray)
    pa = p if hit else HipArray(B._field(p)[0])
    M = np.float32(M_inf)
    s = np.float32(M * M) * np.float32(fluid.gamma)
    cp = 2.0 * (pa / np.float32(p_inf) - 1.0) / s
    return cp if hit else cp.t


def _kind(x):
    """Julia type class of a host scalar: 'i' (Integer), 'f32' (Float32 and narrower), 'f64' (Float64, Python float)."""
    if isinstance(x, (bool, numbers.Integral, np.integer)):
        return "i"
    if isinstance(x, np.floating) and x.dtype.itemsize <= 4:
        return "f32"
    if isinstance(x, (float, np.floating)):
        return "f64"
    raise TypeError(f"expected a real scalar, got {type(x).__name__}")


class _TA:
    """dt forms and flags of ibh_time_average_push (include/ibhip.h)."""
    DT_HOST, DT_DEVICE, DT_PER_VAR, DT_ELEMENT = constants("IBH_TA_", "DT_HOST DT_DEVICE DT_PER_VAR DT_ELEMENT")
    F64, FIRST = constants("IBH_TA_", "F64 FIRST")


class TimeAverage:
    """``CFD.TimeAverage`` (cfd.jl:738-802): exponential moving average ``mu`` and its standard deviation ``sigma`` of a
    device field for the time scale ``tau``.  ``push(Q, dt)`` is one launch (``ibh_time_average_push``) that updates
    ``mu`` and ``sigma`` in place, so a held reference to ``mu`` sees every later push.

    ``dt``: a host scalar (Python / numpy), or a Float32 device tensor that is one element (e.g. the march's device dt:
    no host sync), 1-D of length ``nv`` with a 2-D ``Q`` (per variable: the reference's reshape along the last axis), or
    of ``Q``'s shape (elementwise).  Anything else raises before a launch.  Precision follows Julia's promotion: ``eta =
    dt / tau`` and every product with it are Float64 if ``tau`` or a host ``dt`` is Float64 (a Python float counts),
    otherwise Float32; ``sigma^2`` and ``(mu - Q)^2`` stay Float32.  ``dt > tau`` gives NaN in sigma where the
    reference's ``sqrt`` would throw."""

    def __init__(self, tau):
        _kind(tau)
        self.tau = tau
        self.mu = None
        self.sigma = None

    def _dt_form(self, dt, n, nv, ndim):
        """(form, device tensor or None, numel, ld) of ``dt`` for a Q of shape (n,) / (n, nv); raises for other shapes."""
        if not hasattr(dt, "data_ptr"):
            _kind(dt)
            return _TA.DT_HOST, None, 0, 0
        if not isinstance(dt, torch.Tensor) or not dt.is_cuda or dt.dtype != torch.float32:
            raise TypeError("TimeAverage.push: an array dt must be a Float32 device tensor")
        shape = tuple(dt.shape)
        qshape = (n,) if ndim == 1 else (n, nv)
        if dt.numel() == 1 and dt.ndim <= ndim:
            return _TA.DT_DEVICE, dt.reshape(1), 1, 1
        if ndim == 2 and shape == (nv,):
            return _TA.DT_PER_VAR, dt.contiguous(), nv, nv
        if shape == qshape:
            d, _, ld = B._field(dt)
            return _TA.DT_ELEMENT, d, (nv - 1) * ld + n, ld
        raise ValueError(f"TimeAverage.push: dt of shape {shape} does not broadcast with Q of shape {qshape} "
                         "(DimensionMismatch): dt is a scalar, one element, per variable (nv,) or Q's shape")

    def push(self, Q, dt=np.float32(1)):
        """``push!(avg, Q, dt)``: the first call registers ``mu = copy(Q)``, ``sigma = mu .* 0``; returns ``mu``."""
        from .hiparray import HipArray
        hit = isinstance(Q, HipArray)
        q, nv, ldq = B._field(Q.t if hit else Q)
        n = q.shape[0]
        if self.mu is None:
            mu, sg = B._like(q, n), B._like(q, n)
            B._stream()
            B.call("ibh_time_average_push", n, nv, B._ptr(q), ldq, B._ptr(mu), B._ptr(sg), _TA.DT_HOST, B._ptr(None),
                   0, 0, C.c_double(0.0), C.c_double(1.0), _TA.FIRST)
            self.mu, self.sigma = (HipArray(mu), HipArray(sg)) if hit else (mu, sg)
            return self.mu
        mu, sg = self.mu, self.sigma
        if isinstance(mu, HipArray):
            mu._flush_readers()   # pending broadcasts that read mu / sigma see the old values, as in Julia
            sg._flush_readers()
            mu, sg = mu.t, sg.t
        if tuple(mu.shape) != tuple(q.shape):
            raise ValueError(f"TimeAverage.push: Q of shape {tuple(q.shape)} after {tuple(mu.shape)} (DimensionMismatch)")
        form, d, numel, ldd = self._dt_form(dt, n, nv, q.ndim)
        kt = _kind(self.tau)
        kd = "f32" if d is not None else _kind(dt)
        f64 = "f64" in (kt, kd) or (kt == "i" and kd == "i")    # Int / Int is Float64 in Julia
        real = np.float64 if f64 else np.float32
        tau = real(self.tau)
        eta = real(dt) / tau if d is None else real(0)
        B._stream()
        B.call("ibh_time_average_push", n, nv, B._ptr(q), ldq, B._ptr(mu), B._ptr(sg), form, B._ptr(d), numel, ldd,
               C.c_double(float(eta)), C.c_double(float(tau)), _TA.F64 if f64 else 0)
        return self.mu


# ---------------------------------------------------------------------------------------------------------------------
# free-stream utilities (host scalars, numpy).  Julia's promotion is kept: the reference's constants are Float32, a
# Python float is a Float64 and a Python int an Int (numpy's weak Python scalars would turn them into Float32).
# ---------------------------------------------------------------------------------------------------------------------
_f32 = np.float32


def _jl(x):
    if isinstance(x, (bool, numbers.Integral, np.integer)):
        return int(x)
    if isinstance(x, float) and not isinstance(x, np.floating):
        return np.float64(x)
    return x


_ISA_LAYERS = [  # base altitude [m], base temperature [K], lapse rate [K/km], base pressure [Pa]
    (_f32(0.0), _f32(288.15), _f32(-6.5), _f32(101325.0)),     # Troposphere
    (_f32(11000.0), _f32(216.65), _f32(0.0), _f32(22632.0)),   # Tropopause
    (_f32(20000.0), _f32(216.65), _f32(1.0), _f32(5474.9)),    # Stratosphere 1
    (_f32(32000.0), _f32(228.65), _f32(2.8), _f32(868.02)),    # Stratosphere 2
    (_f32(47000.0), _f32(270.65), _f32(0.0), _f32(110.91)),    # Stratopause
    (_f32(51000.0), _f32(270.65), _f32(-2.8), _f32(66.939)),   # Mesosphere 1
    (_f32(71000.0), _f32(214.65), _f32(-2.0), _f32(3.9564)),   # Mesosphere 2
]


def _ISA_atmosphere(altitude_m, dT=0.0):
    """cfd.jl:304-368: (p, T) of the standard atmosphere.  As in the reference: the loop over ``1:length(layers)-1`` never
    selects the 71 km layer, and isothermal layers use ``T_base + ΔT``."""
    altitude_m, dT = _jl(altitude_m), _jl(dT)
    R, g0 = _f32(287.05287), _f32(9.80665)
    if altitude_m < 0:
        raise ValueError("Altitude cannot be negative")
    elif altitude_m > 86000:
        warnings.warn("Altitude above 86 km - model accuracy decreases")
    layer_idx = 0
    for i in range(len(_ISA_LAYERS) - 1):
        if altitude_m >= _ISA_LAYERS[i][0]:
            layer_idx = i
    h_base, T_base, lapse_rate, P_base = _ISA_LAYERS[layer_idx]
    lapse_rate_per_m = lapse_rate / _f32(1000.0)
    delta_h = altitude_m - h_base
    T = T_base + lapse_rate_per_m * delta_h + dT
    if abs(lapse_rate_per_m) < _f32(1e-10):
        P = P_base * np.exp(-g0 * delta_h / (R * (T_base + dT)))
    else:
        exponent = -g0 / (R * lapse_rate_per_m)
        T_base_offset = T_base + dT
        T_offset = T_base_offset + lapse_rate_per_m * delta_h
        P = P_base * (T_offset / T_base_offset) ** exponent
    return P, T


def _host_speed_of_sound(fluid, T):
    """cfd.jl:62-64 on a host scalar, with the Float32 fluid constants."""
    return np.sqrt(_f32(fluid.gamma) * _f32(fluid.R) * np.clip(T, _f32(10.0), np.float32(np.inf)))


def ISA_atmosphere(altitude_m, dT=_f32(0.0), Mach=_f32(0.0), V=None, u_hat=(_f32(1.0),)):
    """``CFD.ISA_atmosphere(altitude_m; ΔT, Mach, V, û)`` (cfd.jl:370-397): ``(Fluid(), [p, T, u * û])``.  ``V`` overrides
    the Mach number; ``û`` is normalised with ``eps`` added to its norm.  The speed of sound uses ``Fluid()``'s R = 283,
    the pressure the ISA's R = 287.05287, as in the reference.  Negative altitudes raise; above 86 km it warns."""
    p, T = _ISA_atmosphere(altitude_m, dT)
    fluid = Fluid()
    u = _jl(V)
    if u is None:
        a = _host_speed_of_sound(fluid, T)
        u = _jl(Mach) * a
    uh = np.asarray([_jl(x) for x in u_hat])
    if uh.dtype.kind != "f":
        uh = uh.astype(np.float64)
    uh = uh / (np.finfo(uh.dtype).eps + np.sqrt(np.sum(uh * uh)))
    vel = u * uh
    dtype = np.result_type(p, T, vel)
    return fluid, np.concatenate([np.asarray([p, T], dtype=dtype), vel.astype(dtype)])


def _sind(x):
    """Julia's ``sind``: exact at multiples of 90 degrees."""
    r = math.fmod(float(x), 360.0)
    if r % 90.0 == 0.0:
        return (0.0, 1.0, 0.0, -1.0)[int(r // 90.0) % 4]
    return math.sin(math.radians(r))


def _cosd(x):
    r = math.fmod(float(x), 360.0)
    if r % 90.0 == 0.0:
        return (1.0, 0.0, -1.0, 0.0)[int(r // 90.0) % 4]
    return math.cos(math.radians(r))


def streamwise_direction(alpha, beta=None):
    """``CFD.streamwise_direction(α[, β])`` (cfd.jl:401-409, 426-436), angles in degrees: ``[cosd α, sind α]`` in 2-D,
    ``[cosd α cosd β, -cosd α sind β, sind α]`` in 3-D."""
    args = (alpha,) if beta is None else (alpha, beta)
    dtype = np.float32 if all(_kind(x) == "f32" for x in args) else np.float64
    if beta is None:
        return np.array([_cosd(alpha), _sind(alpha)], dtype=dtype)
    if dtype == np.float32:   # each factor is a Float32 in Julia, and so is the product
        ca, cb, sb = _f32(_cosd(alpha)), _f32(_cosd(beta)), _f32(_sind(beta))
        return np.array([ca * cb, -ca * sb, _f32(_sind(alpha))], dtype=dtype)
    return np.array([_cosd(alpha) * _cosd(beta), -_cosd(alpha) * _sind(beta), _sind(alpha)], dtype=dtype)


def _host_dynamic_viscosity(fluid, T):
    """cfd.jl:71-77 (Sutherland, with the reference's exponent 2/3) on a host scalar, Float32 fluid constants."""
    T = np.clip(T, _f32(10.0), np.float32(np.inf))
    Tref, S = _f32(fluid.Tref), _f32(fluid.S)
    return _f32(fluid.mu_ref) * ((T / Tref) ** (_f32(2.0) / 3)) * (Tref + S) / (T + S)


def Reynolds_number(fluid, P_inf, Lref):
    """``CFD.Reynolds_number(fluid, P∞, Lref)`` (cfd.jl:626-638): ``|u∞| Lref ρ / μ(T∞)`` with ``P∞ = [p, T, u...]``."""
    P = np.asarray(P_inf)
    V = np.sqrt(np.sum(P[2:] * P[2:]))
    T = P[1]
    p = P[0]
    rho = p / (_f32(fluid.R) * T)
    mu = _host_dynamic_viscosity(fluid, T)
    return V * _jl(Lref) * rho / mu


def adjust_Reynolds(fluid, P_inf, Lref, Re):
    """``CFD.adjust_Reynolds(fluid, P∞, Lref, Re)`` (cfd.jl:640-654): a new ``Fluid`` whose reference viscosity gives the
    Reynolds number ``Re``."""
    Re_old = Reynolds_number(fluid, P_inf, Lref)
    mu_ref = _f32(fluid.mu_ref) * Re_old / _jl(Re)
    return Fluid(fluid.R, fluid.gamma, fluid.k, float(mu_ref), fluid.Tref, fluid.S)

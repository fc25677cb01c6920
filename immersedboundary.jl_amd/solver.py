"""Device-resident ``FAS!`` (mirror of /root/reference/src/solver.jl:39-91) and ``EulerMarch``, the explicit time march
of the compressible equations (the ``march!`` loop of test/advection.jl:61-89 around the fused Euler sweeps).

Same signature and semantics as the reference (including its quirks: the recursion guard is
``length(coarseners) > 1`` so the last supplied level is never visited, and the coarse problem is solved
before the fine smoothing).  ``Q``, the residuals and the sources are device arrays that never leave the
GPU; coarseners / prolongators are device Accumulators (``to_backend(acc)``: one SpMV kernel each); the
fixed-point update and the norm are libibhip kernels.  The only host round-trip per iteration is the
scalar norm the reference's convergence test needs (solver.jl:84-87).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import backend as B

_eps32 = float(np.finfo(np.float32).eps)


def _norm(r):
    """||r||_2 of a device array (sum of squares accumulated in Float64 on the device)."""
    r, nv, ld = B._field(r)
    flat = r if r.ndim == 1 or ld == r.shape[0] else r.T.contiguous().T
    out = torch.zeros(1, dtype=torch.float64, device=r.device)
    B._stream()
    B.call("ibh_sumsq", int(flat.numel()), B._ptr(flat), B._ptr(out))
    return float(out.item()) ** 0.5


def _update(Q, omega, r):
    """Q += clamp(omega, 0, 1) * r  (solver.jl:82)."""
    if isinstance(omega, torch.Tensor):
        Q += torch.clamp(omega, 0.0, 1.0) * r
        return
    Qf, _, ldq = B._field(Q)
    rf, _, ldr = B._field(r)
    if Qf.data_ptr() != Q.data_ptr() or (Q.ndim == 2 and (ldq != Q.shape[0] or ldr != r.shape[0])):
        Q += min(max(float(omega), 0.0), 1.0) * r
        return
    B._stream()
    B.call("ibh_axpy_clamped", int(Q.numel()), C.c_float(float(omega)), B._ptr(rf), B._ptr(Q))


def _update_norm(Q, omega, r):
    """``_update`` and ``_norm(r)`` in one pass over ``r`` (``ibh_axpy_clamped_sumsq``); None if the arrays do not allow it."""
    return _fas_pass(r, None, Q, omega, True)


def _dense_pair(a, b):
    """True when two device arrays are column-major without padding and of one shape (one flat pass covers both)."""
    if a.shape != b.shape:
        return False
    for t in (a, b):
        f, _, ld = B._field(t)
        if f.data_ptr() != t.data_ptr() or (t.ndim == 2 and ld != t.shape[0]):
            return False
    return True


def _fas_pass(r, source, Q, omega, want_norm):
    """``rr = r [+ source]; [Q += clamp(omega, 0, 1) * rr]; [||rr||]`` in ONE launch (``ibh_fas_update``: solver.jl:80-84 on
    one read of ``r``).  ``source`` and ``Q`` may be None.  Returns the norm (or True when none was asked for), or None when
    the arrays do not allow the flat pass (padded layouts, a per-cell ``omega``): the caller composes the steps then."""
    if isinstance(omega, torch.Tensor):
        return None
    if (source is not None and not _dense_pair(r, source)) or (Q is not None and not _dense_pair(r, Q)):
        return None
    f, _, ld = B._field(r)
    if f.data_ptr() != r.data_ptr() or (r.ndim == 2 and ld != r.shape[0]):
        return None
    out = torch.empty(1, dtype=torch.float64, device=r.device) if want_norm else None
    B._stream()
    B.call("ibh_fas_update", int(r.numel()), C.c_float(float(omega) if omega is not None else 0.0), B._ptr(r),
           B._ptr(source), B._ptr(Q), B._ptr(out))
    return float(out.item()) ** 0.5 if want_norm else True


def _sub(a, b):
    """``a .- b`` of two device arrays as a libibhip broadcast (``ibh_ew_*``), not an ATen kernel."""
    from .hiparray import HipArray
    return (HipArray(a) - HipArray(b)).t


def _add(a, b):
    from .hiparray import HipArray
    return (HipArray(a) + HipArray(b)).t


def FAS(f, Q, coarseners=(), prolongators=(), perscribed_f=None, multigrid_level=0, n_iter=50,
        rtol=1e-1, atol=1e-7, norm=None, check_every=1, exchange=None, level_norm=None):
    """``FAS!(f, Q; coarseners, prolongators, perscribed_f, multigrid_level, n_iter, rtol, atol)``.

    ``f(level, Q) -> (r, omega)`` with device arrays; ``Q`` is updated in place.  Returns the residual-norm
    reduction ratio like the reference.  ``norm``: the norm of a residual array; on a rank of a multi-GPU run pass
    ``distributed.Reductions(...).norm`` (sum over the owned cells of all ranks, one all-reduce), default = local.
    ``check_every``: the convergence test -- the one host round trip (and all-reduce) of an iteration -- is made every
    that many iterations and after the last one; 1 = the reference's loop, larger values may run up to
    ``check_every - 1`` smoothing steps past the reference's exit.
    On a rank of a multi-GPU run (``distributed.RankLevels``: the rank's partition of every level, local transfer
    operators): ``exchange(level, Q)`` refreshes the skirt (and donor) rows of a level's local array -- called before every
    residual evaluation and around the coarse solve, where the prolongation reads coarse skirt rows -- and
    ``level_norm(level, r)`` is the norm over the owned cells of all ranks (``Reductions.norm`` of that level).
    """
    local_norm = level_norm is None and norm is None      # the library's own norm: fused with the update below
    if level_norm is not None:
        def _norm(r, _l=multigrid_level):
            return level_norm(_l, r)
    else:
        _norm = norm if norm is not None else globals()["_norm"]
    l = multigrid_level
    xch = exchange if exchange is not None else (lambda _l, _q: None)
    xch(l, Q)
    fQ, omega = f(l, Q)
    source = None
    if perscribed_f is not None:
        source = _sub(perscribed_f, fQ)
    nr0 = _fas_pass(fQ, source, None, None, True) if local_norm else None    # ||fQ + source|| on one read of fQ
    if nr0 is None:
        nr0 = _norm(fQ if source is None else _add(fQ, source))
    nr = nr0
    if len(coarseners) > 1:
        coars, prolong = B.to_backend(coarseners[0]), B.to_backend(prolongators[0])
        Qc = coars(Q)
        xch(l + 1, Qc)                       # (the prolongation below reads skirt rows of Qc - Qcold)
        Qcold = B._like(Qc, Qc.shape[0])
        Qcold.copy_(Qc)
        pfQc = coars(fQ if source is None else _add(fQ, source))
        FAS(f, Qc, coarseners=coarseners[1:], prolongators=prolongators[1:], perscribed_f=pfQc,
            multigrid_level=multigrid_level + 1, n_iter=n_iter, atol=atol, rtol=rtol, norm=norm,
            check_every=check_every, exchange=exchange, level_norm=level_norm)
        xch(l + 1, Qc)
        prolong.diff_add(Q, Qc, Qcold)       # Q .+= prolong(Qc .- Qcold), one launch
    check_every = max(1, int(check_every))
    for it in range(n_iter):
        xch(l, Q)
        r, omega = f(l, Q)
        check = (it + 1) % check_every == 0 or it == n_iter - 1
        # r .+= source; Q .+= clamp(omega, 0, 1) .* r; norm(r): one launch where the layouts allow (and the norm is local)
        fused = _fas_pass(r, source, Q, omega, check and local_norm)
        if fused is None:
            if source is not None:
                r = _add(r, source)
            _update(Q, omega, r)
            if check:
                fused = _norm(r)
        elif check and not local_norm:
            fused = _norm(r if source is None else _add(r, source))
        if check:
            nr = fused
            if nr < nr0 * rtol + atol:
                break
    return nr / (nr0 + _eps32)


def rk_stages(m):
    """The stage coefficients ``alpha_k = 1/(m-k+1)``, ``k = 1..m``, of the ``m``-stage low-storage (Jameson) Runge-Kutta step
    ``P_k = state2primitive(primitive2state(P_0) + (alpha_k dt) R(P_{k-1}))``: its linear amplification factor is the
    degree-``m`` Taylor polynomial of ``exp``.  ``rk_stages(1) == (1.0,)`` is forward Euler."""
    if isinstance(m, bool) or int(m) != m or int(m) < 1:
        raise ValueError("the number of stages must be an integer >= 1")
    m = int(m)
    return tuple(1.0 / (m - k + 1) for k in range(1, m + 1))


def ssp_stages(order):
    """The Shu-Osher form of the strong-stability-preserving Runge-Kutta scheme of ``order`` 2 or 3 (SSPRK2: Heun's method,
    SSPRK3: Shu and Osher's third-order scheme) as a tuple of ``(a, b, c)`` triples, one per stage:
    ``Q_k = a Q_0 + b Q_{k-1} + c dt R(P_{k-1})`` in conserved variables.  Every stage is a convex combination (``a, b >= 0``,
    ``a + b = 1``, ``c = b``) of the step's input and a forward-Euler step of the previous stage, so the scheme keeps every
    bound forward Euler keeps under the same time step."""
    if isinstance(order, bool) or order not in (2, 3):
        raise ValueError("ssp_stages: order must be 2 or 3")
    if int(order) == 2:
        return ((0.0, 1.0, 1.0), (1.0 / 2, 1.0 / 2, 1.0 / 2))
    return ((0.0, 1.0, 1.0), (3.0 / 4, 1.0 / 4, 1.0 / 4), (1.0 / 3, 2.0 / 3, 2.0 / 3))


class EulerMarch:
    """The explicit time march of an unsteady Euler / LES run on one partition, without the host in the loop: per step

    1. ``timestep_euler`` (the CFL time step from ``P``, left on the device) on every ``dt_every``-th step,
    2. ``step_euler`` (sweep + conservative update: one launch where the 2-D single-kernel sweep applies),
    3. ``bcs(P_new)``: any callable on the new array, e.g. the two ``impose_flow_bc`` calls of
       ``closures.config5_boundary_conditions(fused=True)``,
    4. ``average.push(P_new, dt)`` with the device ``dt`` (``cfd.TimeAverage``, cfd.jl:738-802).

    The march owns the ping-pong arrays, the one-element device ``dt`` (``local_dt``: an ``(nc,)`` array of per-cell time
    steps, the pseudo-time march to a steady state) and the sweep's ``work`` array; ``step(P)`` returns the new array -- one
    of the two ping-pong arrays, valid until the step after the next -- and makes no host read-back and no allocation after
    construction, so ``n`` steps can be captured in ``torch.cuda.graph`` and replayed (a ``TimeAverage`` registers its
    arrays on its first push: push once, or run one step, before capturing).

    ``residual``: a callable ``f(part, P, out)`` that writes the residual of ``[rho E rho*u rho*v (rho*w)]`` into ``out``,
    e.g. ``lambda part, P, out: closures.navier_stokes_les_residual(part, P, Delta, out=out)``; the step is then ``f``
    followed by ``update_euler``.  ``scheme``: "hll" or "sensor" (``residual_euler_hll`` / ``residual_euler_sensor``).

    ``stages``: the number ``m`` of Runge-Kutta stages (``rk_stages(m)``), or the tuple of stage coefficients itself.  With
    ``stages=1`` a step is exactly the calls above.  With more, the time step is computed once from the step's input
    ``P_0`` and step 2 becomes ``m`` calls ``stage_euler(P_{k-1}, P_0, dt, alpha_k) -> P_k`` (with ``residual``: the callable
    into ``work``, then ``update_euler_stage``), ``bcs`` after every one of them -- the next sweep reads the ghost cells --
    and ``average.push(P_m, dt)`` once with the full ``dt``.  The march then owns three arrays: the stages alternate between
    the two that do not hold ``P_0``, so ``P_0`` -- the caller's array or the previous return value -- is never written.
    Either way a returned array stays valid during the next ``step`` and is overwritten by the one after it.

    ``stages`` as a tuple of ``(a, b, c)`` triples (``ssp_stages(order)``) marches in the Shu-Osher form
    ``Q_k = a Q_0 + b Q_{k-1} + c dt R(P_{k-1})``: a stage with ``(a, b) == (0, 1)`` is ``stage_euler(P_{k-1}, P_{k-1}, dt, c)``
    -- no blend -- and every other one ``stage_euler_ssp(P_{k-1}, P_0, dt, a, b, c)`` (with ``residual``: the callable into
    ``work``, then ``update_euler_stage`` / ``update_euler_ssp``); time step, ``bcs``, ``average`` and the three arrays as
    above.

    ``smoothing=(eps, n_iter)``: implicit residual smoothing, the third acceleration of a pseudo-time march beside
    ``local_dt`` and the stages -- it lets ``scale`` exceed the explicit limit of the scheme.  Every stage becomes the
    residual into ``work`` (the sweep alone, or ``residual``), ``smooth_residual(work, eps, n_iter - 1)`` when
    ``n_iter >= 2`` and ``update_euler_smoothed`` with the stage's form, which does the last iteration itself:
    ``n_iter + 1`` launches.  A forward-Euler step is the stage form on the step's input with ``c = 1``.  The smoothing
    arrays (none for ``n_iter = 1``, one for 2, two from 3) are allocated here.  The march is no longer time accurate:
    ``smoothing`` with ``average`` raises, and so do the image-only, phase and single-pass ``flags`` -- the smoothing
    would gather rows the sweep never wrote.

    ``roles``: a ``backend.Roles`` of the partition (``cell_roles``: what every row IS -- fluid, ghost or solid).  After
    every stage, after the stage's ``bcs``, the solid rows are set to the ``Roles``' ``solid_state`` (``Roles.blank``: one
    ``ibh_scatter_rows`` launch more per stage, none without solid rows; it can be captured in a graph), so the cells
    inside a body no longer march a flow of their own; every other row has the bits of the march without roles as long
    as no sweep reads a solid row for it.  ``residual_norms(P)`` is then the norm of the residual over the fluid rows.
    Without ``roles`` the march makes the calls it always made."""

    def __init__(self, part, fluid=None, scheme="hll", scale=0.75, bcs=None, average=None, local_dt=False, dt_every=1,
                 residual=None, flags=0, stages=1, smoothing=None, roles=None):
        from . import cfd
        if roles is not None and not isinstance(roles, B.Roles):
            raise ValueError("roles must be a backend.Roles of the partition (Roles(part, cell_roles(dom)[part.domain], "
                             "solid_state)) or None")
        self.part = B._part(part)
        if roles is not None and (roles.nc, roles.nd) != (self.part.nc, self.part.nd):
            raise ValueError(f"roles are those of a partition of {roles.nc} cells in {roles.nd} dimensions; this one has "
                             f"{self.part.nc} in {self.part.nd}")
        self.roles = roles
        self.fluid = fluid if fluid is not None else cfd.Fluid()
        if scheme not in B._EULER_SCHEMES:
            raise ValueError('scheme must be "hll" or "sensor"')
        if int(dt_every) < 1:
            raise ValueError("dt_every must be >= 1")
        if local_dt and average is not None:
            raise ValueError("a time average needs one time step for all cells: local_dt marches in pseudo-time")
        self.scheme, self.scale, self.bcs, self.average = scheme, float(scale), bcs, average
        self.local_dt, self.dt_every, self.residual, self.flags = bool(local_dt), int(dt_every), residual, int(flags)
        ssp = isinstance(stages, (tuple, list)) and any(isinstance(a, (tuple, list)) for a in stages)
        if ssp:
            if not all(isinstance(a, (tuple, list)) and len(a) == 3 for a in stages):
                raise ValueError("stages in the Shu-Osher form must be (a, b, c) triples, every one of them")
            self.stages = tuple(tuple(float(x) for x in a) for a in stages)
        else:
            self.stages = tuple(float(a) for a in stages) if isinstance(stages, (tuple, list)) else rk_stages(stages)
        if not self.stages:
            raise ValueError("stages must name at least one stage coefficient")
        self._staged = self.stages != (1.0,)
        # one record per stage, (form, base, coefficients, update, fused): which state `_stage` updates, with what, its calls
        if not self._staged:
            records = [("step", "src", ())]
        elif ssp:   # (a, b) == (0, 1): no blend, the low-storage stage on the previous stage itself
            records = [("stage", "src", (c,)) if (a, b) == (0.0, 1.0) else ("ssp", "P0", (a, b, c)) for a, b, c in self.stages]
        else:
            records = [("stage", "P0", (alpha,)) for alpha in self.stages]
        self._records = [r + _stage_calls(r[0], r[2]) for r in records]
        nc, nv = self.part.nc, self.part.nd + 2
        self._buf = tuple(B.colmajor_empty(nc, nv) for _ in range(3 if self._staged else 2))
        self.work = B.colmajor_empty(nc, nv)
        self.dt = B.colmajor_empty(nc) if self.local_dt else torch.empty(1, dtype=torch.float32, device=self.work.device)
        self.smoothing, self._smooth = None, ()
        if smoothing is not None:
            if not isinstance(smoothing, (tuple, list)) or len(smoothing) != 2:
                raise ValueError("smoothing must be (eps, n_iter)")
            self.smoothing = B._smoothing("EulerMarch", *smoothing)
            if average is not None:
                raise ValueError("a time average needs a time-accurate march: residual smoothing marches in pseudo-time")
            if self.flags & (B.IBH_IMAGE_ONLY | B.IBH_PHASE_INTERIOR | B.IBH_PHASE_BOUNDARY | B.IBH_PASS_A_ONLY
                             | B.IBH_PASS_B_ONLY):
                raise ValueError("smoothing: IBH_IMAGE_ONLY, the overlap phases and the single-pass flags are not taken: "
                                 "the smoothing gathers the residual of every cell")
            self._smooth = tuple(B.colmajor_empty(nc, nv) for _ in range(min(self.smoothing[1] - 1, 2)))
        self._norms = torch.zeros(nv, dtype=torch.float64, device=self.work.device) if roles is not None else None
        self.nsteps = 0

    def step(self, P):
        """One step from ``P`` (any ``(nc, nd+2)`` device array, e.g. the previous return value); returns the new array."""
        if not isinstance(P, torch.Tensor):
            P = P.t                                    # a HipArray: its pending broadcasts are evaluated here
        src = self._stages(P, self.nsteps)
        if self.average is not None:
            self.average.push(src, self.dt)
        self.nsteps += 1
        return src

    def _stages(self, P, count, last=None):
        """The time step -- on every ``dt_every``-th ``count`` -- and the stages of one step from ``P``, ``bcs`` after every
        one; returns the array of the last stage: one of the ping-pong arrays, or ``last`` where that is given."""
        if count % self.dt_every == 0:
            if self.local_dt:
                B.timestep_euler(self.part, P, self.fluid, self.scale, out=False, cells=self.dt)
            else:
                B.timestep_euler(self.part, P, self.fluid, self.scale, out=self.dt)
        # stage k sweeps the previous stage into one of the two arrays that are neither the step's input nor its own input
        free = [b for b in self._buf if b.data_ptr() != P.data_ptr()][:2]
        src = P
        for k, record in enumerate(self._records):
            out = last if last is not None and k == len(self._records) - 1 else free[k % 2]
            self._stage(record, src, P, out)
            if self.bcs is not None:
                self.bcs(out)
            if self.roles is not None:
                self.roles.blank(out)
            src = out
        return src

    def sweep(self, P):
        """``R(P)`` into ``work`` (the ``residual`` callable, or the sweep of the march's scheme); returns ``work``."""
        if self.residual is not None:
            self.residual(self.part, P, self.work)
            return self.work
        fn = B.residual_euler_hll if self.scheme == "hll" else B.residual_euler_sensor
        return fn(self.part, P, out=self.work, flags=self.flags, fluid=self.fluid)

    def residual_norms(self, P):
        """The sums of squares of the ``nd + 2`` columns of ``R(P)`` over the FLUID rows, as ``nd + 2`` device doubles: the
        sweep into ``work``, then ``sumsq_roles``.  No read-back and no allocation; the tensor returned is the march's own
        and the next call overwrites it.  Needs ``roles``."""
        if self.roles is None:
            raise ValueError("residual_norms: the march has no roles (EulerMarch(..., roles=Roles(...)))")
        if not isinstance(P, torch.Tensor):
            P = P.t
        return B.sumsq_roles(self.sweep(P), self.roles, out=self._norms)

    def _stage(self, record, src, P0, out):
        """One stage of a step from ``P0`` (the time step is in ``self.dt``): the sweep of the previous stage ``src`` and the
        update of the record's form into ``out``."""
        form, base, coef, update, fused = record
        base = src if base == "src" else P0
        if self.smoothing is not None:
            eps, n_iter = self.smoothing
            if self.residual is not None:
                self.residual(self.part, src, self.work)
            else:
                sweep = B.residual_euler_hll if self.scheme == "hll" else B.residual_euler_sensor
                sweep(self.part, src, out=self.work, flags=self.flags, fluid=self.fluid)
            prev = self.work
            if n_iter >= 2:
                prev = B.smooth_residual(self.part, self.work, eps, n_iter - 1, out=self._smooth[0],
                                         tmp=self._smooth[1] if n_iter >= 3 else None)
            if form == "ssp":
                B.update_euler_smoothed(self.part, P0, src, self.work, prev, eps, self.dt, coef, self.fluid, out=out)
            else:   # a forward-Euler step is the stage on the step's input with c = 1: 1 * dt is exact
                B.update_euler_smoothed(self.part, base, None, self.work, prev, eps, self.dt, coef or (1.0,), self.fluid,
                                        out=out)
            return
        if self.residual is not None:
            self.residual(self.part, src, self.work)
            update(self, base, src, self.work, out)
        else:
            fused(self, src, base, out)

    def _tail(self):
        return dict(fluid=self.fluid, scheme=self.scheme, work=self.work, flags=self.flags)


def _stage_calls(form, coef):
    """``(update, fused)`` of a stage of ``form`` with the coefficients ``coef``: ``update(m, base, src, R, out)``, the update
    that follows a residual callable, and ``fused(m, src, base, out)``, the sweep and the update in one call.  ``m`` is the
    march: what else they pass is read from it at the call, and no record holds it -- a march and its arrays go with the
    last reference to it, without waiting for the cycle collector."""
    if form == "step":
        return (lambda m, base, src, R, out: B.update_euler(src, R, m.dt, m.fluid, out=out),
                lambda m, src, base, out: B.step_euler(m.part, src, m.dt, out, **m._tail()))
    if form == "stage":
        return (lambda m, base, src, R, out: B.update_euler_stage(base, R, m.dt, *coef, m.fluid, out=out),
                lambda m, src, base, out: B.stage_euler(m.part, src, base, m.dt, *coef, out, **m._tail()))
    return (lambda m, base, src, R, out: B.update_euler_ssp(base, src, R, m.dt, *coef, m.fluid, out=out),
            lambda m, src, base, out: B.stage_euler_ssp(m.part, src, base, m.dt, *coef, out, **m._tail()))


def bdf_coefficients(order, dt_real):
    """``(cn, cm, g)`` of the backward difference of ``order`` 1 or 2 with the physical step ``dt_real``:
    ``dQ/dt ~ g Q^{n+1} - cn Q^n - cm Q^{n-1}``, BDF2 ``(2, -0.5, 1.5) / dt_real``, BDF1 ``(1, 0, 1) / dt_real``.  Computed in
    float64 and rounded once to Float32 -- the numbers ``dual_source`` and ``stage_euler_dual`` receive -- returned as Python
    floats."""
    if isinstance(order, bool) or order not in (1, 2):
        raise ValueError("bdf_coefficients: order must be 1 or 2")
    dt_real = float(dt_real)
    if not (dt_real > 0.0 and dt_real != float("inf")):
        raise ValueError("bdf_coefficients: dt_real must be positive and finite")
    w = (2.0, -0.5, 1.5) if int(order) == 2 else (1.0, 0.0, 1.0)
    return tuple(float(np.float32(x / dt_real)) for x in w)


def _dual_calls(alpha):
    """``_stage_calls`` of the dual stage; ``S`` and ``g`` -- BDF1 on the first step -- are the march's at the call."""
    return (lambda m, base, src, R, out: B.update_euler_dual(base, R, m.S, m.dt, alpha, m.g, m.fluid, out=out),
            lambda m, src, base, out: B.stage_euler_dual(m.part, src, base, m.S, m.dt, alpha, m.g, out, **m._tail()))


def _sub_into(a, b):
    """``a .-= b`` of two compact device arrays as a libibhip broadcast, in place: no allocation."""
    from .hiparray import HipArray
    ha = HipArray(a)
    ha -= HipArray(b)
    return a


class _Level(EulerMarch):
    """One level of a ``MultigridMarch``: the arrays, the time step and the stage records of an ``EulerMarch`` on the
    level's partition, and beside the records of the steady stages those of the forced ones, ``stage_euler_dual`` with the
    level's forcing ``S`` and ``g`` -- picked per call of ``smooth``; the stage loop is ``EulerMarch._stages`` either way."""

    def __init__(self, part, fluid, scheme, scale, bcs, local_dt, dt_every, flags, stages, roles=None):
        super().__init__(part, fluid, scheme, scale, bcs, None, local_dt, dt_every, None, flags, stages, roles=roles)
        self._plain = self._records
        self._forced = [("dual", "P0", (alpha,)) + _dual_calls(alpha) for alpha in self.stages]
        self.S, self.g = None, 0.0

    def smooth(self, P, n, S, g):
        """``n`` smoothing steps from ``P`` with the forcing ``S`` (None with ``g == 0``: the steady step of ``EulerMarch``);
        returns the last array, ``P`` itself for ``n == 0``.  ``P`` is not written."""
        self.S, self.g = S, g
        self._records = self._plain if S is None else self._forced
        for _ in range(n):
            P = self._stages(P, self.nsteps)
            self.nsteps += 1
        return P


class MultigridMarch:
    """Multigrid for the pseudo-time march of ``EulerMarch``, the fourth acceleration of a Jameson-type steady solver beside
    the per-cell time step, the Runge-Kutta stages and the residual smoothing: a full-approximation-scheme (FAS) V-cycle
    whose smoother on every level is the march's own step and whose transfers work on conserved variables.

    ``parts``: one single-partition ``Partition`` per level (``to_backend(part, hip)``), finest first.  ``coarseners[l]`` /
    ``prolongators[l]`` connect level ``l`` and ``l + 1``: the lists of ``multigrid(dom)``, whose return order is
    ``(coarse_doms, prolongators, coarseners)``.  ``bcs``: None, or one callable per level (None for a level without).
    EVERY level supplied is visited: the quirk of the reference's ``FAS!`` (and of ``solver.FAS``), whose recursion guard
    leaves the last level out, is not copied.

    ``cycle(P, S=None, g=0.0)`` is one V-cycle from level 0 and returns the new fine array.  On level ``l`` with state
    ``P_l`` and forcing ``S_l`` (conserved variables):

    1. ``pre`` smoothing steps, each ``timestep_euler`` on that level (per cell with ``local_dt``; every ``dt_every``-th
       step of the level) and the stages, ``bcs[l]`` after every stage.  With ``S_l is None`` (then ``g == 0``: level 0 of a
       steady run) the stages are ``step_euler`` / ``stage_euler`` and the step is exactly ``EulerMarch``'s; otherwise they
       are ``stage_euler_dual(P, P0, S_l, dt, alpha, g)``, which with ``g = 0`` is the forced Runge-Kutta stage
       ``s2p(p2s(P0) + (R(P) + S_l) h)``.
    2. If there is a coarser level: the sweep ``R(P_l)`` into the level's ``work``; on level 0 the sum of squares of the
       first column of ``work`` -- the density residual ``R`` alone, not ``R + S``, over every row of the array, ghost cells
       included -- goes into the history; ``restrict_euler`` gives ``P_{l+1}^0`` and ``D = I(R + S_l)``; ``bcs[l+1]``
       on ``P_{l+1}^0``; the sweep of ``P_{l+1}^0``; the coarse forcing ``S_{l+1} = D - R_{l+1}(P_{l+1}^0)`` in place in
       ``D``; the recursion from ``P_{l+1}^0``, which is an array of its own that no step writes; ``prolong_euler(P_l,
       P_{l+1}, P_{l+1}^0)`` into the level's next free ping-pong array; ``bcs[l]``.
    3. ``post`` smoothing steps.  The coarsest level runs ``n_coarsest`` steps and no transfers -- with one level a cycle is
       ``n_coarsest`` steps of ``EulerMarch``.

    ``S`` and ``g`` on level 0 make the cycle the solver of a backward-difference step of a dual time march, ``g Q = R(P) +
    S`` (``dual_source``, ``bdf_coefficients``): ``g`` goes to every level unchanged and the ``g Q`` terms cancel in the coarse
    forcing, because ``P_{l+1}^0`` is the restriction of ``P_l`` and the restriction is linear.  ``g > 0`` needs ``S``.

    ``history=n``: ``n`` device doubles, NaN until written; cycle ``k < n`` writes entry ``k`` (``ibh_sumsq``, which assigns:
    nothing to zero).  ``residual_history()`` is the only read-back and ``cycle`` never calls it.  Everything is allocated
    here; ``cycle`` makes no host read-back and no allocation, so it can be captured in ``torch.cuda.graph`` (run one eager
    cycle first: the library's workspaces come with their first use).  The returned array is one of level 0's ping-pong
    arrays: valid during the next cycle's first step, overwritten later.

    ``roles``: None, or one ``backend.Roles`` per level, each from ``cell_roles`` of that level's own domain.  The cycle
    then knows what every row is: every level's steps blank the solid rows as ``EulerMarch`` does, and so do the two other
    places a state is made -- ``P_{l+1}^0`` after its ``bcs`` and the prolonged array after its ``bcs``; the restriction is
    ``restrict_euler(..., roles=...)``, whose defect takes fluid rows only; the coarse forcing is ``forcing_roles`` with the
    coarse roles, zero outside the fluid rows; and entry ``k`` of the history becomes the ``nd + 2`` sums of squares of
    ``sumsq_roles`` over the fluid rows of level 0's ``work``: ``residual_history()`` is ``(history, nd + 2)``.  Without
    ``roles`` every call and the history's shape are as above.

    Not taken, each with a message: ``smoothing`` (``update_euler_smoothed`` has no source row), Shu-Osher triples (as in
    ``DualTimeMarch``), a ``residual`` callable, the image-only, phase and single-pass ``flags``, a ``TimeAverage``."""

    def __init__(self, parts, coarseners=(), prolongators=(), fluid=None, scheme="hll", scale=0.75, bcs=None, local_dt=True,
                 dt_every=1, stages=1, pre=1, post=1, n_coarsest=2, flags=0, history=0, smoothing=None, residual=None,
                 average=None, roles=None):
        from . import cfd
        parts = list(parts)
        if roles is not None:
            roles = list(roles)
            if len(roles) != len(parts):
                raise ValueError(f"MultigridMarch: roles is None or one Roles per level: {len(parts)} levels, {len(roles)} "
                                 "roles")
            if not all(isinstance(r, B.Roles) for r in roles):
                raise ValueError("MultigridMarch: every entry of roles must be a backend.Roles of its level")
        if smoothing is not None:
            raise ValueError("MultigridMarch: residual smoothing is not taken: update_euler_smoothed has no source row for the "
                             "coarse forcing")
        if isinstance(stages, (tuple, list)) and any(isinstance(a, (tuple, list)) for a in stages):
            raise ValueError("MultigridMarch: stages are rk_stages(m) or plain coefficients; Shu-Osher triples are not taken")
        if residual is not None:
            raise ValueError("MultigridMarch: a residual callable is not taken: the levels sweep with the library's schemes")
        if average is not None:
            raise ValueError("MultigridMarch: a TimeAverage is not taken: the cycle marches in pseudo-time")
        flags = int(flags)
        if flags & (B.IBH_IMAGE_ONLY | B.IBH_PHASE_INTERIOR | B.IBH_PHASE_BOUNDARY | B.IBH_PASS_A_ONLY | B.IBH_PASS_B_ONLY):
            raise ValueError("MultigridMarch: IBH_IMAGE_ONLY, the overlap phases and the single-pass flags are not taken: the "
                             "restriction reads the residual of every cell")
        parts = [B.to_backend(p) for p in parts]
        if not parts:
            raise ValueError("MultigridMarch: at least one level")
        coarseners, prolongators = list(coarseners), list(prolongators)
        if len(coarseners) != len(parts) - 1 or len(prolongators) != len(parts) - 1:
            raise ValueError(f"MultigridMarch: {len(parts)} levels take {len(parts) - 1} coarseners and as many prolongators")
        if bcs is None:
            bcs = [None] * len(parts)
        bcs = list(bcs)
        if len(bcs) != len(parts):
            raise ValueError("MultigridMarch: bcs is None or one callable per level")
        for name, v in (("pre", pre), ("post", post), ("n_coarsest", n_coarsest), ("history", history)):
            if isinstance(v, bool) or int(v) != v or int(v) < 0:
                raise ValueError(f"MultigridMarch: {name} must be an integer >= 0")
        self.pre, self.post, self.n_coarsest = int(pre), int(post), int(n_coarsest)
        self.fluid = fluid if fluid is not None else cfd.Fluid()
        if roles is None:
            roles = [None] * len(parts)
        self.levels = [_Level(p, self.fluid, scheme, scale, b, local_dt, dt_every, flags, stages, r)
                       for p, b, r in zip(parts, bcs, roles)]
        for l, m in enumerate(self.levels):
            host = getattr(m.part, "host", None)
            if host is not None and (len(host.image) != m.part.nc or len(host.domain) != m.part.nc):
                raise ValueError(f"MultigridMarch: level {l} is not a single partition: {len(host.image)} of its "
                                 f"{m.part.nc} cells are its own")
        self.coarseners = [B._transfer("MultigridMarch", a) for a in coarseners]
        self.prolongators = [B._transfer("MultigridMarch", a) for a in prolongators]
        for l, (c, p) in enumerate(zip(self.coarseners, self.prolongators)):
            nf, nk = self.levels[l].part.nc, self.levels[l + 1].part.nc
            if (c.n_input, c.n_output) != (nf, nk) or (p.n_input, p.n_output) != (nk, nf):
                raise ValueError(f"MultigridMarch: levels {l} and {l + 1} have {nf} and {nk} cells; coarseners[{l}] maps "
                                 f"{c.n_input} -> {c.n_output} and prolongators[{l}] {p.n_input} -> {p.n_output} (multigrid(dom) "
                                 "returns (coarse_doms, prolongators, coarseners))")
        for m in self.levels[1:]:
            nc, nv = m.part.nc, m.part.nd + 2
            m.P0, m.D = B.colmajor_empty(nc, nv), B.colmajor_empty(nc, nv)
            m.pack = torch.empty(8 * max(nc, 1), dtype=torch.float32, device=m.work.device)
        self._hist = None
        if int(history):
            shape = (int(history),) if roles[0] is None else (int(history), self.levels[0].part.nd + 2)
            self._hist = torch.full(shape, float("nan"), dtype=torch.float64, device=self.levels[0].work.device)
        self.ncycles = 0

    def cycle(self, P, S=None, g=0.0):
        """One V-cycle from ``P`` (any ``(nc, nd+2)`` device array of level 0, e.g. the previous return value), with the
        level-0 forcing ``S`` (conserved variables) and ``g`` of a backward-difference step; returns the new fine array."""
        if not isinstance(P, torch.Tensor):
            P = P.t
        if S is not None and not isinstance(S, torch.Tensor):
            S = S.t
        g = B._dual_g("MultigridMarch.cycle", g)
        if S is None and g != 0.0:
            raise ValueError("MultigridMarch.cycle: g > 0 needs the source S of the physical step")
        P = self._level(0, P, S, g)
        self.ncycles += 1
        return P

    def _level(self, l, P, S, g):
        m = self.levels[l]
        if l == len(self.levels) - 1:
            return m.smooth(P, self.n_coarsest, S, g)
        P = m.smooth(P, self.pre, S, g)
        m.sweep(P)
        if l == 0 and self._hist is not None and self.ncycles < self._hist.shape[0]:
            if m.roles is not None:
                B.sumsq_roles(m.work, m.roles, out=self._hist[self.ncycles])
            else:
                B._stream()
                B.call("ibh_sumsq", m.part.nc, B._ptr(m.work), B._ptr(self._hist[self.ncycles:]))
        c = self.levels[l + 1]
        B.restrict_euler(self.coarseners[l], P, m.work, S, self.fluid, out=c.P0, out_D=c.D, roles=m.roles)
        if c.bcs is not None:
            c.bcs(c.P0)
        if c.roles is not None:
            c.roles.blank(c.P0)
        c.sweep(c.P0)
        if c.roles is not None:
            B.forcing_roles(c.D, c.work, c.roles)
        else:
            _sub_into(c.D, c.work)
        Pc = self._level(l + 1, c.P0, c.D, g)
        out = next(b for b in m._buf if b.data_ptr() != P.data_ptr())
        B.prolong_euler(self.prolongators[l], P, Pc, c.P0, self.fluid, out=out, pack=c.pack)
        if m.bcs is not None:
            m.bcs(out)
        if m.roles is not None:
            m.roles.blank(out)
        return m.smooth(out, self.post, S, g)

    def residual_history(self):
        """The history as a host array of ``history`` doubles: entry ``k`` is the sum of squares of the density residual that
        cycle ``k`` restricted, NaN where no cycle has written; with ``roles`` ``(history, nd + 2)``: the sums over the fluid
        rows of every column of that residual.  The one read-back of the class."""
        if self._hist is None:
            return np.zeros(0 if self.levels[0].roles is None else (0, self.levels[0].part.nd + 2), dtype=np.float64)
        return self._hist.cpu().numpy()


class DualTimeMarch(EulerMarch):
    """Dual time stepping: an implicit, time-accurate march whose every physical step of size ``dt_real`` is solved by the
    pseudo-time march of ``EulerMarch`` -- per-cell pseudo-time steps and Runge-Kutta stages included -- so that the physical
    step is not bound by the CFL limit of the smallest cell.  With ``dQ/dt = R(P)``, ``Q = primitive2state(P)``, a step solves

        g Q^{n+1} = R(P^{n+1}) + S,      S = cn Q^n + cm Q^{n-1}          (``bdf_coefficients``: BDF2, the first step BDF1)

    by ``n_inner`` pseudo-steps from ``P^n``, each one ``timestep_euler`` (on every ``dt_every``-th pseudo-step of the
    physical step, into the pseudo-time step ``dtau``, per cell with ``local_dt``) and the stages

        P_k = state2primitive((primitive2state(P_0) + (R(P_{k-1}) + S) * h) / (1 + h * g)),      h = alpha_k * dtau

    -- ``stage_euler_dual(P_{k-1}, P_0, S, dtau, alpha_k, g)``, one launch where the 2-D single-kernel sweep applies; with
    ``residual``: the callable into ``work``, then ``update_euler_dual`` -- with ``bcs`` after every stage.  The ``g Q`` term
    is point-implicit (Melson, Sanetrik and Atkins), so ``dtau`` is bound by the explicit scheme alone, and the fixed point
    is the backward-difference equation whatever ``dtau`` and the stages are.  ``step(P)`` is

    1. ``dual_source`` from ``P`` and the state the previous ``step`` started from, into ``S``,
    2. the ``n_inner`` pseudo-steps,
    3. ``average.push(P_new, dt_real)`` with the host number: the march is time accurate in ``dt_real``, a time average is
       legal here with ``local_dt``.

    ``stages``: ``m`` (``rk_stages(m)``) or the tuple of coefficients.  Shu-Osher triples raise, and so does ``smoothing``:
    a smoothed residual moves the fixed point to ``smooth(R) + S = g Q``, which is not the backward-difference equation.

    Everything is allocated here: ``S``, the ping-pong arrays of the stages and four arrays for the history.  ``step``
    returns one of those four; it stays valid during the next ``step`` and is overwritten by a later one.  An array that
    the march did not return (the caller's, on the first step) is copied into the history once and never written.  No host
    read-back in ``step``: it can be captured in ``torch.cuda.graph`` and replayed (the replay reads the history arrays the
    capture saw: it continues the march once; to repeat it, restore them).  ``n_inner`` is fixed: a stopping criterion would
    need a read-back.  ``roles``: as in ``EulerMarch`` -- the solid rows are blanked after every stage's ``bcs``."""

    def __init__(self, part, dt_real, n_inner, order=2, fluid=None, scheme="hll", scale=0.75, bcs=None, average=None,
                 local_dt=True, dt_every=1, residual=None, flags=0, stages=1, smoothing=None, roles=None):
        later = bdf_coefficients(order, dt_real)
        self._bdf = {int(order): later, 1: bdf_coefficients(1, dt_real)}        # (the first step is BDF1)
        if isinstance(n_inner, bool) or int(n_inner) != n_inner or int(n_inner) < 1:
            raise ValueError("DualTimeMarch: n_inner must be an integer >= 1")
        if smoothing is not None:
            raise ValueError("DualTimeMarch: residual smoothing is not taken: the smoothed residual changes the fixed point of "
                             "the inner iterations to smooth(R) + S = g Q, which is not the backward-difference equation")
        if isinstance(stages, (tuple, list)) and any(isinstance(a, (tuple, list)) for a in stages):
            raise ValueError("DualTimeMarch: stages are rk_stages(m) or plain coefficients; Shu-Osher triples are not taken")
        super().__init__(part, fluid, scheme, scale, bcs, None, local_dt, dt_every, residual, flags, stages, roles=roles)
        self.average, self.dt_real, self.n_inner, self.order = average, dt_real, int(n_inner), int(order)
        self._records = [("dual", "P0", (alpha,)) + _dual_calls(alpha) for alpha in self.stages]
        nc, nv = self.part.nc, self.part.nd + 2
        self.S, self.g = B.colmajor_empty(nc, nv), 0.0
        self._hist = tuple(B.colmajor_empty(nc, nv) for _ in range(4))
        self._prev = self._last = None        # the state the previous step started from; the array it returned

    def step(self, P):
        """One physical step from ``P`` (any ``(nc, nd+2)`` device array, e.g. the previous return value); returns the new
        array."""
        if not isinstance(P, torch.Tensor):
            P = P.t
        held = [h.data_ptr() for h in (self._prev, self._last) if h is not None]
        if P.data_ptr() not in [h.data_ptr() for h in self._hist]:      # not ours: it may change under us before the next step
            cur = next(h for h in self._hist if h.data_ptr() not in held)
            cur.copy_(B._primitives(P, self.part.nc, self.part.nd)[0])
        else:
            cur = P
        new = next(h for h in self._hist if h.data_ptr() not in held + [cur.data_ptr()])
        cn, cm, self.g = self._bdf[1 if self._prev is None else self.order]
        B.dual_source(cur, self._prev if self.order == 2 else None, cn, cm, self.fluid, out=self.S)
        src = cur
        for k in range(self.n_inner):
            src = self._stages(src, k, new if k == self.n_inner - 1 else None)
        self._prev, self._last = cur, src
        if self.average is not None:
            self.average.push(src, self.dt_real)
        self.nsteps += 1
        return src

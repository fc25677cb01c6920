"""numpy model of multigrid for the Euler march (``ibh_restrict_euler``, ``ibh_prolong_euler``, ``solver.MultigridMarch``), on
the oracle's operators (imported, not edited) and the pieces of ``euler_step_model`` / ``euler_dual_model``.

Transfers, in conserved variables ``Q = primitive2state(P)`` with ``I`` the coarsener and ``J`` the prolongator of
``multigrid(dom)`` -- a stencil sum is ``t = x * w`` per entry, started from the first entry and added in entry order, the
kernels' rounding order, in Float32 or with the same structure in float64:

    restrict:   P_c = state2primitive(I(Q_f))           D_c = I(R_f + S_f)            (R + S rounded before the multiply)
    forcing:    S_c = D_c - R_c(P_c)
    prolong:    P_f' = state2primitive(Q_f + J(primitive2state(Pc_new) - primitive2state(Pc_old)))

The cycle of level ``l`` (``cycle``): ``pre`` smoothing steps -- the per-cell time step from the step's input, then the stages
``P_k = state2primitive((primitive2state(P_0) + (R(P_{k-1}) + S) h) / (1 + h g))``, ``h = alpha_k dt``, boundary conditions
after every stage; without a forcing ``S`` the stage is the plain one -- then the sweep, the restriction, the coarse boundary
conditions, the coarse sweep, the forcing, the recursion from the restricted state, the prolongation, the boundary
conditions and ``post`` steps; the coarsest level runs ``n_coarsest`` steps.  Every level supplied is visited.

With ``S_f`` the forcing and ``g Q`` the point-implicit term of a backward-difference step, the forcing of the residual
``R + S - g Q`` would be ``I(R_f + S_f - g Q_f) - (R_c - g Q_c)``; because ``Q_c = I(Q_f)`` and ``I`` is linear the ``g`` terms
cancel and it is ``D_c - R_c``: ``g`` goes to every level unchanged and never enters a transfer.
"""
import types

import numpy as np

import euler_dual_model as dm
import euler_stage_model as sm
import euler_step_model as em
import percell as pc
from oracle import cfd as ocfd

f32, f64 = np.float32, np.float64


def corner_mesh():
    """The ``corner`` mesh of tests/test_gpu_percell_regimes.py: a 4^3 box of 8^3 blocks with one refined corner."""
    from ibamd.mesher import Ball, Mesh
    return Mesh(f32([-2, -2, -2]), f32([4, 4, 4]), block_size=8,
                refinement_regions=[(Ball(np.array([-2.0, -2.0, -2.0]), 0.1), f32(0.1))])


def hierarchy(mesh, max_levels, **domain_kw):
    """``(doms, coarseners, prolongators)``: the mesh as one partition and the ``max_levels`` coarser domains of
    ``multigrid``, finest first, with the operators between consecutive levels."""
    import ibamd
    dom = ibamd.Domain(mesh, max_partition_size=10 ** 9, **domain_kw)
    coarse, prolongators, coarseners = ibamd.multigrid(dom, max_levels=max_levels)
    doms = [dom] + list(coarse)
    assert all(len(d.partitions) == 1 for d in doms)
    return doms, coarseners, prolongators


def part_of(dom):
    (part,) = dom.partitions.values()
    return part


def apply(acc, X, dtype=f32):
    """``acc(X)`` per column in the kernels' order: per row ``t = x * w`` entry by entry, the first one assigned, the others
    added in entry order.  ``acc``: a host ``Accumulator`` (CSR); rows without entries give zeros."""
    X = np.asarray(X).astype(dtype)
    out = np.zeros((acc.n_output,) + X.shape[1:], dtype)
    for length, (rows, idx, w) in acc.stencils.items():
        if length == 0:
            continue
        s = None
        for k in range(length):
            t = X[idx[k]]
            if w is not None:
                t = t * w[k].astype(dtype).reshape((-1,) + (1,) * (X.ndim - 1))
            s = t if s is None else s + t
        out[rows] = s
    assert out.dtype == dtype
    return out


def restrict(coarsener, P, R, S=None, dtype=f32):
    """(P_c, D_c) of the restriction."""
    fl = em.fluid_of(dtype)
    P, R = np.asarray(P).astype(dtype), np.asarray(R).astype(dtype)
    with np.errstate(all="ignore"):
        Pc = ocfd.state2primitive(fl, apply(coarsener, ocfd.primitive2state(fl, P), dtype))
        D = apply(coarsener, R if S is None else R + np.asarray(S).astype(dtype), dtype)
    assert Pc.dtype == dtype and D.dtype == dtype
    return Pc, D


def prolong(prolongator, P, Pc_new, Pc_old, dtype=f32):
    """The fine state corrected by the change of the coarse one."""
    fl = em.fluid_of(dtype)
    P, Pc_new, Pc_old = (np.asarray(x).astype(dtype) for x in (P, Pc_new, Pc_old))
    with np.errstate(all="ignore"):
        d = ocfd.primitive2state(fl, Pc_new) - ocfd.primitive2state(fl, Pc_old)
        out = ocfd.state2primitive(fl, ocfd.primitive2state(fl, P) + apply(prolongator, d, dtype))
    assert out.dtype == dtype
    return out


def level(op, bcs=None):
    """One level of the model: ``op`` an oracle view of its partition (``conftest.oracle_view``), ``bcs(P)`` in place or
    None."""
    return types.SimpleNamespace(op=op, bcs=bcs)


def residual(lv, P, dtype):
    return pc.oracle_euler_residual(lv.op, np.ascontiguousarray(P).astype(dtype), em.fluid_of(dtype))


def smooth(lv, P, S, g, stages, scale, dtype, count=None):
    """One smoothing step from ``P``: the per-cell time step, then the stages, ``bcs`` after every one.  ``count``: a dict
    whose ``sweeps`` grows by the level's cell count per sweep."""
    _, dt = em.timestep(lv.op, P, scale, dtype)
    P0 = src = np.asarray(P).astype(dtype)
    for alpha in stages:
        R = residual(lv, src, dtype)
        if count is not None:
            count["sweeps"] += R.shape[0]
        src = sm.update_stage(P0, R, dt, alpha, dtype) if S is None else dm.update_dual(P0, R, S, dt, alpha, g, dtype)
        if lv.bcs is not None:
            lv.bcs(src)
    return src


def cycle(levels, coarseners, prolongators, P, S=None, g=0.0, stages=(1.0,), scale=0.75, pre=1, post=1, n_coarsest=2,
          dtype=f32, l=0, count=None, history=None):
    """One V-cycle from level ``l``; returns the new state of that level.  ``history``: a list that receives the sum of
    squares of the density residual level 0 restricts."""
    lv = levels[l]
    P = np.asarray(P).astype(dtype)
    kw = dict(stages=stages, scale=scale, pre=pre, post=post, n_coarsest=n_coarsest, dtype=dtype, count=count)
    if l == len(levels) - 1:
        for _ in range(n_coarsest):
            P = smooth(lv, P, S, g, stages, scale, dtype, count)
        return P
    for _ in range(pre):
        P = smooth(lv, P, S, g, stages, scale, dtype, count)
    R = residual(lv, P, dtype)
    if count is not None:
        count["sweeps"] += R.shape[0]
    if l == 0 and history is not None:
        history.append(float((R[:, 0].astype(f64) ** 2).sum()))
    c = levels[l + 1]
    Pc0, D = restrict(coarseners[l], P, R, S, dtype)
    if c.bcs is not None:
        c.bcs(Pc0)
    Rc = residual(c, Pc0, dtype)
    if count is not None:
        count["sweeps"] += Rc.shape[0]
    Pc = cycle(levels, coarseners, prolongators, Pc0, D - Rc, g, l=l + 1, **kw)
    P = prolong(prolongators[l], P, Pc, Pc0, dtype)
    if lv.bcs is not None:
        lv.bcs(P)
    for _ in range(post):
        P = smooth(lv, P, S, g, stages, scale, dtype, count)
    return P


def round_trips(n_levels, n_stages, pre, post, n_coarsest):
    """The number of primitive <-> conserved round trips one V-cycle puts a fine value through: one per stage of every
    smoothing step on every level -- a coarse level's reach the fine state through the prolongation -- and one per
    prolongation."""
    return n_stages * ((pre + post) * (n_levels - 1) + n_coarsest) + (n_levels - 1)


def round_trip_error(P, dtype=f32):
    """``e_v = max |state2primitive(primitive2state(P)) - P|`` per column: what one round trip moves a state by."""
    fl = em.fluid_of(dtype)
    P = np.asarray(P).astype(dtype)
    back = ocfd.state2primitive(fl, ocfd.primitive2state(fl, P))
    return np.abs(back.astype(f64) - P.astype(f64)).max(axis=0)

"""numpy model of cell roles in the Euler march (``ibamd.cell_roles``, ``ibh_restrict_euler_roles``, ``ibh_forcing_roles``,
``ibh_sumsq_roles``, ``solver.EulerMarch(roles=...)`` / ``MultigridMarch(roles=...)``), on the multigrid model
``euler_mg_model`` (imported, not edited).  It is the definition the kernels are held to.

A role says what a row IS: ``FLUID`` (0), ``GHOST`` (1: a ghost cell of any boundary) or ``SOLID`` (2: a cell the ghost layer
cuts off from the fluid -- the inside of a body, which the reference lets march a flow of its own).  With ``f`` the rows whose
role is ``FLUID``, ``I`` the coarsener and the stencil arithmetic of ``euler_mg_model.apply``:

    restrict:   P_c = state2primitive(I(Q_f))               (unchanged: a masked row's state is restricted like any other)
                D_c = I(t),  t = R_f + S_f in f, +0 elsewhere   (a select: a NaN in a masked row never reaches D_c)
    forcing:    S_c = D_c - R_c(P_c) in the coarse level's f, +0 elsewhere
    blank:      P[solid rows] = solid_state                  (after the boundary conditions, wherever a state is made)
    norm:       sum over f of R[:, v]^2, per column, in float64

The cycle (``cycle``) is ``euler_mg_model.cycle`` with those four: every smoothing stage blanks after its boundary
conditions, the restricted state and the prolonged state are blanked after theirs, the defect and the forcing are masked,
and the history takes the fluid rows.  The roles of a coarse level are those of its own domain, not restricted ones.
"""
import numpy as np

import euler_mg_model as mg

f32, f64 = np.float32, np.float64
FLUID, GHOST, SOLID = 0, 1, 2


def cell_roles(dom, fluid_seed=None):
    """``uint8[len(dom)]`` in global cell order: ghost rows from every boundary's ``ghost_indices``; a flood through the faces
    of every partition (a mirror face, owner == neighbour, connects nothing) that never enters a ghost row; the component
    of ``fluid_seed`` -- by default the largest one -- is fluid, every other row solid.  Frontier sweeps: the flood grows by
    one ring of face neighbours per sweep."""
    n = len(dom)
    ghost = np.zeros(n, bool)
    for parts in dom.boundaries.values():
        for b in parts.values():
            ghost[b.ghost_indices] = True
    a, b = [], []
    for part in dom.partitions.values():
        g = np.asarray(part.domain)
        for o, nb in part.face_owners_neighbors.values():
            a.append(g[o])
            b.append(g[nb])
    a, b = np.concatenate(a), np.concatenate(b)
    keep = ~ghost[a] & ~ghost[b] & (a != b)
    a, b = a[keep], b[keep]
    comp = np.full(n, -1, np.int64)
    sizes = []
    for start in range(n):
        if ghost[start] or comp[start] >= 0:
            continue
        k = len(sizes)
        comp[start] = k
        count, grew = 1, True
        while grew:
            reach = np.concatenate([b[(comp[a] == k) & (comp[b] < 0)], a[(comp[b] == k) & (comp[a] < 0)]])
            reach = np.unique(reach)
            comp[reach] = k
            count += reach.size
            grew = reach.size > 0
        sizes.append(count)
    roles = np.where(ghost, GHOST, SOLID).astype(np.uint8)
    if sizes:
        k = int(np.argmax(sizes)) if fluid_seed is None else int(comp[fluid_seed])
        assert k >= 0, "the seed is a ghost row"
        roles[comp == k] = FLUID
    return roles


def mask(X, roles, dtype=f32):
    """``X`` in fluid rows, ``+0`` elsewhere: a select."""
    X = np.asarray(X).astype(dtype)
    return np.where((np.asarray(roles) == FLUID).reshape((-1,) + (1,) * (X.ndim - 1)), X, dtype(0))


def restrict(coarsener, P, R, S=None, roles=None, dtype=f32):
    """(P_c, D_c) of the restriction with the fine level's roles."""
    P, R = np.asarray(P).astype(dtype), np.asarray(R).astype(dtype)
    with np.errstate(all="ignore"):
        t = R if S is None else R + np.asarray(S).astype(dtype)
    Pc, _ = mg.restrict(coarsener, P, np.zeros_like(R), None, dtype)
    D = mg.apply(coarsener, mask(t, roles, dtype), dtype)
    assert Pc.dtype == dtype and D.dtype == dtype
    return Pc, D


def forcing(D, Rc, roles, dtype=f32):
    """The coarse forcing with the coarse level's roles."""
    with np.errstate(all="ignore"):
        return mask(np.asarray(D).astype(dtype) - np.asarray(Rc).astype(dtype), roles, dtype)


def sumsq(X, roles):
    """Per column, the sum of squares over the fluid rows in float64."""
    X = np.asarray(X)
    X = X.reshape(X.shape[0], -1)
    return (X[np.asarray(roles) == FLUID].astype(f64) ** 2).sum(axis=0)


def blank(P, roles, solid_state):
    """``solid_state`` into the solid rows of ``P``, in place; returns ``P``."""
    P[np.asarray(roles) == SOLID] = np.asarray(solid_state, dtype=P.dtype)
    return P


def level(op, bcs=None, roles=None, solid_state=None):
    """A level of the model with roles: ``euler_mg_model.level`` whose boundary conditions are followed by the blank, so
    that every stage of ``euler_mg_model.smooth`` blanks after its ``bcs``."""
    def after(P):
        if bcs is not None:
            bcs(P)
        if roles is not None:
            blank(P, roles, solid_state)
    lv = mg.level(op, after)
    lv.roles, lv.solid_state = roles, solid_state
    return lv


def cycle(levels, coarseners, prolongators, P, S=None, g=0.0, stages=(1.0,), scale=0.75, pre=1, post=1, n_coarsest=2,
          dtype=f32, l=0, count=None, history=None):
    """One V-cycle from level ``l`` of levels made by ``level`` (all with roles); returns the new state of that level.
    ``history``: a list that receives the ``nd + 2`` sums of squares over the fluid rows of the residual level 0 restricts."""
    lv = levels[l]
    P = np.asarray(P).astype(dtype)
    kw = dict(stages=stages, scale=scale, pre=pre, post=post, n_coarsest=n_coarsest, dtype=dtype, count=count)
    if l == len(levels) - 1:
        for _ in range(n_coarsest):
            P = mg.smooth(lv, P, S, g, stages, scale, dtype, count)
        return P
    for _ in range(pre):
        P = mg.smooth(lv, P, S, g, stages, scale, dtype, count)
    R = mg.residual(lv, P, dtype)
    if count is not None:
        count["sweeps"] += R.shape[0]
    if l == 0 and history is not None:
        history.append(sumsq(R, lv.roles))
    c = levels[l + 1]
    Pc0, D = restrict(coarseners[l], P, R, S, lv.roles, dtype)
    c.bcs(Pc0)                                       # (the coarse boundary conditions, then the coarse blank)
    Rc = mg.residual(c, Pc0, dtype)
    if count is not None:
        count["sweeps"] += Rc.shape[0]
    Pc = cycle(levels, coarseners, prolongators, Pc0, forcing(D, Rc, c.roles, dtype), g, l=l + 1, **kw)
    P = mg.prolong(prolongators[l], P, Pc, Pc0, dtype)
    lv.bcs(P)
    for _ in range(post):
        P = mg.smooth(lv, P, S, g, stages, scale, dtype, count)
    return P

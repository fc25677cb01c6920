"""Per-element checks of the kernels a solver step runs around the sweep, against float64 statements of the reference.

Test infrastructure in the style of tests/percell.py (whose ``percell_error``, ``nan_pattern_mismatch``, ``report`` and
``to64`` are used here).  Every reference is plain numpy in float64 of the reference's formula and never calls the product;
every scale is |ref| plus the same chain evaluated on magnitudes; every check first requires the NaN
pattern of the result to equal the reference's.

Families and bounds (tests/test_percell_steps.py calibrates the Float32 numpy oracle against the float64 reference and
requires it to stay at or below half of each bound; it prints the maxima quoted here):

- Accumulator application (``k_accumulate``, ``k_accumulate_rows<4|8>`` and its ADD form, ``k_pack_diff8`` +
  ``k_accumulate_packed_add<2..8>``, the ``remap`` gather of ``ibh_bc_interp``): ``BOUND_ACC`` = ``percell.BOUND_OPS`` = 1e-6.
  Float32 oracle: 1.1e-7 on the synthetic accumulators (rows of up to 12 entries), 9.9e-8 with ``diff`` and ``add``.
- Boundary conditions (sequential ``impose_bc!``): ``BOUND_BC`` = 1e-6.  The oracle's ``impose_bc``: 1.1e-7 on the
  synthetic sets, 6.9e-8 on the advection case; device 4.8e-7 (synthetic sets), 2.4e-7 (``BCSet.apply``), 1.7e-7 (``bc_apply``).
- Block apply (``k_apply_blocks<M>``, ``k_mul``): ``BOUND_APPLY`` = 1e-6.  Float32 oracle: 8.5e-8 (M = 2..8).
- Pseudo-inverse (``k_pinv_blocks<M>``): max |got - ref| / max |ref| per block, binned by the decade of sigma_max /
  sigma_min.  The bound cannot be derived, so it is measured: 4 x the worst error of a Float32 LAPACK pinv with the
  cut-off of oracle/point_implicit.py in that bin (``PINV_LAPACK``, M = 2..8, n = 65 and 1000, from test_calibration_pinv,
  which fails if LAPACK measures above the table or below a third of it; see ``pinv_lapack32`` for why the SVD is
  scipy's sgesdd and not ``numpy.linalg.pinv``).  One-sided Jacobi is a different algorithm of comparable backward error; the
  factor covers the difference in the last sweep's convergence test.  Device maxima measured on an MI355X: ``PINV_DEVICE``.
  Other device maxima (MI355X): accumulate 1.1e-7, transfer operators 1.4e-7, ``bc_interp`` 8.9e-8, ``diff_add`` 1.4e-7,
  block apply 9.7e-8, sums 2.2e-16 of sum |t|, element-wise 7.7e-8, time step 1.1e-7 relative.
- Element-wise kernels: 2 ulp of the magnitude scale (``BOUND_EW``).
- Sums (``ibh_sumsq``, ``ibh_dot``, the norm halves): 1e-13 x sum |t_i| against ``math.fsum`` (``BOUND_SUM``): a product of
  two floats is exact in double, a term passes through fewer than 100 additions (thread stride, wave shuffle, four waves,
  partials stride, tree), 100 x 2^-53 = 1.1e-14, times 10.
- Float32 sum of ``ibh_ew_reduce``: D x 2^-24 x sum |a_i| against ``math.fsum`` (``check_sum32``), D = ``ew_sum_depth`` the
  number of additions a term passes through.  The Float32 model of the same order measures 0.06 of the bound at most.
- Time step: relative 4 ulp (``BOUND_DT``): one face average, one sum and two divisions; the maximum itself is exact.
"""
import math

import numpy as np

import percell as pc
from percell import f32, f64, nan_pattern_mismatch, percell_error, to64  # noqa: F401

ULP = 2.0 ** -23                 # Float32 spacing relative to the magnitude
BOUND_ACC = pc.BOUND_OPS
BOUND_BC = pc.BOUND_OPS
BOUND_APPLY = pc.BOUND_OPS
BOUND_EW = 2 * ULP
BOUND_SUM = 1e-13
BOUND_DT = 4 * ULP
EPS32 = float(np.finfo(f32).eps)

# Worst error of the Float32 LAPACK pinv (oracle/point_implicit.py) per bin: decade d holds the full-rank blocks with
# 10^d <= sigma_max / sigma_min < 10^(d+1) (d = 0, 1, 2), "deficient" the exactly rank-deficient ones.
PINV_LAPACK = {0: 1.3e-6, 1: 1.1e-5, 2: 1.2e-4, "deficient": 2.6e-5}   # measured 1.21e-6, 1.08e-5, 1.19e-4, 2.58e-5
PINV_BOUND = {k: 4 * v for k, v in PINV_LAPACK.items()}
# measured maxima of k_pinv_blocks<2..8> on an MI355X (tests/test_gpu_percell_steps.py prints them)
PINV_DEVICE = {0: 7.5e-7, 1: 3.0e-6, 2: 3.2e-5, "deficient": 2.9e-5}

REDUCTION_SIZES = (1, 63, 64, 65, 255, 256, 257, 1000, 256 * 1024 + 1, 256 * 2048 + 3)
ROW_LENGTHS = (0, 1, 3, 4, 5, 7, 8, 9, 12)


def check(got, ref, scale, bound, what=""):
    """NaN pattern first, then max |got - ref| / scale <= bound over the other entries (equal infinities are exact);
    returns the maximum."""
    g, r = np.asarray(got, dtype=f64), np.asarray(ref, dtype=f64)
    assert g.shape == r.shape, (what, g.shape, r.shape)
    bad = nan_pattern_mismatch(g, r)
    if bad.any():
        i = tuple(int(k[0]) for k in np.nonzero(bad))
        raise AssertionError(f"{what}: NaN pattern differs on {int(bad.sum())} entries; first {i}: got {g[i]}, ref {r[i]}")
    skip = np.isnan(r) | (np.isinf(r) & (g == r))
    e = np.where(skip, 0.0, percell_error(np.where(skip, 0.0, g), np.where(skip, 0.0, r),
                                          np.where(skip, 1.0, np.broadcast_to(np.asarray(scale, f64), r.shape))))
    worst = float(e.max()) if e.size else 0.0
    if not worst <= bound:
        i = np.unravel_index(int(np.argmax(e)), e.shape) if e.ndim else ()
        s = np.broadcast_to(np.asarray(scale, f64), r.shape)
        raise AssertionError(f"{what}: error {worst:.3e} > bound {bound:.3e} at {tuple(int(k) for k in i)}: got {g[i]!r}, "
                             f"ref {r[i]!r}, scale {s[i]:.3g}; {int((e > bound).sum())} entries above the bound")
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# 1. Accumulator family
# ---------------------------------------------------------------------------------------------------------------------
def synthetic_csr(n_out, n_in, seed=0, weighted=True):
    """(off, idx, w): rows whose lengths run through ``ROW_LENGTHS`` in an order that starts rows of every length at every
    residue of ``off % 4`` (a seeded shuffle; ``assert_paths_covered`` checks it for n_out >= 255)."""
    rng = np.random.default_rng(seed)
    if n_out == 1:
        ls = np.array([8])
    else:
        # at every row: a length seen least often at the current residue (ties at random), so that the 9 x 4
        # combinations fill evenly
        seen = np.zeros((len(ROW_LENGTHS), 4), np.int64)
        ls, b = np.empty(n_out, np.int64), 0
        for r in range(n_out):
            c = seen[:, b & 3]
            k = rng.choice(np.nonzero(c == c.min())[0])
            seen[k, b & 3] += 1
            ls[r] = ROW_LENGTHS[k]
            b += ls[r]
    off = np.concatenate([[0], np.cumsum(ls)]).astype(np.int32)
    idx = rng.integers(0, n_in, size=int(off[-1])).astype(np.int32)
    w = rng.uniform(-1, 1, size=int(off[-1])).astype(f32) if weighted else None
    return off, idx, w


def path_coverage(off):
    """{row length: set of off % 4 at which a row of that length starts}."""
    off = np.asarray(off, np.int64)
    out = {}
    for b, l in zip(off[:-1], np.diff(off)):
        out.setdefault(int(l), set()).add(int(b & 3))
    return out


def assert_paths_covered(off):
    """Every length of ROW_LENGTHS starts at off % 4 == 0 (rows of four or more entries: the dwordx4 entry path, then the
    tail loop) and at each other residue (the scalar path alone)."""
    cov = path_coverage(off)
    for l in ROW_LENGTHS:
        assert cov.get(l) == {0, 1, 2, 3}, (l, cov.get(l))


def acc_ref(off, idx, w, v, v2=None, out0=None, remap=None):
    """(ref, scale) of out[r] = sum_k w[k] (v - v2)[remap[idx[k]]] (+ out0[r]) in float64; v is (n_in,) or (n_in, nv)."""
    off = np.asarray(off, np.int64)
    j = np.asarray(idx, np.int64)
    if remap is not None:
        j = np.asarray(remap, np.int64)[j]
    v = np.asarray(v, f64)
    one = v.ndim == 1
    V = v[:, None] if one else v
    A = np.abs(V)
    if v2 is not None:
        V2 = np.asarray(v2, f64).reshape(V.shape)
        V, A = V - V2, A + np.abs(V2)
    ww = np.ones(j.size) if w is None else np.asarray(w, f64)
    rows = np.repeat(np.arange(off.size - 1), np.diff(off))
    ref = np.zeros((off.size - 1, V.shape[1]))
    mag = np.zeros_like(ref)
    np.add.at(ref, rows, ww[:, None] * V[j])
    np.add.at(mag, rows, np.abs(ww)[:, None] * A[j])
    if out0 is not None:
        o = np.asarray(out0, f64).reshape(ref.shape)
        ref, mag = ref + o, mag + np.abs(o)
    scale = np.abs(ref) + mag
    return (ref[:, 0], scale[:, 0]) if one else (ref, scale)


def acc_oracle32(off, idx, w, v, v2=None, out0=None):
    """The Float32 numpy oracle (oracle/accumulator.py) on the same rows: acc(v [- v2]) [+ out0]."""
    from oracle.accumulator import Accumulator as OAcc
    off = np.asarray(off, np.int64)
    inds = [np.asarray(idx[off[r]:off[r + 1]], np.int64) for r in range(off.size - 1)]
    ws = None if w is None else [np.asarray(w[off[r]:off[r + 1]], f32) for r in range(off.size - 1)]
    a = OAcc(inds, ws, first_index=True)
    x = np.asarray(v, f32) if v2 is None else np.asarray(v, f32) - np.asarray(v2, f32)
    r = a(x)
    return r if out0 is None else np.asarray(out0, f32) + r


def seeded(shape, seed, lo=-1.0, hi=1.0):
    return np.random.default_rng(seed).uniform(lo, hi, shape).astype(f32)


# ---------------------------------------------------------------------------------------------------------------------
# 2. Boundary conditions: the sequential impose_bc! calls
# ---------------------------------------------------------------------------------------------------------------------
def bc_ref(a, boundaries, dtype=f64):
    """``boundaries``: ordered dicts with ghost (ng,), off / idx / w (the image interpolator in CSR form, donors as rows of
    the field after ``image_domain``), eta (ng,) = ghost_distance / image_distance, mode (0 constant, 1 copy), value.
    For each boundary in order: interpolate all of its ghosts from the field as it stands, apply the closure, blend with
    eta, write.  Returns (field, scale); the scale is zero off the ghosts and |eta| sum |w||a| + |1 - eta| |b| on them
    (that of the last boundary that wrote the cell)."""
    a = np.array(a, dtype=dtype)
    scale = np.zeros(a.shape, f64)
    for b in boundaries:
        g = np.asarray(b["ghost"], np.int64)
        if g.size == 0:
            continue
        off = np.asarray(b["off"], np.int64)
        rows = np.repeat(np.arange(g.size), np.diff(off))
        j = np.asarray(b["idx"], np.int64)
        w = np.asarray(b["w"], dtype)
        if dtype == f64:
            ia = np.zeros(g.size, f64)
            np.add.at(ia, rows, w * a[j])
        else:                                           # Float32: sequential along the stencil, like the oracle
            ia = np.zeros(g.size, dtype)
            first = np.ones(g.size, bool)
            pos = np.arange(j.size) - off[rows]
            for k in range(int(np.diff(off).max())):
                m = pos == k
                t = (w[m] * a[j[m]]).astype(dtype)
                r = rows[m]
                ia[r] = np.where(first[r], t, ia[r] + t)
                first[r] = False
        mag = np.zeros(g.size, f64)
        np.add.at(mag, rows, np.abs(w.astype(f64)) * np.abs(a[j].astype(f64)))
        eta = np.asarray(b["eta"], dtype)
        ba = ia if b["mode"] == 1 else np.full(g.size, dtype(b["value"]))
        bmag = mag if b["mode"] == 1 else np.abs(ba.astype(f64))
        new = eta * ia + (dtype(1) - eta) * ba
        a[g] = new                                      # a ghost listed twice: the later entry wins, as in Julia
        scale[g] = np.abs(eta.astype(f64)) * mag + np.abs(1.0 - eta.astype(f64)) * bmag + np.abs(new.astype(f64))
    return a, scale


def boundary_dict(b, mode, value=0.0):
    """A product ``Boundary`` (host arrays) in the form ``bc_ref`` takes: donors through ``image_domain``, eta as the
    Float32 quotient the reference forms."""
    acc = b.image_interpolator
    return dict(ghost=np.asarray(b.ghost_indices, np.int64), off=np.asarray(acc.off, np.int64),
                idx=np.asarray(b.image_domain, np.int64)[np.asarray(acc.idx, np.int64)], w=np.asarray(acc.w, f32),
                eta=np.asarray(b.ghost_distances, f32) / np.asarray(b.image_distances, f32), mode=int(mode), value=float(value))


def synthetic_boundary(rng, n, ghosts, extra=None, free_from=2000):
    """One boundary on a plain array of ``n`` cells: stencils of 1..8 donors drawn from the cells >= ``free_from`` (never
    ghosts); every third donor is drawn from ``extra`` (cells that are ghosts of this or another boundary) if given."""
    ghosts = np.asarray(ghosts, np.int64)
    ls = rng.integers(1, 9, ghosts.size) if ghosts.size else np.zeros(0, np.int64)
    off = np.concatenate([[0], np.cumsum(ls)]).astype(np.int64)
    idx = rng.integers(free_from, n, int(off[-1]))
    if extra is not None and idx.size:
        idx[::3] = rng.choice(np.asarray(extra, np.int64), idx[::3].size)
    gd = rng.uniform(0.2, 1.5, ghosts.size).astype(f32)
    idist = rng.uniform(0.8, 1.2, ghosts.size).astype(f32)
    return dict(ghost=ghosts, off=off, idx=idx, w=rng.uniform(0, 1, idx.size).astype(f32), eta=gd / idist,
                ghost_distances=gd, image_distances=idist, mode=0, value=0.0)


def synthetic_sets(n, seed=0):
    """{name: (boundaries, n_levels, n_direct_levels)}: sets that each force one branch of the level construction of
    ``ibh_bcset_create`` (a level is direct when none of its ghost cells is one of its donors; otherwise it goes through the
    side buffer)."""
    rng = np.random.default_rng(seed)
    G = [np.arange(40 * k, 40 * (k + 1)) for k in range(8)]

    def mk(ghosts, extra=None, mode=0, value=0.0):
        b = synthetic_boundary(rng, n, ghosts, extra)
        b["mode"], b["value"] = mode, value
        return b
    out = {}
    # 1. boundary 2 reads ghosts of boundary 1: two levels
    out["dependent"] = ([mk(G[0], value=0.7), mk(G[1], extra=G[0], mode=1)], 2, 2)
    # 2. a boundary whose own ghosts are among its donors: one level through the side buffer; without the overlap: direct
    out["hazard"] = ([mk(G[0], extra=G[0], mode=1)], 1, 0)
    out["direct"] = ([mk(G[0], value=-0.4)], 1, 1)
    #    the EARLIER boundary reads ghosts of the later one: same level (it must see them unwritten), side buffer
    out["hazard_later"] = ([mk(G[0], extra=G[1], mode=1), mk(G[1], value=0.3)], 1, 0)
    # 3. one ghost cell listed by two boundaries: the later one wins
    out["shared_ghost"] = ([mk(G[0], value=0.9), mk(np.arange(39, 79), mode=1)], 2, 2)
    # 4. eight boundaries in a dependency chain
    out["chain8"] = ([mk(G[k], extra=G[k - 1] if k else None, mode=k % 2, value=0.1 * k) for k in range(8)], 8, 8)
    # 5. a boundary with zero ghosts in the middle of a set
    out["empty_middle"] = ([mk(G[0], value=0.5), mk(np.zeros(0, np.int64)), mk(G[1], extra=G[0], mode=1)], 2, 2)
    return out


def oracle_boundaries(boundaries):
    """The dicts of ``bc_ref`` as a domain view for ``oracle.domain.impose_bc`` (its Float32 Accumulator, identity
    ``image_domain``): {"b<k>": {1: boundary}}."""
    from oracle.accumulator import Accumulator as OAcc

    class V:
        pass
    dom = V()
    dom.boundaries = {}
    for k, b in enumerate(boundaries):
        ob = V()
        off = np.asarray(b["off"], np.int64)
        ng = off.size - 1
        ob.ghost_indices = np.asarray(b["ghost"], np.int64)
        ob.ghost_distances = np.asarray(b["eta"], f32)
        ob.image_distances = np.ones(ng, f32)
        n_in = int(max([int(np.max(bb["idx"])) for bb in boundaries if len(bb["idx"])] + [0])) + 1
        ob.image_domain = np.arange(max(n_in, 1))
        ob.image_interpolator = OAcc([np.asarray(b["idx"][off[r]:off[r + 1]], np.int64) for r in range(ng)],
                                     [np.asarray(b["w"][off[r]:off[r + 1]], f32) for r in range(ng)], first_index=True)
        dom.boundaries[f"b{k}"] = {1: ob}
    return dom


def oracle_impose(a, dom, names_modes_values):
    """The sequential ``impose_bc`` calls of the Float32 oracle on a copy of ``a``."""
    from oracle import domain as od
    a = np.array(a, dtype=f32)
    for name, mode, value in names_modes_values:
        if not len(next(iter(dom.boundaries[name].values())).ghost_indices):
            continue
        f = (lambda b, ia: ia.copy()) if mode == 1 else (lambda b, ia, v=f32(value): np.full_like(ia, v))
        od.impose_bc(f, dom, name, a)
    return a


# ---------------------------------------------------------------------------------------------------------------------
# 3. Time step
# ---------------------------------------------------------------------------------------------------------------------
def dt_percell(op, C):
    """max_d unsigned_green_gauss(at_faces(C_d, d), d) per cell in float64 (``op``: an oracle view of the partition);
    NaN propagates like Julia's ``max``.  C is (nc, nd) or (nc, nd, k) for k inputs at once."""
    from oracle import domain as od
    C = np.asarray(C, f64)
    per = None
    for d in range(1, op.ndims + 1):
        a = od.unsigned_green_gauss(op, od.at_faces(op, np.ascontiguousarray(C[:, d - 1]), d), d)
        assert a.dtype == f64
        per = a if per is None else np.where(np.isnan(per) | np.isnan(a), np.nan, np.maximum(per, a))
    return per


def dt_ref(per, scale=1.0):
    """scale * 0.5 / maximum(per): no floor at zero, NaN propagates."""
    per = np.asarray(per, f64)
    m = np.nan if np.isnan(per).any() else per.max()
    with np.errstate(divide="ignore"):
        return f64(scale) * 0.5 / m


def check_dt(got, ref, what=""):
    """NaN first, then |got - ref| <= 4 ulp |ref|; returns the relative error."""
    got, ref = float(got), float(ref)
    if math.isnan(got) or math.isnan(ref):
        assert math.isnan(got) and math.isnan(ref), f"{what}: dt {got!r}, reference {ref!r}"
        return 0.0
    err = abs(got - ref)
    assert err <= BOUND_DT * abs(ref), (f"{what}: dt {got!r}, reference {ref!r}: {err / (ULP * abs(ref)):.1f} ulp > "
                                        f"bound {BOUND_DT / ULP:.0f} ulp")
    return err / abs(ref) if ref else 0.0


def face_neighbours(part):
    """Per dimension (0-based): list of (owner, neighbour) index arrays."""
    return [part.face_owners_neighbors[d] for d in range(1, part.ndims + 1)]


def dt_probe_inputs(part, cells, d, wide=None):
    """(nc, k) one-hot columns of C_d: 1 at cells[i]; where ``wide[i]``, 0.25 at the cell's face neighbours as well."""
    nc = part.spacing.shape[0]
    cells = np.asarray(cells, np.int64)
    E = np.zeros((nc, cells.size))
    if wide is not None and np.any(wide):
        col = np.full(nc, -1, np.int64)
        sel = cells[np.asarray(wide)]
        col[sel] = np.nonzero(np.asarray(wide))[0]
        for o, nb in face_neighbours(part):
            o, nb = np.asarray(o, np.int64), np.asarray(nb, np.int64)
            m = col[o] >= 0
            E[nb[m], col[o[m]]] = 0.25
            m = col[nb] >= 0
            E[o[m], col[nb[m]]] = 0.25
    E[cells, np.arange(cells.size)] = 1.0
    return E


def dt_matrix(part, d):
    """The linear map C_d -> unsigned_green_gauss(at_faces(C_d, d), d) as a float64 sparse matrix (``d`` 0-based), from the
    partition's face lists and face accumulators: row c holds (sum over the faces f of c's two sides of w_cf (h_n, h_o)
    / (h_n + h_o) at (owner, neighbour) of f) / h_c.  tests/test_percell_steps.py holds it to the oracle's operators."""
    import scipy.sparse as sp
    o, nb = (np.asarray(a, np.int64) for a in part.face_owners_neighbors[d + 1])
    h = np.asarray(part.spacing, f64)[:, d]
    nf, nc = o.size, h.size
    ho, hn = h[o], h[nb]
    f = np.arange(nf)
    F = sp.csr_matrix((np.concatenate([hn / (hn + ho), ho / (hn + ho)]), (np.concatenate([f, f]), np.concatenate([o, nb]))),
                      shape=(nf, nc))                   # a mirror face names its cell twice: the weights add to 1
    A = None
    for side in (False, True):
        acc = part.face_accumulators[(d + 1, side)]
        w = np.ones(acc.idx.size) if acc.w is None else np.asarray(acc.w, f64)
        a = sp.csr_matrix((w, np.asarray(acc.idx, np.int64), np.asarray(acc.off, np.int64)), shape=(nc, nf))
        A = a if A is None else A + a
    return sp.diags(1.0 / h) @ (A @ F)


def dt_probe_refs(M, part, cells, d, wide=None):
    """Float64 per-cell arrays (nc, k) of the probes C_d = ``dt_probe_inputs`` with the other components zero (their
    per-cell values are 0); ``M`` = ``dt_matrix(part, d)``, ``d`` 0-based."""
    return np.maximum(np.asarray(M @ dt_probe_inputs(part, cells, d, wide)), 0.0)


# ---------------------------------------------------------------------------------------------------------------------
# 4. Reductions and updates
# ---------------------------------------------------------------------------------------------------------------------
def sum_ref(a, b=None):
    """(math.fsum of the float64 products, sum of their magnitudes)."""
    a = np.asarray(a, f64)
    t = a * (a if b is None else np.asarray(b, f64))
    return math.fsum(t.tolist()), math.fsum(np.abs(t).tolist())


def check_sum(got, a, b=None, what=""):
    ref, mag = sum_ref(a, b)
    if math.isnan(ref) or math.isnan(float(got)):
        assert math.isnan(ref) and math.isnan(float(got)), (what, got, ref)
        return 0.0
    err = abs(float(got) - ref)
    assert err <= BOUND_SUM * mag, f"{what}: sum {float(got)!r}, fsum {ref!r}, error {err:.3e} > {BOUND_SUM * mag:.3e}"
    return err / mag if mag else 0.0


# ibh_ew_reduce (sum / maximum / minimum of a flat Float32 array): its totals cover one wave, one workgroup, both sides of
# the one-to-several-workgroups threshold, both sides of the counter / two-launch threshold and the 1 024-workgroup cap
EW_REDUCE_TOTALS = (1, 63, 64, 65, 255, 256, 257, 2048, 2049, 16384, 16385, 256 * 8 * 1024 + 1)


def ew_reduce_stages(total):
    """[(elements, workgroups)] of the stages of ``ibh_ew_reduce``, from the grid formula of ibh_ew.hip: 8 elements per
    thread in at most 1 024 workgroups of 256 threads; more than one workgroup leaves partials that one workgroup reduces
    (the last one to arrive for 2 - 8 workgroups, a second launch above)."""
    nwg = min(1024, -(-total // (256 * 8)))
    return [(total, nwg)] + ([(nwg, 1)] if nwg > 1 else [])


def ew_sum_depth(total):
    """Additions a term of the Float32 sum can pass through, read from the code: per stage the chain of a thread
    (ceil(elements / (workgroups * 256))), 6 shuffle steps and 4 wave slots."""
    return sum(-(-n // (g * 256)) + 6 + 4 for n, g in ew_reduce_stages(total))


def ew_sum_model32(a):
    """The Float32 sum in the order of ibh_reduce_dev.h: per thread its strided chain from 0, the shuffle tree with offsets
    32 ... 1 (lane 0), the wave slots in order; then the same over the workgroup values."""
    v = np.asarray(a, f32)
    for n, g in ew_reduce_stages(v.size):
        t = g * 256
        pad = np.zeros(-(-n // t) * t, f32)
        pad[:n] = v
        acc = np.zeros(t, f32)
        for row in pad.reshape(-1, t):                 # (a thread past the end adds nothing: x + 0 = x)
            acc = acc + row
        w = acc.reshape(g, 4, 64).copy()
        for o in (32, 16, 8, 4, 2, 1):
            w[:, :, :o] = w[:, :, :o] + w[:, :, o:2 * o]
        slot = w[:, :, 0]
        v = ((slot[:, 0] + slot[:, 1]) + slot[:, 2]) + slot[:, 3]
    return v[0]


def check_sum32(got, a, what=""):
    """|got - math.fsum(a)| <= D 2^-24 sum |a_i| with D = ``ew_sum_depth``: every addition rounds by at most 2^-24 of its
    result, which is at most sum |a_i|.  Returns the error relative to the bound."""
    a64 = np.asarray(a, f32).astype(f64)
    ref, mag = math.fsum(a64.tolist()), math.fsum(np.abs(a64).tolist())
    bound = ew_sum_depth(a64.size) * 2.0 ** -24 * mag
    err = abs(float(got) - ref)
    assert err <= bound, f"{what}: sum {float(got)!r}, fsum {ref!r}, error {err:.3e} > {bound:.3e} (depth {ew_sum_depth(a64.size)})"
    return err / bound if bound else 0.0


def extreme_places(n):
    """Where ``test_maxabs`` puts the largest element: first, last, at 63 / 64 and at the start of the last partial
    workgroup."""
    return sorted({0, n - 1, min(63, n - 1), min(64, n - 1), max(0, n - 1 - (n - 1) % 256)})


def clamp_julia(x, lo, hi):
    """Julia's clamp: NaN stays NaN."""
    x = f64(x)
    return x if np.isnan(x) else min(max(x, lo), hi)


def fas_ref(omega, r, src, q):
    """rr = r [+ src] rounded to Float32 (the kernel's and the reference's ``r .+= source`` is a Float32 array);
    (q + clamp(omega, 0, 1) rr, its scale, the terms rr of the norm)."""
    r64 = np.asarray(r, f64)
    rr = r64 if src is None else (np.asarray(r, f32) + np.asarray(src, f32)).astype(f64)
    rr_exact = r64 if src is None else r64 + np.asarray(src, f64)
    w = clamp_julia(f32(omega), 0.0, 1.0)
    if q is None:
        return None, None, rr
    q64 = np.asarray(q, f64)
    ref = q64 + w * rr_exact
    mag = np.abs(q64) + abs(w) * (np.abs(r64) + (0 if src is None else np.abs(np.asarray(src, f64))))
    return ref, np.abs(ref) + mag, rr


def splitmix_signs(n, seed):
    """+-1 from bit 63 of splitmix64(seed * 0x2545F4914F6CDD1D + i), in numpy uint64 arithmetic (wraps)."""
    with np.errstate(over="ignore"):
        x = np.uint64(seed) * np.uint64(0x2545F4914F6CDD1D) + np.arange(n, dtype=np.uint64)
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        x = x ^ (x >> np.uint64(31))
    return np.where((x >> np.uint64(63)).astype(bool), f32(1), f32(-1))


# ---------------------------------------------------------------------------------------------------------------------
# 5. Point-implicit blocks
# ---------------------------------------------------------------------------------------------------------------------
def pinv_blocks(M, n, seed=0):
    """(A (n, M, M) Float32, kind (n,) of str): blocks with prescribed singular values U diag(s) V^T built in float64 and
    rounded (sigma_min / sigma_max in decades from 1 down to 1e-3), blocks with two equal columns (exactly rank deficient
    in Float32), a zero block, a diagonal block, a block scaled by 1e-6 and one by 1e6."""
    rng = np.random.default_rng(1000 * M + seed)
    A = np.empty((n, M, M), f32)
    kind = np.empty(n, dtype=object)
    for p in range(n):
        U, _ = np.linalg.qr(rng.standard_normal((M, M)))
        V, _ = np.linalg.qr(rng.standard_normal((M, M)))
        ratio = 10.0 ** -rng.uniform(0, 3)                        # sigma_min / sigma_max in [1e-3, 1]
        s = np.exp(rng.uniform(np.log(ratio), 0.0, M))
        s[0], s[-1] = 1.0, ratio
        A[p] = (U * s) @ V.T
        kind[p] = "svd"
    special = {}
    if n >= 8:
        special = {1: "equal_columns", 2: "zero", 3: "diagonal", 4: "small", 5: "large", 6: "equal_columns"}
    elif n == 1:
        special = {}
    for p, k in special.items():
        if k == "equal_columns":
            A[p][:, 0] = A[p][:, M - 1]
        elif k == "zero":
            A[p] = 0
        elif k == "diagonal":
            A[p] = np.diag(np.linspace(1.0, 0.01, M)).astype(f32)
        elif k == "small":
            A[p] *= f32(1e-6)
        elif k == "large":
            A[p] *= f32(1e6)
        kind[p] = k
    if n >= 64:
        A[7::16, :, 1] = A[7::16, :, 0]
        kind[7::16] = "equal_columns"
    return A, kind


def pinv_ref(A):
    """(P, bins, sv): float64 pinv with the cut-off eps(Float32) * M * sigma_max; bins[p] is the decade of sigma_max /
    sigma_min (full rank), "deficient" or "zero".  Asserts that float64 and Float32 agree about the rank with a wide
    margin: every singular value is above 100 x or below 0.01 x the cut-off."""
    A64 = np.asarray(A, f64)
    n, M, _ = A64.shape
    U, s, Vt = np.linalg.svd(A64)
    cut = EPS32 * M * s[:, :1]
    assert np.all((s > 100 * cut) | (s < 0.01 * cut) | (s[:, :1] == 0)), "a singular value sits near the cut-off"
    keep = s > cut
    inv = np.where(keep, 1.0 / np.where(keep, s, 1.0), 0.0)
    P = np.einsum("pji,pj,pkj->pik", Vt, inv, U)
    bins = np.empty(n, dtype=object)
    for p in range(n):
        if s[p, 0] == 0:
            bins[p] = "zero"
        elif not keep[p].all():
            bins[p] = "deficient"
        else:
            c = s[p, 0] / s[p, -1]
            assert c <= 1.01e3, c                      # (rounding to Float32 moves 1e3 by a few ulps)
            bins[p] = min(2, int(np.floor(np.log10(c))))
    return P, bins, s


def pinv_lapack32(A):
    """Moore-Penrose inverses by LAPACK's single-precision SVD (sgesdd through scipy) with the cut-off of
    ``oracle.point_implicit.inverse_blocks``.  That oracle calls ``numpy.linalg.pinv``, which converts Float32 input to
    double, runs dgesdd and rounds the result: its error is the final rounding alone (2.3e-7 in every bin) and says
    nothing about a Float32 algorithm, so the calibration measures this one."""
    from scipy.linalg import svd
    A = np.asarray(A, f32)
    out = np.zeros_like(A)
    M = A.shape[1]
    for p in range(A.shape[0]):
        U, s, Vt = svd(A[p], lapack_driver="gesdd")
        assert U.dtype == f32 and s.dtype == f32
        keep = s > f32(EPS32) * f32(M) * s[0]
        inv = np.where(keep, f32(1) / np.where(keep, s, f32(1)), f32(0)).astype(f32)
        out[p] = (Vt.T * inv) @ U.T
    return out


def pinv_error(got, P):
    """max |got - ref| / max |ref| per block; a zero reference wants an exactly zero result."""
    g = np.asarray(got, f64)
    d = np.abs(g - P).max(axis=(1, 2))
    m = np.abs(P).max(axis=(1, 2))
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(m > 0, d / np.where(m > 0, m, 1.0), np.where(d == 0, 0.0, np.inf))


def pinv_binned(err, bins):
    return {k: float(err[bins == k].max()) for k in list(PINV_BOUND) + ["zero"] if np.any(bins == k)}


def check_pinv(got, A, what=""):
    """NaN pattern, per-bin bounds, and the four Moore-Penrose identities in float64 relative to |A||P| (2-norms): the
    identities hold for the reference to rounding, so a result within ``b`` of it misses them by at most 2 b."""
    P, bins, _ = pinv_ref(A)
    g = np.asarray(got, f64)
    assert not np.isnan(g).any(), f"{what}: NaN in the pseudo-inverse"
    worst = pinv_binned(pinv_error(g, P), bins)
    for k, e in worst.items():
        b = 0.0 if k == "zero" else PINV_BOUND[k]
        assert e <= b, f"{what}: bin {k}: {e:.3e} > {b:.3e} ({worst})"
    mp = moore_penrose(A, g)
    for k in PINV_BOUND:
        m = bins == k
        if m.any():
            assert mp[m].max() <= 2 * PINV_BOUND[k], f"{what}: Moore-Penrose identities, bin {k}: {mp[m].max():.3e}"
    return worst


def moore_penrose(A, P):
    """max over the four identities of the residual's 2-norm over |A||P| (times |A| or |P| where the identity has three
    factors), per block, in float64."""
    A = np.asarray(A, f64)
    P = np.asarray(P, f64)
    na = np.linalg.norm(A, 2, axis=(1, 2))
    npn = np.linalg.norm(P, 2, axis=(1, 2))
    AP, PA = A @ P, P @ A
    T = np.swapaxes

    def nrm(x):
        return np.linalg.norm(x, 2, axis=(1, 2))
    den = np.where(na * npn > 0, na * npn, 1.0)
    r = np.stack([nrm(AP @ A - A) / (den * np.where(na > 0, na, 1.0)), nrm(PA @ P - P) / (den * np.where(npn > 0, npn, 1.0)),
                  nrm(T(AP, 1, 2) - AP) / den, nrm(T(PA, 1, 2) - PA) / den])
    return r.max(axis=0)


def apply_ref(invD, v):
    """(ref, scale) of out[p, k] = sum_i v[p, i] invD[p, k, i]; invD (n, M, M) or (n,) with v (n,)."""
    D, V = to64(invD, v)
    if D.ndim == 1:
        r = V * D
        return r, 2 * np.abs(r)
    r = np.einsum("pi,pki->pk", V, D)
    return r, np.abs(r) + np.einsum("pi,pki->pk", np.abs(V), np.abs(D))

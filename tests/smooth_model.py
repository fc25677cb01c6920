"""numpy model of the implicit residual smoothing (csrc/ibh_smooth_dev.h): the executable specification of ``smooth_row``.

Test infrastructure.  ``F(i)``, the faces of cell ``i``: dimensions ascending, in a dimension the left faces in the order of
the accumulator's list (the cell across is the face's owner), then the right faces (the face's neighbour; a mirror face is
across from ``i`` itself).  Per variable, from ``S = R``,

    S_i <- (R_i + eps * sum_{f in F(i)} S[across(f, i)]) / (1 + eps * float(n_i)),        n_i = |F(i)|,

Jacobi on ``(I + eps L) S = R`` with ``L`` the unweighted Laplacian of the face graph.  In ``float32`` the sum starts from its
first term and adds in the order of ``F(i)``, and every product, sum and the divide is rounded on its own: the kernel's bits.
"""
import numpy as np

f32, f64 = np.float32, np.float64


def face_table(part):
    """``(T, n)``: ``T`` is ``(nc, n_max)`` with the cells across the faces of every cell in the order of ``F(i)``, padded with
    -1; ``n`` the face counts."""
    nc = part.spacing.shape[0]
    lists = []                                           # (off, the cells across the listed faces) in the order of F(i)
    for d in range(part.ndims):
        own, nei = (np.asarray(a, dtype=np.int64) for a in part.face_owners_neighbors[d + 1])
        for right, across in ((False, own), (True, nei)):
            acc = part.face_accumulators[(d + 1, right)]
            off, idx = np.asarray(acc.off, dtype=np.int64), np.asarray(acc.idx, dtype=np.int64)
            assert off.shape[0] == nc + 1 and off[0] == 0 and off[-1] == idx.shape[0]
            lists.append((off, across[idx]))
    n = sum(np.diff(off) for off, _ in lists)
    T = np.full((nc, max(int(n.max()), 1)), -1, dtype=np.int64)
    fill = np.zeros(nc, dtype=np.int64)
    for off, cells in lists:
        cnt = np.diff(off)
        row = np.repeat(np.arange(nc), cnt)
        T[row, fill[row] + np.arange(cells.shape[0]) - off[row]] = cells
        fill += cnt
    return T, n


def iterate(T, n, R, S, eps, dtype):
    """One Jacobi iteration from ``S`` in ``dtype``, in the kernel's order of operations."""
    eps = dtype(eps)
    acc = np.zeros_like(R)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(T.shape[1]):
            has = n > k
            x = S[np.where(has, T[:, k], 0)]
            acc[has] = x[has] if k == 0 else (acc[has] + x[has]).astype(dtype)
        den = (dtype(1) + (eps * n.astype(dtype)).astype(dtype)).astype(dtype)
        den = den if R.ndim == 1 else den[:, None]
        return (((R + (eps * acc).astype(dtype)).astype(dtype)) / den).astype(dtype)


def model(part, R, eps, n_iter, dtype=f32, table=None):
    """``n_iter`` iterations on ``R`` (``(nc,)`` or ``(nc, nv)``) in ``dtype`` (float32: the kernel's bits; float64)."""
    T, n = table if table is not None else face_table(part)
    R = np.asarray(R).astype(dtype)
    S = R
    for _ in range(n_iter):
        S = iterate(T, n, R, S, eps, dtype)
    return S


def apply_operator(part, S, eps, table=None):
    """``(I + eps L) S`` in float64: ``S_i + eps * (n_i S_i - sum_{f in F(i)} S[across(f, i)])``."""
    T, n = table if table is not None else face_table(part)
    S = np.asarray(S, dtype=f64)
    nn = n.astype(f64) if S.ndim == 1 else n.astype(f64)[:, None]
    tot = np.zeros_like(S)
    for k in range(T.shape[1]):
        has = n > k
        tot[has] += S[T[has, k]]
    return S + eps * (nn * S - tot)


def rho(n, eps):
    """The contraction factor of the iteration on this mesh: ``max_i eps n_i / (1 + eps n_i)``."""
    return float(np.max(eps * n / (1.0 + eps * n)))

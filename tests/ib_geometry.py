"""The geometry of the immersed-boundary method from its definitions, in float64 (test infrastructure).

Nothing here calls the product's mesher or ``Domain`` or the oracle; a surface comes in as its vertex array ``points
(nd, np)`` and its 1-based ``simplices (nd, ns)`` (segments in 2-D, triangles in 3-D), cells as rows ``X (n, nd)``.

- ``closest_on_surface``: the distance of a point to the union of the simplices and a point that attains it.  Every simplex
  is considered for every point.  The per-simplex closest point is the clamped segment parameter in 2-D and the region test
  of a triangle (vertex, edge and interior regions of its plane) in 3-D.  Pairs (point, simplex) are dropped before that
  arithmetic only by a bound that cannot lose the minimum: the simplex lies inside the ball of radius r_s (largest vertex
  distance) about its centroid c_s, and c_s is itself a point of the surface, so
  ``|x - c_s| - r_s  <=  dist(x, simplex s)`` and ``dist(x, surface) <= min_t |x - c_t|``; a simplex with
  ``|x - c_s| - r_s > min_t |x - c_t|`` is farther than the surface and cannot hold the closest point.
- ``ghost_reference``: the cells with ``d <= ratio * diam`` (diam = the cell's diagonal), the definition of a ghost cell.
- ``boundary_reference``: normal, distances, image point and eta of a ghost from its centre and foot point.
- ``hcube_reference``: ghosts and foot points of the axis-aligned planes of the box.
- ``polyhedron``: area, enclosed volume and area vectors of a closed triangle surface.

``ULP32`` = 2^-23 is the spacing of Float32 relative to the magnitude; ``dist_bound(stl)`` = 2 ULP32 x the largest coordinate
magnitude of the surface: one rounding of a stored Float32 foot point (half an ulp of that magnitude per coordinate, at most
sqrt(3)/2 ulp as a vector) plus the Float32 arithmetic of the foot point (a product and a sum per coordinate, another ulp)."""
import numpy as np

f64 = np.float64
ULP32 = 2.0 ** -23
THRESHOLD_BAND = 8 * ULP32     # |d / (ratio diam) - 1| inside which Float32 roundings of the two distances decide
PAIRS_PER_CHUNK = 400_000


def surface_arrays(stl):
    """(V, nd): the vertices of every simplex, ``V[k]`` = (ns, nd) array of vertex k, in float64."""
    P = np.asarray(stl.points, f64)
    S = np.asarray(stl.simplices, np.int64) - 1
    return [np.ascontiguousarray(P[:, S[k]].T) for k in range(S.shape[0])], P.shape[0]


def dist_bound(stl):
    return 2 * ULP32 * float(np.abs(np.asarray(stl.points, f64)).max())


def closest_on_segments(x, p0, p1):
    """Rows: point x, segment p0-p1.  Returns the barycentric coordinates (m, 2) of the closest point of the segment."""
    u = p1 - p0
    uu = (u * u).sum(axis=1)
    t = ((x - p0) * u).sum(axis=1) / np.where(uu > 0, uu, 1.0)
    t = np.where(uu > 0, np.clip(t, 0.0, 1.0), 0.0)
    return np.stack([1.0 - t, t], axis=1)


def closest_on_triangles(x, a, b, c):
    """Rows: point x, triangle abc.  Returns the barycentric coordinates (m, 3) of the closest point of the triangle: the
    plane of the triangle is cut by the lines through its edges and their normals at the vertices into three vertex regions,
    three edge regions and the interior; the signs of the projections of x - vertex on the edges say which one holds x."""
    ab, ac = b - a, c - a
    ap, bp, cp = x - a, x - b, x - c
    dot = lambda p, q: (p * q).sum(axis=1)    # noqa: E731
    d1, d2 = dot(ab, ap), dot(ac, ap)
    d3, d4 = dot(ab, bp), dot(ac, bp)
    d5, d6 = dot(ab, cp), dot(ac, cp)
    vc = d1 * d4 - d3 * d2
    vb = d5 * d2 - d1 * d6
    va = d3 * d6 - d5 * d4
    one, zero = np.ones_like(d1), np.zeros_like(d1)

    def frac(num, den):
        return num / np.where(den != 0, den, 1.0)
    t_ab = np.clip(frac(d1, d1 - d3), 0.0, 1.0)
    t_ac = np.clip(frac(d2, d2 - d6), 0.0, 1.0)
    t_bc = np.clip(frac(d4 - d3, (d4 - d3) + (d5 - d6)), 0.0, 1.0)
    s = va + vb + vc
    v_in, w_in = frac(vb, s), frac(vc, s)
    regions = [
        ((d1 <= 0) & (d2 <= 0), (one, zero, zero)),                                  # vertex a
        ((d3 >= 0) & (d4 <= d3), (zero, one, zero)),                                 # vertex b
        ((vc <= 0) & (d1 >= 0) & (d3 <= 0), (1.0 - t_ab, t_ab, zero)),               # edge ab
        ((d6 >= 0) & (d5 <= d6), (zero, zero, one)),                                 # vertex c
        ((vb <= 0) & (d2 >= 0) & (d6 <= 0), (1.0 - t_ac, zero, t_ac)),               # edge ac
        ((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0), (zero, 1.0 - t_bc, t_bc)),     # edge bc
    ]
    lam = np.stack([1.0 - v_in - w_in, v_in, w_in], axis=1)                          # interior
    done = np.zeros(d1.shape, bool)
    for cond, bary in regions:
        take = cond & ~done
        for k in range(3):
            lam[take, k] = bary[k][take]
        done |= cond
    return lam


def closest_on_surface(stl, X):
    """(d, Q): the exact distance of every row of ``X (n, nd)`` to the union of the simplices, and a point of it at that
    distance.  See the module docstring for the only pruning it does."""
    V, nd = surface_arrays(stl)
    X = np.asarray(X, f64).reshape(-1, nd)
    n, ns = X.shape[0], V[0].shape[0]
    ctr = sum(V) / len(V)
    rad = np.max(np.stack([np.sqrt(((v - ctr) ** 2).sum(axis=1)) for v in V]), axis=0)
    d_out = np.full(n, np.inf)
    Q = np.full((n, nd), np.nan)
    rows_per_chunk = max(1, PAIRS_PER_CHUNK // max(ns, 1))
    for s in range(0, n, rows_per_chunk):
        x = X[s:s + rows_per_chunk]
        dc = np.sqrt(((x[:, None, :] - ctr[None, :, :]) ** 2).sum(axis=2))           # (m, ns): every simplex
        keep = dc - rad[None, :] <= dc.min(axis=1, keepdims=True)
        i, t = np.nonzero(keep)
        xi = x[i]
        if nd == 2:
            lam = closest_on_segments(xi, V[0][t], V[1][t])
        else:
            lam = closest_on_triangles(xi, V[0][t], V[1][t], V[2][t])
        q = sum(lam[:, k:k + 1] * V[k][t] for k in range(len(V)))
        d = np.sqrt(((q - xi) ** 2).sum(axis=1))
        order = np.lexsort((t, d, i))                                                # per point: the least distance first
        first = order[np.concatenate([[True], i[order][1:] != i[order][:-1]])]
        d_out[s + i[first]] = d[first]
        Q[s + i[first]] = q[first]
    return d_out, Q


def cell_diameters(W):
    W = np.asarray(W, f64)
    return np.sqrt((W * W).sum(axis=1))


def ghost_reference(stl, X, diam, ratio):
    """(ghosts, d, Q, near): the cells with d <= ratio diam in ascending order, the exact distance and foot point of every cell
    that can be one, and the cells within ``THRESHOLD_BAND`` of the threshold.  A cell whose distance to the bounding box of
    the surface exceeds ``2 ratio diam`` is farther than that from the surface itself: it gets d = inf and no search."""
    X = np.asarray(X, f64)
    P = np.asarray(stl.points, f64)
    lo, hi = P.min(axis=1), P.max(axis=1)
    gap = np.maximum(np.maximum(lo[None, :] - X, X - hi[None, :]), 0.0)
    cand = np.nonzero(np.sqrt((gap * gap).sum(axis=1)) <= 2 * ratio * diam)[0]
    d = np.full(X.shape[0], np.inf)
    Q = np.full(X.shape, np.nan)
    d[cand], Q[cand] = closest_on_surface(stl, X[cand])
    thr = ratio * diam
    ghosts = np.nonzero(d <= thr)[0]
    near = np.nonzero(np.abs(d / thr - 1.0) <= THRESHOLD_BAND)[0]
    return ghosts, d, Q, near


def boundary_reference(x, q, width, ratio):
    """Per ghost (rows): unit normal (x - q) / |x - q|, ghost distance |x - q|, image distance |width|_2 ratio, image point
    q + normal * image distance, eta = ghost distance / image distance."""
    x, q, width = np.asarray(x, f64), np.asarray(q, f64), np.asarray(width, f64)
    v = x - q
    gd = np.sqrt((v * v).sum(axis=1))
    n = v / np.where(gd > 0, gd, 1.0)[:, None]
    idist = np.sqrt((width * width).sum(axis=1)) * ratio
    return dict(normals=n, ghost_distances=gd, image_distances=idist, images=q + n * idist[:, None], eta=gd / idist)


def hcube_reference(X, W, origin, widths, hfaces, ratio):
    """Hypercube family ``hfaces`` = [(dim 1-based, front)]: the plane of a face is x_dim = origin[dim] (+ widths[dim] if
    front).  (ghosts, Q, dmin, near): the cells whose distance to any listed plane is < ratio diam, the foot point of each on
    the nearest listed plane (the first listed on a tie), every cell's least distance and the cells within ``THRESHOLD_BAND``
    of the threshold."""
    X, W = np.asarray(X, f64), np.asarray(W, f64)
    o, w = np.asarray(origin, f64), np.asarray(widths, f64)
    diam = cell_diameters(W)
    dmin = np.full(X.shape[0], np.inf)
    Q = X.copy()
    for dim, front in hfaces:
        c = o[dim - 1] + (w[dim - 1] if front else 0.0)
        dd = np.abs(X[:, dim - 1] - c)
        closer = dd < dmin
        foot = X[closer].copy()
        foot[:, dim - 1] = c
        Q[closer] = foot
        dmin = np.where(closer, dd, dmin)
    thr = ratio * diam
    ghosts = np.nonzero(dmin < thr)[0]
    near = np.nonzero(np.abs(dmin / thr - 1.0) <= THRESHOLD_BAND)[0]
    return ghosts, Q[ghosts], dmin, near


def polyhedron(stl):
    """(area, volume, area vectors (ns, 3), centroids (ns, 3)) of a closed, outward-oriented triangle surface: the area vector
    of a triangle is (b - a) x (c - a) / 2, the volume the sum of the signed tetrahedra a . (b x c) / 6 over the origin."""
    (a, b, c), nd = surface_arrays(stl)
    assert nd == 3
    av = np.cross(b - a, c - a) / 2.0
    vol = float((a * np.cross(b, c)).sum() / 6.0)
    return float(np.sqrt((av * av).sum(axis=1)).sum()), vol, av, (a + b + c) / 3.0


def circumradius_about_centre(stl):
    """Largest distance of a vertex of a simplex from the simplex's centroid, over the surface."""
    V, _ = surface_arrays(stl)
    ctr = sum(V) / len(V)
    return float(max(np.sqrt(((v - ctr) ** 2).sum(axis=1)).max() for v in V))


def knn_brute(Xcells, targets, k, rows_per_chunk=256):
    """The k-th smallest distance from each target to the cell centres, by a full distance table (no tree): (n,) float64."""
    Xc = np.asarray(Xcells, f64)
    T = np.asarray(targets, f64)
    out = np.empty(T.shape[0])
    for s in range(0, T.shape[0], rows_per_chunk):
        t = T[s:s + rows_per_chunk]
        d2 = ((t[:, None, :] - Xc[None, :, :]) ** 2).sum(axis=2)
        out[s:s + rows_per_chunk] = np.sqrt(np.partition(d2, k - 1, axis=1)[:, k - 1])
    return out


def row_moments(off, idx, w, Xcells, targets):
    """Float64 moments of CSR interpolation rows on their Float32 weights: (sum w - 1, sum w (X_j - target)) per row."""
    off = np.asarray(off, np.int64)
    rows = np.repeat(np.arange(off.size - 1), np.diff(off))
    j = np.asarray(idx, np.int64)
    ww = np.asarray(w, f64)
    T = np.asarray(targets, f64)
    m0 = np.zeros(off.size - 1)
    np.add.at(m0, rows, ww)
    m1 = np.zeros(T.shape)
    np.add.at(m1, rows, ww[:, None] * (np.asarray(Xcells, f64)[j] - T[rows]))
    return m0 - 1.0, m1

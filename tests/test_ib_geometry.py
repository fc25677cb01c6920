"""The immersed-boundary tables of ``Domain`` against the geometry they stand for (tests/ib_geometry.py, float64, exact
closest-point search): ghost sets, foot points, normals, distances, eta, the image interpolator rows, the hypercube
families and the 3-D ``Surface``.  No device.

The product (and the oracle's ``ghosts_and_projections``, which calls the product's distance field) searches the simplex
CENTRES within ``2 ratio diam`` of a cell and projects on those simplices.  That equals the exact answer only if every simplex
that can hold the foot point of a ghost has its centre inside the search ball: the foot is within ``ratio diam`` of the cell,
the centre within the simplex's circumradius about its centre of the foot.  ``Case.precondition`` asserts
``circumradius <= ratio x (diameter of the smallest ghost cell)`` per mesh (measured: 0.04 .. 0.38 of it) before anything is
compared.

Bounds (``G`` = ib_geometry):
- ``B = G.dist_bound(stl)`` = 2 ulp32 of the largest coordinate magnitude of the surface, derived there, on: the distance of
  the stored foot point from the exact surface, | |proj - x| - d_exact |, ghost and image distances.
- normals: ``B / ghost distance``: a foot point moved by B turns the unit vector from it to the centre by B / distance.
  A ghost closer than 16 B has no defined normal (the bound exceeds 1/16); such ghosts are counted and capped at 0.5 %.
  (The foot must be THE closest point for this, not a point as close as Float32 can tell:
  ``test_normals_against_the_exact_foot_point``.)
- eta = g / i: (1 + eta) B / (i - B), from the two distance bounds (evaluated in float64 on the Float32 tables).
- ghost sets: cells with | d / (ratio diam) - 1 | <= 8 x 2^-23 may differ (the Float32 roundings of the two distances: the
  sum of squares, the root and the product with the ratio on either side, half an ulp each); at most 0.5 % of the ghosts,
  and on these meshes none (asserted).
- interpolator rows: donors within the k-th smallest brute-force distance from the REFERENCE image point + 2 ulp32 of the
  largest cell coordinate; moments about the reference image point within 4 x what the oracle's own
  ``nninterp.Interpolator`` (an independent implementation: per-target ``pinv``) shows about the same point on the same
  targets (the image points the tables call for, formed in the test); the factor covers different ``pinv`` cut-offs.
"""
import numpy as np
import pytest

import ibamd
import ib_geometry as G
from conftest import ADV_FAMILIES, RAE_FAMILIES
from ibamd import domain as D
from ibamd.mesher import Mesh, Stereolitography

f32, f64 = np.float32, np.float64
RATIO = 1.5
CAP = 0.005


# ---------------------------------------------------------------------------------------------------------------------
# meshes
# ---------------------------------------------------------------------------------------------------------------------
def sphere_mesh():
    """The 4 096-cell icosphere mesh of tests/test_3d.py: 64 blocks of 4^3 cells, 7 200 triangles after refinement."""
    from test_3d import icosphere
    return Mesh(f32([-2, -2, -2]), f32([4, 4, 4]), ("sphere", icosphere(1.0, subdiv=2), f32(0.25)), block_size=4)


PLATE_CORNERS = np.array([[-0.2, -0.3, -0.5], [1.1, -0.2, -0.1], [1.0, 1.1, 0.4], [-0.3, 1.0, 0.0]])


def plate_mesh():
    """An open, tilted, slightly warped quadrilateral of two triangles in the box of the sphere: its boundary edges and
    corners are closest to many cells (the edge and vertex branches of ``proj2simplex``)."""
    plate = Stereolitography(PLATE_CORNERS.T.astype(f32), np.array([[1, 2, 3], [1, 3, 4]]).T.astype(np.int64))
    return Mesh(f32([-2, -2, -2]), f32([4, 4, 4]), ("plate", plate, f32(0.25)), block_size=4)


class Case:
    """One domain: its cells from the oracle's ``get_cells`` (float64 copies) and, per immersed boundary, the reference."""

    def __init__(self, name, dom):
        from oracle.mesher import get_cells
        self.name, self.dom = name, dom
        msh = dom.mesh
        c, w = get_cells(msh.block_origins, msh.block_widths, msh.block_size)
        self.X, self.W = np.ascontiguousarray(c.T, dtype=f64), np.ascontiguousarray(w.T, dtype=f64)
        self.diam = G.cell_diameters(self.W)
        self.lo, self.hi = self.X.min(axis=0), self.X.max(axis=0)
        self._ref, self._report = {}, {}

    def stl(self, bname):
        return self.dom.mesh.distance_fields[bname].stl

    def reference(self, bname):
        """ghosts, d, Q, near of ``G.ghost_reference`` and ``G.boundary_reference`` on the reference ghosts (cached)."""
        if bname not in self._ref:
            ghosts, d, Q, near = G.ghost_reference(self.stl(bname), self.X, self.diam, RATIO)
            fields = G.boundary_reference(self.X[ghosts], Q[ghosts], self.W[ghosts], RATIO)
            self._ref[bname] = dict(ghosts=ghosts, d=d, Q=Q, near=near, **fields)
        return self._ref[bname]

    def precondition(self, bname):
        """circumradius about the centre / (ratio x smallest ghost diameter): the comparison is with the exact answer only
        if this is <= 1 (module docstring)."""
        r = self.reference(bname)
        return G.circumradius_about_centre(self.stl(bname)) / (RATIO * self.diam[r["ghosts"]].min())

    def inside(self, images):
        return np.all((images >= self.lo) & (images <= self.hi), axis=1)


def gathered(dom, bname):
    """The chunks of a boundary concatenated in order (float64 copies of the Float32 tables)."""
    parts = dom.boundaries[bname]

    def cat(f, dt=f64):
        return np.concatenate([np.asarray(getattr(parts[k], f)) for k in parts]).astype(dt)
    return dict(ghosts=cat("ghost_indices", np.int64), proj=cat("projections"), normals=cat("normals"),
                gd=cat("ghost_distances"), idist=cat("image_distances"))


@pytest.fixture(scope="module")
def adv_case(adv_mesh):
    return Case("advection", ibamd.Domain(adv_mesh, hypercube_families=ADV_FAMILIES))


@pytest.fixture(scope="module")
def rae_cases(rae_mesh_small):
    dom = ibamd.Domain(rae_mesh_small, hypercube_families=RAE_FAMILIES)
    return [Case(f"rae level {l}", d) for l, d in enumerate([dom] + ibamd.multigrid(dom, max_levels=2)[0])]


@pytest.fixture(scope="module")
def sphere_cases():
    dom = ibamd.Domain(sphere_mesh())
    assert len(dom) == 4096
    coarse = ibamd.multigrid(dom, max_levels=1)[0][0]
    assert len(coarse) == 512
    return [Case("sphere", dom), Case("sphere coarse", coarse)]


@pytest.fixture(scope="module")
def plate_case():
    dom = ibamd.Domain(plate_mesh())
    assert len(dom) == 4096
    return Case("plate", dom)


@pytest.fixture(scope="module")
def chunked_case():
    dom = ibamd.Domain(sphere_mesh(), max_partition_size=500)
    assert len(dom.boundaries["sphere"]) >= 3 and len(dom.partitions) >= 2
    return Case("sphere chunked", dom)


@pytest.fixture(scope="module")
def immersed(adv_case, rae_cases, sphere_cases, plate_case, chunked_case):
    """[(case, boundary name)] of every immersed boundary under test."""
    return ([(adv_case, "upper"), (adv_case, "lower")] + [(c, "wall") for c in rae_cases]
            + [(c, "sphere") for c in sphere_cases] + [(plate_case, "plate"), (chunked_case, "sphere")])


# ---------------------------------------------------------------------------------------------------------------------
# the reference is sound
# ---------------------------------------------------------------------------------------------------------------------
def _dense_sample(V, m=7):
    """Barycentric lattice of a simplex with m intervals per edge: vertices, edge points and interior points."""
    k = len(V)
    if k == 2:
        lam = np.array([[1 - i / m, i / m] for i in range(m + 1)])
    else:
        lam = np.array([[1 - (i + j) / m, i / m, j / m] for i in range(m + 1) for j in range(m + 1 - i)])
    return lam @ np.stack(V)


@pytest.mark.parametrize("nd", [2, 3])
def test_reference_closest_point_on_random_simplices(nd):
    """The returned point lies in the simplex (barycentric coordinates >= -1e-12, sum 1 to rounding) and no point of a dense
    sample of the simplex is closer; needles and far-away query points included."""
    rng = np.random.default_rng(nd)
    n = 600
    V = [rng.uniform(-1, 1, (n, nd)) for _ in range(nd)]
    V[1][::7] = V[0][::7] + 1e-3 * rng.uniform(-1, 1, (V[0][::7].shape))           # short edges: needles
    x = rng.uniform(-2, 2, (n, nd))
    x[::5] = V[0][::5] + 0.05 * rng.uniform(-1, 1, (x[::5].shape))                 # close to a vertex
    x[1::5] = (sum(V) / nd)[1::5] + 0.02 * rng.uniform(-1, 1, (x[1::5].shape))     # close to the centroid
    lam = G.closest_on_segments(x, *V) if nd == 2 else G.closest_on_triangles(x, *V)
    assert lam.min() >= -1e-12 and np.abs(lam.sum(axis=1) - 1).max() <= 1e-12
    q = sum(lam[:, k:k + 1] * V[k] for k in range(nd))
    d = np.sqrt(((q - x) ** 2).sum(axis=1))
    regions = set()
    for i in range(n):
        S = _dense_sample([v[i] for v in V])
        ds = np.sqrt(((S - x[i]) ** 2).sum(axis=1)).min()
        assert d[i] <= ds + 1e-12, (i, d[i], ds)
        regions.add(tuple((lam[i] > 1e-9).tolist()))
    assert len(regions) == 2 ** nd - 1          # every vertex, every edge and the interior came up as the answer
    # the surface search returns the same as the per-simplex minimum over all simplices, for every point
    stl = Stereolitography(np.concatenate(V).T, np.arange(1, nd * n + 1).reshape(nd, n))
    ds, Q = G.closest_on_surface(stl, x[:80])
    for i in range(80):
        xi = np.repeat(x[i:i + 1], n, axis=0)
        l = G.closest_on_segments(xi, *V) if nd == 2 else G.closest_on_triangles(xi, *V)
        qq = sum(l[:, k:k + 1] * V[k] for k in range(nd))
        dall = np.sqrt(((qq - xi) ** 2).sum(axis=1))
        assert ds[i] == dall.min() and np.sqrt(((Q[i] - x[i]) ** 2).sum()) == ds[i]


def test_reference_distance_inside_the_icosphere(sphere_cases):
    """For a point inside the unit icosphere: R_inscribed - |x| <= d <= 1 - |x| (the polyhedron lies between the inscribed
    sphere of its faces and the unit sphere that holds its vertices)."""
    stl = sphere_cases[0].stl("sphere")
    V, _ = G.surface_arrays(stl)
    rv = np.concatenate([np.sqrt((v * v).sum(axis=1)) for v in V])      # (refinement bisects edges in the facets' planes)
    assert rv.max() <= 1 + 1e-6 and rv.max() >= 1 - 1e-6
    _, _, av, ctr = G.polyhedron(stl)
    nrm = av / np.sqrt((av * av).sum(axis=1))[:, None]
    r_in = float((nrm * V[0]).sum(axis=1).min())            # least distance of a face plane from the origin
    assert 0.95 < r_in < 1.0
    rng = np.random.default_rng(0)
    x = rng.normal(size=(400, 3))
    x = x / np.sqrt((x * x).sum(axis=1))[:, None] * rng.uniform(0, 0.97, 400)[:, None]
    d, q = G.closest_on_surface(stl, x)
    r = np.sqrt((x * x).sum(axis=1))
    assert np.all(d >= r_in - r - 1e-6) and np.all(d <= 1 - r + 1e-6)
    assert np.all(np.sqrt((q * q).sum(axis=1)) <= 1 + 1e-6)


def test_reference_hcube_and_polyhedron_known_answers():
    """A cube of side 2 (12 triangles): area 24, volume 8, closed.  Hypercube reference on a 4 x 4 lattice of the unit square:
    the ghosts of the right face at ratio 1.5 are the cells within 1.5 diagonals of x = 1."""
    c = np.array([[x, y, z] for z in (-1, 1) for y in (-1, 1) for x in (-1, 1)], f64)
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    tris = np.array([t for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))]).T + 1
    area, vol, av, ctr = G.polyhedron(Stereolitography(c.T, tris))
    assert abs(area - 24) <= 1e-12 and abs(vol - 8) <= 1e-12 and np.abs(av.sum(axis=0)).max() <= 1e-12
    assert np.all((av * ctr).sum(axis=1) > 0)
    g = (np.arange(4) + 0.5) / 4
    X = np.array([[x, y] for y in g for x in g])
    W = np.full_like(X, 0.25)
    ghosts, Q, dmin, near = G.hcube_reference(X, W, [0, 0], [1, 1], [(1, True)], 1.5)
    assert np.array_equal(ghosts, np.nonzero(1 - X[:, 0] < 1.5 * 0.25 * np.sqrt(2))[0]) and ghosts.size == 8
    assert np.all(Q[:, 0] == 1) and np.array_equal(Q[:, 1], X[ghosts, 1]) and near.size == 0


# ---------------------------------------------------------------------------------------------------------------------
# the comparison
# ---------------------------------------------------------------------------------------------------------------------
def immersed_report(case, bname):
    """(failures, figures) of one immersed boundary against the reference.  ``failures`` is a list of sentences, empty if
    the tables are the geometry's; ``figures`` holds every measured maximum relative to its bound and the counts."""
    stl = case.stl(bname)
    ref = case.reference(bname)
    got = gathered(case.dom, bname)
    B = G.dist_bound(stl)
    fails, fig = [], {"ghosts": int(ref["ghosts"].size), "near_threshold": int(ref["near"].size)}
    differ = np.setxor1d(got["ghosts"], ref["ghosts"])
    unexcused = np.setdiff1d(differ, ref["near"])
    fig["ghost_set_differs"], fig["ghost_set_excused"] = int(differ.size), int(differ.size - unexcused.size)
    if unexcused.size:
        fails.append(f"ghost set: {unexcused.size} cells differ from the reference away from the threshold, first "
                     f"{unexcused[:5].tolist()} (d / threshold {(ref['d'] / (RATIO * case.diam))[unexcused[:5]]})")
    if ref["near"].size > CAP * ref["ghosts"].size:
        fails.append(f"ghost set: {ref['near'].size} cells within the rounding band of the threshold (cap "
                     f"{CAP * ref['ghosts'].size:.1f})")
    if not np.array_equal(np.sort(got["ghosts"]), got["ghosts"]) or np.unique(got["ghosts"]).size != got["ghosts"].size:
        fails.append("ghost indices are not ascending and unique over the chunks")
    # per ghost that both sides list
    _, ig, ir = np.intersect1d(got["ghosts"], ref["ghosts"], return_indices=True)
    x = case.X[got["ghosts"][ig]]
    proj = got["proj"][ig]
    off_surface = G.closest_on_surface(stl, proj)[0]
    derr = np.abs(np.sqrt(((proj - x) ** 2).sum(axis=1)) - ref["d"][got["ghosts"][ig]])
    gd_ref, id_ref = ref["ghost_distances"][ir], ref["image_distances"][ir]
    defined = gd_ref >= 16 * B
    fig["undefined_normals"] = int((~defined).sum())
    nerr = np.sqrt(((got["normals"][ig] - ref["normals"][ir]) ** 2).sum(axis=1))
    eta_got = got["gd"][ig] / got["idist"][ig]
    checks = {
        "projection off the surface": (off_surface, B),
        "| |proj - x| - d_exact |": (derr, B),
        "ghost distance": (np.abs(got["gd"][ig] - gd_ref), B),
        "image distance": (np.abs(got["idist"][ig] - id_ref), B),
        "normal": (np.where(defined, nerr, 0.0), B / np.where(defined, gd_ref, 1.0)),
        "eta": (np.abs(eta_got - ref["eta"][ir]), (1 + ref["eta"][ir]) * B / (id_ref - B)),
    }
    for what, (err, bound) in checks.items():
        ratio = err / bound
        fig[what] = float(ratio.max()) if ratio.size else 0.0
        if ratio.size and not ratio.max() <= 1.0:
            k = int(np.argmax(ratio))
            fails.append(f"{what}: {ratio.max():.3g} x its bound at ghost cell {int(got['ghosts'][ig][k])} "
                         f"({int((ratio > 1).sum())} above)")
    if fig["undefined_normals"] > CAP * ref["ghosts"].size:
        fails.append(f"{fig['undefined_normals']} ghosts closer to the wall than 16 bounds")
    return fails, fig


def cached_report(case, bname):
    if bname not in case._report:
        case._report[bname] = immersed_report(case, bname)
    fails, fig = case._report[bname]
    return list(fails), dict(fig)


def test_precondition_search_radius_holds_every_winning_simplex(immersed):
    worst = {}
    for case, bname in immersed:
        worst[f"{case.name}/{bname}"] = p = case.precondition(bname)
        assert p <= 1.0, (case.name, bname, p)
    print("\ncircumradius about the centre / (ratio x smallest ghost diameter):", {k: round(v, 3) for k, v in worst.items()})
    assert max(worst.values()) <= 0.5       # (measured 0.04 .. 0.38: a mesh change that halves the margin is seen)


def test_ghosts_projections_and_boundary_fields(immersed):
    """Every immersed boundary: ghost set, foot points (on the surface, at the exact distance), normals, distances, eta.
    Worst ratios to the bounds measured: projection off the surface 0.21 (plate; 0.13 on the sphere, 3.0e-8), distance 0.20
    (plate), ghost distance 0.34 and image distance 0.50 (its eps(Float32) summand on a bound of two), eta 0.31; no cell
    within the threshold band, no ghost set differs, no ghost closer than 16 B.  The normals (worst 0.72) are named in a test
    of their own."""
    print()
    for case, bname in immersed:
        fails, fig = cached_report(case, bname)
        print(f"{case.name}/{bname}: " + ", ".join(f"{k} {v:.3g}" if isinstance(v, float) else f"{k} {v}" for k, v in fig.items()))
        assert not fails, (case.name, bname, fails)
        assert fig["near_threshold"] == 0 and fig["ghost_set_differs"] == 0, (case.name, bname, fig)
        assert fig["undefined_normals"] == 0, (case.name, bname, fig)
    counts = {f"{c.name}/{b}": c.reference(b)["ghosts"].size for c, b in immersed}
    assert counts["advection/upper"] == counts["advection/lower"] == 256
    assert [counts[f"rae level {l}/wall"] for l in range(3)] == [1608, 782, 377]
    assert (counts["sphere/sphere"], counts["sphere coarse/sphere"], counts["sphere chunked/sphere"]) == (1200, 408, 1200)


def test_normals_against_the_exact_foot_point(immersed):
    """|n_got - n_ref| <= B / ghost distance, n_ref from the exact foot point, on every ghost farther from the wall than 16 B.

    Measured worst ratios: advection walls 0.50, RAE2822 levels 0.52, plate 0.63, sphere 0.65, coarse sphere 0.72.

    The two projection conditions of ``test_ghosts_projections_and_boundary_fields`` (on the surface and at the exact distance,
    both within B) do not imply this one: a foot may slide along the surface by sqrt(2 d B) and keep both.  It is this
    check that found the builder's Float32 projection out: it read 465 on the sphere (20 of 1 200 ghosts, inside it, as
    close to two facets as Float32 can tell -- distances 2.2e-8 apart at 0.442 -- with the stored foot on the other one, 1.1e-4
    away, and the normal 2.5e-4 off) and 17.7 / 34.7 / 21 on the RAE levels (6 / 3 / 1 ghosts: feet on the neighbouring
    segment, or the nearest simplex CENTRE kept as the foot because its Float32 rounding lay 1.5e-9 closer to the cell than
    the segment itself).  The builder now evaluates feet and distances in Float64 and rounds the chosen foot once."""
    print()
    worst = {}
    for case, bname in immersed:
        fails, fig = cached_report(case, bname)
        worst[f"{case.name}/{bname}"] = fig["normal"]
    print("normals, worst ratio to B / ghost distance:", {k: f"{v:.3g}" for k, v in worst.items()})
    assert max(worst.values()) <= 1.0, worst


# ---------------------------------------------------------------------------------------------------------------------
# image interpolator
# ---------------------------------------------------------------------------------------------------------------------
def oracle_moments(case, targets32, about):
    """(sum w - 1, sum w (X_j - about)) per row of the oracle's ``nninterp.Interpolator`` built on the same cells for the
    Float32 ``targets32``, in float64 about the points ``about``."""
    from oracle import nninterp
    acc = nninterp.Interpolator(case.X.astype(f32), np.asarray(targets32, f32), first_index=True, linear=True)
    ia, wa = acc.decompose()
    off = np.concatenate([[0], np.cumsum([len(i) for i in ia])])
    return G.row_moments(off, np.concatenate(ia), np.concatenate(wa), case.X, about)


def interpolator_report(case, bname):
    """(failures, figures): the image interpolator rows of every chunk against the REFERENCE image points."""
    ref = case.reference(bname)
    got = gathered(case.dom, bname)
    fails, fig = [], {}
    if not np.array_equal(got["ghosts"], ref["ghosts"]):
        return ["ghost sets differ: the rows cannot be matched to reference image points"], fig
    nd = case.X.shape[1]
    k = 2 ** nd
    images = ref["images"]
    inside = case.inside(images)
    fig["excluded"] = int((~inside).sum())
    tie = 2 * G.ULP32 * float(np.abs(case.X).max())
    kth = G.knn_brute(case.X, images, k)
    # "the same targets": the points the tables call for, proj + normal x image distance in the Float32 arithmetic of the
    # builder, formed HERE from the tables (which the field checks pin to the reference); an interpolator built anywhere
    # else shows moments about the reference image point that the oracle's rows for these targets do not
    parts = case.dom.boundaries[bname]
    nominal = np.concatenate([(b.projections + b.normals * b.image_distances[:, None]).astype(f32) for b in parts.values()])
    m0o, m1o = oracle_moments(case, nominal[inside], images[inside])
    diam = case.diam[ref["ghosts"]]
    s0_oracle = float(np.abs(m0o).max())
    s1_oracle = float((np.sqrt((m1o * m1o).sum(axis=1)) / diam[inside]).max())
    s = 0
    s0, s1, far, nrow = [], [], 0, []
    for key, b in case.dom.boundaries[bname].items():
        acc = b.image_interpolator
        ng = b.ghost_indices.size
        donors = np.asarray(b.image_domain, np.int64)[np.asarray(acc.idx, np.int64)]
        rows = np.repeat(np.arange(ng), np.diff(acc.off))
        dd = np.sqrt(((case.X[donors] - images[s:s + ng][rows]) ** 2).sum(axis=1))
        far += int((dd > kth[s:s + ng][rows] + tie).sum())
        nrow.append(np.diff(acc.off))
        m0, m1 = G.row_moments(acc.off, donors, acc.w, case.X, images[s:s + ng])
        s0.append(np.abs(m0))
        s1.append(np.sqrt((m1 * m1).sum(axis=1)) / diam[s:s + ng])
        s += ng
    s0, s1, nrow = np.concatenate(s0), np.concatenate(s1), np.concatenate(nrow)
    fig.update(sum_defect=float(s0[inside].max()), sum_defect_oracle=s0_oracle, moment=float(s1[inside].max()),
               moment_oracle=s1_oracle, moment_outside=float(s1[~inside].max()) if (~inside).any() else 0.0)
    if far:
        fails.append(f"{far} donors are farther from the reference image point than its {k} nearest cells")
    if nrow.min() < 1 or nrow.max() > k:
        fails.append(f"rows of {nrow.min()} .. {nrow.max()} donors")
    if not fig["sum_defect"] <= 4 * s0_oracle:
        fails.append(f"|sum w - 1| = {fig['sum_defect']:.3g} > 4 x the oracle's {s0_oracle:.3g}")
    if not fig["moment"] <= 4 * s1_oracle:
        fails.append(f"|sum w (X - x_img)| / diam = {fig['moment']:.3g} > 4 x the oracle's {s1_oracle:.3g}")
    return fails, fig


# ghosts whose reference image point lies outside the box of cell centres, from the reference geometry: on the 512-cell
# sphere level the image distance (1.5 diagonals of a cell of width 0.5: 1.3) carries 288 of the 408 image points past the
# outermost centres at +-1.75 (96 of them past the mesh box itself, and the 8 donors of 48 of those span no linear field:
# moments near 0.46 of a diameter, sum defects of 0.2 -- a property of the set-up)
EXCLUDED = {"sphere coarse/sphere": 288}


def test_image_interpolator_rows_against_reference_image_points(immersed):
    """Donors are the 2^nd nearest cells of the REFERENCE image point and the rows reproduce constants and linear fields
    there.  Measured, product and oracle alike to three digits (same donors, and about the reference image point the
    moments of both are those of the distance between the tables' image point and the reference's): |sum w - 1| 5.8e-8
    (advection) .. 2.1e-7 (plate, RAE level 0); |sum w (X - x_img)| / diam 1.9e-6 (coarse sphere), 3.0e-5 (plate), 3.5e-5
    (advection), 7.2e-6 (sphere), 1.4e-3 / 1.9e-3 / 1.2e-2 (RAE
    levels 2 / 1 / 0: ghosts at 1e-5 from the wall, whose normal moves by B / distance and the image point with it);
    asserted at 4 x the oracle's."""
    print()
    for case, bname in immersed:
        fails, fig = interpolator_report(case, bname)
        print(f"{case.name}/{bname}: " + ", ".join(f"{k} {v:.3g}" if isinstance(v, float) else f"{k} {v}" for k, v in fig.items()))
        assert not fails, (case.name, bname, fails)
        assert fig["excluded"] == EXCLUDED.get(f"{case.name}/{bname}", 0), (case.name, bname, fig["excluded"])


# ---------------------------------------------------------------------------------------------------------------------
# hypercube families
# ---------------------------------------------------------------------------------------------------------------------
def test_hypercube_families(adv_case, rae_cases):
    """``outlet`` of the advection case and ``farfield`` of the RAE levels: ghost sets equal the reference's (no cell within
    the threshold band), foot points bit for bit (the cell's own coordinates with the plane's coordinate in one place)."""
    for case, bname, hfaces in [(adv_case, *ADV_FAMILIES[0])] + [(c, *RAE_FAMILIES[0]) for c in rae_cases]:
        msh = case.dom.mesh
        ghosts, Q, dmin, near = G.hcube_reference(case.X, case.W, msh.origin, msh.widths, hfaces, RATIO)
        got = gathered(case.dom, bname)
        assert near.size == 0, (case.name, near)
        assert ghosts.size > 0 and np.array_equal(got["ghosts"], ghosts), case.name
        assert np.array_equal(got["proj"], Q), case.name
        fields = G.boundary_reference(case.X[ghosts], Q, case.W[ghosts], RATIO)
        B = 2 * G.ULP32 * float(np.abs(case.X).max())     # the same two-ulp bound on the magnitude of the coordinates
        assert np.abs(got["gd"] - fields["ghost_distances"]).max() <= B
        assert np.abs(got["idist"] - fields["image_distances"]).max() <= B
        assert (np.sqrt(((got["normals"] - fields["normals"]) ** 2).sum(axis=1)) * fields["ghost_distances"]).max() <= B


# ---------------------------------------------------------------------------------------------------------------------
# 3-D surface
# ---------------------------------------------------------------------------------------------------------------------
def test_3d_surface_of_the_sphere(sphere_cases):
    """``Surface`` of the sphere: control points are the triangle centroids, normals point outwards, the areas are those of
    the polyhedron: sum A = area, sum A n = 0 and sum A (c . n) / 3 = volume, each to 1e-5 relative (a bound for Float32 sums of
    7 200 terms; the sums here are float64 over the Float32 tables, whose terms carry a few 2^-24 each); both interpolators reproduce constants and linear fields at the control and offset points within 4 x the
    oracle's moments.  Measured: area 5.2e-9, closure 2.7e-10 of the area, volume 4.7e-9; moments / diam at the control
    points 2.5e-7 / 2.5e-7 (product / oracle), at the offset points 2.6e-7 / 1.9e-7; sum defects 2.8e-7 / 2.8e-7 and
    1.9e-7 / 1.9e-7.  With the reference's tables (areas = norms of the cross products + eps, normals divided by the same)
    the three sums miss by 1.00007, 4e-10 and 1.0: ``make_surface`` departs from it in 3-D."""
    case = sphere_cases[0]
    surf = case.dom.surfaces["sphere"]
    stl = case.stl("sphere")
    area, vol, av, ctr = G.polyhedron(stl)
    assert 0.97 < area / (4 * np.pi) < 1 and 0.95 < vol / (4 * np.pi / 3) < 1        # (inscribed in the unit sphere)
    A, n, c = surf.areas.astype(f64), surf.normals.astype(f64), surf.points.astype(f64)
    assert np.abs(c - ctr).max() <= 2 * G.ULP32
    assert np.all((n * c).sum(axis=1) > 0.9)                                        # outwards: n . c ~ +1
    assert np.abs(np.sqrt((n * n).sum(axis=1)) - 1).max() <= 4 * G.ULP32
    fig = dict(area=abs(A.sum() - area) / area, closure=np.abs((A[:, None] * n).sum(axis=0)).max() / area,
               volume=abs((A * (c * n).sum(axis=1)).sum() / 3 - vol) / vol)
    print("\nsurface integrals against the polyhedron:", {k: f"{v:.3g}" for k, v in fig.items()})
    assert fig["area"] <= 1e-5 and fig["closure"] <= 1e-5 and fig["volume"] <= 1e-5, fig
    # the oracle's own simplex-by-simplex centres and normals are the product's, bit for bit
    from ibamd.mesher import centers_and_normals as product_cn
    from oracle.mesher import centers_and_normals as oracle_cn
    for a, b in zip(product_cn(stl), oracle_cn(stl)):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    # interpolators: rows evaluated AT the control points (donors searched at the biased point), and at the offset points
    h = surf.offsets.astype(f64)
    diam_near = h / 1.01
    targets = {"interpolator": c, "offset_interpolator": c + n * (h * RATIO)[:, None]}
    for name, T in targets.items():
        assert case.inside(T).all()
        acc = getattr(surf, name)
        m0, m1 = G.row_moments(acc.off, acc.idx, acc.w, case.X, T)
        from oracle import nninterp
        bias = (n * h[:, None]).astype(f32) if name == "interpolator" else None
        oacc = nninterp.Interpolator(case.X.astype(f32), T.astype(f32), bias=bias, first_index=True)
        ia, wa = oacc.decompose()
        off = np.concatenate([[0], np.cumsum([len(i) for i in ia])])
        o0, o1 = G.row_moments(off, np.concatenate(ia), np.concatenate(wa), case.X, T)
        s0, s1 = np.abs(m0).max(), (np.sqrt((m1 * m1).sum(axis=1)) / diam_near).max()
        t0, t1 = np.abs(o0).max(), (np.sqrt((o1 * o1).sum(axis=1)) / diam_near).max()
        print(f"{name}: sum defect {s0:.3g} (oracle {t0:.3g}), moment / diam {s1:.3g} (oracle {t1:.3g})")
        assert s0 <= 4 * t0 and s1 <= 4 * t1, (name, s0, t0, s1, t1)


# ---------------------------------------------------------------------------------------------------------------------
# teeth
# ---------------------------------------------------------------------------------------------------------------------
def _sphere_report():
    case = Case("sphere under a defect", ibamd.Domain(sphere_mesh()))
    return immersed_report(case, "sphere")


def test_teeth_nearest_centre_instead_of_projection(monkeypatch):
    """``_project_3d`` replaced by "the nearest simplex centre": a point of the surface, but not the closest one."""
    monkeypatch.setattr(D, "_project_3d", lambda dfield, X, R: dfield.centers[:, dfield.nn(X)[0]].copy())
    fails, fig = _sphere_report()
    assert any("d_exact" in f for f in fails) and fig["projection off the surface"] <= 1.0, (fails, fig)


@pytest.mark.parametrize("scale", [0.5, 0.0])
def test_teeth_pruning_bound_that_drops_winners(monkeypatch, sphere_cases, scale):
    """The pruning of ``_project_3d`` with the simplex radius scaled down: a triangle whose centre is farther than the
    nearest centre by more than ``scale`` radii is dropped although it can hold the closest point.  No wrong table passes:
    either the comparison reports a failure or every foot point is, bit for bit, that of the sound build.

    Halved, the radius drops no winner on this sphere (measured down to a tenth of it: the tables stay bit-identical),
    so there is no wrong table to report.  With the radius dropped from the bound
    (scale 0) 72 ghosts take the foot of the wrong triangle and the distance check reports 2.3e3 x its bound."""
    real = D._tri_cache

    def scaled(dfield):
        T0, T1, T2, (M, pinvM, rmax) = real(dfield)
        return T0, T1, T2, (M, pinvM, rmax * scale)
    monkeypatch.setattr(D, "_tri_cache", scaled)
    case = Case("sphere under a defect", ibamd.Domain(sphere_mesh()))
    fails, fig = immersed_report(case, "sphere")
    sound, got = gathered(sphere_cases[0].dom, "sphere"), gathered(case.dom, "sphere")
    same = all(np.array_equal(sound[k], got[k]) for k in sound)
    assert fails or same, fig
    if scale == 0.0:
        assert any("d_exact" in f for f in fails), (fails, fig)


def test_teeth_negated_normals(monkeypatch):
    real = D._make_boundary

    def negated(*a):
        b = real(*a)
        b.normals = -b.normals
        return b
    monkeypatch.setattr(D, "_make_boundary", negated)
    fails, fig = _sphere_report()
    assert any(f.startswith("normal") for f in fails) and fig["normal"] > 1e4, (fails, fig)

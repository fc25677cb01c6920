"""Flow regimes for the per-cell checks of the fused sweeps: seeded, deterministic Float32 fields of the cell centres.

``conftest.euler_field`` is one state (Mach 0.3, every component positive, noisy p and T) and the advecting velocities of
tests/test_gpu_percell.py never change sign.  The fields here reach the branches those leave alone: the two clamps of the
HLL wave speeds (SR = min(uR - aR, 0), SL = max(uL + aL, 0)), velocities that change sign or vanish, the max(T, 10) clamp,
the 1e-7 floor of the JST sensor, and |C| far from 1 or changing sign inside a block.  ``s`` below is a smooth sin * cos
of the centres normalised to the partition's box, ``r`` uniform noise in [-1, 1].

No field puts a face at SL = SR = 0 (left state supersonic to the left, right state supersonic to the right: 0 / 0):
whether MUSCL's reconstructed states land there differs between Float32 and float64.  ``euler_coverage`` asserts the
distance from that point together with each regime's own branch, from the float64 reference's intermediate values.
"""
import numpy as np

from oracle import cfd as ocfd
from oracle import domain as od

f32, f64 = np.float32, np.float64
FLOOR = f64(f32(1e-7))   # the oracle's Float32 constant
GAP = 0.05   # smallest SL - SR allowed, in sound speeds: a million Float32 roundings away from 0 / 0
A0 = 340.0   # speed of sound at 288.15 K (sqrt(1.4 * 283 * 288.15) = 337.9), rounded

EULER_REGIMES = ("supersonic+", "supersonic-", "transonic", "crossing", "stagnation", "rest", "floor", "cold", "jump")
C_REGIMES = ("crossing", "zero", "big", "tiny")
U_KINDS = ("noisy", "smooth", "flat", "step")


def _xi(x):
    x = np.asarray(x, f64)
    lo, hi = x.min(axis=0), x.max(axis=0)
    return (x - lo) / (hi - lo)


def smooth(x, k=0):
    """s_k in [-1, 1]: sin(2 pi (xi_a + 0.17 k)) cos(2 pi (xi_b + 0.29 k)) with a = k mod nd, b = a + 1 mod nd."""
    xi = _xi(x)
    nd = xi.shape[1]
    return np.sin(2 * np.pi * (xi[:, k % nd] + 0.17 * k)) * np.cos(2 * np.pi * (xi[:, (k + 1) % nd] + 0.29 * k))


def _linear_pressure(part):
    """A pressure that is exactly linear in the cell index, in Float32 and float64 alike: 65536 + c (n_1 + .. + n_nd) with
    n_d the centre's coordinate in half finest spacings (an integer on every level) and c a power of two that keeps p
    below 131072, so every value and every face difference is exact.  The JST sensor of a uniform p is 1e-7 / 1e-7 = 1
    and that of a rounded smooth p is its curvature over its slope; only an exactly linear p puts
    (1e-7 + |green_gauss(dp)|) / (1e-7 + unsigned_green_gauss(|dp|)) below 1e-7, i.e. the sensor on its floor."""
    x = np.asarray(part.centers, f64)
    g = float(np.asarray(part.spacing, f64).min()) / 2
    n = np.rint((x - x.min(axis=0)) / g).sum(axis=1)
    c = 2.0 ** np.floor(np.log2(60000.0 / max(n.max(), 1.0)))
    assert c >= 2.0 ** -7, "mesh too deep for an exactly linear Float32 pressure"
    p = (65536.0 + c * n).astype(f32)
    assert np.array_equal(p.astype(f64), 65536.0 + c * n)
    return p


def euler_regime(part, name, seed=7):
    """P = [p T u v (w)] of regime ``name`` on the cells of ``part``."""
    x = np.asarray(part.centers)
    n, nd = x.shape
    rng = np.random.default_rng(seed)

    def r():
        return rng.uniform(-1, 1, n)
    P = np.empty((n, nd + 2), f64)
    P[:, 0] = 1e5 * (1 + 0.05 * r())
    P[:, 1] = 288.15 * (1 + 0.05 * r())
    sgn = (1.0, -1.0, 1.0)
    if name in ("supersonic+", "supersonic-"):
        for d, M in enumerate((2.0, 1.5, 1.3)[:nd]):
            P[:, 2 + d] = M * A0 * (1 + 0.1 * r())
        if name == "supersonic-":
            P[:, 2:] *= -1
    elif name == "transonic":
        for d in range(nd):
            P[:, 2 + d] = sgn[d] * A0 * (1 + 0.3 * smooth(x, d) + 0.02 * r())
    elif name == "crossing":
        for d in range(nd):
            P[:, 2 + d] = sgn[d] * (3 * A0 * smooth(x, d) + 10 * r())
    elif name == "stagnation":
        for d in range(nd):
            P[:, 2 + d] = 5 * smooth(x, d) + 0.5 * r()
    elif name == "rest":
        P[:, 2:] = 0
    elif name == "floor":
        P[:, 0] = _linear_pressure(part)
        P[:, 1] = 288.15 * (1 + 0.05 * smooth(x, 3))
        for d, (U, sg) in enumerate(((100.0, 1), (50.0, -1), (75.0, 1))[:nd]):
            P[:, 2 + d] = U * (1 + sg * 0.3 * smooth(x, d))
    elif name == "cold":
        # a(10 K) = 63: velocities of +-30 keep every face subsonic, so that the sound speed of both sides enters the flux
        # (at the present 100 m/s every face would have SR = 0 and F = FL, whatever a is)
        P[:, 1] = 10 * (1 + 0.5 * r())
        for d in range(nd):
            P[:, 2 + d] = sgn[d] * 30 * (1 + 0.1 * r())
    elif name == "jump":
        xi = _xi(x)
        up = xi[:, 1] > xi[:, 0]
        P[up] = [1e6, 600.0] + [500.0] * nd
        P[~up] = [1e5, 288.0] + [0.0] * nd
    else:
        raise KeyError(name)
    return P.astype(f32)


def c_regime(part, name, seed=11):
    """Advecting velocity C (nc, nd) of regime ``name``."""
    x = np.asarray(part.centers)
    n, nd = x.shape
    rng = np.random.default_rng(seed)
    sgn = (1.0, -1.0, 1.0)
    if name in ("crossing", "tiny"):
        C = np.stack([sgn[d] * smooth(x, d) + 0.05 * rng.uniform(-1, 1, n) for d in range(nd)], axis=1)
        if name == "tiny":
            C *= 1e-3
    elif name == "zero":
        C = np.zeros((n, nd))
    elif name == "big":
        C = np.stack([50 + 10 * rng.uniform(-1, 1, n), -30 + 10 * rng.uniform(-1, 1, n), np.full(n, 20.0)][:nd], axis=1)
    else:
        raise KeyError(name)
    return np.ascontiguousarray(C.astype(f32))


def u_kind(part, kind, seed=13):
    """Advected scalar: smooth with 10 % noise, smooth without noise, 1 + 1e-6 r, or the step across the diagonal."""
    x = np.asarray(part.centers)
    n = x.shape[0]
    rng = np.random.default_rng(seed)
    if kind == "noisy":
        u = smooth(x, 1) + 0.1 * rng.uniform(-1, 1, n)
    elif kind == "smooth":
        u = smooth(x, 1)
    elif kind == "flat":
        u = 1 + 1e-6 * rng.uniform(-1, 1, n)
    elif kind == "step":
        u = (x[:, 1] > x[:, 0]).astype(f64) + 0.01 * rng.uniform(-1, 1, n)
    else:
        raise KeyError(kind)
    return u.astype(f32)


# ---------------------------------------------------------------------------------------------------------------------
# which branches a field reaches, from the float64 reference's own intermediate values
# ---------------------------------------------------------------------------------------------------------------------
def euler_branches(op, P, fluid=None):
    """Shares of the float64 Euler reference (``op``: an oracle view): faces with SR = 0, with SL = 0, with the sensor
    blend at its floor Df = 1e-7 (``floor``: of all faces; ``floor_uniform``: of the ``uniform`` share of faces, those
    between two cells whose every side is a face to one cell of their own level), cells with T < 10, and the smallest
    SL - SR of any face over the local sound speed."""
    import percell as pc
    same = pc._side_classes(op)["side_same"]
    fluid = fluid or ocfd.Fluid()
    P = np.asarray(P).astype(f64)
    D = od.JST_sensor(op, np.ascontiguousarray(P[:, 0]))
    nf = sr0 = sl0 = fl = nu = flu = 0
    gap = np.inf
    for dim in range(1, op.ndims + 1):
        gP = od.cell_gradient(op, P, dim)
        PL, PR = od.MUSCL(op, P, gP, dim, D=D, high_order=True)
        aL, aR = ocfd.speed_of_sound(fluid, PL[:, 1]), ocfd.speed_of_sound(fluid, PR[:, 1])
        SR = np.minimum(PR[:, 1 + dim] - aR, 0.0)
        SL = np.maximum(PL[:, 1 + dim] + aL, 0.0)
        o, nb = op.face_owners_neighbors[dim]
        Df = np.maximum(np.maximum(D[o], D[nb]), FLOOR)
        nf += SR.size
        sr0 += int((SR == 0).sum())
        sl0 += int((SL == 0).sum())
        fl += int((Df == FLOOR).sum())
        uni = same[o] & same[nb]
        nu += int(uni.sum())
        flu += int((Df[uni] == FLOOR).sum())
        gap = min(gap, float(((SL - SR) / np.maximum(aL, aR)).min()))
    return dict(SR0=sr0 / nf, SL0=sl0 / nf, floor=fl / nf, uniform=nu / nf, floor_uniform=flu / max(nu, 1), cold=float((P[:, 1] < 10).mean()), gap=gap)


def assert_euler_coverage(op, P, name, what=""):
    """The regime reaches its branch on this mesh, and no face is near SL = SR = 0."""
    b = euler_branches(op, P)
    msg = f"{what} {name}: {b}"
    assert b["gap"] >= GAP, msg
    if name == "supersonic+":
        assert b["SR0"] == 1.0 and b["SL0"] == 0.0, msg
    elif name == "supersonic-":
        assert b["SL0"] == 1.0 and b["SR0"] == 0.0, msg
    elif name == "transonic":
        assert b["SR0"] >= 0.01 and b["SL0"] >= 0.01 and b["SR0"] < 0.99 and b["SL0"] < 0.99, msg
    elif name == "crossing":
        assert b["SR0"] >= 0.01 and b["SL0"] >= 0.01, msg
    elif name in ("stagnation", "rest"):
        assert b["SR0"] == 0.0 and b["SL0"] == 0.0, msg
    elif name == "cold":
        assert b["cold"] >= 0.25 and b["SR0"] == 0.0 and b["SL0"] == 0.0, msg
    elif name == "floor":
        # A cell with a face to another level, a mirror face or no face on one side has a sensor of order 1 whatever p
        # is (its two one-sided differences span different distances), so the floor's share of ALL faces is the mesh's
        # share of uniform faces (65 % .. 91 % on the test meshes), not the field's to choose: the field guarantees the
        # floor on every uniform face, and those are the majority.
        assert b["floor_uniform"] == 1.0 and b["floor"] >= b["uniform"] >= 0.5, msg
    return b


def cf_signs_in_blocks(part, C, block=None):
    """Number of blocks (``block`` consecutive cells: 64 in 2-D, 512 in 3-D) inside which the face value of some C_d
    takes both signs, and the number of faces where it is exactly 0."""
    C = np.asarray(C).astype(f64)
    block = block or 8 ** part.ndims
    nb_ = -(-C.shape[0] // block)
    both = np.zeros(nb_, bool)
    zeros = 0
    for d in range(1, part.ndims + 1):
        Cf = od.at_faces(part, np.ascontiguousarray(C[:, d - 1]), d)
        o, _ = part.face_owners_neighbors[d]
        pos = np.bincount(o[Cf > 0] // block, minlength=nb_) > 0
        neg = np.bincount(o[Cf < 0] // block, minlength=nb_) > 0
        both |= pos & neg
        zeros += int((Cf == 0).sum())
    return int(both.sum()), zeros

"""Model of the fused Euler sweep with the sensor-scaled central + Rusanov flux (``ibamd.residual_euler_sensor``).

Test infrastructure.  The closure, composed from the oracle's operators like ``percell.oracle_euler_residual``:

    D = JST_sensor(part, P[:, 1]);  nu = the caller's (nc values), or D
    per dim: gP = cell_gradient(part, P, dim);  PL, PR = MUSCL(part, P, gP, dim; D = D, high_order = true)
             F = inviscid_fluxes(fluid, PL, PR, at_owners(part, nu, dim), at_neighbors(part, nu, dim), dim)   (cfd.jl:516-554)
             R .-= green_gauss(part, F, dim)

Everything is in the dtype of ``P``: Float32 in gives the Float32 oracle the literal device form reproduces bit for bit,
float64 in the reference of the per-cell checks.  ``sensor_scale`` is the scale of those checks and ``BOUND_SENSOR`` their
bound (calibrated in tests/test_euler_sensor.py).
"""
import numpy as np

import percell as pc
from oracle import cfd as ocfd
from oracle import domain as od

f32, f64 = np.float32, np.float64

# Per-cell bound of the device forms against the float64 reference under ``sensor_scale``: 4 x the worst Float32-oracle
# figure of tests/test_euler_sensor.py::test_calibration (the rule of percell.py), rounded up to one digit.  It must not
# exceed percell.BOUND_EULER; the figures are in that module's docstring.
BOUND_SENSOR = 2e-6


def oracle_euler_sensor_residual(part, P, fluid, nu=None):
    """The closure above on an oracle view ``part``, in the dtype of ``P`` (``nu`` is converted to it)."""
    R = np.zeros_like(P)
    D = od.JST_sensor(part, np.ascontiguousarray(P[:, 0]))
    nu = D if nu is None else np.asarray(nu).astype(P.dtype)
    for dim in range(1, part.ndims + 1):
        gP = od.cell_gradient(part, P, dim)
        PL, PR = od.MUSCL(part, P, gP, dim, D=D, high_order=True)
        F = ocfd.inviscid_fluxes_sensor(fluid, PL, PR, od.at_owners(part, nu, dim), od.at_neighbors(part, nu, dim), dim)
        R -= od.green_gauss(part, F, dim)
    return R


def ref64_euler_sensor(part, P, nu=None, fluid=None):
    r = oracle_euler_sensor_residual(part, np.asarray(P).astype(f64), fluid or ocfd.Fluid(), nu)
    assert r.dtype == f64
    return r


def sensor_scale(part, P, ref, fluid=None):
    """(nc, nv) scale of the residual: |ref_v| + max over the cell's two-deep face neighbourhood of
    sum_d [|Uc_v| (|u_d| + a) + |p| in the momentum row d] / h, with Uc = primitive2state(P) carrying E + p in the energy row
    and a = speed_of_sound(T): the flux (UcL + UcR) u / 2 + p + (UcL - UcR) nu (a + |u|) / 2 with every difference turned into
    a sum and nu <= 1, as ``percell.euler_scale_waves`` is for HLL."""
    fluid = fluid or ocfd.Fluid()
    P64 = np.asarray(P).astype(f64)
    Uc = ocfd.primitive2state(fluid, P64)
    Uc[:, 1] += P64[:, 0]
    Uc = np.abs(Uc)
    a = ocfd.speed_of_sound(fluid, P64[:, 1]).astype(f64)
    p = np.abs(P64[:, 0])
    W = np.zeros_like(P64)
    for d in range(1, part.ndims + 1):
        W += Uc * (np.abs(P64[:, 1 + d]) + a)[:, None]
        W[:, 1 + d] += p
    m = pc._face_max(part, pc._face_max(part, W))
    h = np.asarray(part.spacing).min(axis=1).astype(f64)
    return np.abs(np.asarray(ref, dtype=f64)) + m / h[:, None]


def external_nu(n, seed=5):
    """A caller's sensor: uniform noise in [0, 1]."""
    return np.random.default_rng(seed).uniform(0, 1, n).astype(f32)


def regime_partitions(adv_mesh, rae_mesh):
    """{name: partition} of the four small meshes of tests/test_gpu_percell_regimes.py (its ``meshes`` fixture), built on the
    host alone: the advection mesh in one partition, partition 2 of the 6144-cell RAE2822 cut, the corner octree and
    partition 1 of the sphere."""
    import bench
    import ibamd
    from conftest import ADV_FAMILIES, RAE_FAMILIES
    from ibamd.mesher import Ball, Mesh
    out = {}
    dom = ibamd.Domain(adv_mesh, hypercube_families=ADV_FAMILIES, max_partition_size=10 ** 9, boundaries=False)
    (out["adv"],) = dom.partitions.values()
    dom = ibamd.Domain(rae_mesh, hypercube_families=RAE_FAMILIES, max_partition_size=6144, boundaries=False, only=[2])
    out["rae6k_2"] = dom.partitions[2]
    msh = Mesh(f32([-2, -2, -2]), f32([4, 4, 4]), block_size=8,
               refinement_regions=[(Ball(np.array([-2.0, -2.0, -2.0]), 0.1), f32(0.1))])
    dom = ibamd.Domain(msh, max_partition_size=10 ** 9, boundaries=False)
    (out["corner"],) = dom.partitions.values()
    msh = Mesh(f32([-4, -4, -4]), f32([8, 8, 8]), ("sphere", bench.icosphere(subdiv=2), f32(0.2)), block_size=8)
    msh.distance_fields = {}
    mps = -(-(-(-len(msh) // 4)) // 512) * 512
    dom = ibamd.Domain(msh, max_partition_size=mps, boundaries=False, only=[1])
    out["sphere_1"] = dom.partitions[1]
    return out

"""The numpy model of the implicit residual smoothing (tests/smooth_model.py) against the properties of the operator it
iterates on: converged, it solves ``(I + eps L) S = R`` and keeps the sum; a constant is a fixed point; the float32 evaluation
-- the kernel's bits, tests/test_gpu_euler_smooth.py -- stays within a derived bound of the float64 one; ``eps = 0`` is the
identity.  On a uniform-plus-refined 2-D mesh and on a partition with coarse-fine faces, a skirt and CSR walks."""
import math

import numpy as np
import pytest

import ibamd
import smooth_model as sm
from conftest import ADV_FAMILIES, RAE_FAMILIES

f32, f64 = np.float32, np.float64
EPS = (0.5, 2.0)


@pytest.fixture(scope="module")
def cases(adv_mesh_coarse, rae_mesh_small):
    out = {}
    dom = ibamd.Domain(adv_mesh_coarse, hypercube_families=ADV_FAMILIES, max_partition_size=10 ** 9, boundaries=False)
    (part,) = dom.partitions.values()
    out["adv_coarse"] = (part, sm.face_table(part))
    dom = ibamd.Domain(rae_mesh_small, hypercube_families=RAE_FAMILIES, max_partition_size=6144, boundaries=False, only=[2])
    out["rae6k_2"] = (dom.partitions[2], sm.face_table(dom.partitions[2]))
    return out


MESHES = ("adv_coarse", "rae6k_2")


def noise(nc, seed):
    """Three columns of very different size, all positive (so that their sums are far from zero)."""
    rng = np.random.default_rng(seed)
    return (rng.uniform(0.5, 1.5, size=(nc, 3)) * np.array([1.0, 3.0e5, 2.5e2])).astype(f32)


def bound(n_max, eps, R):
    """Per element, for every column: ``2 (n_max + 3) (1 + eps n_max) 2^-24 max|R|``.  An iterate is a convex combination of
    R_i and its neighbours, so it stays within ``max|R|``, and what is rounded before the divide -- at most ``n_max - 1`` sums,
    the product with eps, the sum with R_i -- is bounded by ``(1 + eps n_i) max|R|`` and divided by ``1 + eps n_i``; with the
    denominator's two roundings and the divide that is at most ``n_max + 3`` roundings per iteration, each worth at most
    ``2^-24 max|R|`` in the result.  The error of the previous iterate enters contracted by ``rho = eps n / (1 + eps n)``,
    so the errors sum to at most ``1 / (1 - rho) = 1 + eps n_max`` times one iteration's.  The factor 2 covers second-order
    terms."""
    return 2.0 * (n_max + 3) * (1.0 + eps * n_max) * 2.0 ** -24 * np.abs(R).max(axis=0).astype(f64)


def test_the_meshes_hold_what_they_are_for(cases):
    (_, (_, n2)), (part, (T, n)) = cases["adv_coarse"], cases["rae6k_2"]
    assert n2.min() >= 1 and n.min() >= 1
    assert n.max() > 2 * part.ndims                      # sides with several faces: coarse-fine faces, CSR walks
    assert part.spacing.shape[0] > np.asarray(part.image_in_domain).size      # a skirt


@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("mesh", MESHES)
def test_converged_iteration_solves_the_system_and_keeps_the_sum(cases, mesh, eps):
    part, table = cases[mesh]
    nc = part.spacing.shape[0]
    R = noise(nc, 1).astype(f64)
    rho = sm.rho(table[1], eps)
    assert 0.0 < rho < 1.0
    n_iter = int(math.ceil(math.log(1e-13) / math.log(rho))) + 1
    assert rho ** n_iter < 1e-13
    S = sm.model(part, R, eps, n_iter, f64, table)
    res = np.abs(sm.apply_operator(part, S, eps, table) - R).max(axis=0)
    assert (res <= 1e-10 * np.abs(R).max(axis=0)).all(), res / np.abs(R).max(axis=0)
    dsum = np.abs(S.sum(axis=0) - R.sum(axis=0)) / np.abs(R.sum(axis=0))
    assert (dsum <= 1e-10).all(), dsum


@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("mesh", MESHES)
def test_a_constant_is_a_fixed_point(cases, mesh, eps):
    part, table = cases[mesh]
    nc, n_max = part.spacing.shape[0], int(table[1].max())
    R = np.tile(np.array([1.0, -3.25e5, 7.0e-3], dtype=f32), (nc, 1))
    for n_iter in (1, 8):
        S = sm.model(part, R, eps, n_iter, f32, table)
        assert (np.abs(S.astype(f64) - R.astype(f64)).max(axis=0) <= bound(n_max, eps, R)).all(), (n_iter, eps)
    S64 = sm.model(part, R, eps, 8, f64, table)
    assert (np.abs(S64 - R.astype(f64)).max(axis=0) <= 64 * 2.0 ** -53 * np.abs(R).max(axis=0)).all()


@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("mesh", MESHES)
def test_float32_within_the_bound_of_float64(cases, mesh, eps):
    part, table = cases[mesh]
    nc, n_max = part.spacing.shape[0], int(table[1].max())
    R = noise(nc, 2)
    b = bound(n_max, eps, R)
    for n_iter in (1, 2, 3, 8):
        S32 = sm.model(part, R, eps, n_iter, f32, table)
        S64 = sm.model(part, R, eps, n_iter, f64, table)
        assert S32.dtype == f32 and S64.dtype == f64
        err = np.abs(S32.astype(f64) - S64).max(axis=0)
        assert (err <= b).all(), (n_iter, eps, (err / b).tolist())


@pytest.mark.parametrize("mesh", MESHES)
def test_eps_zero_is_the_identity(cases, mesh):
    part, table = cases[mesh]
    R = noise(part.spacing.shape[0], 3)
    R[::7, 1] *= f32(-1)
    for n_iter in (1, 3):
        S = sm.model(part, R, 0.0, n_iter, f32, table)
        assert np.array_equal(S.view(np.uint32), R.view(np.uint32))
    assert np.array_equal(sm.model(part, R[:, 0].copy(), 0.0, 2, f32, table).view(np.uint32), R[:, 0].copy().view(np.uint32))

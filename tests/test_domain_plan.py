"""Tables of the device-resident domain call (``ibamd.domain.domain_plan_tables``, built the same way by
``ibh_domain_plan_create``): a numpy restatement of the gather / scatter kernels of csrc/ibh_domain.hip run over these
tables reproduces the per-partition copies of ``(dom::Domain)(f, args...)`` (ImmersedBoundary.jl:820-864) and the host
path's write-back.  No GPU needed."""
import types

import numpy as np
import pytest

import ibamd
from conftest import ADV_FAMILIES, RAE_FAMILIES, f32, seeded_field
from ibamd.domain import DOMAIN_PLAN_BLOCK, domain_plan_tables


@pytest.fixture(scope="module")
def adv_dom(adv_mesh):
    return ibamd.Domain(adv_mesh, hypercube_families=ADV_FAMILIES, max_partition_size=4096)


@pytest.fixture(scope="module")
def rae_dom(rae_mesh_small):
    return ibamd.Domain(rae_mesh_small, hypercube_families=RAE_FAMILIES, max_partition_size=16384, boundaries=False)


@pytest.fixture(scope="module")
def only_dom(adv_mesh):
    return ibamd.Domain(adv_mesh, hypercube_families=ADV_FAMILIES, max_partition_size=2048, only=[2, 4])


def _nv(a):
    return 1 if a.ndim == 1 else a.shape[1]


def gather(T, a):
    """k_domain_gather, workgroup by workgroup: ws[nv*ws_off[p] + v*n_p + i] = a[domain_p[i], v]."""
    nv = _nv(a)
    a2 = a.reshape(a.shape[0], nv)
    ws = np.full(nv * T["ws_off"][-1], np.nan, dtype=f32)
    for p, r0 in T["wg_gather"]:
        n_p = T["n"][p]
        i = np.arange(r0, min(r0 + DOMAIN_PLAN_BLOCK, n_p))
        g = T["rows"][T["row_off"][p] + i]
        for v in range(nv):
            ws[nv * T["ws_off"][p] + v * n_p + i] = a2[g, v]
    return ws


def local(T, ws, p, nv, ndim):
    """Partition p's local array: a view (n_p,) / (n_p, nv), column-major with ld = n_p."""
    n_p = T["n"][p]
    blk = ws[nv * T["ws_off"][p]:nv * T["ws_off"][p] + nv * n_p]
    return blk if ndim == 1 else blk.reshape(nv, n_p).T


def scatter(T, ws, a):
    """k_domain_scatter: a[image_p[j], v] = ws[nv*ws_off[p] + v*n_p + image_in_domain_p[j]]."""
    nv = _nv(a)
    a2 = a.reshape(a.shape[0], nv)
    for p, j0 in T["wg_scatter"]:
        n_p = T["n"][p]
        j = np.arange(T["img_off"][p] + j0, min(T["img_off"][p] + j0 + DOMAIN_PLAN_BLOCK, T["img_off"][p + 1]))
        g, li = T["image"][j], T["image_in_domain"][j]
        for v in range(nv):
            a2[g, v] = ws[nv * T["ws_off"][p] + v * n_p + li]


def _check(dom, arrays):
    T = domain_plan_tables(dom)
    assert T["ids"] == list(dom.partitions)
    wss = [gather(T, a) for a in arrays]
    for k, i in enumerate(T["ids"]):
        part = dom.partitions[i]
        for a, ws in zip(arrays, wss):
            loc = local(T, ws, k, _nv(a), a.ndim)
            assert np.array_equal(loc, np.array(a[part.domain]))       # `selectdim(a, 1, part.domain) |> copy`
            loc *= f32(2)                                               # the "closure": writes every local row
            loc += f32(i)
    # the host path's write-back, partition by partition (backend.domain_call with converters)
    exp = [a.copy() for a in arrays]
    for i in dom.partitions:
        part = dom.partitions[i]
        for e, a in zip(exp, arrays):
            e[part.image] = np.array(a[part.domain])[part.image_in_domain] * f32(2) + f32(i)
    got = [a.copy() for a in arrays]
    for g, ws in zip(got, wss):
        scatter(T, ws, g)
    for g, e in zip(got, exp):
        assert np.array_equal(g, e)
    return T


def test_adv_three_partitions_scalar_and_two_fields(adv_dom):
    assert len(adv_dom.partitions) == 3
    X = adv_dom.global_centers()
    T = _check(adv_dom, [seeded_field(X), seeded_field(X, nv=2, seed=3)])
    # every row of every partition is gathered by exactly one workgroup lane, every image row scattered once
    assert len(T["wg_gather"]) == sum(-(-int(n) // DOMAIN_PLAN_BLOCK) for n in T["n"])
    assert T["image"].size == len(adv_dom)   # the images of a full domain cover it


def test_rae_partitions_nv4(rae_dom):
    assert len(rae_dom.partitions) >= 2
    X = rae_dom.global_centers()
    _check(rae_dom, [seeded_field(X, nv=4, seed=7), seeded_field(X, seed=8)])


def test_only_subset_leaves_uncovered_rows(only_dom):
    assert list(only_dom.partitions) == [2, 4]
    X = only_dom.global_centers()
    T = _check(only_dom, [seeded_field(X), seeded_field(X, nv=2, seed=4)])
    assert T["image"].size < len(only_dom)   # rows outside partitions 2 and 4: untouched by _check's comparison


def test_workspace_blocks_are_256_byte_aligned(adv_dom, rae_dom, only_dom):
    for dom in (adv_dom, rae_dom, only_dom):
        T = domain_plan_tables(dom)
        assert T["ws_off"][0] == 0 and np.all(T["ws_off"] % 64 == 0)
        assert np.all(np.diff(T["ws_off"]) >= T["n"])
        for nv in (1, 2, 4, 5):
            assert np.all((nv * T["ws_off"] * 4) % 256 == 0)


def _fake_dom(n, parts):
    """A Domain-shaped object with hand-written partition tables (only what ``domain_plan_tables`` reads)."""
    partitions = {k + 1: types.SimpleNamespace(domain=np.asarray(d, np.int32), image=np.asarray(im, np.int32),
                                               image_in_domain=np.asarray(iid, np.int32))
                  for k, (d, im, iid) in enumerate(parts)}
    return type("FakeDomain", (), {"partitions": partitions, "__len__": lambda self: n})()


def test_overlapping_images_raise():
    ok = _fake_dom(6, [([0, 1, 2, 3], [0, 1, 2], [0, 1, 2]), ([2, 3, 4, 5], [3, 4, 5], [1, 2, 3])])
    domain_plan_tables(ok)
    bad = _fake_dom(6, [([0, 1, 2, 3], [0, 1, 2], [0, 1, 2]), ([2, 3, 4, 5], [2, 3, 4], [0, 1, 2])])
    with pytest.raises(ValueError, match="overlap"):
        domain_plan_tables(bad)


def test_out_of_range_indices_raise():
    with pytest.raises(ValueError, match="domain index"):
        domain_plan_tables(_fake_dom(4, [([0, 1, 4], [0], [0])]))
    with pytest.raises(ValueError, match="image index"):
        domain_plan_tables(_fake_dom(4, [([0, 1, 2], [5], [0])]))
    with pytest.raises(ValueError, match="image_in_domain"):
        domain_plan_tables(_fake_dom(4, [([0, 1, 2], [0], [3])]))

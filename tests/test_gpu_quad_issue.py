"""The quad sweep after the cut of its non-arithmetic vector instructions computes the SAME BITS as before it.

The wave code of ``csrc/ibh_quad2d.h`` (lane table, halo unpack, ring reads, tile reads of the upper neighbours) was
reorganised without touching a floating-point operation or its order.  The form it replaced is not kept in the tree, so
the expected values are recorded results: ``tests/golden/quad_issue_parent.npz`` holds what the library built from the
commit before the change stored for every case below (``python tests/test_gpu_quad_issue.py --record`` with ``IBHIP_LIB``
pointing at that build wrote it).  The comparison is on the bit patterns -- stricter than ``==``: it tells -0 from +0.

Meshes (built in milliseconds, every side class and every wave form of the sweep):
- ``uniform``: 64 x 64 cells, 8 x 8 blocks.  A quad has no mirror side (ibh_build_quads2), so the 32 x 32-cell mesh has
  none; here the four sibling groups in the middle are one complete super-tile of four quads with SAME sides all round,
  and the blocks along the box, with their mirror sides, take the per-block body of the same launch;
- ``corner``: the same with the lower-left block of the first inner quad refined once: its four children are a quad with
  COARSE sides, its former siblings have FINE half-sides and are swept as a pair tile and a single block.
Inputs: the benchmark's ``synthetic_fields``; and a checkerboard of signs (the sign changes across every face between cells
of one size) with exact +0 and -0 cells, under a velocity that takes both signs in both directions.
Forms: the residual sweep (library defaults, table-only halo ids, no pair tiles), the STEP form (``step_advection``) and the
image-only sweep on the partitions of the mesh cut in pieces.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "quad_issue_parent.npz")
f32 = np.float32
FAMILIES = [("outlet", [(1, True), (2, True)])]
TUNINGS = {"default": {}, "table_ids": {"arith_ids": 0}, "no_pairs": {"pairs": 0}}
TUNING_DEFAULTS = {"pairs": 1, "arith_ids": 1}
DT = f32(2.5e-3)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)   # bench.synthetic_fields

pytestmark = pytest.mark.gpu


def quadtree_mesh(refine, depth=3):
    """Blocks of a quadtree over the unit square in the mesher's order (depth first, children x-fastest)."""
    from ibamd.mesher import Mesh
    out = []

    def rec(ox, oy, w, lvl):
        if lvl < depth or refine(ox, oy, lvl):
            hw = f32(w / 2)
            for j in (0, 1):
                for i in (0, 1):
                    rec(f32(ox + i * hw), f32(oy + j * hw), hw, lvl + 1)
        else:
            out.append((ox, oy, w))

    rec(f32(0), f32(0), f32(1), 0)
    bo = np.array([[b[0] for b in out], [b[1] for b in out]], dtype=f32)
    bw = np.array([[b[2] for b in out], [b[2] for b in out]], dtype=f32)
    return Mesh([0.0, 0.0], [1.0, 1.0], block_origins=bo, block_widths=bw, distance_fields={})


def meshes():
    return {"uniform": quadtree_mesh(lambda x, y, lvl: False),
            "corner": quadtree_mesh(lambda x, y, lvl: lvl == 3 and x == f32(0.25) and y == f32(0.25))}


def fields(part):
    """name -> (u, C)"""
    import bench
    centers = part.centers
    u_b, C_b = bench.synthetic_fields(centers)
    x, y = centers[:, 0].astype(np.float64), centers[:, 1].astype(np.float64)
    w = np.asarray(part.spacing)[:, 0].astype(np.float64)
    n = x.shape[0]
    # a checkerboard of signs on each level's own grid: the sign flips across every face between cells of one size, and
    # across one of the two sub-faces of a coarse-fine face
    par = (np.floor(x / w) + np.floor(y / w)).astype(np.int64) & 1
    mag = (0.25 + np.abs(np.sin(7 * x + 0.37) * np.cos(5 * y))).astype(f32)
    u_s = np.where(par == 1, -mag, mag).astype(f32)
    idx = np.arange(n)
    u_s[idx % 7 == 0] = f32(0.0)
    u_s[idx % 11 == 0] = f32(-0.0)
    C_s = np.stack([np.sin(9 * x + 3 * y) + 0.1, np.cos(4 * x - 8 * y) - 0.2], axis=1).astype(f32)
    C_s[idx % 13 == 0, 0] = f32(-0.0)
    assert (C_s[:, 0] > 0).any() and (C_s[:, 0] < 0).any() and (C_s[:, 1] > 0).any() and (C_s[:, 1] < 0).any()
    return {"bench": (u_b, C_b), "signs": (u_s, C_s)}


def _tuned(tuning, fn):
    from ibamd import _lib
    try:
        for k, v in tuning.items():
            _lib.call("ibh_set_tuning", k.encode(), int(v))
        return fn()
    finally:
        for k in tuning:
            _lib.call("ibh_set_tuning", k.encode(), TUNING_DEFAULTS[k])


def compute():
    """Every case with the library that is loaded: name -> float32 array, and the info of the one-partition domains."""
    import torch
    import ibamd
    out, infos = {}, {}
    for mname, msh in meshes().items():
        dom = ibamd.Domain(msh, hypercube_families=FAMILIES, max_partition_size=10 ** 9, boundaries=False)
        (part,) = dom.partitions.values()
        dpart = ibamd.to_backend(part, ibamd.hip)
        infos[mname] = dict(dpart.info)
        for fname, (u, C) in fields(part).items():
            du, dC = ibamd.hip(u), ibamd.hip(C)
            for tname, t in TUNINGS.items():
                res = torch.full((u.shape[0],), float("nan"), dtype=torch.float32, device="cuda")
                _tuned(t, lambda: ibamd.residual_advection(dpart, du, dC, out=res))
                out[f"{mname}/{fname}/residual/{tname}"] = ibamd.to_host(res)
            for tname in ("default", "no_pairs"):
                stp = torch.full((u.shape[0],), float("nan"), dtype=torch.float32, device="cuda")
                _tuned(TUNINGS[tname], lambda: ibamd.step_advection(dpart, du, dC, ibamd.hip(np.full(1, DT, f32)), out=stp))
                out[f"{mname}/{fname}/step/{tname}"] = ibamd.to_host(stp)
        # image-only sweeps: the mesh in partitions of at most 2048 cells (their skirts are not written: they stay NaN)
        pdom = ibamd.Domain(msh, hypercube_families=FAMILIES, max_partition_size=2048, boundaries=False)
        for k, p in pdom.partitions.items():
            dp = ibamd.to_backend(p, ibamd.hip)
            infos[f"{mname}/part{k}"] = dict(dp.info)
            for fname, (u, C) in fields(p).items():
                img = torch.full((u.shape[0],), float("nan"), dtype=torch.float32, device="cuda")
                ibamd.residual_advection(dp, ibamd.hip(u), ibamd.hip(C), out=img, flags=ibamd.IBH_IMAGE_ONLY)
                out[f"{mname}/{fname}/image/part{k}"] = ibamd.to_host(img)
    return out, infos


@pytest.fixture(scope="module")
def computed():
    return compute()


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_meshes_hold_every_side_class_and_wave_form(computed):
    _, infos = computed
    u, c = infos["uniform"], infos["corner"]
    assert u["quads"] == 4 and u["quad_singles"] == 48 and u["sides_mirror"] > 0, u
    assert u["sides_coarse"] == 0 and u["sides_fine"] == 0 and u["sides_same"] > 0, u
    for key in ("quads", "quad_pairs", "quad_singles", "sides_coarse", "sides_fine", "sides_same", "sides_mirror"):
        assert c[key] > 0, (key, c)
    assert sum(i["image_quads"] for n, i in infos.items() if "/part" in n) > 0, infos


def _bits_equal(got, exp):
    import torch
    return torch.equal(torch.from_numpy(np.ascontiguousarray(got)).view(torch.int32),
                       torch.from_numpy(np.ascontiguousarray(exp)).view(torch.int32))


@pytest.mark.parametrize("form", ["residual", "step", "image"])
def test_same_bits_as_before_the_change(computed, golden, form):
    got, _ = computed
    names = [k for k in got if k.split("/")[2] == form]
    assert names and sorted(k for k in golden if k.split("/")[2] == form) == sorted(names)
    bad = []
    for k in names:
        g, e = got[k], golden[k]
        written = ~np.isnan(e)
        assert written.any() and np.isfinite(e[written]).all(), k      # the recorded case computes something finite
        if form != "image":
            assert written.all(), k
        if not _bits_equal(g, e):
            d = np.flatnonzero(g.view(np.int32) != e.view(np.int32))
            bad.append(f"{k}: {d.size} cells differ, first {d[0]}: {g[d[0]]!r} != {e[d[0]]!r}")
    assert not bad, "\n".join(bad)


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: IBHIP_LIB=<library of the commit before the change> python tests/test_gpu_quad_issue.py --record")
    res, inf = compute()
    np.savez_compressed(GOLDEN, **res)
    for name, i in inf.items():
        print(name, {k: i[k] for k in ("quads", "quad_pairs", "quad_singles", "sides_same", "sides_coarse", "sides_fine",
                                       "sides_mirror", "image_quads") if k in i})
    print("recorded", len(res), "arrays,", os.path.getsize(GOLDEN), "bytes")

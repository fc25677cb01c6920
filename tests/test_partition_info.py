"""The summary of a partition (``ibh_partition_info``, ``IBH_H2D_INFO``): the slot table is stated once, every 2-D slot equals
a value derived in numpy from the tables of the same host-only analysis and from the partition's own face arrays, and on the
device the created handle reports what the host-only record does."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ibamd
from conftest import ADV_FAMILIES, advection_mesh
from ibamd import _lib
from ibamd.hostview import analyze2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOT = {name: i for i, name in enumerate(_lib.INFO_SLOTS)}


def _enum():
    """{name: value} of the IBH_INFO_* enumerators of include/ibhip.h, in the order they are written."""
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "ibhip.h")).read(), flags=re.S)
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"\bIBH_INFO_([A-Z0-9_]+)\s*=\s*(\d+)", hdr)}


def test_slot_table_is_stated_once():
    enum = _enum()
    assert enum.pop("COUNT") == _lib.INFO_COUNT == 24
    assert enum.pop("RIM4_ROWS") == enum["QUADS"] == 12          # one slot, 2-D / 3-D
    assert tuple(n.lower() for n in enum) == _lib.INFO_SLOTS      # same names, same order, same count ...
    assert list(enum.values()) == list(range(len(_lib.INFO_SLOTS)))   # ... and the position is the number
    allowed = {_lib.INFO_KEYS.get(n, n) for n in _lib.INFO_SLOTS} | {"rim4_rows"}
    values = list(range(100, 100 + _lib.INFO_COUNT))
    for nd in (2, 3):
        d = _lib.info_dict(nd, values)
        assert set(d) == allowed
        for name in _lib.INFO_SLOTS:
            got = d[_lib.INFO_KEYS.get(name, name)]
            # (the flag and 2-D-only slots are restated here, not taken from _lib: the test stays independent of them)
            if name in ("image_all_eligible", "row_sweep", "tiled"):
                assert got is True
            elif nd == 3 and name in ("quads", "quad_pairs", "quad_arith_half_sides"):
                assert got == 0
            else:
                assert type(got) is int and got == values[SLOT[name]]
        assert d["rim4_rows"] == (values[SLOT["quads"]] if nd == 3 else 0)


@pytest.fixture(scope="module")
def coarse_parts():
    """The coarse advection mesh in partitions of at most 4096 cells."""
    return list(ibamd.Domain(advection_mesh(2e-2), hypercube_families=ADV_FAMILIES, max_partition_size=4096).partitions.values())


@pytest.fixture(scope="module")
def parts2(adv_domains, rae_domains, coarse_parts):
    return list(adv_domains[0].partitions.values()) + list(rae_domains[0].partitions.values()) + coarse_parts


@pytest.fixture(scope="module")
def records2(parts2):
    return [analyze2(p) for p in parts2]


def direct_sides(part):
    """Cells with exactly one face on a side whose owner (right) / neighbour (left) is the cell itself, over (d, side)."""
    n = 0
    for d in range(1, part.ndims + 1):
        own, nei = part.face_owners_neighbors[d]
        for right in (False, True):
            acc = part.face_accumulators[(d, right)]
            off, idx = np.asarray(acc.off, np.int64), np.asarray(acc.idx, np.int64)
            off = off - off[0]
            cells = np.nonzero(np.diff(off) == 1)[0]
            f = idx[off[cells]]
            n += int(np.count_nonzero(np.asarray(own if right else nei)[f] == cells))
    return n


def expected2(part, a):
    """{slot: value} of the 2-D slots, from the tables of the record ``a`` and the partition's face arrays."""
    blocks, nc = a["blocks"], part.spacing.shape[0]
    qa, qi = a["quads_all"], a["quads_image"]
    e = {0: len(blocks), 7: a["nB1"], 8: int(a["fusable"].sum()), 12: len(qa["desc"]), 13: len(qa["singles"]),
         14: len(qi["desc"]), 15: len(qi["singles"]), 17: direct_sides(part), 18: len(qa["pair_desc"]),
         19: int((qa["aux"][:, 32:40] >= 0).sum()),
         20: int(len(blocks) > 0 and 64 * len(blocks) == nc
                 and np.array_equal(blocks["base"], 64 * np.arange(len(blocks))))}
    for k, n in enumerate(np.bincount(blocks["type"].ravel(), minlength=5)):
        e[2 + k] = int(n)
    return e


def test_every_2d_slot_against_an_independent_derivation(parts2, records2):
    seen = dict(fuse_all=set(), tiled=set(), image_quads=set(), irregular=set())
    for part, a in zip(parts2, records2):
        info = a["info"]
        assert info.shape == (_lib.INFO_COUNT,) and not info[len(_lib.INFO_SLOTS):].any()
        for slot, want in expected2(part, a).items():
            assert info[slot] == want, (_lib.INFO_SLOTS[slot], int(info[slot]), want)
        assert info[SLOT["row_sweep"]] in (0, 1) and (not info[SLOT["row_sweep"]] or a["fuse_all"])
        seen["fuse_all"].add(a["fuse_all"])
        seen["tiled"].add(bool(info[SLOT["tiled"]]))
        seen["image_quads"].add(len(a["quads_image"]["desc"]) > 0)
        seen["irregular"].add(info[SLOT["irregular_cells"]] > 0)
    assert seen["fuse_all"] == seen["tiled"] == seen["image_quads"] == {False, True}
    assert True in seen["irregular"]


def _device_info(part):
    dpart = ibamd.backend.DevicePartition(part)
    info = (C.c_int64 * _lib.INFO_COUNT)()
    _lib.call("ibh_partition_info", dpart.handle, info, _lib.INFO_COUNT)
    return np.array(info, dtype=np.int64), dpart


@pytest.mark.gpu
def test_created_handle_reports_the_host_record(parts2, records2):
    for part, a in zip(parts2, records2):
        got, _ = _device_info(part)
        assert np.array_equal(got, a["info"])


@pytest.fixture(scope="module")
def parts3():
    """The small 8^3 octrees of test_3d.py, each as one partition -- one block, 2 x 2 x 2 uniform blocks, a corner refined
    (64 blocks, COARSE and FINE sides) -- and the last one split in two (skirt fragments): (kind, partition)."""
    import les_model
    from ibamd.mesher import Ball, Mesh
    f32 = np.float32

    def mesh(regions):
        return Mesh(f32([-2, -2, -2]), f32([4, 4, 4]), block_size=8, refinement_regions=regions)
    corner = mesh([(Ball(np.array([-2.0, -2.0, -2.0]), 0.1), f32(0.1))])
    out = [("one_block", les_model.one_partition(les_model.single_block_mesh())),
           ("eight_blocks", les_model.one_partition(mesh([(Ball(np.array([0.0, 0.0, 0.0]), 5.0), f32(0.3))]))),
           ("corner_refined", les_model.one_partition(corner))]
    split = ibamd.Domain(corner, max_partition_size=16384, boundaries=False).partitions
    assert len(split) == 2
    return out + [("corner_split", p) for p in split.values()]


@pytest.mark.gpu
def test_3d_summary(parts3):
    for kind, part in parts3:
        got, dpart = _device_info(part)
        info, nc = dpart.info, part.spacing.shape[0]
        nb = info["full_blocks"]
        assert nb == got[SLOT["full_blocks"]] and got[SLOT["sides_same"]:SLOT["sides_general"] + 1].sum() == 6 * nb, kind
        assert info["quads"] == info["quad_pairs"] == info["quad_arith_half_sides"] == 0
        assert info["rim4_rows"] == got[SLOT["quads"]] and info["tiled"] == bool(got[SLOT["tiled"]])
        assert info["fusable_blocks"] in (0, nb) and info["fusable_blocks"] + info["workspace_blocks"] == nb   # all or none
        complete = nb > 0 and info["irregular_cells"] == 0 and 512 * nb == nc
        if kind == "corner_split":
            # skirt fragments: face-list cells, so not tiled and no single-kernel sweep over all blocks
            assert nb > 1 and info["irregular_cells"] > 0 and not complete and not info["tiled"]
            assert info["fusable_blocks"] == 0 and info["image_blocks"] <= nb
            continue
        # one partition made of complete blocks: no skirt and no GENERAL side, so no block moves behind another in the phase
        # order and block b starts at cell 512 b -- tiled exactly; a MIRROR side is 64 faces whose owner is their neighbour
        mirror = sum(int(np.count_nonzero(np.asarray(o) == np.asarray(n))) for o, n in part.face_owners_neighbors.values())
        assert complete and nb == {"one_block": 1, "eight_blocks": 8, "corner_refined": 64}[kind]
        assert info["sides_general"] == 0 and info["tiled"] is True and info["sides_mirror"] * 64 == mirror
        assert info["fusable_blocks"] == info["interior_blocks"] == info["image_blocks"] == nb
        assert info["image_blocks_all_eligible"] is True
        if kind == "one_block":
            assert info["sides_mirror"] == 6 and info["rim4_rows"] == 0
        if kind == "eight_blocks":
            assert info["sides_mirror"] == info["sides_same"] == 24 and info["rim4_rows"] == 0
        if kind == "corner_refined":
            assert info["sides_fine"] > 0 and info["sides_coarse"] == 4 * info["sides_fine"] and info["rim4_rows"] > 0

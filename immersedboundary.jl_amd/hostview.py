"""Host-only view of the block analysis libibhip runs in ``ibh_partition_create`` (2-D, 8x8 blocks).

``analyze2(part)`` returns the block table, the halo / end tables and the 2x2 block groups ("quads") of the
quad sweep as numpy arrays -- the same code path as the device upload, without a device.  Used by the CPU
tests of the library's host logic.
"""
import ctypes as C

import numpy as np

from ._header import constants
from ._lib import c_vp, call

BLOCK_DTYPE = np.dtype([("base", "<i4"), ("type", "<i4", (4,)), ("nb", "<i4", (4, 2)), ("sub", "<i4", (4,)),
                        ("h", "<f4", (2,)), ("rh", "<f4", (2,)), ("q", "<f4", (4,)), ("rt", "<f4", (4,)),
                        ("dt", "<i4")])
QUAD_DTYPE = np.dtype([("base", "<i4"), ("cls", "<u4"), ("rh", "<f4", (2,))])
(BLOCKS, HTAB, ETAB, FUSABLE, QUAD_DESC, QUAD_TAB, SINGLES, COUNTS, INFO, PAIR_DESC, PAIR_TAB, SINGLES2, QUAD_AUX,
 PAIR_AUX) = constants("IBH_H2D_", "BLOCKS HTAB ETAB FUSABLE QUAD_DESC QUAD_TAB SINGLES COUNTS INFO PAIR_DESC PAIR_TAB SINGLES2 "
                       "QUAD_AUX PAIR_AUX")
SIDE_SAME, SIDE_MIRROR, SIDE_COARSE, SIDE_FINE, SIDE_GENERAL = range(5)


def partition_args(part, index_base=0, image_in_domain=None):
    """The arguments ``ibh_partition_create`` and ``ibh_analyze2_host`` share, in their order -- ``nf``, the owners and
    neighbours and the four CSR arrays per dimension, ``n_image``, ``image_in_domain``, ``domain`` -- followed by
    ``index_base``, and the arrays behind the pointers, which must outlive the call: ``(args, keep)``, ``keep`` a dict that also
    holds ``spacing`` (column-major Float32).  Every index is written with ``index_base`` (the partition's are 0-based);
    ``image_in_domain``: other 0-based image ids than the partition's."""
    dims = range(1, part.ndims + 1)
    fon, fa = part.face_owners_neighbors, part.face_accumulators

    def i32(a):
        return np.ascontiguousarray(a if index_base == 0 else np.asarray(a) + index_base, dtype=np.int32)

    faces = [[i32(a) for a in arrs] for arrs in
             ([fon[d][0] for d in dims], [fon[d][1] for d in dims],
              [fa[(d, False)].off for d in dims], [fa[(d, False)].idx for d in dims],
              [fa[(d, True)].off for d in dims], [fa[(d, True)].idx for d in dims])]
    keep = dict(spacing=np.asfortranarray(part.spacing, dtype=np.float32),
                nf=np.array([fon[d][0].shape[0] for d in dims], dtype=np.int32),
                image_in_domain=i32(part.image_in_domain if image_in_domain is None else image_in_domain),
                domain=i32(part.domain), faces=faces)
    args = ((keep["nf"].ctypes.data_as(c_vp),) + tuple((c_vp * part.ndims)(*[a.ctypes.data for a in arrs]) for arrs in faces)
            + (int(keep["image_in_domain"].size), keep["image_in_domain"].ctypes.data_as(c_vp),
               keep["domain"].ctypes.data_as(c_vp), index_base))
    return args, keep


def analyze2(part):
    assert part.ndims == 2
    args, keep = partition_args(part)
    h = c_vp()
    call("ibh_analyze2_host", C.byref(h), part.spacing.shape[0], keep["spacing"].ctypes.data_as(c_vp), *args)

    def get(what, dtype, set_=0):
        n = C.c_int64(0)
        call("ibh_host2d_get", h, what, set_, c_vp(None), 0, C.byref(n))
        buf = np.empty(n.value, dtype=np.uint8)
        if n.value:
            call("ibh_host2d_get", h, what, set_, buf.ctypes.data_as(c_vp), n.value, C.byref(n))
        return buf.view(dtype)

    try:
        out = dict(blocks=get(BLOCKS, BLOCK_DTYPE), htab=get(HTAB, np.int32).reshape(-1, 64),
                   etab=get(ETAB, np.int32).reshape(-1, 16), fusable=get(FUSABLE, np.uint8).astype(bool),
                   info=get(INFO, np.int64))
        for k, name in ((0, "all"), (1, "image")):
            cnt = get(COUNTS, np.int64, k)
            out[f"quads_{name}"] = dict(desc=get(QUAD_DESC, QUAD_DTYPE, k), tab=get(QUAD_TAB, np.int32, k).reshape(-1, 160),
                                        singles=get(SINGLES, np.int32, k), n_interior=int(cnt[2]),
                                        n_singles_interior=int(cnt[4]),
                                        # pair tiles among the single blocks (set 0 of one-partition domains) and what is left
                                        pair_desc=get(PAIR_DESC, QUAD_DTYPE, k),
                                        pair_tab=get(PAIR_TAB, np.int32, k).reshape(-1, 160),
                                        singles2=get(SINGLES2, np.int32, k),
                                        # companion rows: 32 end ids + per half-side the origin of arithmetic halo ids / -1
                                        aux=get(QUAD_AUX, np.int32, k).reshape(-1, 40),
                                        pair_aux=get(PAIR_AUX, np.int32, k).reshape(-1, 40))
            out.update(fuse_all=bool(cnt[5]), img_all_fz=bool(cnt[6]), nB1=int(cnt[7]))
    finally:
        call("ibh_host2d_destroy", h)
    return out

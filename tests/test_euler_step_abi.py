"""``ibh_timestep_euler`` / ``ibh_update_euler`` / ``ibh_step_euler``: exported, bound by ``_lib`` with the header's argument
lists, and every misuse reported through ``ibh_last_error`` before anything is launched -- no GPU needed to be told so."""
import ctypes as C
import re

import pytest

from abi import assert_bound, header_text
from ibamd import _lib
from ibamd import backend as B

NAMES = ("ibh_timestep_euler", "ibh_update_euler", "ibh_step_euler")


def test_exported_and_bound_with_the_headers_prototypes():
    assert_bound(NAMES)
    hdr = header_text()
    for macro, value in (("IBH_EULER_HLL", B.IBH_EULER_HLL), ("IBH_EULER_SENSOR", B.IBH_EULER_SENSOR)):
        assert int(re.search(r"#define\s+" + macro + r"\s+(\d+)", hdr).group(1)) == value


class Args:
    """Well-formed argument lists over host buffers: nothing is dereferenced before the checks, and every case below
    returns from them.  ``part``: a zeroed stand-in for a partition with its two leading fields set -- ``nd`` and ``nc``
    (ibh_common.h) -- so it has no block structure: a handle whose step needs ``work``."""

    def __init__(self, nd=3, nc=40):
        self.buf = (C.c_float * 4096)()
        self.out = (C.c_float * 4096)()
        self.wrk = (C.c_float * 4096)()
        self.dtb = (C.c_float * 64)()
        self.handle = (C.c_char * 8192)()
        C.cast(self.handle, C.POINTER(C.c_int32))[0] = nd
        C.cast(self.handle, C.POINTER(C.c_int32))[1] = nc
        self.fluid = _lib.ibh_fluid(283.0, 1.4, 1.716e-5, 273.15, 110.4, 2, (C.c_float * 4)(0.00646, 6.468e-5, 0, 0))
        self.nd, self.nc = nd, nc
        a = C.addressof
        self.P, self.R, self.dt, self.Pout, self.work, self.p, self.f = (a(self.buf), a(self.wrk), a(self.dtb), a(self.out),
                                                                         a(self.wrk), a(self.handle), C.pointer(self.fluid))

    def timestep(self, **o):
        d = dict(p=self.p, f=self.f, P=self.P, ldp=self.nc, scale=C.c_float(0.75), dt=self.dt, cells=self.Pout)
        d.update(o)
        return [d[k] for k in ("p", "f", "P", "ldp", "scale", "dt", "cells")]

    def update(self, **o):
        d = dict(f=self.f, nd=self.nd, n=self.nc, P=self.P, ldp=self.nc, R=self.R, ldr=self.nc, dt=self.dt, per_cell=0,
                 Pout=self.Pout, ldo=self.nc)
        d.update(o)
        return [d[k] for k in ("f", "nd", "n", "P", "ldp", "R", "ldr", "dt", "per_cell", "Pout", "ldo")]

    def step(self, **o):
        d = dict(p=self.p, f=self.f, scheme=0, P=self.P, ldp=self.nc, Pout=self.Pout, ldo=self.nc, dt=self.dt, per_cell=0,
                 work=self.work, ldw=self.nc, flags=0)
        d.update(o)
        return [d[k] for k in ("p", "f", "scheme", "P", "ldp", "Pout", "ldo", "dt", "per_cell", "work", "ldw", "flags")]


SAME = object()   # "the address of another argument", resolved per case

TIMESTEP = [
    (dict(p=None), b"null"), (dict(f=None), b"null"), (dict(P=None), b"null"),
    (dict(dt=None, cells=None), b"null dt_device and dt_cells"),
    (dict(ldp=39), b"ldp is smaller"),
    ("nd4", b"nd must be 2 or 3"),
    ("nc0", b"empty partition"),
]
UPDATE = [
    (dict(f=None), b"null"), (dict(P=None), b"null"), (dict(R=None), b"null"), (dict(dt=None), b"null"),
    (dict(Pout=None), b"null"),
    (dict(nd=4), b"nd must be 2 or 3"), (dict(nd=1), b"nd must be 2 or 3"),
    (dict(ldp=39), b"leading dimension"), (dict(ldr=39), b"leading dimension"), (dict(ldo=39), b"leading dimension"),
    (dict(n=-1), b"leading dimension"),
    ("Pout=R", b"may not alias"), ("P=R", b"may not alias"),
]
STEP = [
    (dict(p=None), b"null"), (dict(f=None), b"null"), (dict(P=None), b"null"), (dict(Pout=None), b"null"),
    (dict(dt=None), b"null"),
    (dict(scheme=2), b"scheme must be"), (dict(scheme=-1), b"scheme must be"),
    (dict(flags=B.IBH_IMAGE_ONLY), b"IBH_IMAGE_ONLY is not taken"),
    (dict(flags=B.IBH_PHASE_INTERIOR), b"overlap phases"), (dict(flags=B.IBH_PHASE_BOUNDARY), b"overlap phases"),
    (dict(flags=B.IBH_PASS_A_ONLY), b"single pass"),
    ("nd4", b"nd must be 2 or 3"),
    (dict(ldp=39), b"leading dimension"), (dict(ldo=39), b"leading dimension"),
    (dict(work=None), b"work must be"),                     # a handle without a block structure: the two-launch form
    (dict(work=None, per_cell=1), b"work must be"),
    (dict(ldw=39), b"ldw is smaller"),
    ("work=P", b"work may not alias"), ("work=Pout", b"work may not alias"),
]


def _ids(cases):
    return [(c if isinstance(c, str) else "_".join(f"{k}-{v}" for k, v in c.items())).replace(" ", "") + f"_{i}"
            for i, (c, _) in enumerate(cases)]


def _run(entry, over, what):
    lib = _lib.load()
    a = Args(nd=4) if over == "nd4" else Args(nc=0) if over == "nc0" else Args()
    if isinstance(over, str) and "=" in over:
        k, v = over.split("=")
        over = {k: getattr(a, v)}
    elif isinstance(over, str):
        over = {}
    rc = getattr(lib, entry)(*getattr(a, entry.split("_")[1])(**over))
    assert rc != 0 and what in lib.ibh_last_error(), (rc, lib.ibh_last_error())


@pytest.mark.parametrize("over,what", TIMESTEP, ids=_ids(TIMESTEP))
def test_timestep_euler_misuse(over, what):
    _run("ibh_timestep_euler", over, what)


@pytest.mark.parametrize("over,what", UPDATE, ids=_ids(UPDATE))
def test_update_euler_misuse(over, what):
    _run("ibh_update_euler", over, what)


@pytest.mark.parametrize("over,what", STEP, ids=_ids(STEP))
def test_step_euler_misuse(over, what):
    _run("ibh_step_euler", over, what)


def test_nothing_to_do_is_no_error():
    """n = 0 rows / an empty partition: valid arguments, nothing launched."""
    lib = _lib.load()
    assert lib.ibh_update_euler(*Args().update(n=0)) == 0
    assert lib.ibh_step_euler(*Args(nc=0).step()) == 0

"""``ibh_update_euler_ssp`` / ``ibh_stage_euler_ssp``: exported, bound by ``_lib`` with the header's argument lists, named by the
Julia binding, and every misuse reported through ``ibh_last_error`` before anything is launched -- no GPU needed to be told
so."""
import ctypes as C
import os
import re

import pytest

from abi import assert_bound
from ibamd import _lib
from ibamd import backend as B
from test_julia_binding import header_prototypes, julia_ccalls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ibh_update_euler_ssp", "ibh_stage_euler_ssp")


def test_exported_and_bound_with_the_headers_prototypes():
    assert_bound(NAMES)
    # the argument lists the issue names, in the header's order
    proto = dict(header_prototypes())
    assert proto["ibh_update_euler_ssp"][1].count("ptr") == 6 and len(proto["ibh_update_euler_ssp"][1]) == 16
    assert proto["ibh_stage_euler_ssp"][1].count("ptr") == 7 and len(proto["ibh_stage_euler_ssp"][1]) == 17


def test_python_mirrors_are_exported():
    import ibamd
    from ibamd import cfd, solver
    for name in ("update_euler_ssp", "stage_euler_ssp"):
        assert getattr(ibamd, name) is getattr(B, name) is getattr(cfd, name)
    assert ibamd.ssp_stages is solver.ssp_stages


def test_julia_binding_calls_both():
    """``julia/IBHip.jl`` ``ccall``s both names with the header's argument kinds (tests/test_julia_binding.py checks every
    ccall against the header; this one that the two are there, under the names beside ``stage_euler!``)."""
    protos = header_prototypes()
    calls = {c[0]: c for c in julia_ccalls()}
    for name in NAMES:
        assert name in calls, f"julia/IBHip.jl does not ccall {name}"
        assert calls[name][1] == protos[name][0] and calls[name][2] == protos[name][1], name
    src = open(os.path.join(ROOT, "julia", "IBHip.jl")).read()
    assert re.search(r"^function update_euler_ssp!\(", src, re.M) and re.search(r"^function stage_euler_ssp!\(", src, re.M)


class Args:
    """Well-formed argument lists over host buffers: nothing is dereferenced before the checks, and every case below
    returns from them.  ``part``: a zeroed stand-in for a partition with its two leading fields set -- ``nd`` and ``nc``
    (ibh_common.h) -- so it has no block structure: a handle whose stage needs ``work``."""

    def __init__(self, nd=3, nc=40):
        self.buf = (C.c_float * 4096)()
        self.base = (C.c_float * 4096)()
        self.out = (C.c_float * 4096)()
        self.wrk = (C.c_float * 4096)()
        self.dtb = (C.c_float * 64)()
        self.handle = (C.c_char * 8192)()
        C.cast(self.handle, C.POINTER(C.c_int32))[0] = nd
        C.cast(self.handle, C.POINTER(C.c_int32))[1] = nc
        self.fluid = _lib.ibh_fluid(283.0, 1.4, 1.716e-5, 273.15, 110.4, 2, (C.c_float * 4)(0.00646, 6.468e-5, 0, 0))
        self.nd, self.nc = nd, nc
        a = C.addressof
        self.P, self.P0, self.R, self.dt, self.Pout, self.work, self.p, self.f = (
            a(self.buf), a(self.base), a(self.wrk), a(self.dtb), a(self.out), a(self.wrk), a(self.handle), C.pointer(self.fluid))

    def update(self, **o):
        d = dict(f=self.f, nd=self.nd, n=self.nc, P0=self.P0, ld0=self.nc, P=self.P, ldp=self.nc, R=self.R, ldr=self.nc,
                 dt=self.dt, per_cell=0, a=C.c_float(0.75), b=C.c_float(0.25), c=C.c_float(0.25), Pout=self.Pout, ldo=self.nc)
        d.update(o)
        return [d[k] for k in ("f", "nd", "n", "P0", "ld0", "P", "ldp", "R", "ldr", "dt", "per_cell", "a", "b", "c", "Pout",
                               "ldo")]

    def stage(self, **o):
        d = dict(p=self.p, f=self.f, scheme=0, P=self.P, ldp=self.nc, P0=self.P0, ld0=self.nc, Pout=self.Pout, ldo=self.nc,
                 dt=self.dt, per_cell=0, a=C.c_float(0.75), b=C.c_float(0.25), c=C.c_float(0.25), work=self.work, ldw=self.nc,
                 flags=0)
        d.update(o)
        return [d[k] for k in ("p", "f", "scheme", "P", "ldp", "P0", "ld0", "Pout", "ldo", "dt", "per_cell", "a", "b", "c",
                               "work", "ldw", "flags")]


UPDATE = [
    (dict(f=None), b"null"), (dict(P0=None), b"null"), (dict(P=None), b"null"), (dict(R=None), b"null"),
    (dict(dt=None), b"null"), (dict(Pout=None), b"null"),
    (dict(nd=4), b"nd must be 2 or 3"), (dict(nd=1), b"nd must be 2 or 3"),
    (dict(ld0=39), b"leading dimension"), (dict(ldp=39), b"leading dimension"), (dict(ldr=39), b"leading dimension"),
    (dict(ldo=39), b"leading dimension"), (dict(n=-1), b"leading dimension"),
    ("Pout=R", b"may not alias"), ("P0=R", b"may not alias"), ("P=R", b"may not alias"),
]
STAGE = [
    (dict(p=None), b"null"), (dict(f=None), b"null"), (dict(P=None), b"null"), (dict(P0=None), b"null"),
    (dict(Pout=None), b"null"), (dict(dt=None), b"null"),
    (dict(scheme=2), b"scheme must be"), (dict(scheme=-1), b"scheme must be"),
    (dict(flags=B.IBH_IMAGE_ONLY), b"IBH_IMAGE_ONLY is not taken"),
    (dict(flags=B.IBH_PHASE_INTERIOR), b"overlap phases"), (dict(flags=B.IBH_PHASE_BOUNDARY), b"overlap phases"),
    (dict(flags=B.IBH_PASS_A_ONLY), b"single pass"), (dict(flags=B.IBH_PASS_B_ONLY), b"single pass"),
    ("nd4", b"nd must be 2 or 3"), ("nd1", b"nd must be 2 or 3"),
    (dict(ldp=39), b"leading dimension"), (dict(ld0=39), b"leading dimension"), (dict(ldo=39), b"leading dimension"),
    (dict(work=None), b"work must be"),                     # a handle without a block structure: the two-launch form
    (dict(work=None, per_cell=1), b"work must be"),
    (dict(ldw=39), b"ldw is smaller"),
    ("work=P", b"work may not alias"), ("work=P0", b"work may not alias"), ("work=Pout", b"work may not alias"),
    # through the two-launch form, the update's own aliasing rule: the residual is in `work`, so these are the three above;
    # P_out == P0 (with P0 != P), P_out == P and P0 == P are allowed and reach the launch, which a host test cannot make
]


def _ids(cases):
    return [(c if isinstance(c, str) else "_".join(f"{k}-{v}" for k, v in c.items())).replace(" ", "") + f"_{i}"
            for i, (c, _) in enumerate(cases)]


def _run(entry, method, over, what):
    lib = _lib.load()
    a = Args(nd=4) if over == "nd4" else Args(nd=1) if over == "nd1" else Args()
    if isinstance(over, str) and "=" in over:
        k, v = over.split("=")
        over = {k: getattr(a, v)}
    elif isinstance(over, str):
        over = {}
    rc = getattr(lib, entry)(*getattr(a, method)(**over))
    assert rc != 0 and what in lib.ibh_last_error(), (rc, lib.ibh_last_error())


@pytest.mark.parametrize("over,what", UPDATE, ids=_ids(UPDATE))
def test_update_euler_ssp_misuse(over, what):
    _run("ibh_update_euler_ssp", "update", over, what)


@pytest.mark.parametrize("over,what", STAGE, ids=_ids(STAGE))
def test_stage_euler_ssp_misuse(over, what):
    _run("ibh_stage_euler_ssp", "stage", over, what)


def test_nothing_to_do_is_no_error():
    """n = 0 rows / an empty partition: valid arguments, nothing launched."""
    lib = _lib.load()
    assert lib.ibh_update_euler_ssp(*Args().update(n=0)) == 0
    assert lib.ibh_stage_euler_ssp(*Args(nc=0).stage()) == 0
    assert lib.ibh_stage_euler_ssp(*Args(nc=0).stage(per_cell=1, work=None)) == 0

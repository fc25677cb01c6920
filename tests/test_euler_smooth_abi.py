"""``ibh_smooth_residual`` / ``ibh_update_euler_smoothed``: exported, bound by ``_lib`` with the header's argument lists, named
by the Julia binding, and every misuse reported through ``ibh_last_error`` before anything is launched -- no GPU needed to be
told so."""
import ctypes as C
import os
import re

import pytest

from abi import assert_bound
from ibamd import _lib
from ibamd import backend as B
from test_julia_binding import header_prototypes, julia_ccalls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ibh_smooth_residual", "ibh_update_euler_smoothed")


def test_exported_and_bound_with_the_headers_prototypes():
    assert_bound(NAMES)
    # the argument lists the issue names, in the header's order
    proto = dict(header_prototypes())
    assert proto["ibh_smooth_residual"][1].count("ptr") == 4 and len(proto["ibh_smooth_residual"][1]) == 10
    assert proto["ibh_update_euler_smoothed"][1].count("ptr") == 8 and len(proto["ibh_update_euler_smoothed"][1]) == 19


def test_python_mirrors_are_exported():
    import inspect

    import ibamd
    from ibamd import cfd, solver
    for name in ("smooth_residual", "update_euler_smoothed"):
        assert getattr(ibamd, name) is getattr(B, name) is getattr(cfd, name)
    assert "smoothing" in inspect.signature(solver.EulerMarch.__init__).parameters
    assert inspect.signature(solver.EulerMarch.__init__).parameters["smoothing"].default is None


def test_julia_binding_calls_both():
    protos = header_prototypes()
    calls = {c[0]: c for c in julia_ccalls()}
    for name in NAMES:
        assert name in calls, f"julia/IBHip.jl does not ccall {name}"
        assert calls[name][1] == protos[name][0] and calls[name][2] == protos[name][1], name
    src = open(os.path.join(ROOT, "julia", "IBHip.jl")).read()
    assert re.search(r"^function smooth_residual!\(", src, re.M) and re.search(r"^function update_euler_smoothed!\(", src, re.M)


class Args:
    """Well-formed argument lists over host buffers: nothing is dereferenced before the checks, and every case below
    returns from them.  ``part``: a zeroed stand-in for a partition with its two leading fields set -- ``nd`` and ``nc``
    (ibh_common.h) -- so it has no side table: a well-formed call on it is told so, after every other check."""

    def __init__(self, nd=3, nc=40):
        self.bufs = [(C.c_float * 4096)() for _ in range(7)]
        self.dtb = (C.c_float * 64)()
        self.handle = (C.c_char * 8192)()
        C.cast(self.handle, C.POINTER(C.c_int32))[0] = nd
        C.cast(self.handle, C.POINTER(C.c_int32))[1] = nc
        self.fluid = _lib.ibh_fluid(283.0, 1.4, 1.716e-5, 273.15, 110.4, 2, (C.c_float * 4)(0.00646, 6.468e-5, 0, 0))
        self.nd, self.nc = nd, nc
        a = C.addressof
        self.P0, self.P, self.R, self.Sprev, self.Pout, self.S, self.tmp = (a(b) for b in self.bufs)
        self.dt, self.p, self.f = a(self.dtb), a(self.handle), C.pointer(self.fluid)

    def smooth(self, **o):
        d = dict(p=self.p, R=self.R, nv=5, ldr=self.nc, eps=C.c_float(0.5), n_iter=3, S=self.S, lds=self.nc, tmp=self.tmp,
                 ldt=self.nc)
        d.update(o)
        return [d[k] for k in ("p", "R", "nv", "ldr", "eps", "n_iter", "S", "lds", "tmp", "ldt")]

    def update(self, **o):
        d = dict(p=self.p, f=self.f, blend=1, P0=self.P0, ld0=self.nc, P=self.P, ldp=self.nc, R=self.R, ldr=self.nc,
                 Sprev=self.Sprev, lds=self.nc, eps=C.c_float(0.5), dt=self.dt, per_cell=0, a=C.c_float(0.75),
                 b=C.c_float(0.25), c=C.c_float(0.25), Pout=self.Pout, ldo=self.nc)
        d.update(o)
        return [d[k] for k in ("p", "f", "blend", "P0", "ld0", "P", "ldp", "R", "ldr", "Sprev", "lds", "eps", "dt", "per_cell",
                               "a", "b", "c", "Pout", "ldo")]


NAN, INF = C.c_float(float("nan")), C.c_float(float("inf"))
SMOOTH = [
    (dict(p=None), b"null"), (dict(R=None), b"null"), (dict(S=None), b"null"),
    ("nd4", b"nd must be 2 or 3"), ("nd1", b"nd must be 2 or 3"),
    (dict(nv=0), b"nv must be"), (dict(nv=9), b"nv must be"), (dict(nv=-1), b"nv must be"),
    (dict(ldr=39), b"leading dimension"), (dict(lds=39), b"leading dimension"), (dict(ldt=39), b"leading dimension"),
    (dict(eps=C.c_float(-0.5)), b"eps must be"), (dict(eps=NAN), b"eps must be"), (dict(eps=INF), b"eps must be"),
    (dict(n_iter=0), b"n_iter must be"), (dict(n_iter=-2), b"n_iter must be"),
    (dict(tmp=None), b"tmp must be given"), (dict(tmp=None, n_iter=2), b"tmp must be given"),
    ("S=R", b"alias"), ("tmp=R", b"alias"), ("tmp=S", b"alias"), ("S=R,n_iter=1,tmp=None", b"alias"),
    ({}, b"no side table"), (dict(n_iter=1, tmp=None, ldt=0), b"no side table"),
]
UPDATE = [
    (dict(p=None), b"null"), (dict(f=None), b"null"), (dict(P0=None), b"null"), (dict(P=None), b"null"),
    (dict(R=None), b"null"), (dict(Sprev=None), b"null"), (dict(dt=None), b"null"), (dict(Pout=None), b"null"),
    (dict(blend=2), b"blend must be"), (dict(blend=-1), b"blend must be"),
    ("nd4", b"nd must be 2 or 3"), ("nd1", b"nd must be 2 or 3"),
    (dict(ld0=39), b"leading dimension"), (dict(ldp=39), b"leading dimension"), (dict(ldr=39), b"leading dimension"),
    (dict(lds=39), b"leading dimension"), (dict(ldo=39), b"leading dimension"),
    (dict(eps=C.c_float(-1.0)), b"eps must be"), (dict(eps=NAN), b"eps must be"), (dict(eps=INF), b"eps must be"),
    ("Pout=R", b"may not alias"), ("Pout=Sprev", b"may not alias"), ("Pout=R,Sprev=R", b"may not alias"),
    # everything the entry allows reaches the last check on this handle: the stage form without P, Sprev == R, P_out == P0 / P
    ({}, b"no side table"), (dict(blend=0, P=None, ldp=0), b"no side table"), ("Sprev=R", b"no side table"),
    ("Pout=P0", b"no side table"), ("Pout=P", b"no side table"), (dict(per_cell=1), b"no side table"),
]


def _ids(cases):
    return [(c if isinstance(c, str) else "_".join(f"{k}-{getattr(v, 'value', v)}" for k, v in c.items())).replace(" ", "")
            + f"_{i}" for i, (c, _) in enumerate(cases)]


def _run(entry, method, over, what):
    lib = _lib.load()
    a = Args(nd=4) if over == "nd4" else Args(nd=1) if over == "nd1" else Args()
    if isinstance(over, str) and "=" in over:
        d = {}
        for kv in over.split(","):
            k, v = kv.split("=")
            d[k] = None if v == "None" else int(v) if v.lstrip("-").isdigit() else getattr(a, v)
        over = d
    elif isinstance(over, str):
        over = {}
    rc = getattr(lib, entry)(*getattr(a, method)(**over))
    assert rc != 0 and what in lib.ibh_last_error(), (rc, lib.ibh_last_error())


@pytest.mark.parametrize("over,what", SMOOTH, ids=_ids(SMOOTH))
def test_smooth_residual_misuse(over, what):
    _run("ibh_smooth_residual", "smooth", over, what)


@pytest.mark.parametrize("over,what", UPDATE, ids=_ids(UPDATE))
def test_update_euler_smoothed_misuse(over, what):
    _run("ibh_update_euler_smoothed", "update", over, what)


def test_nothing_to_do_is_no_error():
    """An empty partition: valid arguments, nothing launched (and no side table asked for)."""
    lib = _lib.load()
    assert lib.ibh_smooth_residual(*Args(nc=0).smooth()) == 0
    assert lib.ibh_smooth_residual(*Args(nc=0).smooth(n_iter=1, tmp=None)) == 0
    assert lib.ibh_update_euler_smoothed(*Args(nc=0).update()) == 0
    assert lib.ibh_update_euler_smoothed(*Args(nc=0).update(blend=0, P=None, per_cell=1)) == 0

"""``ibh_les_of`` (the LES closure of a velocity field in one launch): exported, declared, bound by ``_lib`` with the header's
argument list and by the Julia shim, and every misuse reported through ``ibh_last_error`` before anything is launched -- no
GPU needed to be told so."""
import ctypes as C
import os
import re

import pytest

from abi import assert_bound
from ibamd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ("p", "vel", "ldv", "Delta", "model", "Cmodel", "nusgs", "ducros", "shock", "S", "G", "ldg")


def test_exported_declared_and_bound():
    assert_bound(("ibh_les_of",))
    sig = _lib._SIGS["ibh_les_of"]
    assert len(sig) == len(ARGS)
    assert sig[ARGS.index("ldv")] is C.c_int64 and sig[ARGS.index("ldg")] is C.c_int64
    assert sig[ARGS.index("model")] is C.c_int and sig[ARGS.index("Cmodel")] is C.c_float


def test_julia_shim_calls_it():
    jl = open(os.path.join(ROOT, "julia", "IBHip.jl")).read()
    assert re.search(r"function les_closure_of!\(", jl)
    assert re.search(r"ccall\(\(:ibh_les_of,\s*lib\)", jl)


def _args(**over):
    """A well-formed argument list over host buffers (nothing is dereferenced before the checks: every case below returns
    from them), with single arguments replaced.  The partition is a zeroed stand-in: nd = 0, nc = 0."""
    buf = (C.c_float * 64)()
    handle = (C.c_char * 8192)()
    b = C.addressof(buf)
    a = dict(p=C.addressof(handle), vel=b, ldv=16, Delta=b, model=1, Cmodel=0.17, nusgs=b, ducros=b, shock=b, S=b, G=b,
             ldg=16)
    a.update(over)
    return [a[k] for k in ARGS], (buf, handle)


NOTHING = dict(model=0, nusgs=None, ducros=None, shock=None, S=None, G=None)
CASES = [
    (dict(p=None), b"null partition or velocity"),
    (dict(vel=None), b"null partition or velocity"),
    (NOTHING, b"no output requested"),
    (dict(model=3), b"model must be 0"),
    (dict(model=-1), b"model must be 0"),
    (dict(Delta=None), b"needs Delta"),
    (dict(model=2, Delta=None), b"needs Delta"),
    (dict(nusgs=None), b"needs nusgs"),
    (dict(model=2, nusgs=None), b"needs nusgs"),
    (dict(model=0), b"nusgs requested without a model"),
    (dict(ldv=-1), b"ldv < nc"),
    (dict(ldg=-1), b"ldg < nc"),
    (dict(model=2), b"WALE model only implemented for 3D"),     # the stand-in is no 3-D partition
]


@pytest.mark.parametrize("over,what", CASES, ids=[w.decode().replace(" ", "_") + f"_{i}" for i, (_, w) in enumerate(CASES)])
def test_misuse_is_reported_before_any_launch(over, what):
    lib = _lib.load()
    args, keep = _args(**dict(over))
    rc = lib.ibh_les_of(*args)
    assert rc != 0 and what in lib.ibh_last_error(), lib.ibh_last_error()


def test_each_misuse_has_its_own_message():
    assert len({w for _, w in CASES}) == 9


@pytest.mark.parametrize("over", [dict(), dict(ldg=-1, G=None), dict(model=0, nusgs=None)],
                         ids=["all_outputs", "ldg_unused_without_G", "no_model"])
def test_an_empty_partition_is_no_error(over):
    lib = _lib.load()
    args, keep = _args(**over)
    assert lib.ibh_les_of(*args) == 0

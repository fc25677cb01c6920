"""``ibh_bc_flow`` / ``ibh_bc_flow_info`` (the FlowBC boundary condition in one launch): exported, bound by ``_lib`` with the
header's argument list, and every misuse reported through ``ibh_last_error`` before anything is launched -- no GPU needed
to be told so."""
import ctypes as C
import os
import re

import pytest

from abi import assert_bound
from ibamd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exported_and_bound():
    assert_bound(("ibh_bc_flow", "ibh_bc_flow_info"))


def test_spec_struct_matches_the_header():
    hdr = open(os.path.join(ROOT, "include", "ibhip.h")).read()
    body = re.search(r"typedef struct ibh_flow_bc_spec \{(.*?)\} ibh_flow_bc_spec;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        m = re.match(r"\s*(int32_t|float)\s+(\w+)(?:\[(\d+)\])?\s*$", decl)
        if m:
            fields.append((m.group(2), m.group(1), int(m.group(3) or 1)))
    got = [(n, "int32_t" if (t._type_ if hasattr(t, "_length_") else t) is C.c_int32 else "float",
            getattr(t, "_length_", 1)) for n, t in _lib.ibh_flow_bc_spec._fields_]
    assert fields == got
    assert C.sizeof(_lib.ibh_flow_bc_spec) == 4 * sum(f[2] for f in fields)


def _args(**over):
    """A well-formed argument list over host buffers (nothing is dereferenced before the checks: every case below
    returns from them), with single arguments replaced."""
    buf = (C.c_float * 64)()
    handle = (C.c_char * 4096)()       # stands in for a boundary; the checks under test come before its first use
    spec = _lib.ibh_flow_bc_spec(1, 1e5, 288.15, (C.c_float * 3)(0, 0, 0), 0.0, 1,
                                 (C.c_float * 8)(0.41, 4.9, 19.0, 0.075, 0.09, 4.2, 360.0, 0.5), 20)
    fluid = _lib.ibh_fluid(283.0, 1.4, 1.716e-5, 273.15, 110.4, 2, (C.c_float * 4)(0.00646, 6.468e-5, 0, 0))
    ns = over.pop("ns", 1)
    a = dict(b=C.addressof(handle), f=C.pointer(fluid), nd=3, normals=C.addressof(buf), ldn=16,
             imd=C.addressof(buf), P=C.addressof(buf), ldp=16, spec=C.pointer(spec), ns=ns,
             scalars=(C.c_void_p * max(ns, 1))(*([C.addressof(buf)] * max(ns, 1))),
             modes=(C.c_int32 * max(ns, 1))(*([2] * max(ns, 1))), values=(C.c_float * max(ns, 1))(), staging=None)
    for k, v in over.pop("spec_fields", {}).items():
        setattr(spec, k, v)
    a.update(over)
    keep = (buf, handle, spec, fluid)
    return [a[k] for k in ("b", "f", "nd", "normals", "ldn", "imd", "P", "ldp", "spec", "ns", "scalars", "modes", "values",
                           "staging")], keep


CASES = [
    (dict(b=None), b"null"),
    (dict(f=None), b"null"),
    (dict(normals=None), b"null"),
    (dict(imd=None), b"null"),
    (dict(P=None), b"null"),
    (dict(spec=None), b"null"),
    (dict(scalars=None), b"null"),
    (dict(modes=None), b"null"),
    (dict(values=None), b"null"),
    (dict(scalars=(C.c_void_p * 1)(None)), b"null scalar field"),
    (dict(nd=1), b"nd must be 2 or 3"),
    (dict(nd=4), b"nd must be 2 or 3"),
    (dict(ns=5), b"at most 4"),
    (dict(ns=-1), b"at most 4"),
    (dict(modes=(C.c_int32 * 1)(6)), b"unknown scalar mode"),
    (dict(modes=(C.c_int32 * 1)(-1)), b"unknown scalar mode"),
    (dict(spec_fields=dict(wall_function=0)), b"needs wall_function"),          # mode nut without the wall function
    (dict(spec_fields=dict(wall_function=2)), b"wall_function must be 0 or 1"),
    (dict(spec_fields=dict(n_iter=-3)), b"n_iter"),
    (dict(spec_fields=dict(u_inf=(C.c_float * 3)(0.0, 1.0, 0.0))), b"normal_flow"),   # normal_flow with a second velocity
]


@pytest.mark.parametrize("over,what", CASES, ids=[w.decode().replace(" ", "_") + f"_{i}" for i, (_, w) in enumerate(CASES)])
def test_misuse_is_reported_before_any_launch(over, what):
    lib = _lib.load()
    args, keep = _args(**dict(over))
    rc = lib.ibh_bc_flow(*args)
    assert rc != 0 and what in lib.ibh_last_error(), lib.ibh_last_error()


def test_info_rejects_null():
    lib = _lib.load()
    d = C.c_int32(7)
    assert lib.ibh_bc_flow_info(None, C.byref(d)) != 0 and b"null" in lib.ibh_last_error()
    handle = (C.c_char * 4096)()
    assert lib.ibh_bc_flow_info(C.addressof(handle), None) != 0 and b"null" in lib.ibh_last_error()

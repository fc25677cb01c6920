"""The C-ABI library loads without a GPU and exports every symbol include/ibhip.h declares."""
import ctypes
import os
import re

import pytest

import ibamd
from abi import assert_bound
from ibamd import _lib
from test_julia_binding import header_prototypes

C = ctypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    text = open(os.path.join(ROOT, "include", "ibhip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(ibh_[a-z0-9_]+)\s*\(", text)))


def test_library_loads_and_exports_header_symbols():
    lib = _lib.load()
    names = _declared()
    assert len(names) >= 35
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/ibhip.h but not exported"
    assert lib.ibh_version() >= 100


def test_binding_covers_header():
    assert set(_declared()) == set(_lib.EXPORTS)


KIND = {C.c_int: "i32", C.c_int32: "i32", C.c_uint32: "u32", C.c_int64: "i64", C.c_uint64: "u64", C.c_size_t: "u64",
        C.c_float: "f32", C.c_double: "f64"}


def test_every_binding_has_the_headers_argument_kinds():
    """``_lib._SIGS`` against tests/test_julia_binding.py's parser of the header, a second reader that shares no code with
    the package's: every prototype, the same number of arguments, the same kind in every position, the same kind returned."""
    protos = header_prototypes()
    assert set(protos) == set(_lib._SIGS) == set(_lib._RESTYPES) and len(protos) >= 143
    for name, (ret, kinds) in protos.items():
        assert [KIND.get(t, "ptr") for t in _lib._SIGS[name]] == kinds, name
        assert KIND.get(_lib._RESTYPES[name], "ptr") == ret, name
    assert_bound(sorted(protos))


def test_signatures_pinned_literally():
    """Entries that between them use every row of the table of C types, written out: a mistake that the two parsers share
    cannot pass here."""
    vp, i, i32, i64, f = C.c_void_p, C.c_int, C.c_int32, C.c_int64, C.c_float
    fluid, spec = C.POINTER(_lib.ibh_fluid), C.POINTER(_lib.ibh_flow_bc_spec)
    pinned = {
        "ibh_malloc": [vp, C.c_size_t],
        "ibh_set_tuning": [C.c_char_p, i],
        "ibh_time_average_push": [i64, i, vp, i64, vp, vp, i, vp, i64, i64, C.c_double, C.c_double, i],
        "ibh_flag_wait": [vp, vp, i, C.c_uint32, vp],
        "ibh_pi_rademacher": [i64, C.c_uint64, vp],
        "ibh_partition_create": [vp, i, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, i, i],
        "ibh_bc_flow": [vp, fluid, i, vp, i64, vp, vp, i64, spec, i, vp, vp, vp, vp],
        "ibh_update_euler_smoothed": [vp, fluid, i, vp, i64, vp, i64, vp, i64, vp, i64, f, vp, i, f, f, f, vp, i64],
        "ibh_last_error": [],
    }
    for name, sig in pinned.items():
        assert _lib._SIGS[name] == sig, name
        assert _lib._RESTYPES[name] is (C.c_char_p if name == "ibh_last_error" else C.c_int), name
    lib = _lib.load()
    assert lib.ibh_last_error.restype is C.c_char_p and lib.ibh_malloc.restype is C.c_int
    assert list(lib.ibh_update_euler_smoothed.argtypes) == pinned["ibh_update_euler_smoothed"]
    assert {t for sig in pinned.values() for t in sig} == set(_lib._CTYPES.values()) | {vp}   # every row of the table


def test_structs_have_the_headers_fields():
    f, i32 = C.c_float, C.c_int32
    assert _lib.ibh_fluid._fields_ == [("R", f), ("gamma", f), ("mu_ref", f), ("Tref", f), ("S", f), ("nk", i32), ("k", f * 4)]
    assert _lib.ibh_flow_bc_spec._fields_ == [("normal_flow", i32), ("p_inf", f), ("T_inf", f), ("u_inf", f * 3),
                                              ("transpiration", f), ("wall_function", i32), ("wall_params", f * 8),
                                              ("n_iter", i32)]
    assert C.sizeof(_lib.ibh_fluid) == 40 and C.sizeof(_lib.ibh_flow_bc_spec) == 68


@pytest.mark.parametrize("text,what", [
    (None, "ibhip.h"),                                                        # no header: the path is in the message
    ("#define IBH_X (1 << 3)\n", "IBH_X"), ("enum { IBH_A = 0, IBH_B };\n", "IBH_B"),
    ("int ibh_f(float* const p);\n", "ibh_f"), ("int ibh_f(unsigned long long n);\n", "ibh_f"),
    ("int ibh_f(int (*cb)(int));\n", "ibh_f"), ("typedef struct ibh_s { float* p; } ibh_s;\n", "ibh_s"),
], ids=["missing", "expression", "implicit-enumerator", "const-after-star", "three-word-scalar", "callback", "pointer-field"])
def test_reader_refuses_what_it_cannot_read(tmp_path, monkeypatch, text, what):
    from ibamd import _header
    path = tmp_path / "ibhip.h"
    if text is not None:
        path.write_text("/* a comment with IBH_Y = 1 << 2 */\n" + text)
    monkeypatch.setattr(_header, "HEADER_PATH", str(path))
    with pytest.raises(_lib.IbhError, match=what):
        _header.read()


def test_reader_and_type_table_accept_the_headers_forms(tmp_path, monkeypatch):
    from ibamd import _header
    path = tmp_path / "ibhip.h"
    path.write_text("#define IBH_H 0x1F /* hex */\nenum { IBH_A = 3, IBH_B = 4 };\ntypedef struct ibh_s { int32_t n; float v[2]; } ibh_s;\n"
                    "const char* ibh_name(void);\nint ibh_f(const ibh_s*, uint64_t seed, const float* const* g);\n")
    monkeypatch.setattr(_header, "HEADER_PATH", str(path))
    protos, consts, structs = _header.read()
    assert consts == {"IBH_H": 31, "IBH_A": 3, "IBH_B": 4} and list(consts) == ["IBH_H", "IBH_A", "IBH_B"]
    assert structs == {"ibh_s": [("int32_t", "n", None), ("float", "v", 2)]}
    assert protos == {"ibh_name": ("const char*", []),
                      "ibh_f": ("int", [("const ibh_s*", ""), ("uint64_t", "seed"), ("const float* const*", "g")])}
    with pytest.raises(_lib.IbhError, match="ibh_f.*unsigned"):
        _lib._ctype("unsigned", "ibh_f")
    assert _lib._ctype("unsigned long long*", "ibh_f") is C.c_void_p


def test_null_arguments_are_reported_not_crashed():
    lib = _lib.load()
    h = ctypes.c_void_p()
    rc = lib.ibh_partition_create(ctypes.byref(h), 2, 0, None, None, None, None, None, None, None, None, None, 0, None,
                                  None, 0, 0)
    assert rc != 0 and b"null" in lib.ibh_last_error()
    assert lib.ibh_partition_destroy(None) == 0


def test_compute_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import numpy as np
    with pytest.raises(_lib.IbhError):
        ibamd.hip(np.zeros(4, dtype=np.float32))


def test_ew_eval_validates_its_program_on_the_host():
    """ibh_ew_eval checks the postfix program before anything is launched (no GPU needed to be told it is malformed)."""
    lib = _lib.load()
    PUSH_A, PUSH_S, ADD, ABS = 32, 33, 0, 16
    buf = (ctypes.c_float * 4)()
    arrs = (ctypes.c_void_p * 1)(ctypes.addressof(buf))
    nvs = (ctypes.c_int32 * 1)(1)
    sc = (ctypes.c_float * 1)(2.0)

    def run(prog, narr=1, nscal=1):
        P = (ctypes.c_int32 * len(prog))(*prog)
        return lib.ibh_ew_eval(0, 1, len(prog), P, narr, arrs, nvs, nscal, sc, ctypes.addressof(buf))

    assert run([PUSH_A, PUSH_S, ADD]) == 0                     # n = 0 rows: valid program, nothing to launch
    assert run([PUSH_A, ABS, PUSH_S | (0 << 8), ADD]) == 0
    for bad, what in (([ADD], b"two operands"), ([PUSH_A, PUSH_A], b"exactly one value"), ([PUSH_A | (3 << 8)], b"array"),
                      ([PUSH_S | (1 << 8)], b"scalar"), ([PUSH_A, 99], b"unknown"), ([PUSH_A] * 9 + [ADD] * 8, b"deeper"),
                      ([PUSH_A, ABS] * 25, b"48 instructions")):
        assert run(bad) != 0 and what in lib.ibh_last_error(), (bad, lib.ibh_last_error())

"""The extended broadcast opcodes without a GPU: ibh_ew_eval validates them on the host, the three bindings agree on their
values, the numpy model states Julia's semantics on hand cases, and the host rewrite of Float64 comparisons is exact."""
import ctypes
import os
import re

import numpy as np
import pytest

from ibamd import _lib
from ibamd import hiparray as H
from ew_model import ARITY, compare_exact, model, same_bits, ulp_distance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NEW_UNARY = list(range(H.EXP, H.INVSQR + 1))
NEW_BINARY = list(range(H.LT, H.BMUL + 1))
NEW_TERNARY = [H.CLAMP, H.IFELSE]


def _eval(prog, narr=1, nscal=4, nv=1):
    lib = _lib.load()
    buf = (ctypes.c_float * 8)()
    arrs = (ctypes.c_void_p * 1)(ctypes.addressof(buf))
    nvs = (ctypes.c_int32 * 1)(nv)
    sc = (ctypes.c_float * 32)(*range(32))
    P = (ctypes.c_int32 * len(prog))(*prog)
    return lib.ibh_ew_eval(0, nv, len(prog), P, narr, arrs, nvs, nscal, sc, ctypes.addressof(buf))


def _err():
    return _lib.load().ibh_last_error()


def test_every_new_opcode_is_accepted_with_n_zero():
    A, S = H.PUSH_ARRAY, H.PUSH_SCALAR
    for op in NEW_UNARY:
        assert _eval([A, op]) == 0, (op, _err())
    for op in NEW_BINARY:
        assert _eval([A, S | (1 << 8), op]) == 0, (op, _err())
    for op in NEW_TERNARY:
        assert _eval([A, S, S | (2 << 8), op]) == 0, (op, _err())
    assert _eval([A, H.PUSH_ROW | (1 << 8), H.ADD], nv=3) == 0, _err()     # row of 3 scalars: 1, 2, 3
    assert _eval([A] + [H.PUSH_SCALAR | (k << 8) for k in range(20)] + [H.ADD] * 20, nscal=32) != 0  # depth > 8
    prog = [A]
    for k in range(20):                                                     # 20 distinct scalars, depth 2
        prog += [S | (k << 8), H.ADD]
    assert _eval(prog, nscal=32) == 0, _err()


def test_arity_and_operand_errors_are_reported():
    A, S = H.PUSH_ARRAY, H.PUSH_SCALAR
    for bad, what in (([A, A, H.CLAMP], b"three operands"), ([A, H.LT], b"two operands"), ([H.EXP], b"empty stack"),
                      ([A, S, S, S, H.IFELSE], b"exactly one value"), ([A, 76], b"unknown"), ([A, 99], b"unknown"),
                      ([A, 114], b"unknown"), ([A, 63], b"unknown"),
                      ([A, H.PUSH_ROW | (2 << 8), H.ADD], b"row vector")):
        assert _eval(bad, nv=3) != 0 and what in _err(), (bad, _err())
    assert _eval([A, S, H.ADD], nscal=33) != 0 and b"32 scalars" in _err()


def _enum_values(text):
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"\bIBH_EW_([A-Z0-9_]+)\s*=\s*(\d+)", text)}


def test_opcode_values_agree_across_header_python_and_julia():
    hdr = _enum_values(open(os.path.join(ROOT, "include", "ibhip.h")).read())
    assert len(hdr) >= 44
    for name, v in hdr.items():
        assert getattr(H, name) == v, name
    jl = open(os.path.join(ROOT, "julia", "IBHip.jl")).read()
    consts = {}
    for m in re.finditer(r"^const ((?:EW_\w+(?:, )?)+) = (.+)$", jl, flags=re.M):
        names = [x.strip() for x in m.group(1).split(",")]
        rhs = m.group(2).strip()
        r = re.fullmatch(r"Cint\.\((\d+):(\d+)\)", rhs)
        if r:
            vals = list(range(int(r.group(1)), int(r.group(2)) + 1))
        else:
            vals = [int(x) for x in re.findall(r"Cint\((\d+)\)", rhs)]
        assert len(vals) == len(names), m.group(0)
        consts.update(zip(names, vals))
    for name, v in hdr.items():
        assert consts.get("EW_" + name) == v, name


def test_model_hand_cases():
    nan, inf = f32(np.nan), f32(np.inf)
    assert same_bits(model(H.SIGN, f32(-0.0)), f32(-0.0)) and same_bits(model(H.SIGN, f32(0.0)), f32(0.0))
    assert np.isnan(model(H.SIGN, nan)) and model(H.SIGN, f32(-3)) == -1 and model(H.SIGN, inf) == 1
    assert np.isnan(model(H.CLAMP, nan, f32(0), f32(1)))                     # not fmaxf / fminf
    assert model(H.CLAMP, f32(5), f32(10), inf) == 10 and model(H.CLAMP, f32(2), f32(0), f32(1)) == 1
    assert same_bits(model(H.BMUL, f32(0), nan), f32(0.0))                   # false * NaN == 0
    assert same_bits(model(H.BMUL, f32(0), f32(-2)), f32(-0.0))              # false * -2f0 == -0f0
    assert same_bits(model(H.BMUL, f32(1), f32(-2)), f32(-2))
    assert model(H.POW0, nan) == 1 and model(H.POW0, inf) == 1
    x = f32(1.1)
    assert same_bits(model(H.SQR, x), x * x) and same_bits(model(H.CUBE, x), (x * x) * x)
    assert same_bits(model(H.INV, x), f32(1) / x)
    i = f32(1) / x
    assert same_bits(model(H.INVSQR, x), i * i)
    assert model(H.POW, f32(1), nan) == 1 and model(H.POW, nan, f32(0)) == 1
    assert model(H.POW, f32(-2), f32(3)) == -8 and np.isnan(model(H.POW, f32(-2), f32(0.5)))
    assert np.isnan(model(H.LOG, f32(-1))) and model(H.LOG, f32(0)) == -inf
    assert model(H.IFELSE, f32(1), f32(2), f32(3)) == 2 and model(H.IFELSE, f32(0), f32(2), nan) != model(H.IFELSE, f32(0), f32(2), nan)
    assert model(H.NOT, f32(0)) == 1 and model(H.AND, f32(1), f32(0)) == 0 and model(H.OR, f32(1), f32(0)) == 1
    assert model(H.LT, nan, f32(1)) == 0 and model(H.NE, nan, nan) == 1
    assert ulp_distance(f32(1), np.nextafter(f32(1), f32(2))) == 1 and ulp_distance(f32(-0.0), f32(0.0)) == 0
    assert set(ARITY) == set(NEW_UNARY + NEW_BINARY + NEW_TERNARY)


@pytest.mark.parametrize("s", [0.1, -0.1, 1e39, -1e39, -0.0, 0.0, float("nan"), 1.0, 2.0 ** -149, 3.0e-46, 16777217.0])
def test_exact_double_comparisons(s):
    """The host rewrite of ``x OP s`` (Float64 s) into one Float32 comparison has Julia's truth table everywhere."""
    rng = np.random.default_rng(1)
    with np.errstate(over="ignore"):
        near = np.float32(s)
    cand = [near, np.nextafter(near, f32(np.inf)), np.nextafter(near, f32(-np.inf)), f32(0), f32(-0.0), f32(np.inf),
            f32(-np.inf), f32(np.nan), np.finfo(f32).max, -np.finfo(f32).max, f32(0.1), f32(-0.1)]
    x = np.concatenate([np.array(cand, f32), rng.standard_normal(200).astype(f32)])
    for op in (H.LT, H.LE, H.GT, H.GE, H.EQ, H.NE):
        op2, t = H._exact_compare(op, s)
        assert np.array_equal(model(op2, x, f32(t)) != 0, compare_exact(x, op, s)), (op, s)
    assert H._exact_compare(H.GT, 0.1) != (H.GT, float(f32(0.1)))            # x > 0.1 is not x > 0.1f0


def test_julia_sum_keeps_the_whole_array_method():
    """Julia does not dispatch on keywords: a `Base.sum(a::HipArray{Float32, 2}; dims)` with a required `dims` would take
    plain `sum(a)` of every matrix away from the whole-array method and throw.  Every `sum` method of the binding that
    takes `dims` must give it a default, and `sum(a)` (dims = :) must still reach `_reduce(EW_SUM, ...)`."""
    jl = open(os.path.join(ROOT, "julia", "IBHip.jl")).read()
    sigs = re.findall(r"^(?:function )?Base\.sum\(([^)]*)\)", jl, flags=re.M)
    assert any("HipArray{Float32}" in s and ";" not in s for s in sigs), sigs
    kw = [s for s in sigs if ";" in s]
    assert kw, "sum(a; dims = 2) is not bound"
    for s in kw:
        for k in s.split(";", 1)[1].split(","):
            assert "=" in k, f"Base.sum({s}): keyword `{k.strip()}` has no default"
    body = jl[jl.index("function Base.sum(a::HipArray{Float32, 2}; dims"):]
    body = body[:body.index("\nend")]
    assert re.search(r"dims === \(:\) && return _reduce\(EW_SUM, a\)", body), body

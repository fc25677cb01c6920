"""``HipArray``: the Python mirror of the device array type of the reference-side binding (julia/IBHip.jl).

In Julia a user closure such as /root/reference/test/advection.jl:67-83 mixes the grid operators with broadcast
arithmetic (``ud .-= green_gauss(part, @. (uL + uR) * Cf / 2 + abs(Cf) * (uL - uR) / 2, dim)``).  The binding gives the
device array a ``Base.Broadcast`` style whose nodes are the elementwise kernels of libibhip (``ibh_ew_*``); this class
does the same through Python's operator protocol, so that the very same expression tree runs through the very same C
entry points.  torch only owns the memory (column-major Float32).
"""
import ctypes as C
import struct
import weakref

import numpy as np
import torch

from . import _lib
from ._header import constants
from ._lib import c_vp, call

# the IBH_EW_* opcodes of include/ibhip.h
ADD, SUB, MUL, DIV, MAX, MIN, SUM = constants("IBH_EW_", "ADD SUB MUL DIV MAX MIN SUM")
ABS, NEG, SQRT, COPY = constants("IBH_EW_", "ABS NEG SQRT COPY")
# the rest of Julia's elementwise Float32 math; Bool values are Float32 0 / 1 on the device
LT, LE, GT, GE, EQ, NE, AND, OR, POW, COPYSIGN, ATAN2, BMUL = constants(
    "IBH_EW_", "LT LE GT GE EQ NE AND OR POW COPYSIGN ATAN2 BMUL")
EXP, EXP2, LOG, LOG2, LOG10, SIN, COS, TANH, ATAN, SIGN, INV, NOT, POW0, SQR, CUBE, INVSQR = constants(
    "IBH_EW_", "EXP EXP2 LOG LOG2 LOG10 SIN COS TANH ATAN SIGN INV NOT POW0 SQR CUBE INVSQR")
CLAMP, IFELSE = constants("IBH_EW_", "CLAMP IFELSE")
_PLAIN_BINARY = (ADD, SUB, MUL, DIV, MAX, MIN)
_PLAIN_UNARY = (ABS, NEG, SQRT, COPY)
_LITERAL_POW = {0: POW0, 1: COPY, 2: SQR, 3: CUBE, -1: INV, -2: INVSQR}   # Base.literal_pow


_backend = None


def _B():
    global _backend
    if _backend is None:
        from . import backend
        _backend = backend
    return _backend


PUSH_ARRAY, PUSH_SCALAR, PUSH_ROW = constants("IBH_EW_", "PUSH_ARRAY PUSH_SCALAR PUSH_ROW")
_MAX_PROG, _MAX_ARR, _MAX_SCAL, _MAX_DEPTH = 48, 8, 32, 8


def _f32bits(x):
    return struct.pack("<f", x)


class _Row:
    """A host row vector (Julia's ``u∞'``): one Float32 per column of an ``(n, nv)`` operand.  It travels in the
    program's scalar table (``IBH_EW_PUSH_ROW``), so it needs no upload and is captured by value in a graph."""

    def __init__(self, values):
        self.values = [float(v) for v in np.asarray(values, dtype=np.float32).ravel()]


def _exact_compare(op, s):
    """``x OP s`` for a Float32 x and a host scalar s compared exactly, as Julia compares Float32 with Float64
    (``x > 0.1`` is not ``x > 0.1f0``): the same truth table as a comparison with one Float32 threshold."""
    s = float(s)
    with np.errstate(over="ignore"):
        f = np.float32(s)
    if np.isnan(s) or float(f) == s:
        return op, float(f)
    up = f if float(f) > s else np.nextafter(f, np.float32(np.inf))
    down = f if float(f) < s else np.nextafter(f, np.float32(-np.inf))
    if op in (GT, GE):                      # x > s  <=>  x > (largest Float32 below s)
        return GT, float(down)
    if op in (LT, LE):
        return LT, float(up)
    if op == EQ:                            # no Float32 equals s: false everywhere (x < -Inf)
        return LT, float("-inf")
    return NE, float("nan")                 # true everywhere (x != NaN)


class HipArray:
    """Device array ``(n,)`` or ``(n, nv)``, column-major Float32.  Arithmetic between HipArrays and scalars builds an
    expression (as a Julia broadcast does before it is materialised); the whole expression runs as ONE launch
    (``ibh_ew_eval``: Julia's broadcast fusion) when its value is needed -- by an operator, ``to_host``, an in-place
    update (``ud -= expr`` evaluates ``ud - expr`` straight into ``ud``).  ``HipArray.fuse = False`` evaluates node by
    node (``ibh_ew_binary`` / ``ibh_ew_unary``), bit-identical.
    The class itself is the ``conv_to_backend`` converter: ``dom(f, args..., conv_to_backend=ibamd.HipArray, ...)``."""

    __array_priority__ = 1000
    fuse = True

    def __init__(self, t):
        B = _B()
        self._bool = False   # a Bool array (Julia's HipArray{Bool}): Float32 0 / 1 on the device
        if isinstance(t, HipArray):
            self._bool = t._bool
            t = t.t
        elif isinstance(t, torch.Tensor):
            if t.dtype == torch.bool:
                t, self._bool = t.to(torch.float32), True
        else:
            t = np.asarray(t)
            if t.dtype == np.bool_:
                t, self._bool = t.astype(np.float32), True
            t = B.hip(t)
        t, _, ld = B._field(t)
        if t.ndim == 2 and t.shape[1] > 1 and ld != t.shape[0]:
            t = t.T.contiguous().T  # broadcast kernels want the columns back to back
        self._t = t
        self._expr = None               # pending (op, a, b) / (op, a): operands HipArray or float
        self._meta = (int(t.shape[0]), 1 if t.ndim == 1 else int(t.shape[1]), t.ndim)
        self._deps = weakref.WeakSet()  # pending expressions that read this array (materialised before it is written)

    @classmethod
    def _pending(cls, expr, n, nv, ndim, bool_=False):
        self = cls.__new__(cls)
        self._t = None
        self._bool = bool_
        self._expr = expr
        self._meta = (n, nv, ndim)
        self._deps = weakref.WeakSet()
        for leaf in self._leaves():
            leaf._deps.add(self)
        return self

    # ---- the value: materialises a pending expression (one launch)
    @property
    def t(self):
        if self._t is None:
            n, nv, ndim = self._meta
            out = _B().colmajor_empty(n) if ndim == 1 else _B().colmajor_empty(n, nv)
            self._evaluate_into(out)
            self._t, self._expr = out, None
        return self._t

    @t.setter
    def t(self, value):
        self._t, self._expr = value, None

    def _leaves(self):
        """Materialised arrays a pending expression reads."""
        if self._expr is None:
            return [self]
        out = []
        for x in self._expr[1:]:
            if isinstance(x, HipArray):
                out += x._leaves()
        return out

    def _flush_readers(self):
        """Before this array's memory is written: evaluate the pending expressions that read it."""
        for d in list(self._deps):
            if d._t is None:
                d.t  # noqa: B018 (materialises)
        self._deps.clear()

    def _emit(self, prog, arrs, scal):
        """Postfix program of this node; returns the stack depth it needs (None: does not fit one launch)."""
        if self._expr is None:
            key = self._t.data_ptr()
            for k, a in enumerate(arrs):
                if a._t.data_ptr() == key and a._meta == self._meta:
                    break
            else:
                if len(arrs) == _MAX_ARR:
                    return None
                arrs.append(self)
                k = len(arrs) - 1
            prog.append(PUSH_ARRAY | (k << 8))
            return 1
        op, depth, width = self._expr[0], 0, 0
        for x in self._expr[1:]:
            if isinstance(x, HipArray):
                d = x._emit(prog, arrs, scal)
                if d is None:
                    return None
            else:
                vals, push = (x.values, PUSH_ROW) if isinstance(x, _Row) else ([x], PUSH_SCALAR)
                bits, have = [_f32bits(v) for v in vals], [_f32bits(v) for v in scal]   # -0.0 is not 0.0
                k = next((i for i in range(len(have) - len(bits) + 1) if have[i:i + len(bits)] == bits), None)
                if k is None:
                    if len(scal) + len(vals) > _MAX_SCAL:
                        return None
                    k = len(scal)
                    scal.extend(vals)
                prog.append(push | (k << 8))
                d = 1
            depth = max(depth, width + d)
            width += 1
        prog.append(op)
        if len(prog) > _MAX_PROG or depth > _MAX_DEPTH:
            return None
        return depth

    def _reads_other_shape(self, out):
        """True if an array this pending expression reads overlaps the tensor ``out`` without being the same elements
        in the same layout (elementwise evaluation in place is then not safe)."""
        lo, hi = out.data_ptr(), out.data_ptr() + out.numel() * out.element_size()
        seen, stack = set(), [self]
        while stack:
            x = stack.pop()
            if id(x) in seen:
                continue
            seen.add(id(x))
            if x._t is None:
                stack.extend(y for y in x._expr[1:] if isinstance(y, HipArray))
                continue
            t = x._t
            a, b = t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()
            if a < hi and lo < b and not (a == lo and t.shape == out.shape and t.stride() == out.stride()):
                return True
        return False

    def _evaluate_into(self, out):
        """Value of the pending expression into the tensor ``out`` (may alias an operand: the kernel is elementwise)."""
        B = _B()
        prog, arrs, scal = [], [], []
        if self._emit(prog, arrs, scal) is None:
            # too large for one launch: materialise the operands that are expressions themselves, then this node
            for x in self._expr[1:]:
                if isinstance(x, HipArray):
                    x.t  # noqa: B018
            prog, arrs, scal = [], [], []
            if self._emit(prog, arrs, scal) is None:
                raise RuntimeError("broadcast expression does not fit ibh_ew_eval")
        n, nv, _ = self._meta
        P = (C.c_int32 * len(prog))(*prog)
        A = (C.c_void_p * max(len(arrs), 1))(*[a._t.data_ptr() for a in arrs])
        V = (C.c_int32 * max(len(arrs), 1))(*[a._meta[1] for a in arrs])
        S = (C.c_float * max(len(scal), 1))(*scal)
        B._stream()
        call("ibh_ew_eval", n, nv, len(prog), P, len(arrs), A, V, len(scal), S, c_vp(out.data_ptr()))

    # ---- array protocol
    @property
    def shape(self):
        n, nv, ndim = self._meta
        return (n,) if ndim == 1 else (n, nv)

    @property
    def ndim(self):
        return self._meta[2]

    def __len__(self):
        return self._meta[0]

    @property
    def n(self):
        return self._meta[0]

    @property
    def nv(self):
        return self._meta[1]

    def similar(self):
        """``similar(a)``."""
        n, nv, ndim = self._meta
        return HipArray(_B().colmajor_empty(n) if ndim == 1 else _B().colmajor_empty(n, nv))

    def copy(self):
        out = self.similar()
        out._bool = self._bool
        _B()._stream()
        call("ibh_ew_unary", COPY, self.t.numel(), c_vp(self.t.data_ptr()), c_vp(out.t.data_ptr()))
        return out

    def col(self, j):
        """``@view a[:, j]`` (1-based like the reference): aliases the parent's memory."""
        if self.ndim != 2:
            raise IndexError("col() of a vector")
        v = HipArray(self.t[:, j - 1])
        v._bool = self._bool
        v._deps = self._deps   # a write through either name flushes the readers of both
        return v

    def fill(self, value):
        """``a .= value``."""
        self._flush_readers()
        _B()._stream()
        call("ibh_ew_fill", self.t.numel(), C.c_float(float(value)), c_vp(self.t.data_ptr()))
        return self

    def to_host(self):
        h = _B().to_host(self.t)
        return h != 0 if self._bool else h

    @property
    def dtype(self):
        return np.bool_ if self._bool else np.float32

    def __bool__(self):
        if self._bool:
            raise TypeError("the truth value of a Bool HipArray is ambiguous (use it in ifelse or copy it back with "
                            "to_host)")
        return len(self) > 0

    def __getitem__(self, i):
        raise TypeError("scalar indexing of a HipArray; copy it back with to_host()")

    # ---- broadcast nodes
    @staticmethod
    def _operand(x):
        if isinstance(x, HipArray):
            return x
        if isinstance(x, (int, float, np.floating, np.integer)):
            return float(np.float32(x))
        if isinstance(x, (list, tuple, np.ndarray)) and np.ndim(x) == 1:
            return _Row(x)   # a host vector broadcasts along the rows: Julia's `u∞'`
        raise TypeError(f"cannot broadcast a HipArray with {type(x).__name__} (convert with HipArray(...))")

    @staticmethod
    def _shape(operands):
        fields = [f for f in operands if isinstance(f, HipArray)]
        rows = [len(r.values) for r in operands if isinstance(r, _Row)]
        n = fields[0].n
        nv = max([f.nv for f in fields] + rows)
        for f in fields:
            if f.n != n or f.nv not in (1, nv):
                raise ValueError(f"shapes {tuple(x.shape for x in fields)} do not broadcast")
        if any(r != nv for r in rows):
            raise ValueError(f"a row vector of length {rows} does not broadcast with {nv} columns")
        ndim = 1 if nv == 1 and not rows and all(f.ndim == 1 for f in fields) else 2
        return n, nv, ndim

    def _node(self, op, operands, bool_=False, out=None):
        """The broadcast node ``op(operands...)`` (operands already typed: HipArray, Float32 scalar or row)."""
        n, nv, ndim = self._shape(operands)
        if out is not None and (out.n != n or out.nv != nv):
            raise ValueError("in-place broadcast changes the shape")
        if out is not None and out._bool != bool_:
            raise TypeError("in-place broadcast changes the element type (Bool / Float32)")
        plain = op in _PLAIN_BINARY + _PLAIN_UNARY and not any(isinstance(x, _Row) for x in operands)
        if HipArray.fuse:
            node = HipArray._pending((op, *operands), n, nv, ndim, bool_)
            if out is None:
                return node
            # `out .= out op other`: the fused expression straight into out's memory
            out.t  # noqa: B018 (out is an operand: it must hold a value)
            readers = [d for d in out._deps if d is not node]
            for d in readers:
                if d._t is None:
                    d.t  # noqa: B018
            if node._reads_other_shape(out._t):
                # a leaf aliases out's memory with another shape (`P ./= P[:, 1]`): threads of other columns would race
                # with the write; Julia's broadcast_unalias copies in that case -- so does this
                tmp = torch.empty_like(out._t)
                node._evaluate_into(tmp)
                out._t.copy_(tmp)
            else:
                node._evaluate_into(out._t)
            node._t, node._expr = out._t, None
            out._deps.clear()
            return out
        B = _B()
        if out is None:
            out = HipArray(B.colmajor_empty(n) if ndim == 1 else B.colmajor_empty(n, nv))
            out._bool = bool_
        else:
            out._flush_readers()
        if plain and len(operands) == 2:
            a, b = operands
            fa, sa = (a, 0.0) if isinstance(a, HipArray) else (None, a)
            fb, sb = (b, 0.0) if isinstance(b, HipArray) else (None, b)
            B._stream()
            call("ibh_ew_binary", op, n, nv, c_vp(fa.t.data_ptr()) if fa is not None else c_vp(None),
                 fa.nv if fa is not None else 0, C.c_float(sa), c_vp(fb.t.data_ptr()) if fb is not None else c_vp(None),
                 fb.nv if fb is not None else 0, C.c_float(sb), c_vp(out.t.data_ptr()))
        elif plain:
            B._stream()
            call("ibh_ew_unary", op, self.t.numel(), c_vp(self.t.data_ptr()), c_vp(out.t.data_ptr()))
        else:
            # any other node: a one-node program (the same device code as inside a fused tree: the same bits)
            HipArray._pending((op, *operands), n, nv, ndim, bool_)._evaluate_into(out.t)
        return out

    def _binary(self, op, other, reverse=False, out=None):
        a, b = (other, self) if reverse else (self, other)
        a, b = self._operand(a), self._operand(b)
        ba, bb = _isbool(a), _isbool(b)
        if op in (AND, OR):
            if not (ba and bb):
                raise TypeError("& and | take Bool operands")
            return self._node(op, (a, b), True, out)
        if op in (LT, LE, GT, GE, EQ, NE):
            return self._node(op, (a, b), True, out)
        if ba and bb:
            raise TypeError("arithmetic between two Bool arrays (Julia gives Int): multiply one by 1f0 first")
        if op == MUL and (ba or bb):   # Julia's strong zero: ifelse(b, x, copysign(0, x))
            return self._node(BMUL, (a, b) if ba else (b, a), False, out)
        if (ba or bb) and op in (POW, COPYSIGN, ATAN2):
            raise TypeError("math functions take Float32 operands (multiply a Bool by 1f0 first)")
        return self._node(op, (a, b), False, out)

    def _unary(self, op):
        if self._bool and op not in (ABS, COPY, NOT):
            raise TypeError("math functions take Float32 operands (multiply a Bool by 1f0 first)")
        if op == NOT and not self._bool:
            raise TypeError("! / ~ takes a Bool array")
        return self._node(op, (self,), self._bool)

    def _compare(self, op, other):
        if isinstance(other, (bool, np.bool_)):
            other = float(other)
        if isinstance(other, (int, float, np.floating, np.integer)) and not isinstance(other, np.float32):
            op, other = _exact_compare(op, other)
        return self._binary(op, other)

    def __add__(self, o): return self._binary(ADD, o)
    def __radd__(self, o): return self._binary(ADD, o, reverse=True)
    def __sub__(self, o): return self._binary(SUB, o)
    def __rsub__(self, o): return self._binary(SUB, o, reverse=True)
    def __mul__(self, o): return self._binary(MUL, o)
    def __rmul__(self, o): return self._binary(MUL, o, reverse=True)
    def __truediv__(self, o): return self._binary(DIV, o)
    def __rtruediv__(self, o): return self._binary(DIV, o, reverse=True)
    def __iadd__(self, o): return self._binary(ADD, o, out=self)   # `a .+= o`
    def __isub__(self, o): return self._binary(SUB, o, out=self)   # `a .-= o`
    def __imul__(self, o): return self._binary(MUL, o, out=self)
    def __itruediv__(self, o): return self._binary(DIV, o, out=self)
    def __neg__(self): return self._unary(NEG)
    def __abs__(self): return self._unary(ABS)
    # comparisons give Bool arrays; == / != stay Python's identity (the arrays live in WeakSets): use eq / ne
    def __lt__(self, o): return self._compare(LT, o)
    def __le__(self, o): return self._compare(LE, o)
    def __gt__(self, o): return self._compare(GT, o)
    def __ge__(self, o): return self._compare(GE, o)
    def __and__(self, o): return self._binary(AND, o)
    def __rand__(self, o): return self._binary(AND, o, reverse=True)
    def __or__(self, o): return self._binary(OR, o)
    def __ror__(self, o): return self._binary(OR, o, reverse=True)
    def __invert__(self): return self._unary(NOT)   # Julia's `!` on a Bool

    def __pow__(self, p):
        """``x .^ p``: a Python int exponent is Julia's literal power (``Base.literal_pow``: x^2 = x*x, x^-1 = inv(x),
        ...); any other exponent is Julia's Float32 ``^``, evaluated in double and rounded once."""
        if isinstance(p, (int, np.integer)) and not isinstance(p, (bool, np.bool_)):
            if int(p) in _LITERAL_POW:
                return self._unary(_LITERAL_POW[int(p)])
            return self._binary(POW, float(p))
        return self._binary(POW, p)

    def __rpow__(self, base):
        return self._binary(POW, base, reverse=True)

    def maximum_with(self, o):
        """``max.(a, o)``."""
        return self._binary(MAX, o)

    def minimum_with(self, o):
        """``min.(a, o)``."""
        return self._binary(MIN, o)

    def sqrt(self):
        return self._unary(SQRT)

    def _reduce(self, op):
        out = torch.empty(1, dtype=torch.float32, device=self.t.device)
        _B()._stream()
        call("ibh_ew_reduce", op, self.t.numel(), c_vp(self.t.data_ptr()), c_vp(out.data_ptr()))
        return float(out.item())

    def maximum(self):
        """``maximum(a)``."""
        return self._reduce(MAX)

    def minimum(self):
        return self._reduce(MIN)

    def sum(self, dims=None):
        """``sum(a)``, or ``sum(a; dims = 2)``: the columns of each row added in order ((a1 + a2) + a3 ..., Julia's
        order), one launch; in Julia the result is ``(n, 1)``, here ``(n,)``."""
        if dims is None:
            return self._reduce(SUM)
        if dims != 2:
            raise ValueError("sum(dims=...) supports dims = 2 (along the rows)")
        if self._bool:
            raise TypeError("sum of a Bool array (Julia gives Int): multiply it by 1f0 first")
        out = HipArray(_B().colmajor_empty(self.n))
        _B()._stream()
        call("ibh_ew_reduce_rows", self.n, self.nv, c_vp(self.t.data_ptr()), c_vp(out.t.data_ptr()))
        return out


def _isbool(x):
    return isinstance(x, HipArray) and x._bool


def _fn1(op):
    def f(x):
        return HipArray._operand(x)._unary(op) if isinstance(x, HipArray) else _host1[op](x)
    return f


_host1 = {EXP: np.exp, EXP2: np.exp2, LOG: np.log, LOG2: np.log2, LOG10: np.log10, SIN: np.sin, COS: np.cos,
          TANH: np.tanh, ATAN: np.arctan, SIGN: np.sign, INV: lambda x: 1 / x}
# Julia's elementwise functions by their Julia names, on HipArrays (host numbers fall through to numpy)
exp, exp2, log, log2, log10 = _fn1(EXP), _fn1(EXP2), _fn1(LOG), _fn1(LOG2), _fn1(LOG10)
sin, cos, tanh, sign, inv = _fn1(SIN), _fn1(COS), _fn1(TANH), _fn1(SIGN), _fn1(INV)


def _first(*xs):
    for x in xs:
        if isinstance(x, HipArray):
            return x
    raise TypeError("expected a HipArray operand")


def atan(y, x=None):
    """``atan(y)`` or ``atan(y, x)`` (the quadrant-aware two-argument form)."""
    if x is None:
        return _fn1(ATAN)(y)
    h = _first(y, x)
    return h._binary(ATAN2, x) if y is h else h._binary(ATAN2, y, reverse=True)


def copysign(x, y):
    h = _first(x, y)
    return h._binary(COPYSIGN, y) if x is h else h._binary(COPYSIGN, x, reverse=True)


def eq(a, b):
    """``a .== b`` (Bool array): HipArray keeps Python's identity ``==``."""
    h = _first(a, b)
    return h._compare(EQ, b if a is h else a)


def ne(a, b):
    """``a .!= b`` (Bool array)."""
    h = _first(a, b)
    return h._compare(NE, b if a is h else a)


def clamp(x, lo, hi):
    """``clamp.(x, lo, hi)`` = ``ifelse(x > hi, hi, ifelse(x < lo, lo, x))``: a NaN in x stays NaN."""
    ops = tuple(HipArray._operand(v) for v in (x, lo, hi))
    if any(_isbool(v) for v in ops):
        raise TypeError("clamp takes Float32 operands")
    return _first(*ops)._node(CLAMP, ops, False)


def ifelse(c, a, b):
    """``ifelse.(c, a, b)``; c must be a Bool array (a comparison)."""
    if not _isbool(c):
        raise TypeError("ifelse needs a Bool condition (a comparison), not a Float32 array or a number")
    ops = (c, HipArray._operand(a), HipArray._operand(b))
    return c._node(IFELSE, ops, _isbool(ops[1]) and _isbool(ops[2]))


def unwrap(x):
    return x.t if isinstance(x, HipArray) else x


def rewrap(result, like_hiparray):
    """Wrap the tensor(s) an operator returns when it was called with HipArray operands."""
    if not like_hiparray:
        return result
    if isinstance(result, torch.Tensor):
        return HipArray(result)
    if isinstance(result, tuple):
        return tuple(rewrap(r, True) for r in result)
    return result

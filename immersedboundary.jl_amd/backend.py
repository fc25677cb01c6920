"""GPU backend: the reference's plug-in surface re-implemented over libibhip.

Mirrors, for the hot path only,
  * ``conv_to_backend`` / ``conv_from_backend`` converters and ``to_backend`` for the structs
    (/root/reference/src/arraybends.jl:14-77, src/ImmersedBoundary.jl:788-790, :846-855);
  * the grid operators on a Partition (src/ImmersedBoundary.jl:873-1157) -- same names,
    argument order and return shapes (fresh arrays), ``dim`` 1-based;
  * ``(dom::Domain)(f, args...)`` (:820-864) -- through the host with converters, or on device-resident arrays
    (``ibh_domain_gather`` / ``ibh_domain_scatter``) -- and ``impose_bc!`` (:1197-1247).

Device memory, streams and (elsewhere) torch.distributed come from PyTorch -- plumbing only;
all arithmetic is in the HIP kernels of libibhip.so, reached through the C ABI with raw device
pointers.  Nothing here computes on the CPU: operators raise if handed host arrays, and loading
fails loudly if the library is missing.

Device field layout = the reference's column-major ``(ncells, nvars)``: a torch tensor of shape
``(n, nv)`` with strides ``(1, ld)``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from ._header import CONSTANTS as _K
from ._lib import call, c_vp
from .accumulator import Accumulator
from .domain import ROLE_FLUID, ROLE_GHOST, ROLE_SOLID, Boundary, Partition, Surface
from .hostview import partition_args

# the sweep flags of include/ibhip.h
IBH_FORCE_GENERAL = _K["IBH_FORCE_GENERAL"]
IBH_IMAGE_ONLY = _K["IBH_IMAGE_ONLY"]
IBH_PASS_A_ONLY = _K["IBH_PASS_A_ONLY"]
IBH_PASS_B_ONLY = _K["IBH_PASS_B_ONLY"]
IBH_EXACT = _K["IBH_EXACT"]
IBH_PHASE_INTERIOR = _K["IBH_PHASE_INTERIOR"]
IBH_PHASE_BOUNDARY = _K["IBH_PHASE_BOUNDARY"]
IBH_NO_FUSE = _K["IBH_NO_FUSE"]
IBH_SWEEP_ONLY = _K["IBH_SWEEP_ONLY"]
IBH_FORCE_MIXED = _K["IBH_FORCE_MIXED"]
IBH_NO_QUAD = _K["IBH_NO_QUAD"]

_initialised = {}


_have_gpu = None


def _dev():
    global _have_gpu
    if _have_gpu is None:
        _have_gpu = bool(torch.cuda.is_available())
    if not _have_gpu:
        raise _lib.IbhError("no HIP device visible: the ImmersedBoundary hot path runs on the GPU only "
                            "(there is no CPU fallback)")
    d = torch.cuda.current_device()
    dev = _initialised.get(d)
    if dev is None:
        call("ibh_init", d)
        dev = _initialised[d] = torch.device("cuda", d)
    return dev


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream():
    """The library launches on torch's current stream (asked for through the raw-handle query: the operators of a user
    closure are host-bound, and `torch.cuda.current_stream()` alone costs as much as a launch)."""
    if _raw_stream is not None:
        call("ibh_set_stream", c_vp(_raw_stream(torch.cuda.current_device())))
    else:
        call("ibh_set_stream", c_vp(torch.cuda.current_stream().cuda_stream))


def _ptr(t):
    return c_vp(t.data_ptr()) if t is not None else c_vp(None)


def _hptr(a):
    return a.ctypes.data_as(c_vp)


# ---------------------------------------------------------------------------
# converters (conv_to_backend / conv_from_backend)
# ---------------------------------------------------------------------------
def colmajor_empty(n, nv=None, dtype=torch.float32):
    """Uninitialised device array ``(n,)`` or ``(n, nv)`` in column-major layout."""
    dev = _dev()
    if nv is None:
        return torch.empty(n, dtype=dtype, device=dev)
    return torch.empty((nv, n), dtype=dtype, device=dev).T


def hip(a):
    """``conv_to_backend``: host array -> device array (column-major)."""
    dev = _dev()
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    a = np.asarray(a)
    if a.dtype == np.float64:
        a = a.astype(np.float32)
    if a.ndim == 1:
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    if a.ndim == 2:
        return torch.from_numpy(np.ascontiguousarray(a.T)).to(dev).T
    raise ValueError("hip(): only 1-D and 2-D fields are supported")


def to_host(t):
    """``conv_from_backend``: device array -> numpy array."""
    if not isinstance(t, torch.Tensor):
        t = t.t  # HipArray
    return np.ascontiguousarray(t.detach().cpu().numpy())


def _hipaware(fn):
    """Operators take and return ``HipArray`` (hiparray.py: broadcast arithmetic through ``ibh_ew_*``) when they are
    called with one: the Python form of Julia's dispatch on the array type (julia/IBHip.jl)."""
    import functools

    H = {}

    @functools.wraps(fn)
    def wrapper(*args, **kwargs):
        if not H:
            from . import hiparray
            H["A"], H["rewrap"] = hiparray.HipArray, hiparray.rewrap
        HipArray = H["A"]
        hit = False

        def un(x):
            nonlocal hit
            if isinstance(x, HipArray):
                hit = True
                return x.t
            if isinstance(x, tuple):
                return tuple(un(v) for v in x)
            return x
        # an operator that writes into a HipArray (out=...): pending broadcasts that read it are evaluated first, so
        # that they see the old values like Julia's eager broadcast would
        if kwargs and isinstance(kwargs.get("out"), HipArray):
            kwargs["out"]._flush_readers()
        a = [un(x) for x in args]
        k = {key: un(v) for key, v in kwargs.items()} if kwargs else kwargs
        out = fn(*a, **k)
        return H["rewrap"](out, True) if hit else out
    return wrapper


def _field(t, n=None):
    """Validate a device field and return (tensor, nv, ld)."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise TypeError("expected a device array (convert with ibamd.hip); there is no CPU path")
    if t.dtype != torch.float32:
        raise TypeError("fields must be Float32")
    if t.ndim == 1:
        if t.stride(0) != 1:
            t = t.contiguous()
        nv, ld = 1, t.shape[0]
    elif t.ndim == 2:
        if t.stride(0) != 1 or (t.shape[1] > 1 and t.stride(1) < t.shape[0]):
            t = t.T.contiguous().T
        nv, ld = t.shape[1], (t.stride(1) if t.shape[1] > 1 else t.shape[0])
    else:
        raise ValueError("fields are (n,) or (n, nv)")
    if n is not None and t.shape[0] != n:
        raise ValueError(f"field has {t.shape[0]} rows, expected {n}")
    return t, nv, ld


def _field_inplace(t, n=None, what="destination"):
    """A device field that a kernel WRITES: it must already be Float32 with the cell index fastest (column-major,
    ``ibamd.hip`` / ``colmajor_empty`` give that), because a silent layout copy would take the update and drop it."""
    f, nv, ld = _field(t, n)
    if f.data_ptr() != t.data_ptr() or f.stride() != t.stride():
        raise TypeError(f"{what} must be a column-major Float32 device array (cell index fastest, e.g. ibamd.hip(a) or "
                        f"colmajor_empty(n, nv)); got strides {tuple(t.stride())} for shape {tuple(t.shape)}: it would "
                        "be copied and the update lost")
    return f, nv, ld


def _like(t, n):
    return colmajor_empty(n) if t.ndim == 1 else colmajor_empty(n, t.shape[1])


# ---------------------------------------------------------------------------
# structs on the device
# ---------------------------------------------------------------------------
class _Handle:
    """A library handle and the name of the entry that destroys it: ``handle`` is set by the subclass once its create call
    has succeeded, and goes to ``_destroy`` once, when the object goes."""
    _destroy = None
    handle = None

    def __del__(self):
        try:
            if self.handle:
                h, self.handle = self.handle, None
                getattr(_lib.load(), self._destroy)(h)
        except Exception:  # noqa: BLE001
            pass


class DevicePartition(_Handle):
    """Device-resident Partition: ``to_backend(part, hip)`` (uploads once, caches the handle)."""
    _destroy = "ibh_partition_destroy"

    def __init__(self, part: Partition):
        dev = _dev()
        self.host = part
        self.id = part.id
        self.nd = part.ndims
        self.nc = part.spacing.shape[0]
        centers = np.asfortranarray(part.centers, dtype=np.float32)
        args, keep = partition_args(part)
        self.nf = [int(n) for n in keep["nf"]]
        h = c_vp()
        call("ibh_partition_create", C.byref(h), self.nd, self.nc, _hptr(keep["spacing"]), _hptr(centers), *args[:-1],
             int(getattr(part, "block_size", 0)), args[-1])
        self.handle = h
        # device copies of what user closures read (part.spacing[:, dim], part.centers)
        self.spacing = hip(part.spacing)
        self.centers = hip(part.centers)
        self.domain = torch.from_numpy(keep["domain"]).to(dev)
        self.image = torch.from_numpy(np.ascontiguousarray(part.image, dtype=np.int32)).to(dev)
        self.image_in_domain = torch.from_numpy(keep["image_in_domain"]).to(dev)
        info = (C.c_int64 * _lib.INFO_COUNT)()
        call("ibh_partition_info", h, info, _lib.INFO_COUNT)
        self.info = _lib.info_dict(self.nd, info)   # the slots by name: include/ibhip.h says what each one counts

    @property
    def ndims(self):
        return self.nd


class DeviceAccumulator(_Handle):
    """Device-resident Accumulator; callable like the reference's (accumulator.jl:78-130)."""
    _destroy = "ibh_acc_destroy"

    def __init__(self, acc: Accumulator):
        _dev()
        self.n_output, self.n_input = acc.n_output, acc.n_input
        self.first_index = acc.first_index
        h = c_vp()
        w = None if acc.w is None else np.ascontiguousarray(acc.w, dtype=np.float32)
        call("ibh_acc_create", C.byref(h), acc.n_output, acc.n_input, _hptr(acc.off), _hptr(acc.idx),
             _hptr(w) if w is not None else c_vp(None), 0)
        self.handle = h

    def __call__(self, v):
        from .hiparray import HipArray
        if isinstance(v, HipArray):
            return HipArray(self(v.t))
        v, nv, ld = _field(v, self.n_input)
        out = _like(v, self.n_output)
        _stream()
        call("ibh_accumulate", self.handle, _ptr(v), nv, ld, _ptr(out), self.n_output)
        return out

    def diff_add(self, out, a, b):
        """``out .+= acc(a .- b)`` in one launch (``ibh_accumulate_diff_add``); same arithmetic as the separate operations."""
        a, nv, ld = _field(a, self.n_input)
        b, nvb, ldb = _field(b, self.n_input)
        o, nvo, ldo = _field_inplace(out, self.n_output, "out")
        if nvb != nv or nvo != nv or ldb != ld:
            out += self(a - b)
            return out
        _stream()
        call("ibh_accumulate_diff_add", self.handle, _ptr(a), _ptr(b), nv, ld, _ptr(o), ldo)
        return out


class DeviceBoundary(_Handle):
    """Device-resident Boundary (ImmersedBoundary.jl:406-414)."""
    _destroy = "ibh_bc_destroy"

    def __init__(self, b: Boundary):
        self.host = b
        self.ng = int(b.ghost_indices.shape[0])
        acc = b.image_interpolator
        h = c_vp()
        gi = np.ascontiguousarray(b.ghost_indices, dtype=np.int32)
        idm = np.ascontiguousarray(b.image_domain, dtype=np.int32)
        gd = np.ascontiguousarray(b.ghost_distances, dtype=np.float32)
        idist = np.ascontiguousarray(b.image_distances, dtype=np.float32)
        _dev()
        call("ibh_bc_create", C.byref(h), self.ng, _hptr(gi), _hptr(gd), _hptr(idist), int(idm.size), _hptr(idm),
             _hptr(acc.off), _hptr(acc.idx), _hptr(np.ascontiguousarray(acc.w, dtype=np.float32)), 0)
        self.handle = h
        self.ghost_indices = torch.from_numpy(gi).to(_dev())
        self.projections = hip(b.projections)
        self.normals = hip(b.normals)
        self.image_distances = hip(b.image_distances)
        self.ghost_distances = hip(b.ghost_distances)


class DeviceSurface:
    """Device-resident Surface (ImmersedBoundary.jl:328-376): two Accumulators + the areas for the integrals."""

    def __init__(self, s: Surface):
        self.host = s
        self.n = int(s.points.shape[0])
        self.interpolator = DeviceAccumulator(s.interpolator)
        self.offset_interpolator = DeviceAccumulator(s.offset_interpolator)
        self.points, self.normals = hip(s.points), hip(s.normals)
        self.offsets, self.areas = hip(s.offsets), hip(s.areas)

    def __call__(self, u):
        """``surf(u)``: values of the field array ``u`` at the surface control points (:364)."""
        return self.interpolator(u)


def at_offset(surf, u):
    """``at_offset(surf, u)`` (:372): values at the offset sampling points."""
    return to_backend(surf).offset_interpolator(u)


def surface_integral(surf, u):
    """``surface_integral(surf, u)`` (:345-357): sum over the control points of ``areas .* u`` per column --
    one elementwise product and one device reduction per column (``ibh_ew_binary`` / ``ibh_ew_reduce``)."""
    from .hiparray import HipArray
    surf = to_backend(surf)
    U = u if isinstance(u, HipArray) else HipArray(u)
    if U.n != surf.n:
        raise ValueError(f"field has {U.n} rows, the surface {surf.n} control points")
    prod = U * HipArray(surf.areas)
    if U.ndim == 1:
        return np.float32(prod.sum())
    return np.array([HipArray(prod.t[:, v]).sum() for v in range(U.nv)], dtype=np.float32)


def volume_integral(dom, A):
    """``volume_integral(dom, A)`` (:1415-1431) on a device-resident global array: A times the cell volumes (the
    widths come from the Domain's cell table), summed per column on the device."""
    from .hiparray import HipArray
    U = A if isinstance(A, HipArray) else HipArray(A)
    if U.n != len(dom):
        raise ValueError("volume_integral takes a global array (one row per cell of the domain)")
    wd = getattr(dom, "_device_widths", None)
    if wd is None:
        from .mesher import get_cells
        _, widths = get_cells(dom.mesh)
        wd = dom._device_widths = [HipArray(np.ascontiguousarray(widths[d], dtype=np.float32))
                                   for d in range(widths.shape[0])]
    prod = U * wd[0]          # `Ai .*= part.spacing[:, dim]` dim by dim, like the reference
    for w in wd[1:]:
        prod *= w
    if U.ndim == 1:
        return np.float32(prod.sum())
    return np.array([HipArray(prod.t[:, v]).sum() for v in range(U.nv)], dtype=np.float32)


def to_backend(x, converter=hip):
    """``ArrayBackends.to_backend`` (arraybends.jl:14-77) for the structs on the hot path."""
    if isinstance(x, (DevicePartition, DeviceAccumulator, DeviceBoundary, DeviceSurface)):
        return x
    if isinstance(x, Surface):
        if getattr(x, "_device", None) is None:
            x._device = DeviceSurface(x)
        return x._device
    if isinstance(x, Partition):
        if getattr(x, "_device", None) is None:
            x._device = DevicePartition(x)
        return x._device
    if isinstance(x, Accumulator):
        if getattr(x, "_device", None) is None:
            x._device = DeviceAccumulator(x)
        return x._device
    if isinstance(x, Boundary):
        if getattr(x, "_device", None) is None:
            x._device = DeviceBoundary(x)
        return x._device
    if isinstance(x, tuple):
        return tuple(to_backend(v, converter) for v in x)
    if isinstance(x, dict):
        return {k: to_backend(v, converter) for k, v in x.items()}
    if isinstance(x, (np.ndarray, torch.Tensor)):
        return converter(x)
    return x


def _part(p):
    if not isinstance(p, DevicePartition):
        raise TypeError("operators run on a device Partition (to_backend(part, hip)); there is no CPU path")
    return p


# ---------------------------------------------------------------------------
# grid operators (ImmersedBoundary.jl:873-1157)
# ---------------------------------------------------------------------------
def _cell_to_face(name, part, u, dim):
    part = _part(part)
    u, nv, ld = _field(u, part.nc)
    out = _like(u, part.nf[dim - 1])
    _stream()
    call(name, part.handle, dim, _ptr(u), nv, ld, _ptr(out), part.nf[dim - 1])
    return out


@_hipaware
def at_owners(part, u, dim):
    """:879"""
    return _cell_to_face("ibh_at_owners", part, u, dim)


@_hipaware
def at_neighbors(part, u, dim):
    """:889"""
    return _cell_to_face("ibh_at_neighbors", part, u, dim)


@_hipaware
def at_faces(part, u, dim):
    """:899"""
    return _cell_to_face("ibh_at_faces", part, u, dim)


@_hipaware
def face_gradient(part, u, a, b=None):
    """:1039 ``face_gradient(part,u,dim)`` / :1051 ``face_gradient(part,u,grad_u,dim)``."""
    if b is None:
        return _cell_to_face("ibh_face_gradient", part, u, a)
    gu, dim = a, b
    return tuple(face_gradient(part, u, dim) if i == dim else at_faces(part, gu[i - 1], dim)
                 for i in range(1, _part(part).nd + 1))


def _gg(part, uf, dim, uns):
    part = _part(part)
    uf, nv, ld = _field(uf, part.nf[dim - 1])
    out = _like(uf, part.nc)
    _stream()
    call("ibh_green_gauss", part.handle, dim, _ptr(uf), nv, ld, _ptr(out), part.nc, uns)
    return out


@_hipaware
def green_gauss(part, uf, dim):
    """:918"""
    return _gg(part, uf, dim, 0)


@_hipaware
def unsigned_green_gauss(part, uf, dim):
    """:934"""
    return _gg(part, uf, dim, 1)


@_hipaware
def divergent(part, uf):
    """:950"""
    s = green_gauss(part, uf[0], 1)
    for d in range(2, _part(part).nd + 1):
        s = s + green_gauss(part, uf[d - 1], d)
    return s


@_hipaware
def cell_gradient(part, u, dim=None):
    """:965 / :980"""
    part = _part(part)
    if dim is None:
        # the tuple form: all dimensions in one sweep per field (ibh_cell_gradient_nd)
        u, nv, ld = _field(u, part.nc)
        nd, nc = part.nd, part.nc
        _stream()
        if nv == 1 and part.info["full_blocks"] > 0:
            # gradients + sensor back to back: the block sweep writes them in place (no copy out of a workspace)
            buf = colmajor_empty(nc, nd + 1)
            call("ibh_cell_gradient_nd", part.handle, _ptr(u), 1, ld, _ptr(buf), nc, c_vp(buf.data_ptr() + 4 * nd * nc), nc)
        elif nv > 1 and part.info["full_blocks"] > 0:
            # several fields: every field's block sweep writes [grad_1 .. grad_nd, sensor] in place, the tuple's arrays are
            # strided views (columns d, d + nd + 1, ...: leading dimension (nd + 1) nc) -- no copies out of a workspace
            buf = colmajor_empty(nc, nv * (nd + 1))
            call("ibh_cell_gradient_fields", part.handle, _ptr(u), nv, ld, _ptr(buf))
            return tuple(buf[:, d::nd + 1] for d in range(nd))
        else:
            buf = colmajor_empty(nc, nd * nv)
            call("ibh_cell_gradient_nd", part.handle, _ptr(u), nv, ld, _ptr(buf), nc, None, 0)
        return tuple(buf[:, d * nv] if u.ndim == 1 else buf[:, d * nv:(d + 1) * nv] for d in range(nd))
    u, nv, ld = _field(u, part.nc)
    out = _like(u, part.nc)
    _stream()
    call("ibh_cell_gradient", part.handle, dim, _ptr(u), nv, ld, _ptr(out), part.nc)
    return out


def cell_gradient_array(part, u):
    """``cell_gradient(part, u)`` of a scalar field as ONE ``(nc, nd)`` array (the tuple form's buffer: no copies)."""
    g = cell_gradient(part, u)
    base = g[0]
    nd = len(g)
    return torch.as_strided(base, (base.shape[0], nd), (1, base.shape[0]), base.storage_offset())


def _dist(name, part, dim):
    part = _part(part)
    out = colmajor_empty(part.nf[dim - 1])
    _stream()
    call(name, part.handle, dim, _ptr(out))
    return out


def face_distance(part, dim):
    """:995"""
    return _dist("ibh_face_distance", part, dim)


def owner_distance(part, dim):
    """:1010"""
    return _dist("ibh_owner_distance", part, dim)


def neighbor_distance(part, dim):
    """:1024"""
    return _dist("ibh_neighbor_distance", part, dim)


@_hipaware
def JST_sensor(part, p, dim=0):
    """:1077"""
    part = _part(part)
    p, nv, ld = _field(p, part.nc)
    out = _like(p, part.nc)
    _stream()
    call("ibh_jst_sensor", part.handle, dim, _ptr(p), nv, ld, _ptr(out), part.nc)
    return out


@_hipaware
def MUSCL(part, u, du, dim, D=None, high_order=False):
    """:1113"""
    part = _part(part)
    u, nv, ld = _field(u, part.nc)
    du, nv2, ld2 = _field(du, part.nc)
    if nv2 != nv:
        raise ValueError("u and du must have the same shape")
    if ld2 != ld and u.ndim == 2:
        du = du.T.contiguous().T
        u = u.T.contiguous().T
        ld = part.nc
    if D is not None:
        D, nvd, _ = _field(D, part.nc)
        if nvd != 1:
            raise ValueError("D must be a vector")
    nf = part.nf[dim - 1]
    uL, uR = _like(u, nf), _like(u, nf)
    _stream()
    call("ibh_muscl", part.handle, dim, _ptr(u), _ptr(du), nv, ld, _ptr(D), int(bool(high_order)), _ptr(uL),
         _ptr(uR), nf)
    return uL, uR


# ---------------------------------------------------------------------------
# fused residual sweeps
# ---------------------------------------------------------------------------
@_hipaware
def residual_advection(part, u, C_, out=None, flags=0):
    """Fused closure of test/advection.jl:67-83 (``ud`` from zero): returns ``ud``."""
    part = _part(part)
    u, nv, _ = _field(u, part.nc)
    if nv != 1:
        raise ValueError("u must be a scalar field")
    C_, nvc, ldc = _field(C_, part.nc)
    if nvc != part.nd:
        raise ValueError("C must be (nc, nd)")
    if out is not None:
        ud, nvo, _ = _field_inplace(out, part.nc, "out")
        if nvo != 1 or out.ndim != 1:
            raise ValueError("out must be a scalar field (nc,)")
    else:
        ud = torch.zeros(part.nc, dtype=torch.float32, device=u.device)
    _stream()
    call("ibh_residual_advection", part.handle, _ptr(u), _ptr(C_), ldc, _ptr(ud), flags)
    return ud


def residual_advection_repeat(part, u, C_, out, n, flags=0):
    """``n`` sweeps of ``residual_advection`` launched back to back by one C call (``ibh_residual_advection_n``): the step
    loop as a compiled host runs it.  ``out`` is written ``n`` times."""
    part = _part(part)
    u, nv, _ = _field(u, part.nc)
    C_, nvc, ldc = _field(C_, part.nc)
    ud, nvo, _ = _field_inplace(out, part.nc, "out")
    if nv != 1 or nvc != part.nd or nvo != 1:
        raise ValueError("u (nc,), C (nc, nd), out (nc,)")
    _stream()
    call("ibh_residual_advection_n", part.handle, _ptr(u), _ptr(C_), ldc, _ptr(ud), flags, int(n))
    return ud


# ---------------------------------------------------------------------------
# an explicit solver step, device resident (test/advection.jl:30-89)
# ---------------------------------------------------------------------------
class BCSet(_Handle):
    """An ordered list of ``impose_bc!`` calls (ImmersedBoundary.jl:1197-1247) whose closures the library knows --
    ``(name, value)``: ``do bdry, u; value end``; ``(name, "copy")``: ``do bdry, u; copy(u) end`` (the three calls of
    test/advection.jl:30-46) -- on the one partition ``ipart`` of ``dom`` whose local cell order is the global one.
    ``apply(u)`` has the semantics of the sequential calls; boundaries that do not read each other's ghost cells share
    their two launches (``n_levels`` pairs in all)."""
    _destroy = "ibh_bcset_destroy"

    def __init__(self, dom, specs, ipart=1):
        part = dom.partitions[ipart]
        if not np.array_equal(part.domain, np.arange(part.domain.size)):
            raise ValueError("BCSet: the partition's local cell order must be the global one (a one-partition domain)")
        self._bcs = []
        modes, values = [], []
        for name, spec in specs:
            self._bcs.append(to_backend(dom.boundaries[name][ipart]))
            modes.append(1 if isinstance(spec, str) and spec == "copy" else 0)
            values.append(0.0 if modes[-1] else float(spec))
        n = len(self._bcs)
        arr = (c_vp * n)(*[bd.handle for bd in self._bcs])
        m = np.asarray(modes, dtype=np.int32)
        v = np.asarray(values, dtype=np.float32)
        h = c_vp()
        _dev()
        call("ibh_bcset_create", C.byref(h), n, arr, _hptr(m), _hptr(v))
        self.handle = h
        ng, nl = C.c_int32(0), C.c_int32(0)
        call("ibh_bcset_info", h, C.byref(ng), C.byref(nl))
        self.n_ghost, self.n_levels = int(ng.value), int(nl.value) & 0xffff
        self.n_direct_levels = int(nl.value) >> 16      # levels blended straight into the field (one launch each)

    def healthy(self):
        """True while the set reports a ghost count that is not negative, which is always: the library has no form of the
        set left that can fail after it was created (``ibh_bcset_info`` is host code and reads nothing back)."""
        ng, nl = C.c_int32(0), C.c_int32(0)
        call("ibh_bcset_info", self.handle, C.byref(ng), C.byref(nl))
        return ng.value >= 0

    def apply(self, u):
        """The boundary conditions on the device field ``u`` (in place)."""
        from .hiparray import HipArray
        if isinstance(u, HipArray):
            u._flush_readers()
            u = u.t
        f, nv, _ = _field_inplace(u, what="BCSet field")
        if nv != 1:
            raise ValueError("BCSet applies to a scalar field")
        _stream()
        call("ibh_bcset_apply", self.handle, _ptr(f))
        return u


def owned_device_memory():
    """``(bytes, buffers)`` of device memory that the live library handles own -- partitions, accumulators, boundaries,
    BC sets and domain plans with the workspaces they allocate on first use (``ibh_owned_device_memory``).  Exact: a failed
    create leaves it unchanged, a destroy takes the handle's share off."""
    nb, nbuf = C.c_int64(0), C.c_int64(0)
    call("ibh_owned_device_memory", C.byref(nb), C.byref(nbuf))
    return int(nb.value), int(nbuf.value)


def timestep_advection(part, C_, scale=1.0, out=None):
    """``scale * 0.5 / maximum(max.(unsigned_green_gauss(part, at_faces(part, C[:, d], d), d) ...))`` (test/advection.jl:
    52-59, :65) as a one-element device tensor: the step loop never reads it back."""
    part = _part(part)
    C_, nvc, ldc = _field(C_, part.nc)
    if nvc != part.nd:
        raise ValueError("C must be (nc, nd)")
    dt = out if out is not None else torch.empty(1, dtype=torch.float32, device=C_.device)
    _stream()
    call("ibh_timestep_advection", part.handle, _ptr(C_), ldc, C.c_float(scale), _ptr(dt))
    return dt


def step_advection(part, u, C_, dt, bcs=None, out=None, next_dt=None, scale=1.0):
    """One ``march!`` of test/advection.jl:61-89 without the host: ``out = u + dt * R(u)`` (sweep and update in one launch
    where the quad sweep applies), then the boundary conditions ``bcs`` (a ``BCSet``) on ``out``.  ``dt``: one-element
    device tensor (``timestep_advection``).  ``u`` and ``out`` must be different arrays (ping-pong).
    ``next_dt`` (a one-element device tensor, may be ``dt`` itself): ``timestep_advection(part, C, scale)`` for the NEXT step
    is evaluated on the way -- it depends on ``C`` alone --, by extra workgroups of the BC set's own launches
    (``ibh_step_advection_dt``) instead of two launches in front of the next sweep; same value."""
    part = _part(part)
    u, nv, _ = _field(u, part.nc)
    if nv != 1:
        raise ValueError("u must be a scalar field")
    C_, nvc, ldc = _field(C_, part.nc)
    if nvc != part.nd:
        raise ValueError("C must be (nc, nd)")
    if out is None:
        out = torch.empty(part.nc, dtype=torch.float32, device=u.device)
    o, nvo, _ = _field_inplace(out, part.nc, "out")
    if nvo != 1 or o.data_ptr() == u.data_ptr():
        raise ValueError("out must be a scalar field other than u")
    _stream()
    if next_dt is not None:
        call("ibh_step_advection_dt", part.handle, _ptr(u), _ptr(o), _ptr(C_), ldc, _ptr(dt),
             bcs.handle if bcs is not None else c_vp(None), C.c_float(scale), _ptr(next_dt))
        return out
    call("ibh_step_advection", part.handle, _ptr(u), _ptr(o), _ptr(C_), ldc, _ptr(dt),
         bcs.handle if bcs is not None else c_vp(None))
    return out


@_hipaware
def residual_euler_hll(part, P, fluid_R=283.0, fluid_gamma=1.4, out=None, flags=0, fluid=None):
    """Fused Euler residual R2: JST(p) + cell_gradient + MUSCL(high_order) + HLL + green_gauss."""
    part = _part(part)
    if fluid is not None:
        fluid_R, fluid_gamma = fluid.R, fluid.gamma
    P, nv, ldp = _field(P, part.nc)
    if nv != part.nd + 2:
        raise ValueError("P must be (nc, nd+2) = [p T u v (w)]")
    R = out if out is not None else torch.zeros((nv, part.nc), dtype=torch.float32, device=P.device).T
    R, nvr, ldr = _field_inplace(R, part.nc, "out")
    if nvr != nv:
        raise ValueError(f"out must be (nc, {nv})")
    fl = _lib.ibh_fluid(float(fluid_R), float(fluid_gamma), 0.0, 1.0, 0.0, 0)
    _stream()
    call("ibh_residual_euler_hll", part.handle, _ptr(P), ldp, _ptr(R), ldr, C.byref(fl), flags)
    return R


@_hipaware
def residual_euler_sensor(part, P, nu=None, out=None, flags=0, fluid=None):
    """Fused Euler residual with the sensor-scaled central + Rusanov flux (cfd.jl:516-554): JST(p) + cell_gradient +
    MUSCL(high_order) + ``inviscid_fluxes(fluid, PL, PR, at_owners(nu), at_neighbors(nu), dim)`` + green_gauss.  ``nu``:
    ``(nc,)`` Float32 device array, or None for the pressure sensor ``JST_sensor(part, P[:, 0])`` (one kernel per sweep
    where ``residual_euler_hll`` has one; a given ``nu`` takes the face-list form)."""
    part = _part(part)
    P, nv, ldp = _field(P, part.nc)
    if nv != part.nd + 2:
        raise ValueError("P must be (nc, nd+2) = [p T u v (w)]")
    if nu is not None:
        if isinstance(nu, torch.Tensor) and nu.ndim != 1:
            raise ValueError("nu must be (nc,)")
        nu, _, _ = _field(nu, part.nc)
    R = out if out is not None else torch.zeros((nv, part.nc), dtype=torch.float32, device=P.device).T
    R, nvr, ldr = _field_inplace(R, part.nc, "out")
    if nvr != nv:
        raise ValueError(f"out must be (nc, {nv})")
    fluid_R, fluid_gamma = (fluid.R, fluid.gamma) if fluid is not None else (283.0, 1.4)
    fl = _lib.ibh_fluid(float(fluid_R), float(fluid_gamma), 0.0, 1.0, 0.0, 0)
    _stream()
    call("ibh_residual_euler_sensor", part.handle, _ptr(P), ldp, _ptr(nu) if nu is not None else c_vp(None), _ptr(R), ldr,
         C.byref(fl), flags)
    return R


# ---------------------------------------------------------------------------
# an explicit Euler step, device resident (rows of P: [p T u v (w)])
# ---------------------------------------------------------------------------
IBH_EULER_HLL, IBH_EULER_SENSOR = _K["IBH_EULER_HLL"], _K["IBH_EULER_SENSOR"]
_EULER_SCHEMES = {"hll": IBH_EULER_HLL, "sensor": IBH_EULER_SENSOR}


def _cfluid(fluid):
    """``ibh_fluid`` of a ``cfd.Fluid`` (None: air, the defaults of cfd.jl:14-53)."""
    if fluid is None:
        from .cfd import Fluid
        fluid = Fluid()
    return fluid._c()


def _primitives(P, n, nd=None):
    P, nv, ldp = _field(P, n)
    if (nd is not None and nv != nd + 2) or nv not in (4, 5):
        raise ValueError("P must be (n, nd+2) = [p T u v (w)]")
    return P, nv, ldp


def _device_dt(dt, n, what):
    """(tensor, per_cell) of a time step: a one-element Float32 device tensor, or ``(n,)`` for a per-cell time step."""
    if not isinstance(dt, torch.Tensor) or not dt.is_cuda or dt.dtype != torch.float32:
        raise TypeError(f"{what}: dt must be a Float32 device tensor (timestep_euler gives one): the step never reads it back")
    if dt.numel() == 1:
        return dt.reshape(1), 0
    if dt.ndim == 1 and dt.shape[0] == n and dt.stride(0) == 1:
        return dt, 1
    raise ValueError(f"{what}: dt has shape {tuple(dt.shape)}; expected one element or ({n},) for a per-cell time step")


@_hipaware
def timestep_euler(part, P, fluid=None, scale=1.0, out=None, cells=None):
    """The CFL time step of an explicit Euler step, ``scale * 0.5 / maximum(max.(unsigned_green_gauss(part, at_faces(part,
    C_d, d), d) ...))`` with ``C_d = abs.(u_d) .+ speed_of_sound(fluid, T)`` (test/advection.jl:52-59, :65), evaluated from
    ``P`` on the fly: bit for bit ``timestep_advection`` on the materialised ``C``, without the array and without a host
    read-back.  Returns the one-element device tensor (``out`` if given).  ``cells``: an ``(nc,)`` device array that
    receives the local time step ``scale * 0.5 / max_d(...)[c]`` of every cell; with ``cells`` and ``out=False`` only that
    is computed (one launch) and ``cells`` is returned."""
    part = _part(part)
    P, _, ldp = _primitives(P, part.nc, part.nd)
    if cells is not None:
        cells, nvc, _ = _field_inplace(cells, part.nc, "cells")
        if nvc != 1 or cells.ndim != 1:
            raise ValueError("cells must be (nc,)")
    if out is False:
        if cells is None:
            raise ValueError("timestep_euler: out=False needs cells")
        dt = None
    else:
        dt = out if out is not None else torch.empty(1, dtype=torch.float32, device=P.device)
        if not isinstance(dt, torch.Tensor) or not dt.is_cuda or dt.dtype != torch.float32 or dt.numel() != 1:
            raise TypeError("out must be a one-element Float32 device tensor")
    f = _cfluid(fluid)
    _stream()
    call("ibh_timestep_euler", part.handle, C.byref(f), _ptr(P), ldp, C.c_float(scale), _ptr(dt), _ptr(cells))
    return dt if dt is not None else cells


def _update_args(what, states, dt, out, R=None, n=None, nd=None):
    """The arguments of an Euler update ``what``, checked: the primitive ``states`` in the order of the C call (the first one
    gives ``n`` and ``nd`` where the partition does not), the residual ``R`` (None for a step, which sweeps it itself), ``dt``
    (None where the call takes none: ``D`` is then empty) and ``out`` (None: a new array).  Returns
    ``(n, nv, S, R, D, O, out, keep)``: ``S``, ``R``, ``D``, ``O`` are the C arguments
    of the states (pointer, leading dimension, ...), of ``R``, of ``dt`` (pointer, per_cell) and of ``out``; ``keep`` holds
    the tensors they point into and stays with the caller until the call has returned."""
    rows, nv, S, keep = "n" if n is None else "nc", None, [], []
    for P in states:
        P, nv, ld = _primitives(P, n, nd if nv is None else nv - 2)
        n = P.shape[0]
        S += [_ptr(P), ld]
        keep.append(P)
    Ra = []
    if R is not None:
        R, nvr, ldr = _field(R, n)
        if nvr != nv:
            raise ValueError(f"R must be (n, {nv})")
        Ra = [_ptr(R), ldr]
        keep.append(R)
    D = []
    if dt is not None:   # (dual_source alone takes no time step)
        dt, per_cell = _device_dt(dt, n, what)
        D = [_ptr(dt), per_cell]
    if out is None:
        out = colmajor_empty(n, nv)
    o, nvo, ldo = _field_inplace(out, n, "out")
    if nvo != nv:
        raise ValueError(f"out must be ({rows}, {nv})")
    return n, nv, S, Ra, D, [_ptr(o), ldo], out, keep + [dt, o]


def _step_args(what, part, states, dt, out, work, scheme):
    """The arguments of a sweep plus update ``what`` on a partition: ``_update_args`` of the states at the partition's size,
    then ``work`` (None, or ``(nc, nd+2)``) and the scheme's number.  Returns ``(part, sch, S, D, O, W, out, keep)``."""
    part = _part(part)
    _, nv, S, _, D, O, out, keep = _update_args(what, states, dt, out, n=part.nc, nd=part.nd)
    w, ldw = None, 0
    if work is not None:
        w, nvw, ldw = _field_inplace(work, part.nc, "work")
        if nvw != nv:
            raise ValueError(f"work must be (nc, {nv})")
    if scheme not in _EULER_SCHEMES:
        raise ValueError('scheme must be "hll" or "sensor"')
    return part, _EULER_SCHEMES[scheme], S, D, O, [_ptr(w), ldw], out, keep + [w]


@_hipaware
def update_euler(P, R, dt, fluid=None, out=None):
    """``state2primitive(fluid, primitive2state(fluid, P) .+ dt .* R)`` in one launch (bit for bit the three).  ``dt``: a
    one-element device tensor, or ``(n,)`` for a per-cell time step.  ``out`` may be ``P`` itself (in place)."""
    n, nv, S, Ra, D, O, out, keep = _update_args("update_euler", (P,), dt, out, R)
    f = _cfluid(fluid)
    _stream()
    call("ibh_update_euler", C.byref(f), nv - 2, n, *S, *Ra, *D, *O)
    return out


@_hipaware
def step_euler(part, P, dt, out, fluid=None, scheme="hll", work=None, flags=0):
    """One explicit Euler step ``out = update_euler(P, residual_euler_hll | residual_euler_sensor(part, P, flags), dt)``
    (``scheme``: "hll" or "sensor").  One launch where the 2-D single-kernel sweep takes the whole partition, ``dt`` is one
    element and ``out`` is not ``P``; elsewhere the sweep goes into ``work`` -- ``(nc, nd+2)``, required there: the step
    allocates nothing -- and the update follows (``out`` may be ``P`` then).  Same bits either way."""
    part, sch, S, D, O, W, out, keep = _step_args("step_euler", part, (P,), dt, out, work, scheme)
    f = _cfluid(fluid)
    _stream()
    call("ibh_step_euler", part.handle, C.byref(f), sch, *S, *O, *D, *W, int(flags))
    return out


@_hipaware
def update_euler_stage(P0, R, dt, alpha, fluid=None, out=None):
    """A Runge-Kutta stage of the low-storage family, ``state2primitive(fluid, primitive2state(fluid, P0) .+ (alpha .* dt)
    .* R)`` in one launch: bit for bit ``update_euler(P0, R, dt .* Float32(alpha))``.  ``dt``: a one-element device tensor,
    or ``(n,)`` for a per-cell time step.  ``out`` may be ``P0`` itself."""
    n, nv, S, Ra, D, O, out, keep = _update_args("update_euler_stage", (P0,), dt, out, R)
    f = _cfluid(fluid)
    _stream()
    call("ibh_update_euler_stage", C.byref(f), nv - 2, n, *S, *Ra, *D, C.c_float(alpha), *O)
    return out


@_hipaware
def stage_euler(part, P, P0, dt, alpha, out, fluid=None, scheme="hll", work=None, flags=0):
    """One stage of a multi-stage step, ``out = update_euler_stage(P0, residual_euler_hll | residual_euler_sensor(part, P,
    flags), dt, alpha)``: ``P`` is the previous stage, ``P0`` the state the step started from (they may be the same array).
    One launch where the 2-D single-kernel sweep takes the whole partition and ``out`` is not ``P`` -- with a one-element
    and with a per-cell ``dt``; elsewhere the sweep goes into ``work`` -- ``(nc, nd+2)``, required there: the stage
    allocates nothing -- and the update follows.  ``out`` may be ``P0`` when ``P0`` is not ``P``.  Same bits either way."""
    part, sch, S, D, O, W, out, keep = _step_args("stage_euler", part, (P, P0), dt, out, work, scheme)
    f = _cfluid(fluid)
    _stream()
    call("ibh_stage_euler", part.handle, C.byref(f), sch, *S, *O, *D, C.c_float(alpha), *W, int(flags))
    return out


@_hipaware
def update_euler_ssp(P0, P, R, dt, a, b, c, fluid=None, out=None):
    """A Shu-Osher stage of a strong-stability-preserving Runge-Kutta scheme, ``state2primitive(fluid, (primitive2state(fluid,
    P0) .* a .+ primitive2state(fluid, P) .* b) .+ R .* (dt .* c))`` in one launch, every product and sum rounded on its own:
    bit for bit that composition of launches.  ``dt``: a one-element device tensor, or ``(n,)`` for a per-cell time step.
    ``out`` may be ``P0`` or ``P``; ``P0`` may be ``P``."""
    n, nv, S, Ra, D, O, out, keep = _update_args("update_euler_ssp", (P0, P), dt, out, R)
    f = _cfluid(fluid)
    _stream()
    call("ibh_update_euler_ssp", C.byref(f), nv - 2, n, *S, *Ra, *D, C.c_float(a), C.c_float(b), C.c_float(c), *O)
    return out


@_hipaware
def stage_euler_ssp(part, P, P0, dt, a, b, c, out, fluid=None, scheme="hll", work=None, flags=0):
    """One Shu-Osher stage, ``out = update_euler_ssp(P0, P, residual_euler_hll | residual_euler_sensor(part, P, flags), dt, a, b,
    c)``: ``P`` is the previous stage -- swept, and blended with weight ``b`` -- and ``P0`` the state the step started from
    (weight ``a``).  One launch where the 2-D single-kernel sweep takes the whole partition and ``out`` is not ``P``, with a
    one-element and with a per-cell ``dt``; elsewhere the sweep goes into ``work`` -- ``(nc, nd+2)``, required there: the stage
    allocates nothing -- and the update follows.  ``out`` may be ``P0`` when ``P0`` is not ``P``.  Same bits either way."""
    part, sch, S, D, O, W, out, keep = _step_args("stage_euler_ssp", part, (P, P0), dt, out, work, scheme)
    f = _cfluid(fluid)
    _stream()
    call("ibh_stage_euler_ssp", part.handle, C.byref(f), sch, *S, *O, *D, C.c_float(a), C.c_float(b), C.c_float(c),
         *W, int(flags))
    return out


def _dual_g(what, g):
    """``g`` of a dual time step, checked: finite and >= 0."""
    g = float(g)
    if not (g >= 0.0 and g != float("inf")):
        raise ValueError(f"{what}: g must be finite and >= 0")
    return g


def _dual_S(what, S, n, nv, others):
    """The C arguments (pointer, leading dimension) of the source ``S`` of a dual time step, ``(n, nv)`` in conserved
    variables; it is none of the arrays ``others`` that the call writes."""
    S, nvs, lds = _field(S, n)
    if nvs != nv:
        raise ValueError(f"{what}: S must be ({n}, {nv})")
    for name, t in others:
        if t is not None and t.data_ptr() == S.data_ptr():
            raise ValueError(f"{what}: S may not be {name}")
    return S, [_ptr(S), lds]


@_hipaware
def dual_source(Pn, Pm, cn, cm, fluid=None, out=None):
    """The source of a physical step of a dual time march, ``primitive2state(fluid, Pn) .* cn .+ primitive2state(fluid, Pm)
    .* cm`` in one launch -- the part of the backward difference that the inner iterations leave alone -- or, with
    ``Pm=None`` (BDF1, the first step), ``primitive2state(fluid, Pn) .* cn``: bit for bit those launches.  ``cn``, ``cm``:
    ``solver.bdf_coefficients``.  Returns ``out`` (None: a new array), conserved variables ``(n, nd+2)``."""
    states = (Pn,) if Pm is None else (Pn, Pm)
    n, nv, S, _, _, O, out, keep = _update_args("dual_source", states, None, out)
    if Pm is None:
        S += [c_vp(None), 0]
    if any(out.data_ptr() == P.data_ptr() for P in keep[:len(states)]):
        raise ValueError("dual_source: out may not be Pn or Pm")
    f = _cfluid(fluid)
    _stream()
    call("ibh_dual_source", C.byref(f), nv - 2, n, *S, C.c_float(cn), C.c_float(cm), *O)
    return out


@_hipaware
def update_euler_dual(P0, R, S, dt, alpha, g, fluid=None, out=None):
    """A pseudo-time stage of a dual time step, ``state2primitive(fluid, (primitive2state(fluid, P0) .+ (R .+ S) .* h) ./ (h
    .* g .+ 1))`` with ``h = dt .* alpha`` in one launch, every sum, product and the divide rounded on its own: bit for bit
    that composition of launches.  ``S``: ``dual_source``; ``g``: the coefficient of the new state in the backward
    difference, taken point-implicitly (``g = 0`` with ``S`` zeros: ``update_euler_stage``).  ``dt``: a one-element device
    tensor, or ``(n,)`` for a per-cell time step.  ``out`` may be ``P0`` itself."""
    g = _dual_g("update_euler_dual", g)
    n, nv, Sa, Ra, D, O, out, keep = _update_args("update_euler_dual", (P0,), dt, out, R)
    S, Sc = _dual_S("update_euler_dual", S, n, nv, (("out", out),))
    f = _cfluid(fluid)
    _stream()
    call("ibh_update_euler_dual", C.byref(f), nv - 2, n, *Sa, *Ra, *Sc, *D, C.c_float(alpha), C.c_float(g), *O)
    return out


@_hipaware
def stage_euler_dual(part, P, P0, S, dt, alpha, g, out, fluid=None, scheme="hll", work=None, flags=0):
    """One pseudo-time stage of a dual time step, ``out = update_euler_dual(P0, residual_euler_hll | residual_euler_sensor(
    part, P, flags), S, dt, alpha, g)``: ``P`` is the previous stage, ``P0`` the state the pseudo-step started from, ``S``
    the source of the physical step.  ``stage_euler``'s dispatch: one launch where the 2-D single-kernel sweep takes the whole
    partition and ``out`` is not ``P``, with a one-element and with a per-cell ``dt``; elsewhere the sweep goes into ``work``
    -- ``(nc, nd+2)``, required there: the stage allocates nothing -- and the update follows.  ``out`` may be ``P0`` when
    ``P0`` is not ``P``; ``S`` is neither ``out`` nor ``work``.  Same bits either way."""
    g = _dual_g("stage_euler_dual", g)
    part, sch, Sa, D, O, W, out, keep = _step_args("stage_euler_dual", part, (P, P0), dt, out, work, scheme)
    S, Sc = _dual_S("stage_euler_dual", S, part.nc, part.nd + 2, (("out", out), ("work", work)))
    f = _cfluid(fluid)
    _stream()
    call("ibh_stage_euler_dual", part.handle, C.byref(f), sch, *Sa, *Sc, *O, *D, C.c_float(alpha), C.c_float(g), *W,
         int(flags))
    return out


def _transfer(what, acc):
    """The device Accumulator of a multigrid transfer ``what`` (``to_backend`` of one of the lists ``multigrid(dom)``
    returns)."""
    acc = to_backend(acc)
    if not isinstance(acc, DeviceAccumulator):
        raise TypeError(f"{what}: the operator must be an Accumulator (one of the lists multigrid(dom) returns)")
    return acc


def _coarse_out(what, name, t, n, nv):
    """``t`` (None: a new array) as an output ``(n, nv)`` of a transfer, with its C arguments."""
    if t is None:
        t = colmajor_empty(n, nv)
    o, nvo, ld = _field_inplace(t, n, name)
    if nvo != nv:
        raise ValueError(f"{what}: {name} must be ({n}, {nv})")
    return t, [_ptr(o), ld]


class Roles:
    """The cell roles of one partition on the device (``domain.cell_roles``: fluid, ghost, solid) and what blanks its solid
    rows: ``roles``, the ``uint8`` array ``(nc,)``; ``solid``, the ``int32`` list of the solid rows; ``solid_rows``, a
    compact ``(n_solid, nd+2)`` array whose every row is ``solid_state`` -- ``blank(P)`` scatters it into the solid rows of
    ``P`` (``ibh_scatter_rows``: one launch, none without solid rows).

    ``part``: the partition, host or device; ``roles``: ``cell_roles(dom)[part.domain]``, ``nc`` values of ``ROLE_*``;
    ``solid_state``: the ``nd + 2`` primitives the solid rows are held at, e.g. the free stream.  A wrong length of either
    raises ``ValueError`` before anything is asked of the device."""

    def __init__(self, part, roles, solid_state):
        nd = int(part.ndims)
        nc = int(part.nc) if hasattr(part, "nc") else int(part.spacing.shape[0])
        r = np.asarray(roles)
        if r.ndim != 1 or r.shape[0] != nc:
            raise ValueError(f"Roles: roles must be one value per cell of the partition, ({nc},); got {tuple(r.shape)}")
        if r.size and not np.isin(r, (ROLE_FLUID, ROLE_GHOST, ROLE_SOLID)).all():
            raise ValueError("Roles: roles are ROLE_FLUID (0), ROLE_GHOST (1) or ROLE_SOLID (2)")
        st = np.asarray(solid_state, dtype=np.float32)
        if st.ndim != 1 or st.shape[0] != nd + 2:
            raise ValueError(f"Roles: solid_state must be the nd + 2 = {nd + 2} primitives of a row; got shape {tuple(st.shape)}")
        r = np.ascontiguousarray(r, dtype=np.uint8)
        solid = np.nonzero(r == ROLE_SOLID)[0].astype(np.int32)
        dev = _dev()
        self.nc, self.nd, self.n_solid = nc, nd, int(solid.size)
        self.counts = tuple(int(x) for x in np.bincount(r, minlength=3))     # (fluid, ghost, solid)
        self.roles = torch.from_numpy(r).to(dev)
        self.solid = torch.from_numpy(solid).to(dev)
        self.solid_rows = hip(np.tile(st, (max(self.n_solid, 1), 1)))[:self.n_solid]

    def blank(self, P):
        """``solid_state`` into the solid rows of ``P`` (column-major ``(nc, nd+2)``), in place; returns ``P``."""
        if self.n_solid:
            f, nv, ld = _field_inplace(P, self.nc, "P")
            if nv != self.nd + 2:
                raise ValueError(f"Roles.blank: P must be ({self.nc}, {self.nd + 2})")
            _stream()
            call("ibh_scatter_rows", _ptr(self.solid), self.n_solid, _ptr(self.solid_rows), nv, self.n_solid, _ptr(f), ld)
        return P


def _roles(what, roles, n):
    """The device ``uint8`` array of ``n`` role bytes from a ``Roles`` or such a tensor."""
    r = roles.roles if isinstance(roles, Roles) else roles
    if not isinstance(r, torch.Tensor) or not r.is_cuda or r.dtype != torch.uint8 or r.ndim != 1 or not r.is_contiguous():
        raise TypeError(f"{what}: roles must be a Roles or a contiguous uint8 device tensor")
    if r.shape[0] != n:
        raise ValueError(f"{what}: roles has {r.shape[0]} entries, expected {n}")
    return r


@_hipaware
def restrict_euler(coarsener, P, R, S=None, fluid=None, out=None, out_D=None, roles=None):
    """The restriction of a multigrid cycle of the Euler march in conserved variables, one launch:
    ``P_c = state2primitive(fluid, coarsener(primitive2state(fluid, P)))`` and ``D_c = coarsener(R .+ S)`` (``S=None``:
    ``coarsener(R)``), bit for bit those launches.  ``P``: the fine primitives ``(n_input, nd+2)``; ``R``, ``S``: the fine
    residual and forcing in conserved variables.  Returns ``(P_c, D_c)`` -- ``out`` and ``out_D`` where given, ``(n_output,
    nd+2)``, which alias neither each other nor an input.  The coarse forcing of the cycle is ``D_c .- R_c(P_c)``.

    ``roles`` (a ``Roles`` of the fine partition or its ``uint8`` device array): ``D_c = coarsener(t)`` with ``t = R .+ S`` in
    fluid rows and ``+0`` in every other one (``ibh_restrict_euler_roles``, a select: a NaN in a masked row never reaches
    ``D_c``); ``P_c`` is unchanged."""
    acc = _transfer("restrict_euler", coarsener)
    P, nv, ldp = _primitives(P, acc.n_input)
    R, nvr, ldr = _field(R, acc.n_input)
    if nvr != nv:
        raise ValueError(f"restrict_euler: R must be ({acc.n_input}, {nv})")
    Sc = [c_vp(None), 0]
    if S is not None:
        S, nvs, lds = _field(S, acc.n_input)
        if nvs != nv:
            raise ValueError(f"restrict_euler: S must be ({acc.n_input}, {nv})")
        Sc = [_ptr(S), lds]
    out, O = _coarse_out("restrict_euler", "out", out, acc.n_output, nv)
    out_D, D = _coarse_out("restrict_euler", "out_D", out_D, acc.n_output, nv)
    if roles is not None:
        roles = _roles("restrict_euler", roles, acc.n_input)
    if acc.n_output == 0:     # (no rows: nothing to launch, and an empty array has no address to pass)
        return out, out_D
    f = _cfluid(fluid)
    _stream()
    if roles is not None:
        call("ibh_restrict_euler_roles", acc.handle, C.byref(f), nv - 2, _ptr(P), ldp, _ptr(R), ldr, *Sc, _ptr(roles), *O, *D)
    else:
        call("ibh_restrict_euler", acc.handle, C.byref(f), nv - 2, _ptr(P), ldp, _ptr(R), ldr, *Sc, *O, *D)
    return out, out_D


@_hipaware
def forcing_roles(D, R, roles):
    """The coarse forcing of a multigrid cycle with cell roles, in place and in one launch: ``D = D .- R`` in fluid rows and
    ``+0`` in every other one (``ibh_forcing_roles``), bit for bit the broadcast and the select.  ``D`` (column-major, written)
    and ``R``: ``(n, nv)``, ``nv <= 8``; ``roles``: a ``Roles`` or its ``uint8`` device array.  Returns ``D``."""
    Df, nv, ldd = _field_inplace(D, None, "D")
    n = Df.shape[0]
    Rf, nvr, ldr = _field(R, n)
    if nvr != nv:
        raise ValueError(f"forcing_roles: R must be ({n}, {nv})")
    if nv > 8:
        raise ValueError("forcing_roles: D has more than 8 columns")
    roles = _roles("forcing_roles", roles, n)
    if n == 0:
        return D
    _stream()
    call("ibh_forcing_roles", n, nv, _ptr(Df), ldd, _ptr(Rf), ldr, _ptr(roles))
    return D


@_hipaware
def sumsq_roles(x, roles, out=None):
    """Per column of ``x`` (``(n,)`` or ``(n, nv)``, ``nv <= 8``) the sum of squares over the fluid rows, accumulated in double
    on the device (``ibh_sumsq_roles``: one launch for all columns and the one-launch final stage).  Returns ``out``: ``nv``
    device doubles, assigned (None: a new tensor).  No read-back."""
    xf, nv, ldx = _field(x)
    n = xf.shape[0]
    if nv > 8:
        raise ValueError("sumsq_roles: x has more than 8 columns")
    roles = _roles("sumsq_roles", roles, n)
    if out is None:
        out = torch.zeros(nv, dtype=torch.float64, device=xf.device)
    elif not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != torch.float64 or out.ndim != 1 \
            or out.shape[0] != nv or not out.is_contiguous():
        raise ValueError(f"sumsq_roles: out must be a contiguous Float64 device tensor of {nv} elements")
    if n == 0:
        out.zero_()
        return out
    _stream()
    call("ibh_sumsq_roles", n, nv, _ptr(xf), ldx, _ptr(roles), _ptr(out))
    return out


@_hipaware
def prolong_euler(prolongator, P, Pc_new, Pc_old, fluid=None, out=None, pack=None):
    """The prolongation of a multigrid cycle of the Euler march, the correction of the fine state by the change of the coarse
    one in conserved variables: ``state2primitive(fluid, primitive2state(fluid, P) .+ prolongator(primitive2state(fluid,
    Pc_new) .- primitive2state(fluid, Pc_old)))`` in two launches -- the difference of the coarse states packed once, 8 floats
    per coarse row, then one thread per fine row -- bit for bit ``primitive2state`` three times, ``prolongator.diff_add`` and
    ``state2primitive``.  ``out`` (None: a new array) may be ``P`` itself.  ``pack``: ``8 * n_input`` Float32 on the device,
    32-byte aligned; None: an array kept with the operator, allocated on its first use (a caller that captures graphs passes
    its own)."""
    acc = _transfer("prolong_euler", prolongator)
    P, nv, ldp = _primitives(P, acc.n_output)
    Pn, _, ldn = _primitives(Pc_new, acc.n_input, nv - 2)
    Po, _, ldo_ = _primitives(Pc_old, acc.n_input, nv - 2)
    if ldn != ldo_:
        raise ValueError("prolong_euler: Pc_new and Pc_old must have one leading dimension")
    out, O = _coarse_out("prolong_euler", "out", out, acc.n_output, nv)
    if pack is None:
        pack = getattr(acc, "_pack", None)
        if pack is None:
            pack = acc._pack = torch.empty(8 * max(acc.n_input, 1), dtype=torch.float32, device=P.device)
    if not isinstance(pack, torch.Tensor) or not pack.is_cuda or pack.dtype != torch.float32 or not pack.is_contiguous() \
            or pack.numel() < 8 * acc.n_input:
        raise ValueError(f"prolong_euler: pack must be a contiguous Float32 device tensor of at least {8 * acc.n_input} "
                         "elements")
    if acc.n_output == 0:
        return out
    f = _cfluid(fluid)
    _stream()
    call("ibh_prolong_euler", acc.handle, C.byref(f), nv - 2, _ptr(Pn), _ptr(Po), ldn, _ptr(pack), _ptr(P), ldp, *O)
    return out


def _smoothing(what, eps, n_iter):
    """``(eps, n_iter)`` of a residual smoothing, checked: ``eps`` finite and >= 0, ``n_iter`` an integer >= 1."""
    eps = float(eps)
    if not (eps >= 0.0 and eps != float("inf")):
        raise ValueError(f"{what}: eps must be finite and >= 0")
    if isinstance(n_iter, bool) or int(n_iter) != n_iter or int(n_iter) < 1:
        raise ValueError(f"{what}: n_iter must be an integer >= 1")
    return eps, int(n_iter)


@_hipaware
def smooth_residual(part, R, eps, n_iter, out=None, tmp=None):
    """Implicit residual smoothing (not in the reference): ``n_iter`` Jacobi iterations on ``(I + eps L) S = R``, ``L`` the
    unweighted Laplacian of the partition's face graph,
    ``S_i <- (R_i + eps * sum(S[across(f, i)] for f in faces(i))) / (1 + eps * n_i)`` from ``S = R``, per column of ``R``
    (``(nc,)`` or ``(nc, nv)``, ``nv <= 8``), one launch per iteration.  Returns ``out`` (None: a new array).  ``tmp``, the
    ping-pong partner from ``n_iter = 2``, is allocated when it is not given; ``out`` and ``tmp`` alias neither each other nor
    ``R``."""
    part = _part(part)
    eps, n_iter = _smoothing("smooth_residual", eps, n_iter)
    R, nv, ldr = _field(R, part.nc)
    if nv > 8:
        raise ValueError("smooth_residual: R has more than 8 columns")
    if out is None:
        out = _like(R, part.nc)
    o, nvo, ldo = _field_inplace(out, part.nc, "out")
    if nvo != nv or o.ndim != R.ndim:
        raise ValueError(f"out must have the shape of R, {tuple(R.shape)}")
    t, ldt = None, 0
    if n_iter >= 2:
        if tmp is None:
            tmp = _like(R, part.nc)
        t, nvt, ldt = _field_inplace(tmp, part.nc, "tmp")
        if nvt != nv:
            raise ValueError(f"tmp must have the shape of R, {tuple(R.shape)}")
    _stream()
    call("ibh_smooth_residual", part.handle, _ptr(R), nv, ldr, C.c_float(eps), n_iter, _ptr(o), ldo, _ptr(t), ldt)
    return out


@_hipaware
def update_euler_smoothed(part, P0, P, R, Sprev, eps, dt, coef, fluid=None, out=None):
    """The last Jacobi iteration of a residual smoothing inside the update, in one launch: with ``S`` one iteration of
    ``smooth_residual`` from ``Sprev`` (``Sprev`` may be ``R``: the only iteration), ``coef = (c,)`` gives
    ``update_euler_stage(P0, S, dt, c)`` (``P`` is ignored and may be None) and ``coef = (a, b, c)`` gives
    ``update_euler_ssp(P0, P, S, dt, a, b, c)``, bit for bit, without ``S`` being written.  ``out`` may be ``P0`` or ``P``,
    not ``R`` or ``Sprev``."""
    part = _part(part)
    eps, _ = _smoothing("update_euler_smoothed", eps, 1)
    coef = tuple(float(x) for x in coef)
    if len(coef) not in (1, 3):
        raise ValueError("update_euler_smoothed: coef must be (c,) or (a, b, c)")
    blend = len(coef) == 3
    a, b, c = coef if blend else (0.0, 1.0, coef[0])
    states = (P0, P) if blend else (P0,)
    _, nv, S, Ra, D, O, out, keep = _update_args("update_euler_smoothed", states, dt, out, R, n=part.nc, nd=part.nd)
    if not blend:
        S += [c_vp(None), 0]
    Sp, nvs, lds = _field(Sprev, part.nc)
    if nvs != nv:
        raise ValueError(f"Sprev must be (nc, {nv})")
    f = _cfluid(fluid)
    _stream()
    call("ibh_update_euler_smoothed", part.handle, C.byref(f), int(blend), *S, *Ra, _ptr(Sp), lds, C.c_float(eps), *D,
         C.c_float(a), C.c_float(b), C.c_float(c), *O)
    return out


# ---------------------------------------------------------------------------
# partition runtime and ghost-cell BC
# ---------------------------------------------------------------------------
def domain_call(dom, f, args, conv_to_backend, conv_from_backend, kwargs):
    """``(dom::Domain)(f, args...)`` (ImmersedBoundary.jl:820-864) with the GPU backend.

    With both converters: per partition, the host gathers ``a[part.domain]``, converts it, runs ``f`` and writes the
    image rows back (the reference's loop, sequential).  Without converters and with every argument a device array
    (CUDA/HIP ``torch.Tensor`` or ``HipArray``, at least one): ``_domain_call_device``.  Anything else raises."""
    if (conv_to_backend is None) != (conv_from_backend is None):
        raise AssertionError("Backend converters must be provided at the same time")
    if conv_to_backend is None:
        if args and all(_on_device(a) for a in args):
            return _domain_call_device(dom, f, args, kwargs)
        raise TypeError("Domain call needs conv_to_backend=ibamd.hip, conv_from_backend=ibamd.to_host, or device arrays "
                        "only (no host array among them): the per-partition compute runs on the GPU only (no CPU path)")
    results = []
    for i in dom.partitions:
        part = dom.partitions[i]
        dargs = [np.array(a[part.domain]) for a in args]
        dargs = [conv_to_backend(a) for a in dargs]
        dpart = to_backend(part, conv_to_backend)
        r = f(dpart, *dargs, **kwargs)
        dargs = [conv_from_backend(a) for a in dargs]
        for a, da in zip(args, dargs):
            a[part.image] = da[part.image_in_domain]
        results.append(r)
    return results


def _on_device(a):
    from .hiparray import HipArray
    return isinstance(a, HipArray) or (isinstance(a, torch.Tensor) and a.is_cuda)


class DomainPlan(_Handle):
    """Device tables of the domain call of one Domain (``ibh_domain_plan_create``; ``domain_plan_tables`` is the same
    construction in numpy) plus the partitions' ``to_backend`` handles, in call order.  Cached on the Domain."""
    _destroy = "ibh_domain_plan_destroy"

    def __init__(self, dom):
        from .domain import domain_plan_tables
        T = domain_plan_tables(dom)   # validates: indices in range, images disjoint
        _dev()
        self.ids = T["ids"]
        self.n = [int(x) for x in T["n"]]
        self.ws_off = [int(x) for x in T["ws_off"]]
        self.parts = [to_backend(dom.partitions[i], hip) for i in self.ids]
        np_ = len(self.ids)
        keep = []

        def ptrs(arrs):
            arrs = [np.ascontiguousarray(a, dtype=np.int32) for a in arrs]
            keep.append(arrs)
            return (c_vp * max(np_, 1))(*[a.ctypes.data for a in arrs])
        parts = [dom.partitions[i] for i in self.ids]
        nd = np.array([p.domain.size for p in parts], dtype=np.int32)
        ni = np.array([p.image.size for p in parts], dtype=np.int32)
        h = c_vp()
        call("ibh_domain_plan_create", C.byref(h), np_, ptrs([p.domain for p in parts]), _hptr(nd),
             ptrs([p.image for p in parts]), ptrs([p.image_in_domain for p in parts]), _hptr(ni), len(dom), 0)
        self.handle = h
        off = (C.c_int64 * (np_ + 1))()
        call("ibh_domain_plan_info", h, off, np_ + 1)
        if list(off) != self.ws_off:
            raise _lib.IbhError(f"domain plan: workspace offsets of the library {list(off)} != {self.ws_off}")

    def _run(self, name, a, nvs, lds, b):
        k = len(a)
        call(name, self.handle, k, (c_vp * k)(*a), _hptr(np.asarray(nvs, dtype=np.int32)),
             _hptr(np.asarray(lds, dtype=np.int64)), (c_vp * k)(*b))


def domain_plan(dom):
    """The Domain's ``DomainPlan`` (built on first use)."""
    plan = getattr(dom, "_device_plan", None)
    if plan is None:
        plan = dom._device_plan = DomainPlan(dom)
    return plan


def _domain_call_device(dom, f, args, kwargs):
    """``(dom::Domain)(f, args...)`` on device-resident global arrays: nothing goes through the host.

    1. one ``ibh_domain_gather`` launch copies ``a[part.domain]`` of every argument and every partition into stacked
       workspaces (torch's allocator: no host sync, capturable in a graph);
    2. ``f(device_partition, local_args...; kwargs...)`` runs per partition, in ``dom.partitions`` order; each local
       argument is a view ``(n_p,)`` / ``(n_p, nv)``, column-major with ``ld = n_p`` (the layout ``hip()`` gives), of
       the kind given (torch tensor or ``HipArray``);
    3. one ``ibh_domain_scatter`` launch writes ``a[part.image] = local[part.image_in_domain]`` for every argument.

    These are snapshot semantics: every partition reads the arguments as they were before the call -- the deterministic
    form of the reference's threaded ``tmap``.  For every closure whose result does not depend on the order of the
    partitions (one that reads its inputs and writes outputs, e.g. test/advection.jl:67-83) it equals the sequential
    host path bit for bit.  Returns the per-partition results in partition order."""
    from .hiparray import HipArray
    n = len(dom)
    for a in args:   # validate everything before anything is launched
        if isinstance(a, HipArray):
            if a.n != n:
                raise ValueError(f"domain call argument has {a.n} rows, the domain {n} cells")
        else:
            _field_inplace(a, n, "domain call argument")
            if a.ndim == 2 and a.shape[1] == 0:
                raise ValueError("domain call argument has no columns")
    for a in args:
        if isinstance(a, HipArray):
            a._flush_readers()   # pending broadcasts that read it see the old values
    tens = [a.t if isinstance(a, HipArray) else a for a in args]   # (materialises pending expressions)
    fields = [_field_inplace(t, n, "domain call argument") for t in tens]
    plan = domain_plan(dom)
    dev = tens[0].device
    wss = [torch.empty(nv * plan.ws_off[-1], dtype=torch.float32, device=dev) for (_, nv, _) in fields]
    nvs = [nv for (_, nv, _) in fields]
    lds = [ld for (_, _, ld) in fields]
    _stream()
    plan._run("ibh_domain_gather", [t.data_ptr() for t in tens], nvs, lds, [w.data_ptr() for w in wss])
    results = []
    for k, dpart in enumerate(plan.parts):
        n_p = plan.n[k]
        local = []
        for t, ws, nv, wrap in zip(tens, wss, nvs, (isinstance(a, HipArray) for a in args)):
            o = nv * plan.ws_off[k]
            v = ws[o:o + n_p] if t.ndim == 1 else torch.as_strided(ws, (n_p, nv), (1, n_p), o)
            local.append(HipArray(v) if wrap else v)
        results.append(f(dpart, *local, **kwargs))
    for a in args:
        if isinstance(a, HipArray):
            a._flush_readers()   # the arguments are written in place: pending broadcasts that read them go first
    _stream()
    plan._run("ibh_domain_scatter", [w.data_ptr() for w in wss], nvs, lds, [t.data_ptr() for t in tens])
    return results


def impose_bc(f, dom, bname, *args, conv_to_backend=None, conv_from_backend=None, **kwargs):
    """``impose_bc!(f, dom, bname, args...)`` (ImmersedBoundary.jl:1197-1247).

    ``args`` are global arrays.  Device arrays are updated in place on the GPU; host arrays need
    both converters (the reference's calling convention) and are copied back.
    """
    if (conv_to_backend is None) != (conv_from_backend is None):
        raise AssertionError("Backend converters must be provided at the same time")
    from .hiparray import HipArray

    def on_device(a):
        return isinstance(a, HipArray) or (isinstance(a, torch.Tensor) and a.is_cuda)
    host_args = None
    if not all(on_device(a) for a in args):
        if conv_to_backend is None:
            raise TypeError("impose_bc needs device arrays or conv_to_backend/conv_from_backend (no CPU path)")
        host_args = args
        args = tuple(a if on_device(a) else conv_to_backend(a) for a in args)   # (the converter may return HipArrays)
    wrapped = any(isinstance(a, HipArray) for a in args)
    for a in args:
        if isinstance(a, HipArray):
            a._flush_readers()   # the arrays are written in place: pending broadcasts that read them go first
    args = tuple(a.t if isinstance(a, HipArray) else a for a in args)
    fields = [_field_inplace(a, what="impose_bc argument") for a in args]  # updated in place (:1241-1245)
    for ipart in dom.boundaries[bname]:
        bdry = to_backend(dom.boundaries[bname][ipart])
        iargs = []
        _stream()
        for (a, nv, ld) in fields:
            ia = _like(a, bdry.ng)
            call("ibh_bc_interp", bdry.handle, _ptr(a), nv, ld, _ptr(ia), bdry.ng)
            iargs.append(ia)
        r = f(bdry, *([HipArray(ia) for ia in iargs] if wrapped else iargs), **kwargs)
        if not isinstance(r, tuple):
            r = (r,)
        r = tuple(x.t if isinstance(x, HipArray) else x for x in r)
        for (a, nv, ld), ba, ia in zip(fields, r, iargs):
            if isinstance(ba, torch.Tensor):
                ba, nvb, ldb = _field(ba.expand_as(ia) if ba.shape != ia.shape else ba, bdry.ng)
                call("ibh_bc_blend", bdry.handle, _ptr(a), nv, ld, _ptr(ia), bdry.ng, _ptr(ba), ldb, c_vp(None))
            else:
                const = np.full(nv, ba, dtype=np.float32) if np.isscalar(ba) else np.asarray(ba, dtype=np.float32)
                call("ibh_bc_blend", bdry.handle, _ptr(a), nv, ld, _ptr(ia), bdry.ng, c_vp(None), 0, _hptr(const))
    if host_args is not None:
        for h, (a, _, _) in zip(host_args, fields):
            if not on_device(h):
                h[...] = conv_from_backend(a)


_FLOW_BC_SCALAR_MODES = {s: _K["IBH_BC_SCALAR_" + s.upper()] for s in ("copy", "nut", "k", "omega", "epsilon")}
_WALL_PARAMS = ("kappa", "C_", "A", "beta", "betastar", "D", "Aplus", "omega_fixed_point")


def impose_flow_bc(dom, bname, bc, P, scalars=(), wall_function=None, transpiration=0.0):
    """``impose_bc!`` with a ``FlowBC`` closure in ONE launch per boundary partition (``ibh_bc_flow``): what

        impose_bc(lambda b, Pi, *si: (bc(Pi, b.normals, [du_dn=wf["du_dn"], image_distances=b.image_distances,]
                                         transpiration=transpiration), *values), dom, bname, P, *fields)

    computes, bit for bit, where with ``wall_function`` (``None``, or a dict of ``turbulence.wall_function``'s keywords, ``{}``
    for its defaults) ``wf = wall_function(b.image_distances, ut, nu)`` at the image points with ``ut`` the tangential speed
    and ``nu = dynamic_viscosity(T) / rho`` (turbulence.jl:72-98).

    ``bc`` is a ``cfd.FlowBC``; ``P`` the global ``(n, nd + 2)`` device array ``[p T u v (w)]``; ``scalars`` a sequence of up to
    four ``(field, spec)`` pairs, ``field`` a global device vector and ``spec`` its boundary value: a float, ``"copy"`` (the
    interpolated value), or -- with ``wall_function`` -- one of ``"nut"``, ``"k"``, ``"omega"``, ``"epsilon"``.  The arrays
    (``torch`` or ``HipArray``) are updated in place, boundary partitions in ``dom.boundaries[bname]`` order, each seeing the
    previous one's writes.  Every ghost cell is interpolated from the arrays as they were before any ghost cell of its
    partition is written: a boundary with ghost cells among its donors goes through a staging buffer and a second launch."""
    from .hiparray import HipArray
    from . import turbulence
    nd = dom.ndims
    if nd not in (2, 3):
        raise ValueError("impose_flow_bc: the domain must have 2 or 3 dimensions")
    n = len(dom)
    bparts = dom.boundaries[bname]
    scalars = [tuple(s) for s in scalars]
    if len(scalars) > 4:
        raise ValueError("impose_flow_bc: at most 4 scalar fields")
    if any(len(s) != 2 for s in scalars):
        raise ValueError("impose_flow_bc: scalars are (field, spec) pairs")
    wpar, n_iter = [0.0] * 8, 0
    if wall_function is not None:
        kw = dict(turbulence.wall_function.__kwdefaults__)
        unknown = set(wall_function) - set(kw)
        if unknown:
            raise ValueError(f"impose_flow_bc: wall_function has no keyword {sorted(unknown)}")
        kw.update(wall_function)
        wpar, n_iter = [float(kw[k]) for k in _WALL_PARAMS], int(kw["n_iter"])
        if n_iter < 0:
            raise ValueError("impose_flow_bc: n_iter must not be negative")
    modes, values = [], []
    for _, spec in scalars:
        if isinstance(spec, str):
            if spec not in _FLOW_BC_SCALAR_MODES:
                raise ValueError(f"impose_flow_bc: scalar spec {spec!r}: a float, 'copy', 'nut', 'k', 'omega' or 'epsilon'")
            if spec != "copy" and wall_function is None:
                raise ValueError(f"impose_flow_bc: scalar spec {spec!r} needs wall_function")
            modes.append(_FLOW_BC_SCALAR_MODES[spec])
            values.append(0.0)
        else:
            modes.append(_K["IBH_BC_SCALAR_CONST"])
            values.append(float(spec))
    if bc.normal_flow:
        if bc.u_inf.size != 1:
            raise ValueError("Only 3 parcels in P (p, T and normal flow) allowed for normal_flow = true BC")
    elif bc.u_inf.size != nd:
        raise ValueError("FlowBC needs one free-stream velocity component per dimension")
    arrays = [P] + [f for f, _ in scalars]
    tens = [a.t if isinstance(a, HipArray) else a for a in arrays]
    Pt, nvp, ldp = _field_inplace(tens[0], n, "impose_flow_bc: P")
    if tens[0].ndim != 2 or nvp != nd + 2:
        raise ValueError(f"impose_flow_bc: P must be (n, {nd + 2}) = [p T u v (w)]")
    fields = []
    for t in tens[1:]:
        f, nv, _ = _field_inplace(t, n, "impose_flow_bc: scalar field")
        if f.ndim != 1:
            raise ValueError("impose_flow_bc: scalar fields are vectors of n values")
        fields.append(f)
    for a in arrays:
        if isinstance(a, HipArray):
            a._flush_readers()   # the arrays are written in place: pending broadcasts that read them go first
    ns = len(fields)
    u_inf = [float(x) for x in bc.u_inf] + [0.0] * (3 - bc.u_inf.size)
    spec = _lib.ibh_flow_bc_spec(int(bc.normal_flow), bc.p_inf, bc.T_inf, (C.c_float * 3)(*u_inf), float(transpiration),
                                 int(wall_function is not None), (C.c_float * 8)(*wpar), n_iter)
    fluid = bc.fluid._c()
    ptrs = (c_vp * ns)(*[f.data_ptr() for f in fields]) if ns else None
    cmodes = (C.c_int32 * max(ns, 1))(*modes)
    cvalues = (C.c_float * max(ns, 1))(*values)
    for ipart in bparts:
        bdry = to_backend(bparts[ipart])
        _stream()
        direct = getattr(bdry, "flow_direct", None)
        if direct is None:
            d = C.c_int32()
            call("ibh_bc_flow_info", bdry.handle, C.byref(d))
            direct = bdry.flow_direct = bool(d.value)
        # (torch's allocator: in a graph capture the buffer comes from the graph's pool)
        staging = None if direct or bdry.ng == 0 else torch.empty(bdry.ng * (nd + 2 + ns), dtype=torch.float32,
                                                                  device=Pt.device)
        nrm, _, ldn = _field(bdry.normals, bdry.ng)
        call("ibh_bc_flow", bdry.handle, C.byref(fluid), nd, _ptr(nrm), ldn, _ptr(bdry.image_distances), _ptr(Pt), ldp,
             C.byref(spec), ns, ptrs, C.cast(cmodes, c_vp), C.cast(cvalues, c_vp), _ptr(staging))


class GraphedClosure:
    """A user closure at operator granularity captured ONCE in a HIP graph and replayed.

    The reference calls ``f(part, args...)`` once per partition and per iteration (ImmersedBoundary.jl:848-850); every
    operator and broadcast of such a closure is a kernel launch here, a few microseconds of GPU work behind tens of
    microseconds of host work each.  The launches of one call are fixed (same partition, same arrays), so they are
    recorded on a capture stream -- every libibhip launch goes to ``ibh_set_stream(current stream)``, temporaries come
    from the graph's private pool -- and ``g()`` replays them as one graph launch: the arrays are read and written in
    place, so new contents of the same arrays are what a replay sees.

    ``GraphedClosure(f, part, u, ud, C)`` runs ``f`` ``warmup`` times eagerly first (library workspaces are allocated on
    first use and nothing may be allocated during capture); the contents of the array arguments are saved before and
    restored after, so constructing it does not change them.  The closure must not read values back to the host
    (``.item()``, ``to_host``): that cannot be captured and raises.
    """

    def __init__(self, f, *args, warmup=2, **kwargs):
        from .hiparray import HipArray
        tens = [a.t if isinstance(a, HipArray) else a for a in args]
        tens = [t for t in tens if isinstance(t, torch.Tensor) and t.is_cuda]
        saved = [t.clone() for t in tens]
        self._keep = (f, args, kwargs)
        self.stream = torch.cuda.Stream()
        self.stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self.stream):
            for _ in range(max(1, int(warmup))):
                f(*args, **kwargs)
            for t, s in zip(tens, saved):
                t.copy_(s)
        self.stream.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=self.stream):
            self.result = f(*args, **kwargs)
            for a in args:                      # pending broadcasts of the arguments belong to the call
                if isinstance(a, HipArray):
                    a.t
            if isinstance(self.result, HipArray):
                self.result.t
        _stream()

    def __call__(self):
        self.graph.replay()
        return self.result

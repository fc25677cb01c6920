"""ctypes binding of libibhip.so, derived from the C ABI declared in include/ibhip.h (read by ``_header``): a new entry
point needs its declaration there and nothing here.

There is no CPU fallback: if the shared library is missing, or a call returns
an error code, an exception is raised.
"""
import ctypes as C
import os

from ._header import CONSTANTS, PROTOTYPES, STRUCTS, IbhError

_here = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("IBHIP_LIB") or os.path.join(_here, "libibhip.so")  # IBHIP_LIB: A/B builds

c_vp = C.c_void_p

# The named slots of ibh_partition_info in slot order: the IBH_INFO_* enumerators in lower case, as the header writes them
# (slot 12 is ``quads`` on a 2-D partition and ``rim4_rows``, its alias, on a 3-D one); INFO_COUNT entries are reported, the
# rest are zero.
INFO_SLOTS = tuple(k[len("IBH_INFO_"):].lower() for k in CONSTANTS
                   if k.startswith("IBH_INFO_") and k not in ("IBH_INFO_COUNT", "IBH_INFO_RIM4_ROWS"))
INFO_COUNT = CONSTANTS["IBH_INFO_COUNT"]
INFO_BOOLS = ("image_all_eligible", "row_sweep", "tiled")
INFO_2D_ONLY = ("quads", "quad_pairs", "quad_arith_half_sides")
INFO_KEYS = {"image_all_eligible": "image_blocks_all_eligible"}   # keys of DevicePartition.info that are not the slot's name


def info_dict(nd, values):
    """``DevicePartition.info``: the named slots of ``values`` (what ibh_partition_info reports) for a partition of ``nd``
    dimensions -- flags as bool, the 2-D slots zero in 3-D, and slot 12 under its 3-D name ``rim4_rows`` (zero in 2-D)."""
    out = {}
    for name, x in zip(INFO_SLOTS, values):
        x = bool(x) if name in INFO_BOOLS else int(x)
        out[INFO_KEYS.get(name, name)] = 0 if (nd != 2 and name in INFO_2D_ONLY) else x
    out["rim4_rows"] = int(values[INFO_SLOTS.index("quads")]) if nd == 3 else 0
    return out


_CTYPES = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64,
           "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double, "const char*": C.c_char_p}


def _ctype(ctext, where):
    """The ctypes type of a C type of the header: a row of ``_CTYPES``, or an address for any other pointer."""
    if ctext in _CTYPES:
        return _CTYPES[ctext]
    if not ctext.endswith("*"):
        raise IbhError(f"include/ibhip.h: {where}: no ctypes type is assigned to `{ctext}`")
    return c_vp


def _fields(struct):
    return [(name, _ctype(t, struct) * n if n else _ctype(t, struct)) for t, name, n in STRUCTS[struct]]


class ibh_fluid(C.Structure):
    _fields_ = _fields("ibh_fluid")


class ibh_flow_bc_spec(C.Structure):
    _fields_ = _fields("ibh_flow_bc_spec")


_CTYPES.update({"const ibh_fluid*": C.POINTER(ibh_fluid), "const ibh_flow_bc_spec*": C.POINTER(ibh_flow_bc_spec)})

# argument types and return type of every prototype of the header
_SIGS = {name: [_ctype(t, name) for t, _ in params] for name, (_, params) in PROTOTYPES.items()}
_RESTYPES = {name: _ctype(ret, name) for name, (ret, _) in PROTOTYPES.items()}
EXPORTS = sorted(PROTOTYPES)

_lib = None


def load():
    """Load libibhip.so (no GPU needed for loading); raises if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise IbhError(
            f"{LIB_PATH} not found: the HIP library is not built "
            "(run `python -c 'import __graft_entry__ as g; g.build()'` or `make -C immersedboundary.jl_amd/csrc`). "
            "There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, args in _SIGS.items():
        fn = getattr(lib, name, None)
        if fn is None:
            if os.environ.get("IBHIP_LIB"):   # A/B against an older build: entries it lacks fail when they are called
                continue
            raise IbhError(f"{LIB_PATH} does not export {name}: stale build")
        fn.argtypes = args
        fn.restype = _RESTYPES[name]
    _lib = lib
    return lib


def call(name, *args):
    lib = _lib if _lib is not None else load()
    rc = getattr(lib, name)(*args)
    if rc != 0:
        raise IbhError(f"{name} failed (code {rc}): {lib.ibh_last_error().decode()}")
    return rc

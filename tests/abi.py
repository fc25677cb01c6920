"""The check every "exported and bound with the header's prototypes" test makes for its entry points, stated once: the
library exports the name, ``_lib`` binds it, and ``_lib._SIGS`` has the header's argument list -- the same count, the exact
ctypes type of every scalar, an address (``c_void_p``) for every pointer but the strings and the two structs.  The header
is read here with a regex of its own, and the count is compared with tests/test_julia_binding.py's parser as well: neither
is the reader of the package."""
import ctypes as C
import os
import re

from ibamd import _lib
from test_julia_binding import header_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALAR = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64,
          "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double}
POINTER = {"const char": C.c_char_p, "const ibh_fluid": C.POINTER(_lib.ibh_fluid),
           "const ibh_flow_bc_spec": C.POINTER(_lib.ibh_flow_bc_spec)}


def header_text():
    """include/ibhip.h without its comments."""
    return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "ibhip.h")).read(), flags=re.S)


def assert_bound(names):
    lib, hdr, protos = _lib.load(), header_text(), header_prototypes()
    for name in names:
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _lib._SIGS and name in _lib.EXPORTS, name
        args = [" ".join(a.split()) for a in re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", hdr).group(1).split(",")]
        args = [] if args == ["void"] else args
        sig = _lib._SIGS[name]
        assert len(args) == len(sig) == len(protos[name][1]), name
        for a, t in zip(args, sig):
            if "*" in a:        # every pointer is passed as an address; a string and the two structs as pointers to them
                assert t is POINTER.get(a[:a.index("*")].strip(), C.c_void_p), (name, a, t)
            else:
                assert t is SCALAR[a.split()[0]], (name, a, t)

"""Reader of include/ibhip.h, the one statement of libibhip's C ABI: the ``ibh_*`` prototypes, the ``IBH_*`` integer
constants and the fields of the structs that cross the boundary, read once when the package is imported.

It accepts what the header is written in and nothing else -- plain C89 declarations: ``ret ibh_name(type [name], ...);``,
``#define IBH_X <integer>``, ``enum { IBH_X = <integer>, ... };`` and ``typedef struct s { type name; type name[N]; } s;``,
every integer a decimal or hex literal.  Anything else is an ``IbhError`` that names the declaration; nothing is guessed.
"""
import os
import re

HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ibhip.h")


class IbhError(RuntimeError):
    pass


def _integer(name, text):
    if not re.fullmatch(r"0[xX][0-9a-fA-F]+|\d+", text):
        raise IbhError(f"{HEADER_PATH}: {name} = `{text}` is not a plain decimal or hex integer literal")
    return int(text, 0)


def _ctype_text(text):
    return " ".join(text.split()).replace(" *", "*")


def _parameter(proto, text):
    """``(C type text, name or "")`` of one parameter: ``int64_t ldp``, ``const ibh_part*``, ``const float* const* g``."""
    head, star, tail = text.rpartition("*")      # a pointer's name, if it has one, follows the last `*`
    words = tail.split()
    if (not (star or words) or len(words) > (1 if star else 2) or "const" in words
            or not all(w.isidentifier() for w in words)):
        raise IbhError(f"{HEADER_PATH}: {proto}: cannot read the parameter `{text.strip()}`")
    if star:
        return _ctype_text(head + star), words[0] if words else ""
    return words[0], words[1] if len(words) == 2 else ""


def read():
    """``(prototypes, constants, structs)``: ``{name: (return type, [(type, parameter name), ...])}``, ``{IBH_X: int}`` in
    written order, ``{struct: [(type, field, array length or None), ...]}``."""
    try:
        with open(HEADER_PATH) as f:
            text = f.read()
    except OSError as e:
        raise IbhError(f"{HEADER_PATH}: cannot read the header that declares the C ABI ({e.strerror})") from None
    text = re.sub(r"/\*[^*]*\*+(?:[^/*][^*]*\*+)*/|//[^\n]*", " ", text)     # comments

    constants = {}
    for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(IBH_\w+)[ \t]*(.*)$|\benum\s*\{([^}]*)\}", text, flags=re.M):
        if m.group(1):
            constants[m.group(1)] = _integer(m.group(1), m.group(2).strip())
            continue
        for item in filter(None, (x.strip() for x in m.group(3).split(","))):
            name, _, value = (x.strip() for x in item.partition("="))
            constants[name] = _integer(name, value)
    text = re.sub(r"^\s*#[^\n]*", " ", text, flags=re.M)

    structs = {}
    for m in re.finditer(r"\btypedef\s+struct\s+(\w+)\s*\{([^}]*)\}\s*\1\s*;", text):
        fields = structs[m.group(1)] = []
        for decl in filter(None, (x.strip() for x in m.group(2).split(";"))):
            f = re.fullmatch(r"(\w+)\s+(\w+)(?:\[(\d+)\])?", decl)
            if not f:
                raise IbhError(f"{HEADER_PATH}: struct {m.group(1)}: cannot read the field `{decl}`")
            fields.append((f.group(1), f.group(2), int(f.group(3)) if f.group(3) else None))

    prototypes = {}
    for m in re.finditer(r"((?:const\s+)?\b\w+[\s*]+)(ibh_\w+)\s*\(([^();{}]*)\)\s*;", text):
        name, params = m.group(2), m.group(3).strip()
        prototypes[name] = (_ctype_text(m.group(1)),
                            [] if params in ("", "void") else [_parameter(name, p) for p in params.split(",")])
    unread = set(re.findall(r"\b(ibh_\w+)\s*\(", text)) - set(prototypes)
    if unread:
        raise IbhError(f"{HEADER_PATH}: cannot read the declaration of {sorted(unread)}")
    return prototypes, constants, structs


PROTOTYPES, CONSTANTS, STRUCTS = read()


def constants(prefix, names):
    """The values of ``prefix + name`` for the blank-separated ``names``, in their order."""
    try:
        return [CONSTANTS[prefix + n] for n in names.split()]
    except KeyError as e:
        raise IbhError(f"{HEADER_PATH} defines no constant {e.args[0]}") from None

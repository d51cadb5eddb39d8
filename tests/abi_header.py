"""include/gnx.h as the CPU tests read it: the declared names, one entry's prototype, and the ctypes types a binding of that prototype
must use.  Parsed here with its own few lines, on purpose NOT with gnntf._native.parse_header: "the binding agrees with the header"
must not compare a function with itself."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# C type of a by-value argument -> the ctypes type the binding must use (pointers and handles of every kind cross as void *)
CTYPES = {"float": ctypes.c_float, "double": ctypes.c_double, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64, "int": ctypes.c_int}
HANDLES = ("gnx_graph_t", "gnx_halo_plan_t")


def text():
    """The header as written, comments included (the documented kernel names live there)."""
    return open(os.path.join(ROOT, "include", "gnx.h")).read()


def code():
    """The header without its comments."""
    return re.sub(r"/\*.*?\*/", "", text(), flags=re.S)


def declared():
    return sorted(set(re.findall(r"\b(gnx_[a-z_0-9]+)\s*\(", code())))


def declaration(name):
    """(return type, [normalised "type name" strings]) of one entry; `(void)` is no argument."""
    found = re.search(r"^([\w \*]+?)\b" + name + r"\s*\(([^)]*)\)\s*;", code(), flags=re.M)
    assert found, f"include/gnx.h does not declare {name}"
    args = [" ".join(arg.split()) for arg in found.group(2).split(",")]
    return " ".join(found.group(1).split()), [] if args == ["void"] else args


def prototype(name):
    return declaration(name)[1]


def restype_of(name):
    return {"const char *": ctypes.c_char_p, **CTYPES}[declaration(name)[0]]


def ctypes_of(args):
    return [ctypes.c_void_p if "*" in arg or arg.startswith(HANDLES) else CTYPES[arg.rsplit(" ", 1)[0]] for arg in args]

"""ctypes binding of libgnx.so (include/gnx.h) -- the only way the package reaches the GPU.

There is deliberately NO fallback: if the library is missing or a call fails, an Exception
is raised.  Nothing here imports the CPU oracle.
"""
from __future__ import annotations

import ctypes
import os
import re
from ctypes import c_char_p, c_double, c_float, c_int, c_int64, c_uint64, c_void_p

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
ABI_VERSION = 900         # the ABI this package's call sites are written against; include/gnx.h GNX_ABI_VERSION must equal it
HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", "gnx.h")
# GNX_LIBRARY: another build of the same library (the tuning build of tools/, `make TUNING=1` -> lib/tune/libgnx.so)
LIB_PATH = os.environ.get("GNX_LIBRARY") or os.path.join(os.path.dirname(_HERE), "lib", "libgnx.so")

NORM = {"none": 0, "symmetric": 1, "bipartite": 2}
EYE = {"none": 0, "before": 1, "after": 2}
ACT_NONE, ACT_RELU, ACT_SKIP_EMPTY = 0, 1, 256
ACT_LEAKY = 2             # tf.nn.leaky_relu at slope 0.2: gnx_ngcf_step and gnx_ngcf_back_gate only
HALO_ALL, HALO_PULL, HALO_PUSH = 0, 1, 2
RESERVE_TRANSPOSED, RESERVE_K_LOOP, RESERVE_TRAIN_GATHER, RESERVE_GATHER_HINTS = 1, 2, 4, 8
ORD_X, ORD_OUT = 1, 2     # `order` of the _ord training entries: X stored in the handle's gather order / the result written in it

# C scalar type -> ctypes type; every pointer and every handle typedef crosses as void * (byref(x), a ctypes array or None at the
# call site), `const char *` comes back as c_char_p
SCALARS = {"int": c_int, "int64_t": c_int64, "uint64_t": c_uint64, "float": c_float, "double": c_double}


def parse_header():
    """({name: (restype, argtypes)} of every prototype HEADER_PATH declares, the names of those whose last parameter is `void *stream`).
    Refuses instead of guessing: a header of another ABI number, a scalar type outside SCALARS, or a gnx_ name followed by `(` that did
    not read as a prototype raises."""
    if not os.path.exists(HEADER_PATH):
        raise Exception(f"gnntf: the header {HEADER_PATH} is missing -- the binding of libgnx.so is read from it; there is no other table")
    text = re.sub(r"/\*.*?\*/", "", open(HEADER_PATH).read(), flags=re.S)
    version = re.search(r"#define\s+GNX_ABI_VERSION\s+(\d+)", text)
    if version is None or int(version.group(1)) != ABI_VERSION:
        raise Exception(f"gnntf: {HEADER_PATH} declares ABI {version.group(1) if version else 'nothing'}, this package's call sites are "
                        f"written against ABI {ABI_VERSION}")
    handles = set(re.findall(r"typedef\s+struct\s+\w+\s*\*\s*(\w+)\s*;", text))

    def scalar(entry, what, c_type):
        if c_type not in SCALARS:
            raise Exception(f"gnntf: {HEADER_PATH}: {entry}: {what} has type `{c_type}`, which the binding has no rule for")
        return SCALARS[c_type]

    def parameter(entry, arg):
        c_type = arg.rpartition(" ")[0].removeprefix("const ")          # "int64_t ldx" -> "int64_t"
        return c_void_p if "*" in arg or c_type in handles else scalar(entry, f"parameter `{arg}`", c_type)

    signatures, streamed = {}, set()
    for ret, name, args in re.findall(r"([A-Za-z_][A-Za-z_0-9 \*]*?)\b(gnx_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", text):
        ret, args = " ".join(ret.split()), [" ".join(arg.split()) for arg in args.split(",")]
        signatures[name] = (c_char_p if ret == "const char *" else scalar(name, "the return value", ret),
                            [] if args == ["void"] else [parameter(name, arg) for arg in args])
        if args[-1] == "void *stream":
            streamed.add(name)
    named = set(re.findall(r"\b(gnx_[a-z_0-9]+)\s*\(", text))
    if len(signatures) != len(named):
        raise Exception(f"gnntf: {HEADER_PATH} names {len(named)} entries and {len(signatures)} read as prototypes; not read: "
                        f"{sorted(named - set(signatures))}")
    return signatures, frozenset(streamed)


# name -> (restype, argtypes) of every symbol include/gnx.h declares, read from the header at import: nothing is typed here by hand;
# STREAMED: the entries that end in `void *stream` (launch() hands them torch's current stream)
SIGNATURES, STREAMED = parse_header()

# entries added within ABI 0.9 that a library of the same minor version may lack: found by probing (has_symbol); their callers raise
PROBED = ("gnx_step_wide_ngcf", "gnx_step_back_wide_ngcf", "gnx_step_spectral_gcn", "gnx_step_spectral_gcn_dropped", "gnx_dense_drop",
          "gnx_dense_wgrad_drop", "gnx_signal_project", "gnx_signal_spmv", "gnx_signal_ppr", "gnx_signal_smoothness",
          "gnx_signal_smoothness_back", "gnx_signal_uniform")

_lib = None


def has_symbol(name: str) -> bool:
    """Whether the loaded library exports ``name`` (the entries of PROBED)."""
    return hasattr(lib(), name)


def lib():
    """Loads libgnx.so once; raises if it has not been built (no CPU fallback exists)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise Exception(f"gnntf: the HIP library {LIB_PATH} is missing -- build it with "
                            f"`make -C gnn-tf_amd/csrc` (or __graft_entry__.build()); there is no CPU fallback")
        handle = ctypes.CDLL(LIB_PATH)
        for name, (restype, argtypes) in SIGNATURES.items():
            if name in PROBED and not hasattr(handle, name):
                continue
            fn = getattr(handle, name)  # AttributeError if a declared symbol is not exported
            fn.restype = restype
            fn.argtypes = argtypes
        # the argument lists of several entries changed under the same names at 0.3 (include/gnx.h, GNX_ABI_VERSION): a library
        # of another minor version would be called with shifted arguments -- refused, not tried
        version = int(handle.gnx_version())
        if version // 100 != ABI_VERSION // 100:
            raise Exception(f"gnntf: {LIB_PATH} implements ABI {version}, this package binds ABI {ABI_VERSION}: rebuild the library "
                            f"(make -C gnn-tf_amd/csrc)")
        _lib = handle
    return _lib


def check(rc: int):
    if rc != 0:
        msg = lib().gnx_last_error()
        raise Exception((msg.decode() if msg else "") or f"libgnx error {rc}")


def ptr(t):
    """Device pointer of a torch tensor (None -> NULL)."""
    return None if t is None else c_void_p(t.data_ptr())


def current_stream():
    """The raw hipStream_t of torch's current stream on the current device (the cheap accessor: this sits on every launch)."""
    return c_void_p(torch._C._cuda_getCurrentRawStream(torch.cuda.current_device()))


# how launch() passes an argument on, by the parameter's declared type: the expression over the argument ``{a}``.  A pointer or handle
# parameter takes a tensor's device pointer, and None, byref(x), ctypes arrays and handles as they are
CONVERSIONS = {c_void_p: "{a} if {a} is None or type({a}) is c_void_p else c_void_p({a}.data_ptr()) if isinstance({a}, Tensor) else {a}",
               c_int: "int({a})", c_int64: "int({a})", c_uint64: "int({a}) & 0xFFFFFFFFFFFFFFFF", c_float: "float({a})", c_double: "float({a})"}


def _converter(argtypes):
    """lambda a0, a1, ...: [every argument converted by its parameter's type]: one expression per entry, made once -- launch() sits on
    every call of launch-bound steps, and a converter called per argument measured slower than the hand-written call sites were."""
    names = [f"a{k}" for k in range(len(argtypes))]
    converted = ", ".join(CONVERSIONS[t].format(a=a) for t, a in zip(argtypes, names))
    return eval(f"lambda {', '.join(names)}: [{converted}]", {"c_void_p": c_void_p, "Tensor": torch.Tensor})


def _call(name, argtypes):
    given = argtypes[:-1] if name in STREAMED else argtypes
    return len(given), name in STREAMED, _converter(given)


# name -> (the number of arguments the caller passes: all but a closing stream, whether launch() appends the stream, their converter)
CALLS = {name: _call(name, argtypes) for name, (_, argtypes) in SIGNATURES.items()}


def launch(device, name, *args):
    """One call of the entry ``name`` with ``device`` current: every argument converted by its parameter's declared type (tensor ->
    device pointer, int / float scalars, uint64_t masked to 64 bits), torch's current stream appended where the prototype ends in
    `void *stream`, the status checked.  The function is looked up on lib() at every call: a spy put in lib's place sees all of them."""
    count, streamed, convert = CALLS[name]
    if len(args) != count:
        raise Exception(f"gnntf: {name} takes {count} arguments" + (" and the stream" if streamed else "") + f", {len(args)} given")
    with on_device(device):
        args = convert(*args)
        if streamed:
            args.append(current_stream())
        check(getattr(lib(), name)(*args))


class on_device:
    """``with on_device(t.device):`` -- makes the tensor's device current for the launch; free when it already is
    (the usual case: one process per GPU)."""

    __slots__ = ("index", "prev")

    def __init__(self, device):
        self.index = device.index

    def __enter__(self):
        self.prev = torch.cuda.current_device()
        if self.index is None:
            self.index = self.prev
        if self.prev != self.index:
            torch.cuda.set_device(self.index)

    def __exit__(self, *exc):
        if self.prev != self.index:
            torch.cuda.set_device(self.prev)


def require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise Exception("gnntf: the propagation path runs on the GPU only (tensor on %s); there is no CPU "
                            "fallback" % t.device)

"""_native.launch, the one crossing into libgnx.so, over a fake library object: what it converts, when it appends the stream, what it
refuses and where it looks the function up.  No device and no library call: on_device and current_stream are stand-ins."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

from abi_header import declared, prototype

STREAM = ctypes.c_void_p(0x5EED)
CPU = torch.device("cpu")
DUMMY = {"int": 3, "int64_t": 5, "uint64_t": 7, "float": 0.5, "double": 0.25}


class FakeLibrary:
    """Every gnx_ entry records (name, args) and answers ``status``; gnx_last_error answers ``error`` unless that is None."""

    def __init__(self, status=0, error=None):
        self.calls, self.status, self.error = [], status, error

    def __getattr__(self, name):
        if not name.startswith("gnx_"):
            raise AttributeError(name)
        if name == "gnx_last_error" and self.error is not None:
            return lambda: self.error
        return lambda *args: self.calls.append((name, args)) or self.status


@pytest.fixture
def nat(monkeypatch):
    from gnntf import _native
    monkeypatch.setattr(_native, "current_stream", lambda: STREAM)
    monkeypatch.setattr(_native, "on_device", lambda device: contextlib.nullcontext())
    return _native


def use(monkeypatch, nat, **how):
    fake = FakeLibrary(**how)
    monkeypatch.setattr(nat, "lib", lambda: fake)
    return fake


def offered(name):
    """One argument per parameter the caller of ``name`` passes: a closing stream is left to launch."""
    args = prototype(name)
    if args and args[-1] == "void *stream":
        args = args[:-1]
    return [None if "*" in arg or arg.startswith("gnx_") else DUMMY[arg.rsplit(" ", 1)[0].removeprefix("const ")] for arg in args]


def test_pointers_cross_as_void_p_none_or_untouched(nat, monkeypatch):
    fake = use(monkeypatch, nat)
    src, dst, count = torch.zeros(6), torch.zeros(6, dtype=torch.bfloat16), ctypes.c_int64()
    nat.launch(CPU, "gnx_cast_bf16", src, 2, 3, 3, dst, 3)                        # (src, n_rows, C, lds, dst, ldd, stream)
    (name, args), = fake.calls
    assert name == "gnx_cast_bf16" and len(args) == 7
    assert [type(args[k]) for k in (0, 4)] == [ctypes.c_void_p] * 2 and (args[0].value, args[4].value) == (src.data_ptr(), dst.data_ptr())
    ref, handle = ctypes.byref(count), ctypes.c_void_p(64)
    nat.launch(CPU, "gnx_graph_gather_hints", handle, None, ref, None)            # (handle, cols, hot, last): no stream
    assert fake.calls[1] == ("gnx_graph_gather_hints", (handle, None, ref, None))
    assert fake.calls[1][1][0] is handle and fake.calls[1][1][2] is ref


def test_scalars_cross_as_python_numbers_of_the_declared_type(nat, monkeypatch):
    fake = use(monkeypatch, nat)
    handle, D = ctypes.c_void_p(64), torch.zeros(4)
    # gnx_graph_colsum_streams(handle, float p, uint64_t seed, uint64_t first_stream, int64_t n_streams, D, stream)
    nat.launch(CPU, "gnx_graph_colsum_streams", handle, 1, -1, np.int64(9), np.int64(4), D)
    nat.launch(CPU, "gnx_graph_colsum_streams", handle, 0.5, 2 ** 64 + 3, True, torch.tensor(4), D)
    nat.launch(CPU, "gnx_graph_colsum_streams", handle, np.float32(0.25), 0, 0, True, D)
    first, second, third = (args for _, args in fake.calls)
    assert type(first[1]) is float and first[1] == 1.0                            # an int offered for a float parameter
    assert type(first[2]) is int and first[2] == 2 ** 64 - 1                      # a seed of -1, masked to 64 bits
    assert type(first[3]) is int and first[3] == 9 and type(first[4]) is int and first[4] == 4      # numpy int64
    assert second[2] == 3 and type(second[3]) is int and second[3] == 1           # masked; a bool for uint64_t
    assert type(second[4]) is int and second[4] == 4                              # a 0-dim tensor for int64_t
    assert type(third[1]) is float and third[1] == 0.25 and type(third[4]) is int and third[4] == 1   # a bool for int64_t
    assert all(args[-1] is STREAM and len(args) == 7 for args in (first, second, third))


def test_an_int_parameter_takes_a_bool_as_its_flag(nat, monkeypatch):
    fake = use(monkeypatch, nat)
    nat.launch(CPU, "gnx_signal_project", torch.zeros(2, 3), 3, 2, 3, torch.zeros(3), True, torch.zeros(2))   # (..., int sigmoid, out, stream)
    assert type(fake.calls[0][1][5]) is int and fake.calls[0][1][5] == 1


@pytest.mark.parametrize("name", declared())
def test_the_stream_is_appended_exactly_where_the_prototype_ends_in_it(nat, monkeypatch, name):
    fake = use(monkeypatch, nat)
    args = prototype(name)
    given = offered(name)
    nat.launch(CPU, name, *given)
    (called, got), = fake.calls
    assert called == name and len(got) == len(args)
    if args and args[-1] == "void *stream":
        assert got[-1] is STREAM and len(given) == len(args) - 1 and name in nat.STREAMED
    else:
        assert len(given) == len(args) and name not in nat.STREAMED
    assert not any(arg is STREAM for arg in got[:-1])


def test_the_creators_and_the_streamless_entries_get_nothing_appended(nat):
    without = [name for name in declared() if name not in nat.STREAMED]
    assert len(nat.STREAMED) == 89 and len(without) == 20
    assert {"gnx_graph_create_coo", "gnx_graph_create_csr"} <= set(without)      # the stream stands mid-list: the caller passes it
    for name in ("gnx_graph_create_coo", "gnx_graph_create_csr"):
        assert "void *stream" in prototype(name)[:-1] and nat.CALLS[name][:2] == (len(prototype(name)), False)


@pytest.mark.parametrize("extra", (-1, 1))
def test_a_wrong_argument_count_names_the_entry(nat, monkeypatch, extra):
    fake = use(monkeypatch, nat)
    given = offered("gnx_cast_bf16")
    given = given[:-1] if extra < 0 else given + [None]
    with pytest.raises(Exception, match=r"gnx_cast_bf16 takes 6 arguments and the stream, " + str(len(given)) + " given"):
        nat.launch(CPU, "gnx_cast_bf16", *given)
    with pytest.raises(Exception, match=r"gnx_graph_info takes 5 arguments, 4 given"):
        nat.launch(CPU, "gnx_graph_info", *offered("gnx_graph_info")[:-1])
    assert fake.calls == []


def test_a_nonzero_status_raises_with_the_librarys_text(nat, monkeypatch):
    use(monkeypatch, nat, status=-1, error=b"gnx_cast_bf16: negative row count")
    with pytest.raises(Exception, match="gnx_cast_bf16: negative row count"):
        nat.launch(CPU, "gnx_cast_bf16", *offered("gnx_cast_bf16"))


def test_the_function_is_fetched_from_lib_at_every_call(nat, monkeypatch):
    first = use(monkeypatch, nat)
    nat.launch(CPU, "gnx_cast_bf16", *offered("gnx_cast_bf16"))
    second = use(monkeypatch, nat)
    nat.launch(CPU, "gnx_cast_bf16", *offered("gnx_cast_bf16"))
    assert len(first.calls) == 1 and len(second.calls) == 1


def test_the_device_is_made_current_around_the_call(monkeypatch):
    from gnntf import _native
    fake, seen = FakeLibrary(), []

    @contextlib.contextmanager
    def on_device(device):
        seen.append(("enter", device))
        yield
        seen.append(("exit", device))

    monkeypatch.setattr(_native, "on_device", on_device)
    monkeypatch.setattr(_native, "current_stream", lambda: seen.append("stream") or STREAM)
    monkeypatch.setattr(_native, "lib", lambda: seen.append("lib") or fake)
    _native.launch(CPU, "gnx_cast_bf16", *offered("gnx_cast_bf16"))
    assert seen == [("enter", CPU), "stream", "lib", ("exit", CPU)]

"""The gather order of the training loops (gnx_graph_gather_order, gnx_spmm_dropped_chained_ord, gnx_spmm_dropped_back_ord,
sparse.ppr_loop(gather_order=), GNN(train_gather_order=)): what can be checked without a GPU -- header, exports, binding, the
argument checks of the Python layer and what "auto" resolves to."""
import ctypes
import re

import pytest
import torch

import abi_header

SYMBOLS = ("gnx_graph_gather_order", "gnx_spmm_dropped_chained_ord", "gnx_spmm_dropped_back_ord")


def test_header_declares_the_symbols_within_abi_900():
    text, code = abi_header.text(), abi_header.code()
    for name in SYMBOLS:
        assert abi_header.declaration(name)[0] == "int", name
    assert re.search(r"#define GNX_ABI_VERSION 900\b", text)
    assert re.search(r"GNX_RESERVE_TRAIN_GATHER\s*=\s*4\b", code)
    assert re.search(r"GNX_ORD_X\s*=\s*1\b", code) and re.search(r"GNX_ORD_OUT\s*=\s*2\b", code)
    # the _ord entries take the namesake's arguments plus `int order` before the stream
    for name in SYMBOLS[1:]:
        ours, theirs = ", ".join(abi_header.prototype(name)), ", ".join(abi_header.prototype(name[:-len("_ord")]))
        assert ours == theirs.replace(", void *stream", ", int order, void *stream")
    assert "bitwise" in text.lower()                                # the statement the issue asks the header to make


def test_library_exports_and_binding_lists_them():
    from gnntf import _native
    handle = ctypes.CDLL(_native.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(handle, name), name
        assert name in _native.SIGNATURES
    assert _native.lib().gnx_version() == 900 == _native.ABI_VERSION
    assert (_native.RESERVE_TRAIN_GATHER, _native.ORD_X, _native.ORD_OUT) == (4, 1, 2)
    for ord_name in SYMBOLS[1:]:                                     # one more int than the namesake, before the stream
        ours, theirs = _native.SIGNATURES[ord_name][1], _native.SIGNATURES[ord_name[:-len("_ord")]][1]
        assert ours == theirs[:-1] + [ctypes.c_int, ctypes.c_void_p]


def test_null_handles_are_refused_without_a_device():
    from gnntf import _native
    lib = _native.lib()
    assert lib.gnx_graph_gather_order(None, None, None) == -1 and b"NULL handle" in lib.gnx_last_error()
    for order in (0, 1, 2, 3):
        assert lib.gnx_spmm_dropped_chained_ord(None, None, 0.5, 0, 0, 0, None, None, 8, 8, None, 8, 0.9, 0.1, 0, None, 8, order, None) == -1
        assert b"NULL handle" in lib.gnx_last_error()
        assert lib.gnx_spmm_dropped_back_ord(None, None, 0.5, 0, 0, 0, None, None, 8, 8, None, 8, 1.0, 0.9, None, 8, 0.9, None, 8, 0, order,
                                             None) == -1
        assert b"NULL handle" in lib.gnx_last_error()
    assert lib.gnx_graph_reserve(None, 8, _native.RESERVE_TRAIN_GATHER, None) == -1


def test_unknown_gather_order_is_rejected():
    import gnntf
    from gnntf import sparse
    with pytest.raises(Exception, match="gather_order"):
        sparse.ppr_loop(lambda k, bwd=False: None, torch.zeros(4, 4), 0.1, 2, gather_order="hubs")
    with pytest.raises(Exception, match="gather_order"):
        sparse.resolve_gather_order("degree", 10, 8)
    coo = gnntf.SparseCOO([[0, 1], [1, 0]], [1.0, 1.0], (2, 2))
    with pytest.raises(Exception, match="train_gather_order"):
        gnntf.GNN(coo, torch.zeros(2, 3), train_gather_order="hubs")
    with pytest.raises(Exception, match="train_gather_order"):
        gnntf.APPNP(coo, torch.zeros(2, 3), num_classes=2, train_gather_order=None)


def test_auto_follows_the_allowance(monkeypatch):
    """Outside the allowance "auto" is "caller"; with the allowance empty (no width has measured a gain) it is "caller" everywhere;
    the explicit modes are never changed."""
    from gnntf import sparse
    sizes = (3_000, sparse.TRAIN_GATHER_MIN_ROWS, 10 ** 7)
    widths = (1, 7, 8, 16, 32, 40, 64, 128, 256)
    for n in sizes:
        for width in widths:
            inside = width <= sparse.TRAIN_GATHER_MAX_WIDTH and n >= sparse.TRAIN_GATHER_MIN_ROWS
            assert sparse.resolve_gather_order("auto", n, width) == ("relabelled" if inside else "caller")
            assert sparse.resolve_gather_order("caller", n, width) == "caller"
            assert sparse.resolve_gather_order("relabelled", n, width) == "relabelled"
    monkeypatch.setattr(sparse, "TRAIN_GATHER_MAX_WIDTH", 0)        # the empty allowance
    assert all(sparse.resolve_gather_order("auto", n, width) == "caller" for n in sizes for width in widths)
    monkeypatch.setattr(sparse, "TRAIN_GATHER_MAX_WIDTH", 16)
    monkeypatch.setattr(sparse, "TRAIN_GATHER_MIN_ROWS", 1_000_000)
    assert sparse.resolve_gather_order("auto", 10 ** 7, 16) == "relabelled"
    assert sparse.resolve_gather_order("auto", 10 ** 7, 32) == "caller"
    assert sparse.resolve_gather_order("auto", 999_999, 8) == "caller"


def test_the_default_of_the_model_is_auto_and_of_the_loop_is_caller():
    import inspect
    import gnntf
    from gnntf import sparse
    assert inspect.signature(gnntf.GNN.__init__).parameters["train_gather_order"].default == "auto"
    assert inspect.signature(sparse.ppr_loop).parameters["gather_order"].default == "caller"
    assert sparse.GATHER_ORDERS == ("caller", "relabelled", "auto")

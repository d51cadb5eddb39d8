"""The fused backward of the GCNII layer (gnx_gcnii_step_back), as far as it goes without a GPU: the header declares the entry, the
library exports it, gnntf/_native.py binds it with the declared argument types, the ABI number did not move, and the options
gcnii_step(backward=) / GNN(gcnii_backward=) refuse values they do not know."""
import ctypes
import re

import numpy as np
import pytest
import torch

from abi_header import ctypes_of, prototype as header_prototype, text as header_text

NAME = "gnx_gcnii_step_back"


def test_header_declares_the_entry():
    assert header_prototype(NAME) == [
        "gnx_graph_t g", "const float *d_vals_t", "const float *d_G", "float a", "int64_t C", "const float *d_Mt", "int64_t ldmt",
        "float *d_dH", "const float *d_S_in", "float s_alpha", "float *d_S_out", "float *d_work", "void *stream"]
    text = header_text()
    assert "spmm_gcnii_back_mfma" in text and "dense+spmm_back" in text          # the reported names are documented
    assert re.search(r"#define\s+GNX_ABI_VERSION\s+900\b", text)


def test_library_exports_the_entry():
    from gnntf import _native
    assert hasattr(ctypes.CDLL(_native.LIB_PATH), NAME)


def test_native_binds_the_declared_argument_types():
    from gnntf import _native
    restype, argtypes = _native.SIGNATURES[NAME]
    want = ctypes_of(header_prototype(NAME))
    assert len(want) == 13
    assert restype is ctypes.c_int and argtypes == want
    fn = getattr(_native.lib(), NAME)
    assert fn.argtypes == want and fn.restype is ctypes.c_int


def test_version_is_still_900():
    from gnntf import _native
    assert _native.lib().gnx_version() == 900 == _native.ABI_VERSION


def test_checks_that_need_no_device():
    """A NULL handle is refused before anything touches a device."""
    from gnntf import _native
    lib = _native.lib()
    assert lib.gnx_gcnii_step_back(None, None, 16, 0.1, 16, 16, 16, 32, None, 1.0, None, None, None) == -1
    assert b"gnx_gcnii_step_back: NULL handle" in lib.gnx_last_error()


def test_unknown_backward_options_raise():
    import gnntf
    from gnntf import sparse
    assert sparse.GCNII_BACKWARDS == ("composed", "fused")
    assert gnntf.gcnii_step_back is sparse.gcnii_step_back
    H, H0, M = torch.zeros(4, 16, requires_grad=True), torch.zeros(4, 16), torch.eye(16)
    with pytest.raises(Exception, match="backward must be one of"):
        sparse.gcnii_step(None, H, H0, 0.1, M, backward="nonsense")
    coo = np.array([[0, 1], [1, 0]], dtype=np.int64)
    graph = gnntf.SparseCOO(coo, np.ones(2, dtype=np.float32), (2, 2))
    with pytest.raises(Exception, match="gcnii_backward must be one of"):
        gnntf.GNN(graph, np.zeros((2, 3), dtype=np.float32), gcnii_backward="nonsense")
    with pytest.raises(Exception, match="gcnii_backward must be one of"):
        gnntf.GCNII(graph, np.zeros((2, 3), dtype=np.float32), 2, iterations=1, gcnii_backward="nonsense")

"""Opt-in bf16 feature storage of the fused GCNII layer, as far as it goes without a GPU: the header declares gnx_gcnii_step_bf16,
the library exports it, gnntf/_native.py binds it with the declared argument types, the ABI number did not move, and
sparse.gcnii_step(storage=torch.bfloat16) refuses autograd."""
import ctypes
import re

import pytest
import torch

from abi_header import ctypes_of, prototype as header_prototype, text as header_text


def test_header_declares_the_entry():
    args = header_prototype("gnx_gcnii_step_bf16")
    assert args == ["gnx_graph_t g", "const float *d_vals", "const uint16_t *d_H", "const float *d_H0", "float a", "int64_t C",
                    "const float *d_M", "int64_t ldm", "int act", "void *d_out", "int out_bf16", "float *d_work", "void *stream"]
    text = header_text()
    assert "spmm_gcnii_mfma_bf16" in text and "spmm+dense_mfma_bf16" in text       # the reported names are documented
    assert re.search(r"#define\s+GNX_ABI_VERSION\s+900\b", text)


def test_library_exports_the_entry():
    from gnntf import _native
    raw = ctypes.CDLL(_native.LIB_PATH)
    assert hasattr(raw, "gnx_gcnii_step_bf16")


def test_native_binds_the_declared_argument_types():
    from gnntf import _native
    restype, argtypes = _native.SIGNATURES["gnx_gcnii_step_bf16"]
    want = ctypes_of(header_prototype("gnx_gcnii_step_bf16"))
    assert restype is ctypes.c_int and argtypes == want
    fn = _native.lib().gnx_gcnii_step_bf16
    assert fn.argtypes == want and fn.restype is ctypes.c_int


def test_version_still_equals_the_header():
    from gnntf import _native
    text = header_text()
    number = int(re.search(r"#define\s+GNX_ABI_VERSION\s+(\d+)", text).group(1))
    assert _native.lib().gnx_version() == number == _native.ABI_VERSION


def test_checks_that_need_no_device():
    """A NULL handle is refused before anything touches a device."""
    from gnntf import _native
    lib = _native.lib()
    assert lib.gnx_gcnii_step_bf16(None, None, 8, 8, 0.1, 16, 8, 16, 0, 16, 0, None, None) == -1
    assert b"gnx_gcnii_step_bf16: NULL handle" in lib.gnx_last_error()


def test_bf16_storage_refuses_autograd():
    from gnntf import sparse
    H = torch.zeros(4, 16, requires_grad=True)
    H0, M = torch.zeros(4, 16), torch.eye(16)
    with pytest.raises(Exception, match="bf16 storage is inference only"):
        sparse.gcnii_step(None, H, H0, 0.1, M, storage=torch.bfloat16)
    with pytest.raises(Exception, match="bf16 storage is inference only"):
        sparse.gcnii_step(None, H.detach(), H0, 0.1, M.requires_grad_(), storage=torch.bfloat16, out_storage=torch.bfloat16)
    with pytest.raises(Exception, match="storage must be"):
        sparse.gcnii_step(None, H, H0, 0.1, M, storage=torch.float16)

"""Where the NULL-handle check of the fused training entries sits, without a device: gnx_spmm_dropped, the three chained and the
three back entries, each with a NULL handle and otherwise valid (fake, never dereferenced) pointers.  The f32 and _ord entries look
at the handle first; the bf16 entries make their handle-free checks first (tests/test_bf16_train_host.py exercises those)."""
import ctypes

import pytest

D, D_NEXT, X, H0, OUT, Y = (ctypes.c_void_p(v) for v in (0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000))
C = 8


def lib():
    from gnntf import _native
    return _native.lib()


def forward(name, x=X):
    """One call of a forward entry with a NULL handle; ``x``: the gathered operand."""
    L = lib()
    head = (None, D, 0.5, 1, 2, 0)
    mix = (x, C, C, H0, C, 0.9, 0.1, 0, OUT)
    if name == "gnx_spmm_dropped":
        return L.gnx_spmm_dropped(*head, *mix, C, None)
    if name == "gnx_spmm_dropped_chained":
        return L.gnx_spmm_dropped_chained(*head, D_NEXT, *mix, C, None)
    if name == "gnx_spmm_dropped_chained_ord":
        return L.gnx_spmm_dropped_chained_ord(*head, D_NEXT, *mix, C, 3, None)
    return L.gnx_spmm_dropped_chained_bf16(*head, D_NEXT, *mix, 1, C, None)


def back(name, x=X):
    """One call of a back entry with a NULL handle: the running sum updated in place, a pre-scaled output of its own."""
    L = lib()
    args = (None, D, 0.5, 1, 2, 1, D_NEXT, x, C, C, H0, C, 1.0, 0.09, H0, C, 0.9, Y, C, 0)
    if name == "gnx_spmm_dropped_back_ord":
        return L.gnx_spmm_dropped_back_ord(*args, 3, None)
    return getattr(L, name)(*args, None)


ENTRIES = [("gnx_spmm_dropped", forward), ("gnx_spmm_dropped_chained", forward), ("gnx_spmm_dropped_chained_ord", forward),
           ("gnx_spmm_dropped_chained_bf16", forward), ("gnx_spmm_dropped_back", back), ("gnx_spmm_dropped_back_ord", back),
           ("gnx_spmm_dropped_back_bf16", back)]


@pytest.mark.parametrize("name,call", ENTRIES, ids=[name for name, _ in ENTRIES])
def test_null_handle_is_named_by_its_entry(name, call):
    assert call(name) == -1
    assert lib().gnx_last_error().decode() == name + ": NULL handle"


@pytest.mark.parametrize("name,call", ENTRIES, ids=[name for name, _ in ENTRIES])
def test_null_handle_together_with_a_null_operand(name, call):
    """The f32 and _ord entries report the handle, the bf16 entries the operand (their handle check comes last)."""
    assert call(name, x=None) == -1
    want = name + (": NULL X/out" if name.endswith("_bf16") else ": NULL handle")
    assert lib().gnx_last_error().decode() == want


@pytest.mark.parametrize("name", ["gnx_spmm_dropped_chained_ord", "gnx_spmm_dropped_back_ord"])
def test_order_zero_is_the_plain_entry(name):
    L = lib()
    if "chained" in name:
        rc = L.gnx_spmm_dropped_chained_ord(None, D, 0.5, 1, 2, 0, D_NEXT, X, C, C, H0, C, 0.9, 0.1, 0, OUT, C, 0, None)
    else:
        rc = L.gnx_spmm_dropped_back_ord(None, D, 0.5, 1, 2, 1, D_NEXT, X, C, C, H0, C, 1.0, 0.09, H0, C, 0.9, Y, C, 0, 0, None)
    assert rc == -1 and L.gnx_last_error().decode() == name[:-len("_ord")] + ": NULL handle"

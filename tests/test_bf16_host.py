"""The opt-in bf16 storage without a GPU: argument errors of the three C entries, the bf16 emulation the GPU tests judge against,
and the Python layer's checks that run before any launch."""
import ctypes

import numpy as np
import pytest
import torch

from bf16_ref import U, bf16_bits, bf16_decode, bf16_round

FAKE = ctypes.c_void_p(0x1000)          # a non-NULL device pointer; never dereferenced: every call below fails its checks first


def lib():
    from gnntf import _native
    return _native.lib()


def err():
    return lib().gnx_last_error()


def test_cast_argument_errors():
    L = lib()
    assert L.gnx_cast_bf16(FAKE, 4, 0, 4, FAKE, 4, None) == -1 and b"feature width" in err()
    assert L.gnx_cast_bf16(FAKE, 4, 8, 7, ctypes.c_void_p(0x2000), 8, None) == -1 and b"leading dimension" in err()
    assert L.gnx_cast_bf16(FAKE, 4, 8, 8, ctypes.c_void_p(0x2000), 4, None) == -1 and b"leading dimension" in err()
    assert L.gnx_cast_bf16(None, 4, 8, 8, FAKE, 8, None) == -1 and b"NULL buffer" in err()
    assert L.gnx_cast_bf16(FAKE, 4, 8, 8, FAKE, 8, None) == -1 and b"alias" in err()
    assert L.gnx_cast_bf16(FAKE, -1, 8, 8, FAKE, 8, None) == -1 and b"negative" in err()
    assert L.gnx_cast_bf16(None, 0, 8, 8, None, 8, None) == 0             # nothing to do


def test_spmm_bf16_argument_errors():
    L = lib()
    X, H0, out = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x2000), ctypes.c_void_p(0x3000)
    assert L.gnx_spmm_bf16(None, None, None, X, 8, 8, H0, 8, 1.0, 0.0, 0, out, 0, 8, None) == -1 and b"NULL handle" in err()


def test_appnp_bf16_argument_errors():
    L = lib()
    H0, out, work = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x2000), ctypes.c_void_p(0x3000)
    call = lambda K=2, C=8, act=0, h=H0, o=out, w=work: L.gnx_appnp_propagate_bf16(None, None, None, h, 0.1, K, C, act, o, w, None)
    assert call(K=-1) == -1 and b"negative iteration count" in err()
    assert call(C=0) == -1 and b"feature width" in err()
    assert call(act=7) == -1 and b"invalid activation" in err()
    assert call(w=None) == -1 and b"NULL buffer" in err()
    assert call(K=1, w=None) == -1 and b"NULL buffer" in err()          # K = 1 needs the work buffer as well (H~_0 lives there)
    assert call(o=H0) == -1 and b"distinct" in err()
    assert call(w=out) == -1 and b"distinct" in err()
    assert call() == -1 and b"NULL handle" in err()


def test_emulation_matches_torch_cast():
    """bf16_ref against torch's CPU cast: ties (both directions), subnormals, +-inf, NaN, max-finite and the overflow to inf."""
    f32 = lambda bits: np.array(bits, dtype=np.uint32).view(np.float32)
    special = np.concatenate([
        f32([0x3F808000, 0x3F818000, 0x3F80_8001, 0x3F80_7FFF, 0xBF808000, 0xBF818000]),     # ties to even, just above / below
        f32([0x00000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x80000001, 0x80018000]),        # subnormals (with ties)
        f32([0x7F7F0000, 0x7F7F7FFF, 0x7F7F8000, 0x7F7FFFFF, 0xFF7FFFFF]),                    # max-finite bf16, rounding up to inf
        np.array([np.inf, -np.inf, 0.0, -0.0, 1.0, -2.5, 3.14159265, 1e-40, 65504.0], dtype=np.float32),
    ])
    rng = np.random.default_rng(0)
    rand = rng.standard_normal(100000).astype(np.float32) * np.float32(10.0) ** rng.integers(-30, 30, 100000).astype(np.float32)
    x = np.concatenate([special, rand])
    got = bf16_bits(x)
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    np.testing.assert_array_equal(got, want)
    assert bf16_decode(bf16_bits(f32([0x7F7FFFFF])))[0] == np.inf
    assert bf16_decode(bf16_bits(f32([0x7F7F7FFF])))[0] == np.float32(3.3895314e38)
    nans = f32([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF, 0x7F80FFFF])
    assert np.isnan(bf16_round(nans)).all() and np.isnan(torch.from_numpy(nans).to(torch.bfloat16).float().numpy()).all()
    finite = rand[np.isfinite(rand) & (np.abs(rand) > 1e-30) & (np.abs(rand) < 1e30)]
    assert np.max(np.abs(bf16_round(finite) - finite) / np.abs(finite)) <= U


def test_storage_keyword_is_checked_before_any_launch():
    from gnntf import sparse
    with pytest.raises(Exception, match="storage must be"):
        sparse._bf16(torch.float16)
    with pytest.raises(Exception, match="inference only"):
        sparse._no_grad_for_bf16("spmm", torch.zeros(2, 2, requires_grad=True))
    with torch.no_grad():
        sparse._no_grad_for_bf16("spmm", torch.zeros(2, 2, requires_grad=True))


def test_friendly_width_bf16():
    from gnntf import sparse
    n = sparse.PAD_MIN_ROWS
    assert [sparse.friendly_width_bf16(c, n) for c in (5, 7, 8, 9, 17, 33, 40, 64)] == [5, 8, 8, 16, 32, 64, 64, 64]
    assert sparse.friendly_width_bf16(128, n) == 128 and sparse.friendly_width_bf16(256, n) == 256
    for c in range(65, 520):
        w = sparse.friendly_width_bf16(c, n)
        assert w >= c and w % 8 == 0 and sparse.lines_per_row(w, 2) <= sparse.lines_per_row((c + 7) // 8 * 8, 2)
    assert sparse.friendly_width_bf16(40, n - 1) == 40                   # small graphs: no pad
    assert sparse.lines_per_row(64, 2) == 1.0 and sparse.lines_per_row(40, 2) == 1.5
    assert sparse.lines_per_row(40) == sparse.lines_per_row(40, 4)       # the f32 default is unchanged


def test_inference_dtype_is_validated():
    import gnntf
    with pytest.raises(Exception, match="inference_dtype"):
        gnntf.GNN.__init__(object.__new__(gnntf.GNN), None, None, inference_dtype=torch.float16)

"""The opt-in bf16 training storage without a GPU: the emulation the GPU tests judge against (tests/bf16_train_ref.py) is the
reference arithmetic plus the stated roundings and nothing else; the handle-free argument checks of the two C entries; the Python
layer's checks that run before any launch."""
import ctypes
import types

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import bf16_train_ref as ref
import graphs
from oracle import gnntf_oracle as orc


def lib():
    from gnntf import _native
    return _native.lib()


def err():
    return lib().gnx_last_error()


def _graphs():
    n = 300
    coo, vals, shape = graphs.rmat_symmetric_coo(n, 2500, seed=11)
    doubled = orc.graph2adj(range(n), [tuple(e) for e in coo])                       # every entry twice
    unequal = graphs.random_coo(n, n, 4000, seed=12, weighted=True, dup_frac=0.3)    # duplicates with unequal values
    return {"plain": (coo, vals, shape), "doubled": doubled, "unequal": unequal}


@pytest.mark.parametrize("name", ["plain", "doubled", "unequal"])
@pytest.mark.parametrize("K,p", [(1, 0.5), (2, 0.1), (10, 0.5)])
def test_emulation_without_rounding_is_the_reference(name, K, p):
    """bf() replaced by the identity and float64 coefficients: the forward equals oracle.appnp_propagate in training mode, the
    backward equals K applications of oracle.ppr_iteration_backward, to float64 rounding (the f32 degree scales of the emulation
    are widened, the oracle's float64 run makes its own: compared at 1e-6, the f32 rounding of D)."""
    coo, vals, shape = _graphs()[name]
    rng = np.random.default_rng(K)
    H0 = rng.standard_normal((shape[0], 6)).astype(np.float32)
    g = rng.standard_normal((shape[0], 6)).astype(np.float32)
    a, seed, first = 0.1, 1234, 7
    mats = ref.dropped_matrices(coo, vals, shape, p, seed, first, K)
    # the emulation keeps the library's f32 scales; give it the oracle's float64 ones for the exact comparison
    exact = []
    for k, (B, _) in enumerate(mats):
        v = orc.sparse_dropout(coo, np.asarray(vals, dtype=np.float64), p, True, seed, first + k)
        D = orc.divide_no_nan(np.float64(1.0), np.sqrt(orc.sparse_reduce_sum_axis0(coo, v, shape)))
        exact.append((sp.coo_matrix((v, (coo[:, 0], coo[:, 1])), shape=shape).tocsr(), D))
    fwd = ref.forward(exact, H0, a, rnd=ref.identity, coef=np.float64)
    want = ref.oracle_forward(coo, vals, shape, H0, a, K, p, seed, first)
    assert ref.rel_fro(fwd, want) < 1e-12
    bwd = ref.backward(exact, g, a, rnd=ref.identity, coef=np.float64)
    want_b = ref.oracle_backward(coo, vals, shape, g, a, K, p, seed, first)
    assert ref.rel_fro(bwd, want_b) < 1e-12
    # with the f32 scales and f32 coefficients (what the GPU tests use): f32 rounding of D and of 1/(1-p) only
    assert ref.rel_fro(ref.forward(mats, H0, a, rnd=ref.identity), want) < 1e-5
    assert ref.rel_fro(ref.backward(mats, g, a, rnd=ref.identity), want_b) < 1e-5
    # and the roundings move it by about u = 2^-8, not more: the stated rounding points and nothing else
    assert 0 < ref.rel_fro(ref.forward(mats, H0, a), want) < 2.0 ** -7
    assert 0 < ref.rel_fro(ref.backward(mats, g, a), want_b) < 2.0 ** -7


def test_chained_bf16_argument_errors():
    L = lib()
    D, X, H0, out = (ctypes.c_void_p(v) for v in (0x1000, 0x2000, 0x3000, 0x4000))

    def call(d=D, p=0.5, x=X, ldx=8, C=8, h=H0, ldh=8, act=0, o=out, obf=1, ldo=8):
        return L.gnx_spmm_dropped_chained_bf16(None, d, p, 1, 2, 0, None, x, ldx, C, h, ldh, 0.9, 0.1, act, o, obf, ldo, None)
    assert call(C=0) == -1 and b"feature width" in err()
    assert call(x=None) == -1 and b"NULL X/out" in err()
    assert call(ldx=7) == -1 and b"leading dimension" in err()
    assert call(ldh=4) == -1 and b"leading dimension" in err()
    assert call(o=X) == -1 and b"alias" in err()
    assert call(obf=2) == -1 and b"out_bf16" in err()
    assert call(act=7) == -1 and b"invalid activation" in err()
    assert call(d=None) == -1 and b"NULL degree scales" in err()
    assert call(p=1.0) == -1 and b"dropout rate" in err()
    assert call() == -1 and b"NULL handle" in err() and b"gnx_spmm_dropped_chained_bf16" in err()


def test_back_bf16_argument_errors():
    L = lib()
    D, X, S, Y = (ctypes.c_void_p(v) for v in (0x1000, 0x2000, 0x3000, 0x4000))

    def call(d=D, p=0.5, x=X, C=8, s_in=S, s_out=S, y=Y, ldy=8, act=256):
        return L.gnx_spmm_dropped_back_bf16(None, d, p, 1, 2, 1, D, x, 8, C, s_in, 8, 1.0, 0.09, s_out, 8, 0.9, y, ldy, act, None)
    assert call(C=0) == -1 and b"feature width" in err()
    assert call(x=None) == -1 and b"NULL X/out" in err()
    assert call(s_out=X) == -1 and b"alias" in err()
    assert call(act=1) == -1 and b"GNX_ACT_NONE or GNX_ACT_SKIP_EMPTY" in err()
    assert call(s_in=ctypes.c_void_p(0x5000)) == -1 and b"in place" in err()
    assert call(s_in=None, act=0) == -1 and b"running sum" in err()
    assert call(d=None) == -1 and b"NULL degree scales" in err()
    assert call(y=S) == -1 and b"buffer of its own" in err()
    assert call(ldy=4) == -1 and b"buffer of its own" in err()
    assert call(p=-0.1) == -1 and b"dropout rate" in err()
    assert call() == -1 and b"NULL handle" in err() and b"gnx_spmm_dropped_back_bf16" in err()


def test_training_dtype_is_validated():
    import gnntf
    with pytest.raises(Exception, match="training_dtype"):
        gnntf.GNN.__init__(object.__new__(gnntf.GNN), None, None, training_dtype=torch.float16)


def test_ppr_loop_storage_is_checked_before_any_launch():
    from gnntf import sparse
    with pytest.raises(Exception, match="storage must be"):
        sparse.ppr_loop(lambda k, bwd=False: None, torch.zeros(2, 2), 0.1, 1, storage=torch.float16)
    W, R = sparse.BF16_TRAIN_MIN_WIDTH, sparse.BF16_TRAIN_MIN_ROWS
    assert isinstance(W, int) and W >= 1 and isinstance(R, int) and R >= 0
    # the allowance, on a stand-in for a DroppedAdjacency (no device): K = 0, relu, an adjacency that is no DroppedAdjacency, a
    # graph that is not square, widths below BF16_TRAIN_MIN_WIDTH and graphs below BF16_TRAIN_MIN_ROWS keep f32
    def adjacency(n_rows, n_cols):
        adj = object.__new__(sparse.DroppedAdjacency)
        adj.graph = types.SimpleNamespace(n_rows=n_rows, n_cols=n_cols)
        return adj
    big = adjacency(max(R, 1), max(R, 1))
    assert sparse._bf16_training_applies(big, 10, False, W) and sparse._bf16_training_applies(big, 1, False, W + 100)
    assert not sparse._bf16_training_applies(None, 0, False, W)
    assert not sparse._bf16_training_applies(big, 0, False, W)
    assert not sparse._bf16_training_applies(big, 10, True, W)
    assert not sparse._bf16_training_applies(object(), 10, False, W)
    assert not sparse._bf16_training_applies(adjacency(max(R, 1), max(R, 1) + 1), 10, False, W)
    if W > 1:
        assert not sparse._bf16_training_applies(big, 10, False, W - 1)
    if R > 1:
        assert not sparse._bf16_training_applies(adjacency(R - 1, R - 1), 10, False, W)

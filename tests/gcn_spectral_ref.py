"""numpy helpers for the fused GCNSpectralPreservingLayer (gnx_step_spectral_gcn, gnx_step_spectral_gcn_dropped,
sparse.gcn_step_spectral): the float64 reference, its derived bound, the float32 emulations the bound must admit and the operands of the
tests.  The any-order bounds are those of tests/gcn_fused_ref.py (forward_ref for P', backward_ref for the gradients), the gate-word
helpers, the masks and the backward's gate pass those of tests/gcnii_spectral_ref.py; both imported, neither edited.  numpy and scipy
only: imports without a GPU.

The layer (gcn.py:92-105):  agg = A . X,  P' = agg . W + b,  Y = act(P') - b,  out = 2 m s Y  -- m the keep mask, s the f32
1 / (1 - p) taken as it is (the kernels multiply by that float, so the reference does too, in float64).

The bound.  gcn_fused_ref.forward_ref(relu=False, p=0) gives P' and E, the first-order bound of a float32 evaluation of agg . W + b in
any order.  The layer's stated rounding points add, as in gcnii_spectral_ref:
    P^' = fl(P^ + b):        |P^' - P'| <= E + u |P'|            =: P_bound  (the bound of the pre-activation, and the gate's band)
    Y^  = fl(act(P^') - b):  |Y^ - Y|   <= P_bound + u |Y|       (act is 1-Lipschitz)
    Z^  = fl(Y^ s):          |Z^ - Y s| <= s (P_bound + u |Y|) + u s |Y|      (only where a mask scales: p > 0)
and the doubling is exact.  So
    out_bound = 2 s (P_bound + u |Y| + [p > 0] u |Y|),
zero error where the mask drops.  Nothing in it is taken from a kernel; tests/test_gcn_spectral_cpu.py holds the float32 emulations
("library", "sequential", "chunked") against it.

The gate.  ONE BIT of the forward is kept, P' > 0.  Against float64 the bit is decided wherever |P'| > P_bound; the share of the
elements inside the band may not exceed gcnii_spectral_ref.AMBIGUOUS_SHARE -- a condition on the operands below, asserted on the float64
reference alone in the CPU test.  The operands: gcn_fused_ref.operands with the bias drawn away from 0 (|b| in [0.05, 0.3), either
sign), so that a row without entries -- P' = b exactly -- is decided and carries both signs.

The criterion everywhere is  max |got - want| / bound <= 1."""
import numpy as np

import gcn_fused_ref as gref
import gcnii_spectral_ref as sref
from gcn_fused_ref import U32, f64, ratio, ratio_rows, regime_graph  # noqa: F401
from gcnii_spectral_ref import AMBIGUOUS_SHARE, gate_check, gate_pass_f32, gate_words, keep, pack_gate, scale, unpack_gate  # noqa: F401

FUSED_SHAPES = ((16, 16), (32, 32), (64, 64), (64, 40), (64, 33), (64, 7), (32, 1))      # (C_in, C_out) of the one launch, regime T
COMPOSED_SHAPES = ((24, 24), (16, 32))                                                   # the composition inside the entry, regime T
CASES = [("T",) + s for s in FUSED_SHAPES + COMPOSED_SHAPES] + [("S", 64, 40)]
RATES = (0.0, 0.5)


def operands(n, C_in, C_out):
    """gcn_fused_ref.operands (X, G, W; seeded by the shape) with bias = +-uniform[0.05, 0.3) as float32 [C_out], a generator of its
    own; read-only."""
    seed = 900 + 7 * C_in + C_out
    out = dict(gref.operands(n, C_in, C_out, seed))
    rng = np.random.default_rng(seed + 77)
    bias = (rng.uniform(0.05, 0.3, size=C_out) * rng.choice([-1.0, 1.0], size=C_out)).astype(np.float32)
    if C_out >= 2:                                         # both signs, whatever the draw
        bias[0], bias[1] = abs(bias[0]), -abs(bias[1])
    bias.setflags(write=False)
    out["bias"] = bias
    return out


def act(x, relu):
    return np.maximum(x, 0) if relu else x


def spectral_ref(A, X, W, bias, relu, p=0.0, mask=None, L=None):
    """float64: dict(agg, agg_bound, P (= P'), P_bound, out, out_bound) -- see the module docstring.  ``bias`` None: zeros.
    ``mask``: bool [n, C_out] (None: all kept)."""
    fwd = gref.forward_ref(A, X, W, bias, False, L=L)
    P = fwd["P"]
    b = np.zeros(P.shape[1]) if bias is None else f64(bias).reshape(1, -1)
    P_bound = fwd["out_bound"] + U32 * np.abs(P)
    Y = act(P, relu) - b
    s = float(scale(p))
    m = np.ones(P.shape) if mask is None else f64(mask)
    scaled = 1.0 if p != 0 else 0.0
    return dict(agg=fwd["agg"], agg_bound=fwd["agg_bound"], P=P, P_bound=P_bound, out=2.0 * s * m * Y,
                out_bound=2.0 * s * (P_bound + (1.0 + scaled) * U32 * np.abs(Y)))


def spectral_f32(A32, X, W, bias, relu, order, L, p=0.0, mask=None):
    """(agg, P', out) of the layer in float32 under ``order`` (gcn_fused_ref.forward_f32), every operation rounded once, at the stated
    rounding points: + bias, the activation, - bias, the mask's scale, the doubling."""
    agg, P = gref.forward_f32(A32, X, W, bias, False, order, L)
    b = np.zeros((1, P.shape[1]), dtype=np.float32) if bias is None else np.asarray(bias, dtype=np.float32).reshape(1, -1)
    Y = (act(P, relu) - b).astype(np.float32)
    if p != 0:
        Y = np.where(mask, Y * scale(p), np.float32(0)).astype(np.float32)
    return agg, P, (np.float32(2) * Y).astype(np.float32)


def backward_ref(A, agg32, G32, terms32, W, L=None):
    """float64 over the float32 data the launches hold (the kept rows agg32, the gated gradient G32 and the bias gradient's terms of
    gate_pass_f32): gcn_fused_ref.backward_ref's dX and dW with their any-order bounds, and dbias = the column sums of the terms with
    the bound of a float32 sum of n terms in any order."""
    want = gref.backward_ref(A, agg32, G32, W, L=L)
    db, db_bound = sref.column_sum_ref(terms32)
    return dict(dX=want["dX"], dX_bound=want["dX_bound"], dW=want["dW"], dW_bound=want["dW_bound"], db=db, db_bound=db_bound)


def saved_bytes(n, C_in, C_out, relu=True):
    """What the fused node saves per layer: A . X and W as float32 and, with the relu, one bit per element in whole int32 words."""
    return 4 * n * C_in + 4 * C_in * C_out + (4 * n * gate_words(C_out) if relu else 0)

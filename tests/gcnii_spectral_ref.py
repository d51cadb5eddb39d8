"""numpy helpers for the fused GCNIISpectralPreservingLayer (gnx_gcnii_step_spectral, gnx_gcnii_spectral_back): the float64 reference,
its derived bound, the float32 emulations the bound must admit, the gate-bit layout and the float64 backward.  Graphs, operands and the
first-order terms are those of tests/gcnii_shapes_ref.py; the masks are the oracle's.  numpy and scipy only: imports without a GPU.

The layer:  P' = T . M + bias,  Y = act(P') - bias,  out = 2 m s Y  with T = beta A H + alpha H0, m the keep mask and s the f32
1 / (1 - p) taken as it is (the kernels multiply by that float, so the reference does too, in float64).

The bound.  forward_ref's out_bound E covers the float32 evaluation of T . M in any order.  The layer adds two rounded operations:
    P^' = fl(P^ + b):      |P^' - P'| <= E + u |P'|                 =: P_bound (the forward bound of the pre-activation)
    Y^  = fl(act(P^') - b): |Y^ - Y|  <= P_bound + u |Y|             (act is 1-Lipschitz)
and the scaling by s and the doubling, which multiply the error by 2 s (the rounding of Y s itself, u |Y| s, is second order against
the C + 6 terms E already counts and gets no term of its own).  So
    out_bound = 2 s (E + u |P'| + u |Y|),
zero error where the mask drops.  Nothing in it is taken from a kernel; tests/test_gcnii_spectral_cpu.py holds the float32 emulations
of gcnii_shapes_ref ("library", "sequential", "chunked") against it.

The gate.  The kernels keep ONE BIT of the forward, P' > 0.  Against float64 the bit is decided wherever |P'| > P_bound; the elements
inside the band may fall either way and are left out (their share is asserted: at most 0.1 %)."""
import functools

import numpy as np

import gcnii_shapes_ref as ref
from oracle import gnntf_oracle as orc

U32 = ref.U32
AMBIGUOUS_SHARE = 1e-3                                 # the share of the matrix the gate comparison may leave out


def scale(p):
    """The f32 scale of the dropout as the kernels form it: 1.0f / (1.0f - (float)p)."""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


@functools.lru_cache(maxsize=None)
def keep(seed, stream, p, n, C):
    """The keep mask [n, C] of (seed, stream) at rate p, from the oracle: element (i, c) is entry (i, c) with duplicate rank 0."""
    if p == 0:
        m = np.ones((n, C), dtype=bool)
    else:
        idx = np.stack([np.repeat(np.arange(n), C), np.tile(np.arange(C), n)], axis=1)
        m = np.asarray(orc.keep_mask(idx, p, seed, stream)).reshape(n, C)
    m.setflags(write=False)
    return m


def operands(n, C, seed):
    """gcnii_shapes_ref.operands plus bias = 0.5 N(0, 1) as float32 [C] (a generator of its own: the other operands keep their draws)."""
    out = dict(ref.operands(n, C, seed))
    bias = (0.5 * np.random.default_rng(seed + 77).standard_normal(C)).astype(np.float32)
    bias.setflags(write=False)
    out["bias"] = bias
    return out


def act(x, relu):
    return np.maximum(x, 0) if relu else x


def spectral_ref(A, H, H0, M, bias, a, relu, p=0.0, mask=None, L=None):
    """float64: dict(T, T_bound, P (= P'), P_bound, out, out_bound) -- see the module docstring.  ``mask``: bool [n, C] (None: all kept)."""
    n, C = H.shape
    fwd = ref.forward_ref(A, H, H0, M, a, False, L)
    b = ref.f64(bias)[None, :]
    P = fwd["out"] + b
    P_bound = fwd["out_bound"] + U32 * np.abs(P)
    Y = act(P, relu) - b
    s = float(scale(p))
    m = np.ones((n, C)) if mask is None else ref.f64(mask)
    return dict(T=fwd["T"], T_bound=fwd["T_bound"], P=P, P_bound=P_bound, out=2.0 * s * m * Y, out_bound=2.0 * s * (P_bound + U32 * np.abs(Y)))


def spectral_f32(A32, H, H0, M, bias, a, relu, order, L, p=0.0, mask=None):
    """(T, P', out) of the layer in float32 under ``order`` (gcnii_shapes_ref.forward_f32), every operation rounded once."""
    T, P = ref.forward_f32(A32, H, H0, M, a, False, order, L)
    b = np.asarray(bias, dtype=np.float32)[None, :]
    P = (P + b).astype(np.float32)
    Y = (act(P, relu) - b).astype(np.float32)
    if p != 0:
        Y = np.where(mask, Y * scale(p), np.float32(0)).astype(np.float32)
    return T, P, (np.float32(2) * Y).astype(np.float32)


# ---- the gate words: bit c & 31 of word row * ceil(C / 32) + (c >> 5) (include/gnx.h) -----------------------------------------------------
def gate_words(C):
    return (C + 31) // 32


def pack_gate(bits):
    """bool [n, C] -> the words as int32 [n, ceil(C / 32)] (what torch holds), pad bits 0."""
    n, C = bits.shape
    W = gate_words(C)
    padded = np.zeros((n, 32 * W), dtype=np.uint64)
    padded[:, :C] = bits
    words = (padded.reshape(n, W, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)
    return words.view(np.int32)


def unpack_gate(words, C):
    """int32 / uint32 [n, ceil(C / 32)] -> (bool [n, C], bool: every pad bit is 0)."""
    w = np.ascontiguousarray(words).view(np.uint32)
    n, W = w.shape
    assert W == gate_words(C)
    every = ((w[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).reshape(n, 32 * W)
    return every[:, :C], not every[:, C:].any()


def gate_check(bits, P, P_bound):
    """(wrong, share): the decided elements (|P'| > P_bound) whose bit is not P' > 0, and the share of the matrix left undecided."""
    decided = np.abs(P) > P_bound
    return int((decided & (bits != (P > 0))).sum()), float(1.0 - decided.mean())


# ---- the backward ----------------------------------------------------------------------------------------------------------------------
def gate_pass_f32(g, bits, p, mask):
    """G' of gnx_gcnii_spectral_back in float32, bit for bit: gate ? 2 (kept ? g s : 0) : 0 (``bits`` None: the identity, G' = u), and
    the terms of the bias gradient, -(gate ? 0 : u)."""
    g = np.asarray(g, dtype=np.float32)
    u = np.float32(2) * (np.where(mask, g * scale(p), np.float32(0)) if mask is not None else g * scale(p)).astype(np.float32)
    if bits is None:
        return u, np.zeros_like(u)
    return np.where(bits, u, np.float32(0)), np.where(bits, np.float32(0), -u)


def column_sum_ref(terms):
    """(the float64 column sums, the bound of a float32 sum of the n terms in any order: (n + 2) u sum |term|)."""
    t = ref.f64(terms)
    return t.sum(axis=0), (len(t) + 2) * U32 * np.abs(t).sum(axis=0)


def wgrad_ref(T, G):
    """dM = T^T G in float64 over the float32 T and G' the launches hold, and the any-order bound (n + 2) u |T|^T |G'|."""
    T, G = ref.f64(T), ref.f64(G)
    return T.T @ G, (len(T) + 2) * U32 * (np.abs(T).T @ np.abs(G))

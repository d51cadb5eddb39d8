"""bf16 emulation for the tests of the opt-in bf16 storage (numpy, CPU): round to nearest even on the f32 bits, NaN kept a NaN,
overflow to infinity -- what a plain f32 -> bf16 cast does -- and the APPNP recurrence with the bf16 roundings at the points where
gnx_appnp_propagate_bf16 rounds, its sums in float64."""
import numpy as np

U = 2.0 ** -8                     # bf16 unit roundoff


def bf16_bits(x) -> np.ndarray:
    """uint16 bit patterns of bf(x) for float32 (or wider: first rounded to float32) input."""
    x = np.asarray(x, dtype=np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)     # RNE; a carry out of the largest finite values gives inf
    nan = np.isnan(x)
    r[nan] = ((u[nan] >> 16) | 0x0040).astype(np.uint16)            # NaN stays NaN (quiet bit set: never rounds to inf / zero)
    return r


def bf16_decode(bits) -> np.ndarray:
    """float32 values of uint16 bf16 bit patterns (exact)."""
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def bf16_round(x) -> np.ndarray:
    """bf(x) as float32."""
    return bf16_decode(bf16_bits(x))


def appnp_bf16(A, H0, a, K, relu=False, diag=None):
    """The bf16 K-loop in float64 arithmetic: H~_0 = bf(H0); H_{k+1} = act((1-a)(A H~_k + diag H~_k) + a H0); H~_{k+1} = bf(H_{k+1})
    for k < K-1; returns H_K (float64).  ``A``: a scipy sparse matrix (any value dtype)."""
    H0 = np.asarray(H0, dtype=np.float32)
    if K == 0:
        return H0.astype(np.float64)
    A = A.astype(np.float64)
    beta = float(np.float32(1.0 - float(a)))
    Ht = bf16_round(H0).astype(np.float64)
    H = None
    for k in range(K):
        S = A @ Ht
        if diag is not None:
            S = S + np.asarray(diag, dtype=np.float64)[:, None] * Ht
        H = beta * S + float(np.float32(a)) * H0.astype(np.float64)
        if relu:
            H = np.maximum(H, 0.0)
        if k < K - 1:
            Ht = bf16_round(H).astype(np.float64)
    return H

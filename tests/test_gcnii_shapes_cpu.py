"""tests/gcnii_shapes_ref.py without a GPU: the builder keeps its promises, float32 evaluations of the GCNII forward and backward in
three summation orders stay within the derived bound, and every mutant of a correct float32 result -- the defects the GPU tests of
tests/test_gpu_gcnii_shapes.py are there to catch -- exceeds it on the rows it touches.  The second half is what makes the bound a
test and not a formality.  The weights are the raw values (uniform in [0.5, 1.5)); the printed ratios are recorded in
profiles/NOTES.md, "GCNII at every long-row regime"."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import gcnii_shapes_ref as ref
from bf16_ref import bf16_round
from oracle import gnntf_oracle as orc

A_MIX = 0.1
WIDTHS = (16, 64)
ORDERS = ("library", "sequential", "chunked")


@functools.lru_cache(maxsize=None)
def graph(name, seed=0):
    coo, vals, shape, info = ref.regime_graph(name, seed)
    return dict(A32=ref.csr_of(coo, vals, shape, np.float32), A=ref.csr_of(coo, vals, shape), n=shape[0], info=info, L=info["L"], coo=coo)


@functools.lru_cache(maxsize=None)
def forward_case(name, C, relu=False):
    """The operands, the float64 reference and ONE correct float32 result (the chunked order: the one closest to the kernels)."""
    g = graph(name)
    op = ref.operands(g["n"], C, seed=C)
    want = ref.forward_ref(g["A"], op["H"], op["H0"], op["M"], A_MIX, relu)
    T, out = ref.forward_f32(g["A32"], op["H"], op["H0"], op["M"], A_MIX, relu, "chunked", g["L"])
    return op, want, T, out


@functools.lru_cache(maxsize=None)
def backward_case(name, C):
    g = graph(name)
    op = ref.operands(g["n"], C, seed=C)
    want = ref.backward_ref(g["A"], op["G"], op["Mt"], A_MIX, op["S_in"], 0.5)
    dH, S = ref.backward_f32(g["A32"], op["G"], op["Mt"], A_MIX, op["S_in"], 0.5, "chunked", g["L"])
    return op, want, dH, S


# ---- the builder ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("name", ["T", "S"])
def test_builder_keeps_its_promises(name, seed):
    n, L, n_hub = ref.REGIMES[name]
    coo, vals, shape, info = ref.planted_graph(n, L, n_hub, seed)                    # (asserts the lengths, the hub count, the columns)
    assert shape == (n, n) and vals.dtype == np.float32 and 0.5 <= vals.min() and vals.max() < 1.5
    assert len(np.unique(coo[:, 0] * n + coo[:, 1])) == len(coo)
    assert not (np.diff(coo[:, 0] * n + coo[:, 1]) > 0).all()                        # shuffled
    deg = np.bincount(coo[:, 0], minlength=n)
    for d in ref.planted_lengths(L):
        assert len(info["rows_of"][d]) >= 1 and all(deg[r] == d for r in info["rows_of"][d])
    assert len(info["hub"]) == 4 + n_hub and 0 in info["hub"] and n - 1 in info["hub"]
    assert len(info["hub"]) > (16 if name == "T" else 128)                           # more than one MFMA tile / one block of the dense kernel
    assert n % 16 != 0 and np.intersect1d(info["hub"], info["ragged"]).size >= 1
    assert (deg[16:32] == 0).all() and deg[n // 2] == 0
    assert np.bincount(coo[:, 1], minlength=n).max() <= L
    assert ref.plan_threshold(n) == L
    rest = np.setdiff1d(np.arange(n), info["planted"])
    assert 5 * n < deg[rest].sum() < 7 * n and deg[rest].max() < L - 1


def test_boundary_graph_is_one_graph_on_both_sides():
    below, above = (ref.boundary_graph(n) for n in ref.BOUNDARY_NS)
    assert np.array_equal(below[0], above[0]) and np.array_equal(below[1], above[1])
    assert below[2] == (2 ** 15 - 1,) * 2 and above[2] == (2 ** 15,) * 2
    assert ref.plan_threshold(below[2][0]) == 512 > ref.BOUNDARY_LEN > ref.plan_threshold(above[2][0]) == 128
    assert below[0].max() < 2 ** 15 - 1


# ---- float32 evaluations meet the bound ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("name", ["T", "S"])
def test_float32_emulations_meet_the_bound(name, C, capsys):
    g = graph(name)
    op = ref.operands(g["n"], C, seed=C)
    worst = {}
    wants = {relu: ref.forward_ref(g["A"], op["H"], op["H0"], op["M"], A_MIX, relu) for relu in (False, True)}
    backs = {s_alpha: ref.backward_ref(g["A"], op["G"], op["Mt"], A_MIX, op["S_in"], s_alpha) for s_alpha in (1.0, 0.5)}
    for order in ORDERS:
        T, plain = ref.forward_f32(g["A32"], op["H"], op["H0"], op["M"], A_MIX, False, order, g["L"])
        for relu, want in wants.items():                            # (the activation is the last step: one evaluation serves both)
            out = np.maximum(plain, np.float32(0)) if relu else plain
            worst["T", order] = max(worst.get(("T", order), 0), ref.ratio(T, want["T"], want["T_bound"]))
            worst["out", order] = max(worst.get(("out", order), 0), ref.ratio(out, want["out"], want["out_bound"]))
        dH, own = ref.backward_f32(g["A32"], op["G"], op["Mt"], A_MIX, None, 1.0, order, g["L"])
        for s_alpha, want in backs.items():                         # (S = s_alpha S_in + the row's own product, as backward_f32 adds them)
            S = np.float32(s_alpha) * op["S_in"] + own
            worst["dH", order] = max(worst.get(("dH", order), 0), ref.ratio(dH, want["dH"], want["dH_bound"]))
            worst["S", order] = max(worst.get(("S", order), 0), ref.ratio(S, want["S"], want["S_bound"]))
        # rows nothing points at: exactly zero
        assert (dH[g["info"]["no_in"]] == 0).all() and (backs[0.5]["dH_bound"][g["info"]["no_in"]] == 0).all()
    with capsys.disabled():
        print(f"\n[gcnii shapes, CPU float32, regime {name}, C={C}] error / bound: "
              + ", ".join(f"{what} {order} {value:.3f}" for (what, order), value in sorted(worst.items())))
    assert max(worst.values()) <= 1.0, worst
    assert min(worst.values()) > 0.01                                                # ... and the bound is not orders of magnitude loose


# ---- mutants exceed it ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("name", ["T", "S"])
def test_mutant_one_entry_dropped(name, C, capsys):
    """Every planted length (and the hub rows at ids 0 and n - 1): the row's result without ONE of its entries."""
    g = graph(name)
    op, want, T, out = forward_case(name, C)
    beta = np.float32(1.0 - A_MIX)
    A32, rows_of = g["A32"], g["info"]["rows_of"]
    margins = {}
    for d in ref.planted_lengths(g["L"])[1:] + (-1, -2):
        r = {-1: 0, -2: g["n"] - 1}[d] if d < 0 else rows_of[d][0]
        e = A32.indptr[r] + (A32.indptr[r + 1] - A32.indptr[r]) // 2                  # the middle entry
        T_row = T[r] - beta * A32.data[e] * op["H"][A32.indices[e]]
        out_row = ref.matmul_f32(T_row[None], op["M"], "sequential")
        margins[d] = (ref.ratio(T_row[None], want["T"][r:r + 1], want["T_bound"][r:r + 1]),
                      ref.ratio(out_row, want["out"][r:r + 1], want["out_bound"][r:r + 1]))
        assert ref.ratio(out[r:r + 1], want["out"][r:r + 1], want["out_bound"][r:r + 1]) <= 1          # the unmutated row passes
    with capsys.disabled():
        print(f"\n[gcnii shapes, mutant 'one entry dropped', regime {name}, C={C}] error / bound of (T, out) per planted length: "
              + ", ".join(f"{d}: {t:.0f} / {o:.0f}" for d, (t, o) in margins.items()))
    assert all(t > 1 and o > 1 for t, o in margins.values()), margins


@pytest.mark.parametrize("name", ["T", "S"])
def test_mutant_boundary_row_unwritten_or_written_twice(name):
    """The row of exactly L entries, where the plan's d > L and the kernels' end - beg <= L must agree: taken by neither path (the
    buffer's NaN stays) or by both (here: its sum added twice)."""
    g = graph(name)
    for C in WIDTHS:
        op, want, T, out = forward_case(name, C)
        r = g["info"]["rows_of"][g["L"]][0]
        for mutant in (np.full((1, C), np.nan, dtype=np.float32), 2 * out[r:r + 1]):
            assert ref.ratio(mutant, want["out"][r:r + 1], want["out_bound"][r:r + 1]) > 1
        whole = out.copy()
        whole[r] = np.nan
        assert ref.ratio(whole, want["out"], want["out_bound"]) == np.inf             # ... and the criterion over all rows sees it
        assert ref.ratio(out, want["out"], want["out_bound"]) <= 1


@pytest.mark.parametrize("name", ["T", "S"])
def test_mutant_untransposed_backward(name):
    """A walked where A^T belongs."""
    g = graph(name)
    for C in WIDTHS:
        op, want, dH, S = backward_case(name, C)
        wrong, _ = ref.backward_f32(sp.csr_matrix(g["A32"].T), op["G"], op["Mt"], A_MIX, None, 1.0, "chunked", g["L"])
        rows = ref.ratio_rows(wrong, want["dH"], want["dH_bound"])
        differs = np.flatnonzero(np.diff(g["A"].indptr) + g["info"]["in_deg"] > 0)    # rows with an entry in A or in A^T
        assert (rows[differs] > 1).all() and rows[g["info"]["hub"]].min() > 100
        assert ref.ratio(dH, want["dH"], want["dH_bound"]) <= 1


@pytest.mark.parametrize("name", ["T", "S"])
def test_mutant_hub_list_shifted_by_one(name):
    """Row long_rows[i] receives the result of row long_rows[i + 1]: an off-by-one between a row-list pass and the list."""
    g = graph(name)
    hub = g["info"]["hub"]
    for C in WIDTHS:
        op, want, T, out = forward_case(name, C)
        shifted = out.copy()
        shifted[hub] = out[np.roll(hub, -1)]
        rows = ref.ratio_rows(shifted, want["out"], want["out_bound"])
        assert (rows[hub] > 1).all() and np.delete(rows, hub).max() <= 1


@pytest.mark.parametrize("name", ["T", "S"])
def test_mutant_running_sum_from_rounded_gradient(name):
    """S from bf(G): what the bf16 backward must NOT do (the row's own product reads the f32 G)."""
    g = graph(name)
    for C in WIDTHS:
        op, want, dH, S = backward_case(name, C)
        _, rounded = ref.backward_f32(g["A32"], bf16_round(op["G"]), op["Mt"], A_MIX, op["S_in"], 0.5, "chunked", g["L"])
        assert (ref.ratio_rows(rounded, want["S"], want["S_bound"]) > 1).all()
        assert ref.ratio(S, want["S"], want["S_bound"]) <= 1


def keep_mask(p, rows, C, seed=7, stream=2):
    """kept iff hash_u24(seed, stream, row, col, 0) >= dropout_threshold(p), for the row ids ``rows``."""
    r, c = np.repeat(np.asarray(rows, dtype=np.int64), C), np.tile(np.arange(C), len(rows))
    return (orc.hash_u24(seed, stream, r, c, np.zeros(len(r), dtype=np.int64)) >= orc.dropout_threshold(p)).reshape(len(rows), C)


@pytest.mark.parametrize("name", ["T", "S"])
def test_mutant_mask_keyed_by_slot(name):
    """The mask hashed with a row's SLOT in the launch order (where its tile sits) instead of its id."""
    g = graph(name)
    n, p = g["n"], 0.6
    scale = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    order = ref.degree_order(np.diff(g["A"].indptr), g["L"])
    assert sorted(order) == list(range(n))
    slot_of = np.empty(n, dtype=np.int64)
    slot_of[order] = np.arange(n)
    for C in WIDTHS:
        op, want, T, out = forward_case(name, C)
        right, wrong = keep_mask(p, np.arange(n), C), keep_mask(p, slot_of, C)
        want_out = np.where(right, want["out"] * float(scale), 0.0)
        bound = want["out_bound"] * float(scale) + ref.U32 * np.abs(want_out)           # one more rounding: the scaling
        assert ref.ratio(np.where(right, out * scale, np.float32(0)), want_out, bound) <= 1
        rows = ref.ratio_rows(np.where(wrong, out * scale, np.float32(0)), want_out, bound)
        moved = np.flatnonzero(slot_of != np.arange(n))
        assert len(moved) > n // 2 and (rows[moved] > 1).mean() > 0.99 and (rows[np.intersect1d(moved, g["info"]["hub"])] > 1).all()
        assert (rows[slot_of == np.arange(n)] <= 1).all()

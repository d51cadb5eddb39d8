"""CPU checks of tests/spmm_bf16_forms_ref.py: the operand layouts force the vector width they claim under the restated pick_vec of
Bf16RowsT, the launch table of tests/test_gpu_spmm_bf16_forms.py covers every entry x result type x row class x vector width and
every option value, the float64 bound and the bf16 interval criterion admit float32 sums of bf16-exact operands in two orders
(sharply: at least 90 % of the intervals are a single bf16 value), and both reject planted mistakes at every structure."""
import numpy as np
import pytest
import scipy.sparse as sp

import spmm_bf16_forms_ref as B
import spmm_forms_ref as R
from bf16_ref import bf16_bits, bf16_decode, bf16_round

C_CPU = 8                                           # the emulations walk every entry in Python-level steps: a narrow operand
SID = lambda k: f"{k[0]}a{'r' if k[1] else 's'}"


def _case(key, h0_form="full", diag=False, relu=False, seed=0):
    st = B.structure(*key)
    A, deg, L = st["A"], st["deg"], st["L"]
    if key[0] == "L":                               # as on the GPU: the hub rows, the planted rows and a few thousand others
        sel = B.l_sample(st, 1)
        A, deg = A[sel], deg[sel]
    rng = np.random.default_rng([seed, 5])
    _, x = B.bf16_normal(rng, (A.shape[1], C_CPU))
    full = rng.standard_normal((A.shape[0], C_CPU), dtype=np.float32)
    h0_rows = None if h0_form == "none" else full if h0_form == "full" else np.broadcast_to(full[:1], full.shape)
    d = rng.uniform(0.5, 1.5, size=A.shape[0]).astype(np.float32) if diag else None
    return dict(st=st, A=A, deg=deg, L=L, x=x, full=full, h0_rows=h0_rows, d=d, relu=relu, ref=R.reference(A, deg, L, x, h0_rows, d, relu=relu))


# ---- helpers ---------------------------------------------------------------------------------------------------------------------------
def test_bf_is_the_f32_cast_where_both_apply():
    rng = np.random.default_rng(0)
    x = (rng.standard_normal(200000) * 10.0 ** rng.integers(-30, 30, 200000)).astype(np.float32)
    # ties between two bf16 values (the low half exactly 0x8000) over an even and over an odd kept part, and their neighbours
    ties = np.array([0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001, 0xBF808000, 0xBF818000, 0x3FFF8000, 0x407F8000,
                     0x00808000, 0x7E7F8000], dtype=np.uint32).view(np.float32)
    x = np.concatenate([x, ties, [0.0, -0.0, 1.0, -1.0]]).astype(np.float32)
    assert (B.bf(x.astype(np.float64)) == bf16_decode(bf16_bits(x)).astype(np.float64)).all()
    assert B.bf(np.float64(np.float32(1.00390625))) == 1.0 and B.bf(1.01171875) == 1.015625          # 1 + 2^-8 -> even, 1 + 3 * 2^-8 -> even
    # straight from float64: a value just above a tie that float32 would first round ONTO the tie
    v = 1.0 + 2.0 ** -8 + 2.0 ** -40
    assert np.float32(v) == np.float32(1.0 + 2.0 ** -8) and B.bf(v) == 1.0 + 2.0 ** -7 and bf16_round(np.array([v]))[0] == 1.0
    assert (B.bf_truncated(np.array([1.0078, -1.0078, 3.999])) == np.array([1.0, -1.0, 3.984375])).all()
    with pytest.raises(AssertionError):
        B.bf(1e-40)
    assert bf16_decode(bf16_bits(np.array([B.SENTINEL])))[0] == B.SENTINEL and float(B.SENTINEL) == -12288.0
    assert np.isnan(bf16_decode(np.array([B.BF16_NAN]))).all()
    buf, view = B.window(np.ones((3, 5), dtype=np.uint16), 4, 2, B.BF16_NAN)
    assert buf.dtype == np.uint16 and buf.shape == (3, 9) and (buf[:, :2] == B.BF16_NAN).all() and (buf[:, 7:] == B.BF16_NAN).all() and (view == 1).all()


def test_structures():
    for key in B.STRUCTURES:
        st = B.structure(*key)
        n, n_cols = st["shape"]
        assert n == (1547 if key[0] == "T" else 2 ** 15 + 11) and n_cols == n + (R.EXTRA_COLS if key[1] else 0)
        assert st["L"] == (512 if key[0] == "T" else 128) and (st["deg"] > st["L"]).any() and (st["deg"] == 0).sum() >= 3
    st = B.structure("L", False)
    n, L, deg = st["shape"][0], st["L"], st["deg"]
    assert n == st["shape"][1] == 2 ** 20 + 11 >= B.SMALL_ROWS and L == 512
    assert all((deg == d).any() for d in (0, L - 1, L, L + 1, 2 * L + 1)) and 0 < (deg > L).sum() < 16
    rows = B.l_sample(st, 1)
    assert set(st["info"]["hub"]) <= set(rows) and set(st["info"]["planted"]) <= set(rows) and B.L_RANDOM_ROWS <= len(rows) <= B.L_RANDOM_ROWS + 32


# ---- layouts and dispatch ----------------------------------------------------------------------------------------------------------------
def test_expected_vec_restates_pick_vec():
    ev = B.expected_vec_bf16
    assert ev(128, (128, 128, 128), (0, 0, 0), True) == 8 and ev(128, (128, None, 128), (0, None, 0), False) == 8
    assert ev(128, (128, 0, 128), (0, 0, 0), True) == 8                                      # ldh0 = 0 divides everything
    assert ev(128, (132, 128, 128), (0, 0, 0), True) == 4 and ev(128, (128, 130, 128), (0, 0, 0), True) == 2 and ev(128, (128, 128, 129), (0, 0, 0), True) == 1
    # the same element offset, different widths per operand: 4 elements into X or a bf16 out (8 bytes) allow 4; into an f32 operand
    # (16 bytes) they allow 8
    assert ev(128, (128, 128, 128), (8, 0, 0), True) == 4 and ev(128, (128, 128, 128), (0, 0, 8), True) == 4
    assert ev(128, (128, 128, 128), (0, 0, 0), False) == 8 and ev(128, (128, 128, 128), (0, 0, 8), False) == 2
    assert ev(128, (128, 128, 128), (0, 8, 0), True) == 2 and ev(128, (128, 128, 128), (0, 4, 0), True) == 1
    assert ev(128, (128, 128, 128), (4, 0, 0), True) == 2 and ev(128, (128, 128, 128), (2, 0, 0), True) == 1
    assert ev(128, (128, 128, 128), (0, 0, 4), True) == 2 and ev(128, (128, 128, 128), (0, 0, 4), False) == 1
    assert ev(12, (16, 16, 16), (0, 0, 0), True) == 4 and ev(7, (8, 8, 8), (0, 0, 0), True) == 1
    # no 16-byte aligned f32 operand forces 4 over 8: resolve_breaker knows
    assert B.resolve_breaker(4, 4, "full", True) == (1, 0) and B.resolve_breaker(4, 5, "full", False) == (2, 0) and B.resolve_breaker(4, 5, "full", True) == (2, 1)
    assert B.resolve_breaker(2, 4, "full", True) == (1, 1) and B.resolve_breaker(2, 1, "bias", True) == (0, 0) and B.resolve_breaker(2, 4, "bias", True) == (1, 1)
    assert B.resolve_breaker(4, 4, "bias", True) == (0, 1) and B.resolve_breaker(1, 4, "none", True) == (0, 1)


def test_layouts_force_the_vector_width():
    seen, forced_by = set(), set()
    for s in B.launch_table():
        what = B.launch_id(s)
        lds, offs = B.geometry(s)
        assert B.expected_vec_bf16(s["C"], lds, offs, s["out_bf16"]) == s["vec"], what
        assert B.row_class(s["C"], s["vec"]) == s["cls"]
        # the f32-result launch a bf16 result is tied to picks the same width over the same X and H0 windows
        lds32, offs32 = B.geometry(dict(s, out_bf16=False), s["lay_f32"])
        assert B.expected_vec_bf16(s["C"], lds32, offs32, False) == s["vec"] and s["lay_f32"][:2] == s["lay"][:2], what
        if B.forcible(s["vec"], s["C"]):
            # exactly one reason: the neutral layout allows more, and so does undoing the pushed operand alone
            neutral = B.geometry(s, B.layouts_for_bf16(8, 8 * s["C"], 0, s["out_bf16"]))
            assert B.expected_vec_bf16(s["C"], neutral[0], neutral[1], s["out_bf16"]) >= 2 * s["vec"], what
            forced_by.add(B.resolve_breaker(s["vec"], s["breaker"], s["h0"], s["out_bf16"]) + (s["vec"],))
        for (pad, off) in s["lay"]:
            assert 0 <= off <= pad
        seen.add((lds[0] % 8, lds[2] % 8, offs[0], offs[2], None if lds[1] is None else lds[1] % 8, offs[1], s["out_bf16"]))
    assert len(seen) >= 12, len(seen)                                                        # the reason a width is chosen varies
    # every operand forces a width through its leading dimension and through its first byte; an f32 operand's first byte only below 4
    assert {(w, t) for w, t, _ in forced_by} == {(w, t) for w in range(3) for t in range(2)}, forced_by
    assert {v for _, _, v in forced_by} == {4, 2, 1}
    assert (1, 1, 4) not in forced_by and (0, 1, 4) in forced_by and (2, 1, 4) in forced_by


def test_launch_table_coverage():
    table = B.launch_table()
    assert len(table) <= 220 and len({B.launch_id(s) for s in table}) == len(table)
    assert len(B.REACHABLE) == 20 and set(B.REACHABLE) == {(c, v) for c in B.CLASSES for v in B.VECS}
    assert {C for C, _ in B.COMBOS} == set(B.WIDTHS)
    main = [s for s in table if s["regime"] != "L"]
    for entry in B.ENTRIES:
        for out_bf16 in (False, True):
            rows = [s for s in main if s["entry"] == entry and s["out_bf16"] == out_bf16]
            assert {(s["cls"], s["vec"]) for s in rows} == set(B.REACHABLE), (entry, out_bf16)
            assert {s["C"] for s in rows} == set(B.WIDTHS)
            for cls in B.CLASSES:
                in_cls = [s for s in rows if s["cls"] == cls]
                assert {s["h0"] for s in in_cls} == set(B.H0_FORMS), (entry, out_bf16, cls)
                assert {s["relu"] for s in in_cls} == {False, True}, (entry, out_bf16, cls)
                assert {s["skip"] for s in in_cls} == {False, True}, (entry, out_bf16, cls)
                assert {s["diag"] for s in in_cls} == ({False, True} if entry == "spmm" else {False}), (entry, out_bf16, cls)
            assert {s["regime"] for s in rows} == {"T", "S"} and {s["rect"] for s in rows} == {False, True}
            assert {(s["regime"], s["rect"]) for s in rows} == {(r, q) for r in "TS" for q in (False, True)}
    assert all(s["kind"] == "a" for s in table) and all(not (s["diag"] and s["rect"]) for s in table)
    assert any(s["diag"] and s["skip"] for s in table)                                       # the skip flag ignored under a diagonal
    assert all(s["regime"] == "T" for s in main if s["C"] > B.T_ONLY_ABOVE)
    # the L launches
    big = [s for s in table if s["regime"] == "L"]
    assert 4 <= len(big) <= 8 and all(s["C"] <= 40 and not s["diag"] and not s["rect"] for s in big)
    lanes = [-(-s["C"] // s["vec"]) for s in big]
    assert any(n <= 4 for n in lanes) and any(4 < n <= 8 for n in lanes) and {s["cls"] for s in big} == {"g8", "g16", "g32"}
    assert {s["vec"] for s in big} == {8, 4, 2} and {s["entry"] for s in big} == set(B.ENTRIES) and {s["out_bf16"] for s in big} == {False, True}
    assert {s["h0"] for s in big} == set(B.H0_FORMS) and {s["skip"] for s in big} == {False, True}
    # the names the GPU test must see over the whole table, from the dispatch rule
    names = predicted_names(table)
    stems = {"spmm_wave", "spmm_group32", "spmm_group16", "spmm_group8"}
    assert {n.split("+")[0].replace("_bf16", "") for n in names} >= stems
    assert {"spmm_" + g + "+chunks_bf16" for g in ("group32", "group16", "group8", "group4")} <= names
    assert {"spmm_wave+long_bf16", "spmm_group32+long_bf16", "spmm_group16+long_bf16", "spmm_group8+long_bf16"} <= names
    assert {n for s, n in zip(table, predicted_list(table)) if s["regime"] == "L"} == {"spmm_" + g + "+long_bf16" for g in ("group32", "group16", "group8")}
    # the bare class is what a structure without hub rows reports (the table has none: the bf16 entries walk kind "a" only)
    assert {B.kernel_name_bf16(C, v, 1547, 0) for C, v in B.COMBOS} == {s + "_bf16" for s in stems}
    assert B.kernel_name_bf16(24, 8, B.SMALL_ROWS - 1, 3) == "spmm_group4+chunks_bf16" and B.kernel_name_bf16(24, 8, B.SMALL_ROWS, 3) == "spmm_group8+long_bf16"


def predicted_list(table):
    out = []
    for s in table:
        st = B.structure(s["regime"], s["rect"])
        out.append(B.kernel_name_bf16(s["C"], s["vec"], st["shape"][0], int((st["deg"] > st["L"]).sum())))
    return out


def predicted_names(table):
    return set(predicted_list(table))


def test_expected_out_marks_the_map_and_skipped_rows():
    table = B.launch_table()
    for skip in (False, True):
        s = next(t for t in table if t["entry"] == "rows" and t["regime"] == "T" and t["C"] <= 24 and t["skip"] == skip)
        ops = B.operands(B.structure(s["regime"], s["rect"]), s)
        want, bound, written = B.expected_out(s, ops)
        live = int((ops["deg"] > 0).sum()) if skip else ops["n_res"]
        assert written.sum() == live and (want[~written] == float(B.SENTINEL)).all() and (bound[~written] == 0).all()
        assert want.shape[0] == ops["n_out"] == ops["n_res"] + R.ROWS_TALLER and (np.diff(ops["rows"]) > 0).all() and ops["rows"][-1] < ops["n_out"]
        assert (bf16_decode(ops["xbits"]) == ops["x"]).all() and (bf16_round(ops["x"]) == ops["x"]).all()     # x is what the kernel widens


# ---- the criteria admit float32 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", B.STRUCTURES, ids=SID)
@pytest.mark.parametrize("order", ["sequential", "chunked"])
@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
def test_criteria_admit_float32_sums(key, order, relu):
    """Float32 entry by entry and in the long-row path's chunk order over bf16-exact x, every other option on: within the bound and
    not by much; its RNE cast inside every interval; and the inputs make the interval test sharp: at least 90 % of the intervals are
    one bf16 value.  Under relu that holds for the elements the activation lets through; a clamped element's interval,
    [bf(-bound), bf(+bound)], is never one value (it admits what the f32 criterion admits there: anything within the bound of 0)."""
    c = _case(key, "full", diag=not key[1], relu=relu)
    A32 = sp.csr_matrix(c["A"], dtype=np.float32)
    got = R.emulate_f32(A32, c["L"], c["x"], c["h0_rows"], c["d"], order, relu=relu)
    want, bound = c["ref"]["want"], c["ref"]["bound"]
    r = R.ratio(got, want, bound)
    assert 0.1 < r <= 1.0, (key, order, r)
    bad, share = B.judge_bf16(bf16_round(got), want, bound)
    assert bad == 0, (key, order, bad)
    lo, hi = B.interval(want, bound)
    through = c["ref"]["pre"] > 0 if relu else np.ones(want.shape, dtype=bool)
    assert (lo == hi)[through].mean() >= 0.9, (key, order, share)      # a condition on the inputs, met by the reference alone
    if not relu:
        assert share >= 0.9


@pytest.mark.parametrize("key", B.STRUCTURES + [("L", False)], ids=SID)
def test_intervals_are_sharp_in_every_h0_form(key):
    for h0_form in B.H0_FORMS:
        c = _case(key, h0_form)
        lo, hi = B.interval(c["ref"]["want"], c["ref"]["bound"])
        assert (lo == hi).mean() >= 0.9, (key, h0_form)


# ---- planted mistakes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", B.STRUCTURES + [("L", False)], ids=SID)
def test_criteria_reject_planted_mistakes(key):
    """Each mistake is applied to the float64 value itself (the best a wrong kernel could do).  A wrong value must miss the bound
    (an f32 result) AND, rounded to nearest even, its interval (a bf16 result); the two rounding mistakes concern the interval alone."""
    c = _case(key, "full")
    A, deg, L, x, ref = c["A"], c["deg"], c["L"], c["x"], c["ref"]
    b, a = float(np.float32(B.BETA)), float(np.float32(B.ALPHA))
    hub = int(np.flatnonzero(deg == 2 * L + 1)[0])            # three chunks: L, L, 1

    def rejected(got, rf=ref, as_bf16_too=True):
        f32 = R.ratio(got, rf["want"], rf["bound"]) > 1.0
        b16 = B.judge_bf16(B.bf(got), rf["want"], rf["bound"])[0] > 0
        return f32 and (b16 or not as_bf16_too)

    assert not rejected(ref["want"]) and B.judge_bf16(B.bf(ref["want"]), ref["want"], ref["bound"])[0] == 0
    assert R.ratio(ref["want"], ref["want"], ref["bound"]) == 0.0
    # ---- from the f32 table
    # one entry of a hub row left out
    beg = A.indptr[hub]
    wrong = ref["pre"].copy()
    wrong[hub] -= b * A.data[beg + 3] * x[A.indices[beg + 3]].astype(np.float64)
    assert rejected(wrong), "entry left out"
    # a chunk of a hub row added twice, and one added never
    chunks = []
    for which in range(3):
        e = np.arange(beg + which * L, min(beg + (which + 1) * L, A.indptr[hub + 1]))
        chunks.append((A.data[e][:, None] * x[A.indices[e]].astype(np.float64)).sum(0))
    for which, sign in ((1, +1.0), (1, -1.0), (2, +1.0), (2, -1.0)):
        wrong = ref["pre"].copy()
        wrong[hub] += sign * b * chunks[which]
        assert rejected(wrong), ("chunk", which, sign)
    # H0 at the compact row instead of the mapped row (gnx_spmm_rows_bf16: map_h0)
    _, rows, n_out = R.row_maps(A.shape[0], 1)
    tall = np.random.default_rng(9).standard_normal((n_out, C_CPU), dtype=np.float32)
    mapped = R.reference(A, deg, L, x, tall[rows], None)
    assert rejected(R.reference(A, deg, L, x, tall[:A.shape[0]], None)["want"], mapped), "map_h0"
    # a bias row read with ldh0 = C: row i of the buffer instead of row 0
    biased = R.reference(A, deg, L, x, np.broadcast_to(c["full"][:1], c["full"].shape), None)
    assert rejected(ref["want"], biased), "ldh0"
    # relu omitted
    with_relu = R.reference(A, deg, L, x, c["h0_rows"], None, relu=True)
    assert rejected(ref["pre"], with_relu), "relu"
    # the diagonal term omitted (square structures; a rectangular one has none, and of L only some rows are taken)
    if A.shape[0] == A.shape[1]:
        d = np.random.default_rng(2).uniform(0.5, 1.5, size=A.shape[0]).astype(np.float32)
        assert rejected(ref["want"], R.reference(A, deg, L, x, c["h0_rows"], d)), "diagonal"
    # ---- new for bf16 rows
    # columns 2k and 2k + 1 swapped (the pair decode of bload: w << 16 and w & 0xFFFF0000 the wrong way round)
    wrong = ref["want"].copy()
    wrong[:, 0::2], wrong[:, 1::2] = ref["want"][:, 1::2], ref["want"][:, 0::2]
    assert rejected(wrong), "pair decode"
    # columns 0 .. 3 and 4 .. 7 swapped (the halves of a uint4)
    assert rejected(ref["want"][:, [4, 5, 6, 7, 0, 1, 2, 3]]), "uint4 halves"
    # H0 rounded to bf16 before the mix
    assert rejected(R.reference(A, deg, L, x, bf16_round(c["h0_rows"]), None)["want"]), "H0 as bf16"
    # the partial sums of the hub rows rounded to bf16 before they are added (a bf16 slab).  An f32 result shows it; a bf16 result
    # cannot be asked to: the mistake is of the size of the result's own rounding (2^-9 of a chunk's sum).
    wrong = ref["pre"].copy()
    for h in np.flatnonzero(deg > L):
        e0, e1 = A.indptr[h], A.indptr[h + 1]
        parts = [(A.data[e:min(e + L, e1)][:, None] * x[A.indices[e:min(e + L, e1)]].astype(np.float64)).sum(0) for e in range(e0, e1, L)]
        assert np.abs(ref["pre"][h] - (b * sum(parts) + a * c["h0_rows"][h].astype(np.float64))).max() < 1e-9
        wrong[h] = b * sum(B.bf(part) for part in parts) + a * c["h0_rows"][h].astype(np.float64)
    assert rejected(wrong, as_bf16_too=False), "slab as bf16"
    # a bf16 result produced by truncation and not RNE
    assert B.judge_bf16(B.bf_truncated(ref["want"]), ref["want"], ref["bound"])[0] > 0, "truncating store"
    # a bf16 result rounded from the value of the wrong activation, either way
    assert B.judge_bf16(B.bf(ref["pre"]), with_relu["want"], with_relu["bound"])[0] > 0, "relu left out before the rounding"
    assert B.judge_bf16(B.bf(with_relu["want"]), ref["want"], ref["bound"])[0] > 0, "relu applied before the rounding"
    # rounded twice: to bf16, mixed, and again (H0 added after the rounding store)
    mix = a * c["h0_rows"].astype(np.float64)
    twice = B.bf(B.bf(ref["pre"] - mix) + mix)
    assert B.judge_bf16(twice, ref["want"], ref["bound"])[0] > 0, "rounded twice"

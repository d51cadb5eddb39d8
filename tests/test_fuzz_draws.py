"""The seeded fuzz's draws on the host (tests/fuzz_kernels.py; no GPU): the stream ``draw_case`` reads is the seed's contract, and the
riders' inputs must be ones their criteria can judge."""
import json
import os

import numpy as np
import pytest

import fuzz_kernels as fz

SEED, CASES = 11, 200                       # the fixed slice tests/test_gpu_fuzz.py runs


@pytest.fixture(scope="module")
def slice_cases():
    rng = np.random.default_rng(SEED)
    return [fz.draw_case(rng, case) for case in range(CASES)]


def test_draw_case_reproduces_the_recorded_digests(golden_dir, slice_cases):
    """tests/golden/fuzz_seed11_draw_digests.json: sha256 of every case of seed 11 as draw_case drew it BEFORE the riders were
    added.  The riders draw from child generators of (seed, case, tag); a draw added to the parent stream changes every later case."""
    with open(os.path.join(golden_dir, "fuzz_seed11_draw_digests.json")) as f:
        rec = json.load(f)
    assert (rec["seed"], rec["cases"], len(rec["sha256"])) == (SEED, CASES, CASES)
    got = [fz.case_digest(s) for s in slice_cases]
    assert got == rec["sha256"], [c for c in range(CASES) if got[c] != rec["sha256"][c]][:10]
    # draw_extra takes nothing from the parent stream and names the same inputs on every call; replay carries it along
    s = fz.replay(SEED, 9)
    assert fz.case_digest({k: v for k, v in s.items() if k[:2] not in ("e_", "b_", "f_")}) == rec["sha256"][9]
    again = fz.draw_extra(SEED, 9, slice_cases[9])
    assert set(again) == {"e_mode", "e_idx", "e_vals"} and all(np.array_equal(again[k], s[k]) for k in again)


def test_riders_cover_the_slice(slice_cases):
    """At least 20 cases of each rider in the slice (what test_fixed_slice_of_the_fuzz demands on the GPU), every duplicate mode
    among them, and the "many" mode's slots at several of the multiplicities around the byte's limit."""
    extras = [fz.draw_extra(SEED, c, s) for c, s in enumerate(slice_cases)]
    entries = [x for x in extras if "e_idx" in x]
    assert len(entries) >= 20 and sum("b_pad" in x for x in extras) >= 20
    assert {x["e_mode"] for x in entries} == set(range(len(fz.ENTRY_MODES)))
    for s, x in zip(slice_cases, extras):
        if "e_idx" not in x:
            continue
        assert x["e_idx"].shape == (len(x["e_vals"]), 2) and x["e_vals"].dtype == np.float32
        assert len(x["e_idx"]) > s["nnz"] == len(np.unique(x["e_idx"], axis=0))          # duplicates, and the case's own slots
        counts = np.unique(x["e_idx"], axis=0, return_counts=True)[1]
        if x["e_mode"] == 2:
            assert counts.max() in fz.MANY
    many = {int(np.unique(x["e_idx"], axis=0, return_counts=True)[1].max()) for x in entries if x["e_mode"] == 2}
    assert len(many) >= 3, many


def test_bf16_rider_cancelling_share_stays_under_the_cap(slice_cases):
    """The bf16 result of an element whose sum cancels to less than 1e-4 of the size of its terms is not judged by the one-ulp rule
    (fz.BF16_BAND).  That exclusion must not hide a failure: in every kind-0 case of the slice at most 1 % of the elements lie in
    the band -- a condition on the inputs, shown here with numpy alone (the one-element cases, n = 1 and C = 1, included)."""
    seen = small = 0
    for case, s in enumerate(slice_cases):
        if s["kind"] != 0:
            continue
        s = dict(s, **fz.draw_extra(SEED, case, s))
        pre, mag = fz.bf16_spmm_reference(s)
        assert pre.shape == (s["n"], s["C"]) and (mag >= np.abs(pre) * (1 - 1e-12)).all()
        band = np.abs(pre) < fz.BF16_BAND * mag
        assert band.mean() <= fz.BF16_BAND_CAP, (case, s["n"], s["C"], float(band.mean()))
        seen += 1
        small += pre.size <= 100
    assert seen == CASES // 8 and small >= 1


def test_f32_rider_covers_entries_widths_and_options(slice_cases):
    """Rider "f32" over the slice's 25 kind-0 cases: every entry, every per-lane vector width and every value of every option occurs
    at least 3 times -- per entry, for the options and the widths -- and the drawn layouts and maps are ones the entries accept."""
    from collections import Counter
    seen, n_cases = Counter(), 0
    for case, s in enumerate(slice_cases):
        x = fz.draw_extra(SEED, case, s)
        assert ("f_perm" in x) == (s["kind"] == 0)
        if s["kind"] != 0:
            continue
        n_cases += 1
        s = dict(s, **x)
        n, n_cols = s["n"], s["n_cols"]
        assert sorted(s["f_perm"].tolist()) == list(range(n)) and s["f_perm"].dtype == np.int32
        assert len(s["f_rows"]) == n and (np.diff(s["f_rows"]) > 0).all() and 0 <= s["f_rows"][0] and s["f_rows"][-1] < s["f_n_out"]
        assert s["f_H0_cols"].shape == (n_cols, s["C"]) and s["f_H0_tall"].shape == (s["f_n_out"], s["C"])
        for e in fz.F32_ENTRIES:
            pad, off = s[f"f_{e}_pad"], s[f"f_{e}_off"]
            assert pad.shape == off.shape == (3,) and (0 <= off).all() and (off <= pad).all()
            assert not (s[f"f_{e}_diag"] and (not s["sq"] or e == "rows")) and not (s[f"f_{e}_skip"] and e not in ("spmm", "rows"))
            lds, offs, vec = fz.f32_layout(s, e)
            assert vec in (4, 2, 1) and s["C"] % vec == 0
            seen[e] += 1
            seen[e, "vec", vec] += 1
            seen[e, "h0", fz.F32_H0[s[f"f_{e}_h0"]]] += 1
            seen[e, "relu", s[f"f_{e}_relu"]] += 1
            seen[e, "diag", s[f"f_{e}_diag"]] += 1
            seen[e, "skip", s[f"f_{e}_skip"]] += 1
            seen["rect", not s["sq"], e in ("t", "tv")] += 1
    assert n_cases == CASES // 8
    for e in fz.F32_ENTRIES:
        assert seen[e] == n_cases
        for vec in (4, 2, 1):
            assert seen[e, "vec", vec] >= 3, (e, vec, seen[e, "vec", vec])
        for form in fz.F32_H0:
            assert seen[e, "h0", form] >= 3, (e, form)
        for value in (False, True):
            assert seen[e, "relu", value] >= 3, (e, "relu", value)
            if e != "rows":
                assert seen[e, "diag", value] >= 3, (e, "diag", value)
            if e in ("spmm", "rows"):
                assert seen[e, "skip", value] >= 3, (e, "skip", value)
    assert seen["rect", True, True] >= 3 * 2                                 # the transposed entries on rectangular cases, which the base case skips


def test_f32_rider_reference_on_a_small_case(slice_cases):
    """f32_reference with numpy alone on the slice's smallest kind-0 cases: shapes, the map and the rows a skipping launch leaves."""
    done = 0
    for case, s in enumerate(slice_cases):
        if s["kind"] != 0 or s["n"] * s["C"] > 20000:
            continue
        s = dict(s, **fz.draw_extra(SEED, case, s))
        for e in fz.F32_ENTRIES:
            want, mag, to, live = fz.f32_reference(s, e)
            n_res = s["n_cols"] if e in ("t", "tv") else s["n"]
            assert want.shape == mag.shape == (n_res, s["C"]) and len(to) == len(live) == n_res and (mag >= np.abs(want) * (1 - 1e-12)).all()
            assert live.all() or (s[f"f_{e}_skip"] and not s[f"f_{e}_diag"])
        done += 1
    assert done >= 3

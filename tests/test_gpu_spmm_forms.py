"""The f32 eval SpMM in every operand form against float64: the five entries (gnx_spmm, gnx_spmm_scatter, gnx_spmm_rows, gnx_spmm_t,
gnx_spmm_tv) over the fixed launch table of tests/spmm_forms_ref.py -- every row class at every per-lane vector width, the mix
operand absent / full / one bias row, diagonal, relu, GNX_ACT_SKIP_EMPTY, row maps, column windows of wider buffers -- at both
long-row regimes, hub rows in either orientation, square and rectangular.  tests/test_spmm_forms_cpu.py asserts what the table
covers and that the bound rejects planted mistakes; here each launch is judged by  max |got - want| / bound <= 1  and by the
sentinel it must leave wherever it has nothing to write, and the entries are tied to each other bit for bit."""
import numpy as np
import pytest
import torch

import spmm_forms_ref as R

pytestmark = pytest.mark.gpu
DEVICE = "cuda:0"
TABLE = R.launch_table()
RATIOS, NAMES, RAN = {}, set(), set()


@pytest.fixture(scope="module")
def gnntf():
    import gnntf
    gnntf.set_default_device(DEVICE)
    yield gnntf
    gnntf.set_default_device(None)


@pytest.fixture(scope="module")
def handles(gnntf):
    """structure key -> (structure, DeviceGraph, transposed-order raw values), built on first use."""
    from gnntf import _native as nat
    made = {}

    def get(key):
        if key not in made:
            st = R.structure(*key)
            g = gnntf.DeviceGraph(gnntf.SparseCOO(st["coo"], st["vals"], st["shape"]), device=DEVICE)
            vals_t = torch.empty(g.nnz, dtype=torch.float32, device=DEVICE)
            nat.check(nat.lib().gnx_graph_permute_values_t(g.handle, None, nat.ptr(vals_t), nat.current_stream()))
            made[key] = (st, g, vals_t)
        return made[key]
    return get


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEVICE)


def windowed(values, pad, off, fill):
    """(device buffer, its window): a torch [r, C] tensor as columns [off, off + C) of a buffer C + pad wide."""
    buf = torch.full((values.shape[0], values.shape[1] + pad), float(fill), dtype=torch.float32, device=DEVICE)
    view = buf[:, off:off + values.shape[1]]
    view.copy_(values)
    return buf, view


def call(g, vals_t, s, entry, X, H0, d, out, row_map, skip):
    """One launch through the C entry (the wrappers cannot express an offset ``out`` or ldh0 = 0 on gnx_spmm_rows)."""
    from gnntf import _native as nat
    lib, C = nat.lib(), s["C"]
    act = (nat.ACT_RELU if s["relu"] else nat.ACT_NONE) | (nat.ACT_SKIP_EMPTY if skip else 0)
    ldh0 = 0 if H0 is None or (s["h0"] == "bias") else H0.stride(0)
    tail = (nat.ptr(X), X.stride(0), C, nat.ptr(H0), ldh0, R.BETA, R.ALPHA, act)
    end = (nat.ptr(out), out.stride(0), nat.current_stream())
    if entry == "spmm":
        rc = lib.gnx_spmm(g.handle, None, nat.ptr(d), *tail, *end)
    elif entry == "t":
        rc = lib.gnx_spmm_t(g.handle, None, nat.ptr(d), *tail, *end)
    elif entry == "tv":
        rc = lib.gnx_spmm_tv(g.handle, nat.ptr(vals_t), nat.ptr(d), *tail, *end)
    elif entry == "scatter":
        rc = lib.gnx_spmm_scatter(g.handle, None, nat.ptr(d), *tail, nat.ptr(row_map), *end)
    else:
        assert entry == "rows" and d is None
        rc = lib.gnx_spmm_rows(g.handle, None, *tail, nat.ptr(row_map), *end)
    nat.check(rc)
    return g.last_kernel()


def bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("s", TABLE, ids=R.launch_id)
def test_launch_against_float64(gnntf, handles, s):
    st, g, vals_t = handles((s["regime"], s["kind"], s["rect"]))
    entry, C = s["entry"], s["C"]
    ops = R.operands(st, s)
    (px, ox), (ph, oh), (po, oo) = s["lay"]
    _, X = windowed(dev(ops["x"]), px, ox, np.nan)
    H0 = None if ops["h0"] is None else windowed(dev(ops["h0"]), ph, oh, np.nan)[1]
    d = None if ops["d"] is None else dev(ops["d"])
    row_map = dev(ops["perm"]) if entry == "scatter" else dev(ops["rows"]) if entry == "rows" else None
    fresh = lambda rows: windowed(torch.full((rows, C), float(R.SENTINEL), device=DEVICE), po, oo, R.SENTINEL)
    buf, out = fresh(ops["tall"])
    name = call(g, vals_t, s, entry, X, H0, d, out, row_map, s["skip"])
    NAMES.add(name)
    what = R.launch_id(s)
    RAN.add(what)
    # ---- the dispatch: the vector width shows in the class
    lds = (X.stride(0), None if H0 is None else 0 if s["h0"] == "bias" else H0.stride(0), out.stride(0))
    offs = (X.data_ptr() % 16, None if H0 is None else H0.data_ptr() % 16, out.data_ptr() % 16)
    assert R.expected_vec(C, lds, offs) == s["vec"], (what, lds, offs)
    n_long = int((ops["deg"] > ops["L"]).sum())
    assert name == R.kernel_name(C, s["vec"], ops["n_res"], n_long), (what, name)
    # ---- float64, the sentinel, no NaN from the padding
    want, bound, written = R.expected_out(s, ops)
    whole = buf.cpu().numpy()
    got = whole[:, oo:oo + C]
    assert (whole[:, :oo] == R.SENTINEL).all() and (whole[:, oo + C:] == R.SENTINEL).all(), (what, "padding columns written")
    assert (got[~written] == R.SENTINEL).all(), (what, "rows outside the map / without entries written", int((got[~written] != R.SENTINEL).any(1).sum()))
    assert np.isfinite(got).all(), (what, "NaN or Inf in the result")
    assert not (got[written] == R.SENTINEL).all(1).any(), (what, "a live row was left alone")
    r = R.ratio(got[written], want[written], bound[written])
    key = (entry, s["regime"] + (" hub rows" if n_long else " no hub rows"))
    RATIOS[key] = max(RATIOS.get(key, 0.0), r)
    print(f"{what}: {name} error / bound {r:.3f}")
    assert r <= 1.0, (what, name, r)
    if s["skip"] and s["diag"]:                                        # the flag is ignored under a diagonal: every row written
        assert written.all()
    # ---- a second run leaves the same bits
    buf2, out2 = fresh(ops["tall"])
    call(g, vals_t, s, entry, X, H0, d, out2, row_map, s["skip"])
    assert torch.equal(bits(buf), bits(buf2)), (what, "not repeatable")
    # ---- the entries tied to each other, bit for bit, under the same operand layout (the same vector width and row class)
    if entry == "tv":
        buf3, out3 = fresh(ops["tall"])
        call(g, vals_t, s, "t", X, H0, d, out3, None, False)
        assert torch.equal(bits(buf), bits(buf3)), (what, "gnx_spmm_tv on permuted values is not gnx_spmm_t")
    elif entry in ("scatter", "rows"):
        H0c = H0
        if entry == "rows" and s["h0"] == "full":
            H0c = windowed(H0.index_select(0, row_map.long()), ph, oh, np.nan)[1]
        _, compact = fresh(ops["n_res"])
        call(g, vals_t, s, "spmm", X, H0c, d, compact, None, s["skip"])
        buf3, out3 = fresh(ops["tall"])
        out3[row_map.long()] = compact
        assert torch.equal(bits(buf), bits(buf3)), (what, "not the plain launch sent through the map")


def test_rows_refusals(gnntf, handles):
    """gnx_spmm_rows refuses a NULL row map and a mix operand whose leading dimension is neither 0 nor at least C; it has no
    diagonal argument to misuse.  Nothing is written by a refused call."""
    from gnntf import _native as nat
    st, g, _ = handles(("T", "a", True))
    n, n_cols = st["shape"]
    C = 8
    X, H0 = torch.randn(n_cols, C, device=DEVICE), torch.randn(n + R.ROWS_TALLER, C, device=DEVICE)
    out = torch.full((n + R.ROWS_TALLER, C), float(R.SENTINEL), device=DEVICE)
    rows = dev(R.row_maps(n, 0)[1])
    lib = nat.lib()
    with pytest.raises(Exception, match="NULL row map"):
        nat.check(lib.gnx_spmm_rows(g.handle, None, nat.ptr(X), C, C, nat.ptr(H0), C, 0.8, 0.2, 0, None, nat.ptr(out), C, nat.current_stream()))
    for ldh0 in (1, C - 1):
        with pytest.raises(Exception, match="leading dimension smaller than C"):
            nat.check(lib.gnx_spmm_rows(g.handle, None, nat.ptr(X), C, C, nat.ptr(H0), ldh0, 0.8, 0.2, 0, nat.ptr(rows), nat.ptr(out), C,
                                        nat.current_stream()))
    with pytest.raises(Exception, match="invalid activation"):
        nat.check(lib.gnx_spmm_rows(g.handle, None, nat.ptr(X), C, C, nat.ptr(H0), C, 0.8, 0.2, 2, nat.ptr(rows), nat.ptr(out), C,
                                    nat.current_stream()))
    for fn in (lib.gnx_spmm_t, lib.gnx_spmm_tv):                           # only gnx_spmm and gnx_spmm_rows take the skip flag
        with pytest.raises(Exception, match="invalid activation"):
            nat.check(fn(g.handle, None, None, nat.ptr(H0[:n]), C, C, None, 0, 1.0, 0.0, nat.ACT_SKIP_EMPTY, nat.ptr(out), C, nat.current_stream()))
    with pytest.raises(Exception, match="diag needs a square graph"):
        nat.check(lib.gnx_spmm(g.handle, None, nat.ptr(H0), nat.ptr(X), C, C, None, 0, 1.0, 0.0, 0, nat.ptr(out), C, nat.current_stream()))
    torch.cuda.synchronize()
    assert bool((out == float(R.SENTINEL)).all())


def test_report_the_worst_ratios(capsys):
    """Not a check of its own: prints what the launches above measured (profiles/NOTES.md records a run), and asserts what only
    the whole table can show: every class name and the merged chunks launch occurred."""
    with capsys.disabled():
        print("\n[f32 SpMM forms, MI355X] worst error / bound per entry and regime:")
        for (entry, regime), value in sorted(RATIOS.items()):
            print(f"    {entry:10s} {regime:20s} {value:.3f}")
        print("    names:", " ".join(sorted(NAMES)))
    assert all(value <= 1.0 for value in RATIOS.values())
    if len(RAN) == len(TABLE):                                             # (the whole table ran, not a selection of it)
        assert {n.split("+")[0] for n in NAMES} >= {"spmm_wave", "spmm_group32", "spmm_group16", "spmm_group8"}, NAMES
        assert any(n.endswith("+chunks") for n in NAMES) and not any("+long" in n for n in NAMES), NAMES

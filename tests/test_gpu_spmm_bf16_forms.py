"""The bf16-storage eval SpMM in every operand form against float64: gnx_spmm_bf16 and gnx_spmm_rows_bf16, f32 and bf16 results,
over the fixed launch table of tests/spmm_bf16_forms_ref.py -- every row class at every per-lane vector width 8 / 4 / 2 / 1, forced
through a leading dimension or the first byte of X (2-byte elements), H0 (4) or out (2 or 4), the mix operand absent / full / one
bias row, diagonal, relu, GNX_ACT_SKIP_EMPTY, a row map, column windows of wider buffers -- at the long-row regimes T and S, square
and rectangular, and at n = 2^20 + 11, where the sub-wave classes run the hub rows' chunks in launches of their own.
tests/test_spmm_bf16_forms_cpu.py asserts what the table covers and that the criteria reject planted mistakes; here each launch is
judged by  max |got - want| / bound <= 1  (an f32 result) or by the monotone interval [bf(want - bound), bf(want + bound)] (a bf16
result), by the sentinel it must leave wherever it has nothing to write, and bit for bit against its siblings.  gnx_cast_bf16 is
tested into windows, and the entries' refusals are shown to write nothing."""
import numpy as np
import pytest
import torch

import spmm_bf16_forms_ref as B
import spmm_forms_ref as R
from bf16_ref import bf16_decode

pytestmark = pytest.mark.gpu
DEVICE = "cuda:0"
TABLE = B.launch_table()
RATIOS, SHARES, NAMES, RAN = {}, {}, set(), set()
S = float(B.SENTINEL)


@pytest.fixture(scope="module")
def gnntf():
    import gnntf
    gnntf.set_default_device(DEVICE)
    yield gnntf
    gnntf.set_default_device(None)


@pytest.fixture(scope="module")
def handles(gnntf):
    """(regime, rect) -> (structure, DeviceGraph), built on first use, once per module (structure L takes a few seconds)."""
    made = {}

    def get(key):
        if key not in made:
            st = B.structure(*key)
            made[key] = (st, gnntf.DeviceGraph(gnntf.SparseCOO(st["coo"], st["vals"], st["shape"]), device=DEVICE))
        return made[key]
    return get


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEVICE)


def dev_bf16(bits):
    """uint16 bit patterns -> a bfloat16 device tensor of those bits."""
    return dev(np.ascontiguousarray(bits).view(np.int16)).view(torch.bfloat16)


def windowed(values, pad, off, fill):
    """(device buffer, its window): a torch [r, C] tensor as columns [off, off + C) of a buffer C + pad wide of the same dtype."""
    buf = torch.full((values.shape[0], values.shape[1] + pad), float(fill), dtype=values.dtype, device=DEVICE)
    view = buf[:, off:off + values.shape[1]]
    view.copy_(values)
    return buf, view


def fresh(rows, C, out_bf16, pad, off):
    dtype = torch.bfloat16 if out_bf16 else torch.float32
    buf = torch.full((rows, C + pad), S, dtype=dtype, device=DEVICE)
    return buf, buf[:, off:off + C]


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def host(t):
    """A device tensor's values as float64 (bf16 decoded exactly)."""
    if t.dtype == torch.bfloat16:
        return bf16_decode(t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)).astype(np.float64)
    return t.cpu().numpy().astype(np.float64)


def call(g, s, entry, X, H0, d, out, row_map, skip, out_bf16=None):
    """One launch through the C entry (the wrappers cannot express an offset ``out`` or a bias row on gnx_spmm_rows_bf16)."""
    from gnntf import _native as nat
    lib, C = nat.lib(), s["C"]
    out_bf16 = int(out.dtype == torch.bfloat16) if out_bf16 is None else out_bf16
    act = (nat.ACT_RELU if s["relu"] else nat.ACT_NONE) | (nat.ACT_SKIP_EMPTY if skip else 0)
    ldh0 = 0 if H0 is None or (s["h0"] == "bias") else H0.stride(0)
    tail = (nat.ptr(X), X.stride(0), C, nat.ptr(H0), ldh0, B.BETA, B.ALPHA, act)
    end = (nat.ptr(out), out_bf16, out.stride(0), nat.current_stream())
    if entry == "spmm":
        rc = lib.gnx_spmm_bf16(g.handle, None, nat.ptr(d), *tail, *end)
    else:
        assert entry == "rows" and d is None
        rc = lib.gnx_spmm_rows_bf16(g.handle, None, *tail, nat.ptr(row_map), *end)
    nat.check(rc)
    return g.last_kernel()


def picked_vec(s, X, H0, out):
    """The mirror of pick_vec on the operands as they lie on the device."""
    lds = (X.stride(0), None if H0 is None else 0 if s["h0"] == "bias" else H0.stride(0), out.stride(0))
    offs = (X.data_ptr() % 16, None if H0 is None else H0.data_ptr() % 16, out.data_ptr() % 16)
    return B.expected_vec_bf16(s["C"], lds, offs, out.dtype == torch.bfloat16), (lds, offs)


def record(s, rows_kind, ratio=None, share=None):
    key = (s["entry"], "bf16" if s["out_bf16"] else "f32", s["regime"], rows_kind)
    if ratio is not None:
        RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)
    if share is not None:                             # (one-value intervals, elements): summed per result type and kind of row
        one, of = SHARES.get((key[1], rows_kind), (0, 0))
        SHARES[(key[1], rows_kind)] = (one + share[0], of + share[1])


def judge(s, what, name, got, want, bound, hub):
    """The criterion of the launch's result type over rows ``got`` (float64 values), the hub rows and the others apart.  The share of
    one-value intervals is a property of the reference alone; it is recorded for either result type, over the elements the activation
    lets through (a clamped element's interval, [bf(-bound), bf(+bound)], is never one value)."""
    for rows_kind, sel in (("hub rows", hub), ("other rows", ~hub)):
        if not sel.any():
            continue
        through = want[sel] != 0
        lo, hi = B.interval(want[sel][through], bound[sel][through])
        share = (int((lo == hi).sum()), int(through.sum()))
        if s["out_bf16"]:
            bad, all_share = B.judge_bf16(got[sel], want[sel], bound[sel])
            record(s, rows_kind, ratio=float(bad), share=share)
            print(f"{what}: {name} {rows_kind}: {bad} outside their interval, {all_share:.3f} of all intervals one value")
            assert bad == 0, (what, name, rows_kind, bad)
        else:
            r = R.ratio(got[sel], want[sel], bound[sel])
            record(s, rows_kind, ratio=r, share=share)
            print(f"{what}: {name} {rows_kind}: error / bound {r:.3f}")
            assert r <= 1.0, (what, name, rows_kind, r)


def device_operands(s, ops):
    (px, ox), (ph, oh), _ = s["lay"]
    X = windowed(dev_bf16(ops["xbits"]), px, ox, np.nan)[1]
    H0 = None if ops["h0"] is None else windowed(dev(ops["h0"]), ph, oh, np.nan)[1]
    d = None if ops["d"] is None else dev(ops["d"])
    row_map = dev(ops["rows"]) if s["entry"] == "rows" else None
    return X, H0, d, row_map


def ties(g, s, name, ops, X, H0, d, row_map, buf, out):
    """Bit for bit: a second run; ``rows`` against the compact launch sent through the map; a bf16 result against the cast of the
    f32 result of the same launch at the same vector width."""
    what, entry, C = B.launch_id(s), s["entry"], s["C"]
    (_, _), (ph, oh), (po, oo) = s["lay"]
    buf2, out2 = fresh(ops["tall"], C, s["out_bf16"], po, oo)
    call(g, s, entry, X, H0, d, out2, row_map, s["skip"])
    assert torch.equal(bits(buf), bits(buf2)), (what, "not repeatable")
    if entry == "rows":
        H0c = H0
        if s["h0"] == "full":
            H0c = windowed(H0.index_select(0, row_map.long()), ph, oh, np.nan)[1]
        _, compact = fresh(ops["n_res"], C, s["out_bf16"], po, oo)
        call(g, s, "spmm", X, H0c, None, compact, None, s["skip"])
        assert picked_vec(s, X, H0c, compact)[0] == s["vec"]
        buf3, out3 = fresh(ops["tall"], C, s["out_bf16"], po, oo)
        out3[row_map.long()] = compact
        assert torch.equal(bits(buf), bits(buf3)), (what, "not the plain launch sent through the map")
    if s["out_bf16"]:
        p32, o32 = s["lay_f32"][2]
        buf4, out4 = fresh(ops["tall"], C, False, p32, o32)
        name4 = call(g, s, entry, X, H0, d, out4, row_map, s["skip"])
        assert picked_vec(s, X, H0, out4)[0] == s["vec"], (what, "the f32 sibling picks another width")
        assert name4 == name and torch.equal(bits(out), bits(out4.to(torch.bfloat16))), (what, "not the f32 result rounded once, to nearest even")


@pytest.mark.parametrize("s", [s for s in TABLE if s["regime"] != "L"], ids=B.launch_id)
def test_launch_against_float64(gnntf, handles, s):
    st, g = handles((s["regime"], s["rect"]))
    entry, C = s["entry"], s["C"]
    ops = B.operands(st, s)
    X, H0, d, row_map = device_operands(s, ops)
    po, oo = s["lay"][2]
    buf, out = fresh(ops["tall"], C, s["out_bf16"], po, oo)
    name = call(g, s, entry, X, H0, d, out, row_map, s["skip"])
    NAMES.add(name)
    what = B.launch_id(s)
    RAN.add(what)
    # ---- the dispatch: the chosen width shows in the class, the hub rows' route in the name
    vec, where = picked_vec(s, X, H0, out)
    assert vec == s["vec"], (what, where)
    n_long = int((ops["deg"] > ops["L"]).sum())
    assert name == B.kernel_name_bf16(C, s["vec"], ops["n_res"], n_long), (what, name)
    # ---- the sentinel, no NaN from the padding, the criterion
    want, bound, written = B.expected_out(s, ops)
    whole = host(buf)
    got = whole[:, oo:oo + C]
    assert (whole[:, :oo] == S).all() and (whole[:, oo + C:] == S).all(), (what, "padding columns written")
    assert (got[~written] == S).all(), (what, "rows outside the map / without entries written", int((got[~written] != S).any(1).sum()))
    assert np.isfinite(got).all(), (what, "NaN or Inf in the result")
    assert not (got[written] == S).all(1).any(), (what, "a live row was left alone")
    hub = np.zeros(ops["tall"], dtype=bool)
    hub[B.destination(s, ops)[ops["deg"] > ops["L"]]] = True
    judge(s, what, name, got[written], want[written], bound[written], hub[written])
    if s["skip"] and s["diag"]:                                        # the flag is ignored under a diagonal: every row written
        assert written.all()
    ties(g, s, name, ops, X, H0, d, row_map, buf, out)


@pytest.mark.parametrize("s", [s for s in TABLE if s["regime"] == "L"], ids=B.launch_id)
def test_large_launch_against_float64(gnntf, handles, s):
    """n = 2^20 + 11: the short rows and the hub rows' chunks in launches of their own.  Float64 on every hub row, every planted row
    and 8192 random rows; the sentinel, padding and NaN conditions on the device over the whole buffer."""
    st, g = handles(("L", False))
    entry, C = s["entry"], s["C"]
    sel = B.l_sample(st, s["seed"])
    ops = B.operands(st, s, rows=sel)
    X, H0, d, row_map = device_operands(s, ops)
    po, oo = s["lay"][2]
    buf, out = fresh(ops["tall"], C, s["out_bf16"], po, oo)
    name = call(g, s, entry, X, H0, d, out, row_map, s["skip"])
    NAMES.add(name)
    what = B.launch_id(s)
    RAN.add(what)
    vec, where = picked_vec(s, X, H0, out)
    assert vec == s["vec"], (what, where)
    n_long = int((ops["deg"] > ops["L"]).sum())
    assert name == B.kernel_name_bf16(C, s["vec"], ops["n_res"], n_long) and name.endswith("+long_bf16"), (what, name)
    # ---- on the device, the whole buffer
    live, to = B.live_rows(s, ops), B.destination(s, ops)
    written = np.zeros(ops["tall"], dtype=bool)
    written[to[live]] = True
    w = dev(written)
    assert bool((buf[:, :oo] == S).all()) and bool((buf[:, oo + C:] == S).all()), (what, "padding columns written")
    assert bool((out[~w] == S).all()), (what, "rows outside the map / without entries written")
    assert bool(torch.isfinite(out.float()).all()), (what, "NaN or Inf in the result")
    assert not bool((out[w] == S).all(1).any()), (what, "a live row was left alone")
    assert (~written).sum() >= (R.ROWS_TALLER if entry == "rows" else 0) + (int((ops["deg"] == 0).sum()) if s["skip"] else 0)
    # ---- float64 on the chosen rows
    keep = live[sel]
    got = host(out.index_select(0, dev(to[sel][keep].astype(np.int64))))
    hub = (ops["deg"][sel] > ops["L"])[keep]
    assert hub.sum() == n_long
    judge(s, what, name, got, ops["ref"]["want"][keep], ops["ref"]["bound"][keep], hub)
    ties(g, s, name, ops, X, H0, d, row_map, buf, out)


def test_one_element_offset_two_kernels(gnntf, handles):
    """``out`` four elements into its buffer: 8 bytes for a bf16 result (4 values per lane, 32-lane groups at C = 128), 16 bytes for an
    f32 result (8 per lane, 16-lane groups).  Two kernels, both judged; a short row's entries are added in ascending order whatever
    the lane width, so off the hub rows the bf16 result is still the f32 result rounded once, bit for bit."""
    st, g = handles(("T", False))
    s = dict(entry="spmm", out_bf16=True, C=128, vec=4, regime="T", kind="a", rect=False, h0="full", diag=True, relu=False, skip=False, seed=77,
             lay=((16, 8), (8, 4), (8, 4)))
    ops = B.operands(st, s)
    X, H0, d, _ = device_operands(s, ops)
    want, bound, written = B.expected_out(s, ops)
    hub = ops["deg"] > ops["L"]
    outs = {}
    for out_bf16, vec, name in ((True, 4, "spmm_group32+chunks_bf16"), (False, 8, "spmm_group16+chunks_bf16")):
        t = dict(s, out_bf16=out_bf16, vec=vec)
        buf, out = fresh(ops["tall"], 128, out_bf16, 8, 4)
        got_name = call(g, t, "spmm", X, H0, d, out, None, False)
        assert picked_vec(t, X, H0, out)[0] == vec == B.expected_vec_bf16(128, B.geometry(t)[0], B.geometry(t)[1], out_bf16)
        assert got_name == name == B.kernel_name_bf16(128, vec, ops["n_res"], int(hub.sum())), got_name
        whole = host(buf)
        assert (whole[:, :4] == S).all() and (whole[:, 132:] == S).all() and written.all()
        judge(t, "offset-4 " + ("bf16" if out_bf16 else "f32"), got_name, whole[:, 4:132], want, bound, hub)
        outs[out_bf16] = out
    short = dev(~hub)
    assert torch.equal(bits(outs[True][short]), bits(outs[False][short].to(torch.bfloat16)))


# ---- gnx_cast_bf16 into windows ------------------------------------------------------------------------------------------------------------
CAST_LAYOUTS = {                                     # name -> ((pad, off) of src in f32 elements, (pad, off) of dst in bf16 elements)
    "wide": ((8, 4), (8, 4)),                        # lds, ldd = C + 8; src 16 bytes in, dst 8 bytes in: four per item where C allows
    "lds": ((10, 4), (8, 4)),
    "ldd": ((8, 4), (10, 4)),
    "src": ((8, 6), (8, 4)),                         # 24 bytes in: 8-byte but not 16-byte aligned
    "dst": ((8, 4), (8, 6)),                         # 12 bytes in: 4-byte but not 8-byte aligned
    "dst2": ((8, 4), (8, 5)),                        # 10 bytes in
}


@pytest.mark.parametrize("layout", list(CAST_LAYOUTS))
@pytest.mark.parametrize("C", [1, 7, 8, 36, 64])
def test_cast_into_windows(gnntf, C, layout):
    from gnntf import _native as nat
    (ps, os_), (pd, od) = CAST_LAYOUTS[layout]
    n = 301                                          # 301 * 64 / 4 items: more than one block of 256 either way
    rng = np.random.default_rng([C, len(layout)])
    x = rng.standard_normal((n, C)).astype(np.float32) * np.float32(10.0) ** rng.integers(-3, 4, (n, C)).astype(np.float32)
    ties_ = np.array([0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0xBF808000, 0xBF818000, 0x80000000], dtype=np.uint32).view(np.float32)
    x.reshape(-1)[:min(len(ties_), x.size)] = ties_[:min(len(ties_), x.size)]
    _, src = windowed(dev(x), ps, os_, np.nan)
    buf, dst = fresh(n, C, True, pd, od)
    v4 = C % 4 == 0 and src.stride(0) % 4 == 0 and dst.stride(0) % 4 == 0 and src.data_ptr() % 16 == 0 and dst.data_ptr() % 8 == 0
    assert v4 == (layout == "wide" and C % 4 == 0), (C, layout)             # the layout allows / forbids what it says
    nat.check(nat.lib().gnx_cast_bf16(nat.ptr(src), n, C, src.stride(0), nat.ptr(dst), dst.stride(0), nat.current_stream()))
    assert torch.equal(bits(dst), bits(src.to(torch.bfloat16))), (C, layout)
    assert bool((buf[:, :od] == S).all()) and bool((buf[:, od + C:] == S).all()), (C, layout, "padding written")


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(gnntf, handles):
    from gnntf import _native as nat
    st, g = handles(("T", True))
    n, n_cols = st["shape"]
    C = 8
    lib, stream = nat.lib(), nat.current_stream()
    X = torch.randn(n_cols, C, device=DEVICE).to(torch.bfloat16)
    X0 = X.clone()
    H0 = torch.randn(n + R.ROWS_TALLER, C, device=DEVICE)
    dg = torch.ones(n, device=DEVICE)
    out = torch.full((n + R.ROWS_TALLER, C), S, device=DEVICE)
    rows = dev(R.row_maps(n, 0)[1])

    def spmm(diag=None, X=X, ldh0=C, act=0, out=out, out_bf16=0):
        return lib.gnx_spmm_bf16(g.handle, None, nat.ptr(diag), nat.ptr(X), C, C, nat.ptr(H0), ldh0, 0.8, 0.2, act, nat.ptr(out), out_bf16, C, stream)

    def by_rows(row_map=rows, X=X, ldh0=C, act=0, out=out, out_bf16=0):
        return lib.gnx_spmm_rows_bf16(g.handle, None, nat.ptr(X), C, C, nat.ptr(H0), ldh0, 0.8, 0.2, act, nat.ptr(row_map), nat.ptr(out), out_bf16, C, stream)

    for fn in (spmm, by_rows):
        for bad in (2, -1):
            with pytest.raises(Exception, match="out_bf16 must be 0 or 1"):
                nat.check(fn(out_bf16=bad))
        for bad in (2, nat.ACT_SKIP_EMPTY | 2, 512):
            with pytest.raises(Exception, match="invalid activation"):
                nat.check(fn(act=bad))
        for bad in (1, C - 1):
            with pytest.raises(Exception, match="leading dimension smaller than C"):
                nat.check(fn(ldh0=bad))
        with pytest.raises(Exception, match="out must not alias X"):
            nat.check(fn(out=X, out_bf16=1))
    with pytest.raises(Exception, match="NULL row map"):
        nat.check(by_rows(row_map=None))
    with pytest.raises(Exception, match="diag needs a square graph"):
        nat.check(spmm(diag=dg))
    torch.cuda.synchronize()
    assert bool((out == S).all()) and torch.equal(bits(X), bits(X0))
    # (the accepted forms of the same calls do write)
    nat.check(spmm())
    nat.check(by_rows(out_bf16=0))
    assert not bool((out[rows.long()] == S).all(1).any())


def test_report_the_worst_ratios(capsys):
    """Not a check of its own: prints what the launches above measured (profiles/NOTES.md records a run), and asserts what only
    the whole table can show: every name the dispatch rule predicts on the CPU occurred."""
    with capsys.disabled():
        print("\n[bf16 SpMM forms, MI355X] f32 results: worst error / bound; bf16 results: elements outside their interval:")
        for (entry, kind, regime, rows_kind), value in sorted(RATIOS.items()):
            print(f"    {entry:5s} {kind:5s} {regime} {rows_kind:11s} {value:.3f}")
        for (kind, rows_kind), (one, of) in sorted(SHARES.items()):
            print(f"    one-value intervals, {kind} results, {rows_kind}: {one / max(of, 1):.4f} of {of} elements the activation lets through")
        print("    names:", " ".join(sorted(NAMES)))
    assert all(value <= 1.0 for (_, kind, _, _), value in RATIOS.items() if kind == "f32")
    assert all(value == 0 for (_, kind, _, _), value in RATIOS.items() if kind == "bf16")
    if len(RAN) == len(TABLE):                                             # (the whole table ran, not a selection of it)
        predicted = set()
        for s in TABLE:
            st = B.structure(s["regime"], s["rect"])
            predicted.add(B.kernel_name_bf16(s["C"], s["vec"], st["shape"][0], int((st["deg"] > st["L"]).sum())))
        assert NAMES == predicted, (NAMES ^ predicted)
        assert {"spmm_group4+chunks_bf16", "spmm_wave+long_bf16", "spmm_group8+long_bf16", "spmm_group16+long_bf16", "spmm_group32+long_bf16"} <= NAMES

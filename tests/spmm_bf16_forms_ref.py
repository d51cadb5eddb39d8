"""Structures, operand layouts, the dispatch mirror, the criteria and the launch table for the bf16-storage eval SpMM in every
operand form (gnx_spmm_bf16, gnx_spmm_rows_bf16; csrc/gnx_spmm_bf16.hip: the kernels of csrc/gnx_spmm_eval.h over Bf16RowsT<false>,
csrc/gnx_spmm_device.h).  numpy and scipy only: imports without a GPU.  The f32 table is tests/spmm_forms_ref.py; what is shared
comes from there unchanged.

Structures: regimes T and S of spmm_forms_ref as kind "a" (the bf16 entries walk the forward structure), square or with 37 extra
columns, and "L": planted_graph at n = 2^20 + 11 (threshold 512), where the sub-wave classes run the hub rows' chunks in launches
of their own.  X is standard normal ROUNDED TO bf16, so the float64 reference reads exactly what the kernel widens; H0 and the
diagonal are f32.  X's window is padded with bf16 NaN, H0's with f32 NaN, ``out`` is filled with a sentinel that bf16 holds exactly.

Criteria (R.reference unchanged: bound = (deg + chunks + 4 + [diag]) 2^-24 mag, nothing added for the exact widening):
    f32 result:   max |got - want| / bound <= 1
    bf16 result:  rounding to nearest even is monotone, so a kernel that rounds ONCE an f32 value within ``bound`` of ``want`` lands
                  in [bf(want - bound), bf(want + bound)], bf = RNE of the float64 value straight to bf16 (not through float32:
                  double rounding is not monotone-safe at ties).  Compared as decoded values."""
import numpy as np

import spmm_forms_ref as R
from bf16_ref import bf16_bits, bf16_decode
from gcnii_shapes_ref import SMALL_ROWS, csr_of, planted_graph, plan_threshold

ENTRIES = ("spmm", "rows")
WIDTHS = (1, 7, 8, 12, 16, 17, 24, 40, 64, 100, 128, 136, 260, 264, 520)
VECS = (8, 4, 2, 1)
CLASSES, H0_FORMS = R.CLASSES, R.H0_FORMS
BETA, ALPHA = R.BETA, R.ALPHA
SENTINEL = np.float32(-12288.0)                      # -1.5 * 2^13: exact in bf16
BF16_NAN = np.uint16(0x7FC0)
assert (bf16_decode(bf16_bits(np.array([SENTINEL]))) == SENTINEL).all()
L_ROWS, L_HUBS = SMALL_ROWS + 11, 5
L_RANDOM_ROWS = 8192
T_ONLY_ABOVE = 260                                   # wider operands stay on regime T

_cache = {}


# ---- structures ------------------------------------------------------------------------------------------------------------------------
def structure(regime, rect):
    """The dict of R.structure (kind "a") for regimes T and S; for "L" the same keys but the transpose's, plus ``info`` of planted_graph."""
    if regime != "L":
        return R.structure(regime, "a", rect)
    assert not rect
    if "L" not in _cache:
        L = plan_threshold(L_ROWS)
        coo, vals, shape, info = planted_graph(L_ROWS, L, L_HUBS, seed=0)
        A = csr_of(coo, vals, shape)
        deg = np.diff(A.indptr)
        assert L == 512 and shape[0] >= SMALL_ROWS and (deg > L).sum() == 4 + L_HUBS
        assert all((deg == d).any() for d in (0, L - 1, L, L + 1, 2 * L + 1))
        _cache["L"] = dict(coo=coo, vals=vals, shape=shape, A=A, deg=deg, L=L, regime="L", kind="a", rect=False, name="Las", info=info)
    return _cache["L"]


STRUCTURES = [("T", False), ("T", True), ("S", False), ("S", True)]        # (and ("L", False), where a test can afford it)


# ---- the dispatch as the host code decides it ------------------------------------------------------------------------------------------
def expected_vec_bf16(C, lds, byte_offsets, out_bf16):
    """pick_vec as Bf16RowsT::vec feeds it: the widest of 8, 4, 2, 1 values per lane that C, the leading dimensions of X, H0, out
    (``lds``; None: no H0; 0, a bias row, divides everything) and the operands' first bytes (``byte_offsets`` modulo 16; None: no H0)
    allow.  Elements are 2 (X), 4 (H0) and 2 or 4 (out) bytes, an access is at most 16 bytes: 8 f32 go as two 16-byte accesses, so a
    16-byte aligned f32 operand never stands in the way of 8."""
    sizes = (2, 4, 2 if out_bf16 else 4)
    for v in (8, 4, 2):
        if C % v == 0 and all(ld % v == 0 for ld in lds if ld is not None) and \
                all(b % min(size * v, 16) == 0 for b, size in zip(byte_offsets, sizes) if b is not None):
            return v
    return 1


row_class = R.row_class


def kernel_name_bf16(C, vec, n_rows, n_long):
    """What gnx_graph_last_kernel reports for a bf16 eval launch (launch_eval<Bf16Rows>, NAMES_LONG): one wave per row above 32 lanes,
    "+long" when hub rows went through the chunk kernels; below, the hub rows' chunks ride in the row launch ("+chunks"; rows of up to 4
    lanes on 4-lane groups) on structures of fewer than SMALL_ROWS rows (launch_rows_and_chunks) and run in launches of their own
    ("+long", the row launch on at least 8 lanes) at or above; the bare class without hub rows."""
    lanes = -(-C // vec)
    if lanes > 32:
        return "spmm_wave" + ("+long" if n_long > 0 else "") + "_bf16"
    group = "group32" if lanes > 16 else "group16" if lanes > 8 else "group8"
    if n_long > 0 and n_rows < SMALL_ROWS:
        return "spmm_" + ("group4" if lanes <= 4 else group) + "+chunks_bf16"
    return "spmm_" + group + ("+long" if n_long > 0 else "") + "_bf16"


REACHABLE = sorted({(row_class(C, v), v) for C in WIDTHS for v in VECS if C % v == 0})


# ---- operand layouts -----------------------------------------------------------------------------------------------------------------
def forcible(vec, C):
    """Whether a layout has anything to force: C itself allows twice ``vec``."""
    return vec < 8 and C % (2 * vec) == 0


def resolve_breaker(vec, breaker, h0, out_bf16):
    """(which operand: 0 X, 1 H0, 2 out; what: 0 its leading dimension, 1 its first byte) that can force ``vec`` over twice ``vec``.
    Some cannot: an f32 operand (H0, an f32 out) whose first byte allows 4 per lane is 16-byte aligned and allows 8 as well (two
    16-byte accesses), so only its leading dimension forces 4; a bias row has ldh0 = 0, which divides everything, so only its first
    byte forces anything; an absent H0 forces nothing.  What cannot falls back: to the leading dimension, then to X."""
    which, what = breaker % 3, (breaker // 3) % 2
    four_byte = which == 1 or (which == 2 and not out_bf16)
    if what == 1 and four_byte and vec == 4:
        what = 0
    if which == 1 and (h0 == "none" or (h0 == "bias" and what == 0)):
        which = 0
        what = (breaker // 3) % 2
    return which, what


def layouts_for_bf16(vec, C, breaker, out_bf16, h0="full"):
    """((pad, off) of X, of H0, of out), in elements, under which pick_vec must choose exactly ``vec``: every window 16-byte aligned
    with a leading dimension of C plus a multiple of 8, but for the one operand that ``breaker`` (0 .. 5) pushes off by ``vec``
    elements, in its leading dimension or in its first byte (resolve_breaker).  Nothing is pushed where C itself allows no more."""
    assert C % vec == 0
    lay = [[16, 8], [8, 4], [24, 8] if out_bf16 else [16, 8]]
    if forcible(vec, C):
        which, what = resolve_breaker(vec, breaker, h0, out_bf16)
        if what == 0:
            lay[which][0] += vec
        else:
            lay[which][1] += vec
            lay[which][0] += 8
    return tuple(tuple(x) for x in lay)


def geometry(s, lay=None):
    """(lds, byte offsets modulo 16) of X, H0, out under layout ``lay`` of launch ``s`` (buffers start 256-byte aligned); None where
    no H0 is given; a bias row has ldh0 = 0."""
    (px, ox), (ph, oh), (po, oo) = s["lay"] if lay is None else lay
    C = s["C"]
    ldh0 = None if s["h0"] == "none" else 0 if s["h0"] == "bias" else C + ph
    return (C + px, ldh0, C + po), ((2 * ox) % 16, None if s["h0"] == "none" else (4 * oh) % 16, ((2 if s["out_bf16"] else 4) * oo) % 16)


def window(values, pad, off, fill):
    """(buffer, view): ``values`` [r, C] (any dtype) as columns [off, off + C) of a buffer C + pad wide filled with ``fill``."""
    r, C = values.shape
    assert 0 <= off <= pad
    buf = np.full((r, C + pad), fill, dtype=values.dtype)
    buf[:, off:off + C] = values
    return buf, buf[:, off:off + C]


# ---- the launch table ------------------------------------------------------------------------------------------------------------------
COMBOS = (
    (8, 8), (24, 8), (64, 8), (128, 8), (136, 8), (264, 8), (520, 8),                      # g8 g8 g8 g16 g32 wave1 wave2
    (12, 4), (40, 4), (64, 4), (100, 4), (128, 4), (136, 4), (260, 4),                     # g8 g16 g16 g32 g32 wave1 wave2
    (8, 2), (24, 2), (40, 2), (64, 2), (128, 2), (260, 2),                                 # g8 g16 g32 g32 wave1 wave2 (all forced)
    (1, 1), (7, 1), (12, 1), (16, 1), (17, 1), (24, 1), (40, 1), (64, 1), (100, 1),        # g8 g8 g16 g16 g32 g32 wave1 wave1 wave2
)

# regime L: C <= 40; up to 4 lanes (the hub chunks on 4-lane groups), 5 .. 8, 16-lane and 32-lane groups; no diagonal (the reference
# is computed for chosen rows only)
L_LAUNCHES = (
    dict(entry="spmm", out_bf16=False, C=24, vec=8, h0="full", relu=True, skip=False, breaker=0),
    dict(entry="rows", out_bf16=True, C=16, vec=4, h0="bias", relu=False, skip=False, breaker=5),
    dict(entry="spmm", out_bf16=True, C=40, vec=4, h0="full", relu=False, skip=False, breaker=2),
    dict(entry="rows", out_bf16=False, C=24, vec=2, h0="none", relu=True, skip=True, breaker=3),
    dict(entry="spmm", out_bf16=True, C=40, vec=2, h0="bias", relu=True, skip=True, breaker=4),
    dict(entry="rows", out_bf16=False, C=40, vec=8, h0="full", relu=False, skip=False, breaker=0),
)


def _row(entry, out_bf16, C, vec, regime, rect, h0, diag, relu, skip, breaker, seed):
    lay = layouts_for_bf16(vec, C, breaker, out_bf16, h0)
    # the f32-result launch a bf16-result launch is tied to: the same X and H0 windows, ``out`` laid out for the same width
    lay_f32 = layouts_for_bf16(vec, C, breaker, False, h0)
    assert lay[:2] == lay_f32[:2]                    # (the result type only ever changes how ``out`` itself is pushed)
    return dict(entry=entry, out_bf16=out_bf16, C=C, vec=vec, cls=row_class(C, vec), regime=regime, kind="a", rect=rect, h0=h0, diag=diag,
                relu=relu, skip=skip, breaker=breaker, lay=lay, lay_f32=lay_f32, seed=seed)


def launch_table():
    """The fixed table: dicts(entry, out_bf16, C, vec, cls, regime, kind, rect, h0, diag, relu, skip, breaker, lay, lay_f32, seed).
    Per entry and result type every combination of COMBOS once; inside an (entry, result type, class) the options cycle, so that every
    value meets every class; the L launches follow.  test_spmm_bf16_forms_cpu.py asserts the coverage."""
    table = []
    for e, (entry, out_bf16) in enumerate((en, ob) for en in ENTRIES for ob in (False, True)):
        seen = dict.fromkeys(CLASSES, 0)
        for j, (C, vec) in enumerate(COMBOS):
            cls = row_class(C, vec)
            k = seen[cls]
            seen[cls] += 1
            diag = entry == "spmm" and (k // 2) % 2 == 1
            table.append(_row(entry, out_bf16, C, vec, "T" if C > T_ONLY_ABOVE else "TS"[(j + e) % 2], (not diag) and (j + k) % 2 == 1,
                              H0_FORMS[k % 3], diag, k % 2 == 1, (k + k // 2) % 2 == 1, j + e, 1000 * e + j))
    for i, s in enumerate(L_LAUNCHES):
        table.append(_row(regime="L", rect=False, diag=False, seed=5000 + i, **s))
    return table


def launch_id(s):
    return (f"{s['entry']}-{'bf16' if s['out_bf16'] else 'f32'}-{s['regime']}a{'r' if s['rect'] else 's'}-C{s['C']}v{s['vec']}-{s['h0']}"
            + ("-diag" if s["diag"] else "") + ("-relu" if s["relu"] else "") + ("-skip" if s["skip"] else ""))


# ---- operands and the reference of one launch -------------------------------------------------------------------------------------------
def bf16_normal(rng, shape):
    """(bits uint16, values float32): standard normal rounded to bf16."""
    bits = bf16_bits(rng.standard_normal(shape, dtype=np.float32))
    return bits, bf16_decode(bits)


def operands(st, s, rows=None):
    """The host side of launch ``s`` on structure ``st``: dict(xbits, x, h0, h0_rows, d, rows, n_out, n_res, tall, deg, L, ref): x [n_in, C]
    the decoded bf16 values; h0 as stored ([n_res or n_out, C], [1, C] for a bias row, None); h0_rows as each compact result row
    reads it; ref = R.reference() -- for the compact rows ``rows`` only when given (regime L)."""
    entry, C = s["entry"], s["C"]
    A, deg, L = st["A"], st["deg"], st["L"]
    n_res, n_in = A.shape
    rng = np.random.default_rng([s["seed"], 3])
    xbits, x = bf16_normal(rng, (n_in, C))
    _, row_map, n_out = R.row_maps(n_res, s["seed"])
    tall = n_out if entry == "rows" else n_res
    h0 = h0_rows = None
    if s["h0"] == "full":
        h0 = rng.standard_normal((tall, C), dtype=np.float32)
        h0_rows = h0[row_map] if entry == "rows" else h0
    elif s["h0"] == "bias":
        h0 = rng.standard_normal((1, C), dtype=np.float32)
        h0_rows = np.broadcast_to(h0, (n_res, C))
    d = rng.uniform(0.5, 1.5, size=n_res).astype(np.float32) if s["diag"] else None
    if rows is None:
        ref = R.reference(A, deg, L, x, h0_rows, d, relu=s["relu"])
    else:
        assert d is None
        ref = R.reference(A[rows], deg[rows], L, x, None if h0_rows is None else h0_rows[rows], None, relu=s["relu"])
    return dict(xbits=xbits, x=x, h0=h0, h0_rows=h0_rows, d=d, rows=row_map, n_out=n_out, n_res=n_res, tall=tall, ref=ref, deg=deg, L=L)


def live_rows(s, ops):
    """[n_res] bool: the compact rows the launch writes (under GNX_ACT_SKIP_EMPTY without a diagonal: those with entries)."""
    return ops["deg"] > 0 if s["skip"] and not s["diag"] else np.ones(ops["n_res"], dtype=bool)


def destination(s, ops):
    return ops["rows"] if s["entry"] == "rows" else np.arange(ops["n_res"])


def expected_out(s, ops):
    """(want [tall, C] float64, bound, written [tall] bool): the result buffer's window as the launch must leave it -- the reference at
    the rows the entry's map sends it to, the sentinel in every row outside the map and, under GNX_ACT_SKIP_EMPTY without a diagonal, in
    every row without entries."""
    ref, live, to = ops["ref"], live_rows(s, ops), destination(s, ops)
    want = np.full((ops["tall"], s["C"]), float(SENTINEL))
    bound = np.zeros_like(want)
    written = np.zeros(ops["tall"], dtype=bool)
    want[to[live]], bound[to[live]], written[to[live]] = ref["want"][live], ref["bound"][live], True
    return want, bound, written


def l_sample(st, seed):
    """Compact rows of structure L judged against float64: every hub row, every planted row, L_RANDOM_ROWS random ones (ascending)."""
    rng = np.random.default_rng([seed, 13])
    return np.unique(np.concatenate([st["info"]["hub"], st["info"]["planted"], rng.choice(st["shape"][0], size=L_RANDOM_ROWS, replace=False)]))


# ---- the bf16 criterion ------------------------------------------------------------------------------------------------------------------
MIN_NORMAL = 2.0 ** -126


def bf(v):
    """RNE of float64 values straight to bf16 (8 significant bits), returned as float64.  Normal range only (asserted)."""
    v = np.asarray(v, dtype=np.float64)
    assert np.isfinite(v).all()
    m, e = np.frexp(v)                               # v = m 2^e, 0.5 <= |m| < 1
    r = np.ldexp(np.rint(m * 256.0), e - 8)          # rint: ties to even
    assert ((r == 0) == (v == 0)).all() and (np.abs(r[r != 0]) >= MIN_NORMAL).all() and (np.abs(r) < 2.0 ** 127).all(), "outside bf16's normal range"
    return r


def bf_truncated(v):
    """float64 -> bf16 by dropping the bits below (round toward zero): the planted mistake."""
    m, e = np.frexp(np.asarray(v, dtype=np.float64))
    return np.ldexp(np.trunc(m * 256.0), e - 8)


def interval(want, bound):
    """(lo, hi) = (bf(want - bound), bf(want + bound)): where a kernel that rounds once a value within the bound must land."""
    return bf(want - bound), bf(want + bound)


def judge_bf16(got, want, bound):
    """(number of elements outside their interval, share of elements whose interval is a single value); ``got`` decoded bf16 values."""
    got = np.asarray(got, dtype=np.float64)
    lo, hi = interval(want, bound)
    bad = ~((lo <= got) & (got <= hi))               # (a NaN is outside)
    return int(bad.sum()), float((lo == hi).mean()) if lo.size else 1.0

"""Structures, operand layouts, float64 references and the launch table for the f32 eval SpMM in every operand form
(gnx_spmm, gnx_spmm_scatter, gnx_spmm_rows, gnx_spmm_t, gnx_spmm_tv; csrc/gnx_spmm_eval.h, epilogue in csrc/gnx_spmm_device.h).
numpy and scipy only: imports without a GPU.

Structures are the long-row regimes of gcnii_shapes_ref (T: n = 1547, threshold 512; S: n = 2^15 + 11, threshold 128) as kind "a"
(hub rows in the forward structure) and kind "t" (columns swapped: the hub rows are the transpose's), square or with 37 extra
columns.  Operands are column windows of wider buffers, NaN around X and H0 and a sentinel all over ``out``, so that a vector access
that leaves its window, a row written outside a map and a row written under GNX_ACT_SKIP_EMPTY all show.

The reference takes the float32 weights in float64:
    pre   = beta (A x + d * x_rows) + alpha h0
    mag   = |beta| (|A| |x| + |d| |x|) + |alpha h0|
    bound = (deg + chunks + 4 + [diag]) U32 mag          forward_ref's T_bound: first order, a float32 sum IN ANY ORDER, nothing tuned
(relu leaves the bound: |relu x - relu y| <= |x - y|).  The criterion is  max |got - want| / bound <= 1."""
import numpy as np
import scipy.sparse as sp

from gcnii_shapes_ref import U32, SMALL_ROWS, chunk_counts, csr_of, f64, plan_threshold, ratio, regime_graph, spmm_f32  # noqa: F401

ENTRIES = ("spmm", "scatter", "rows", "t", "tv")
WIDTHS = (1, 7, 8, 17, 40, 64, 100, 128, 132, 260)
VECS = (4, 2, 1)
H0_FORMS = ("none", "full", "bias")
CLASSES = ("g8", "g16", "g32", "wave1", "wave2")     # 8 / 16 / 32 lanes per row, one wave per row over one tile / over two and more
SENTINEL = np.float32(-12345.5)
EXTRA_COLS, EXTRA_ENTRIES = 37, 200
ROWS_TALLER = 29                                     # gnx_spmm_rows: the result buffer holds this many rows more than the handle
BETA, ALPHA = 0.8, 0.2
ACCEPTS_SKIP = ("spmm", "rows")
ACCEPTS_DIAG = ("spmm", "scatter", "t", "tv")
HUB_KIND = dict(spmm="a", scatter="a", rows="a", t="t", tv="t")      # the kind whose hub rows the entry walks

_cache = {}


def structure(regime, kind, rect):
    """dict(coo, vals, shape, A, At, deg, deg_t, L, L_t, regime, kind, rect): A the float64 CSR of the float32 weights, At its
    transpose, deg / L and deg_t / L_t the row lengths and long-row threshold of either."""
    key = (regime, kind, rect)
    if key in _cache:
        return _cache[key]
    coo, vals, shape, info = regime_graph(regime)
    n = shape[0]
    if kind == "t":
        coo = np.ascontiguousarray(coo[:, ::-1])
    n_cols = n
    if rect:
        # background entries in EXTRA_COLS more columns, in rows that are neither planted (their lengths are the point) nor empty
        rng = np.random.default_rng([11, regime == "S", kind == "t"])
        deg = np.bincount(coo[:, 0], minlength=n)
        rows = np.setdiff1d(np.flatnonzero(deg > 0), info["planted"])
        key_ = np.unique(rng.choice(rows, size=EXTRA_ENTRIES) * EXTRA_COLS + rng.integers(0, EXTRA_COLS, size=EXTRA_ENTRIES))
        more = np.stack([key_ // EXTRA_COLS, n + key_ % EXTRA_COLS], axis=1).astype(np.int64)
        coo = np.concatenate([coo, more])
        vals = np.concatenate([vals, rng.uniform(0.5, 1.5, size=len(more)).astype(np.float32)])
        n_cols = n + EXTRA_COLS
        assert abs(len(more) - EXTRA_ENTRIES) < 20 and len(np.unique(more[:, 1])) == EXTRA_COLS
    shape = (n, n_cols)
    A = csr_of(coo, vals, shape)
    At = sp.csr_matrix(A.T)
    At.sort_indices()
    st = dict(coo=coo, vals=vals, shape=shape, A=A, At=At, deg=np.diff(A.indptr), deg_t=np.diff(At.indptr), L=plan_threshold(n),
              L_t=plan_threshold(n_cols), regime=regime, kind=kind, rect=rect, name=f"{regime}{kind}{'r' if rect else 's'}")
    hub, hub_t = (st["deg"] > st["L"]).sum(), (st["deg_t"] > st["L_t"]).sum()
    assert (hub > 0 and hub_t == 0) if kind == "a" else (hub == 0 and hub_t > 0), (key, hub, hub_t)
    lengths = st["deg"] if kind == "a" else st["deg_t"]
    L = st["L"] if kind == "a" else st["L_t"]
    assert all((lengths == d).any() for d in (0, L - 1, L, L + 1, 2 * L, 2 * L + 1))
    _cache[key] = st
    return st


STRUCTURES = [(r, k, rect) for r in ("T", "S") for k in ("a", "t") for rect in (False, True)]


def walked(st, entry):
    """(CSR the entry walks, row lengths, threshold): the transpose for ``t`` / ``tv``."""
    return (st["At"], st["deg_t"], st["L_t"]) if entry in ("t", "tv") else (st["A"], st["deg"], st["L"])


# ---- the dispatch as the host code decides it ------------------------------------------------------------------------------------------
def expected_vec(C, lds, byte_offsets):
    """pick_vec: the widest of 4, 2, 1 values per lane that C, every leading dimension and every operand's first byte allow (an
    access is at most 16 bytes; buffers themselves start 256-byte aligned).  ``None`` entries: an operand that is not given."""
    for v in (4, 2):
        if C % v == 0 and all(ld % v == 0 for ld in lds if ld is not None) and all(b % (4 * v) == 0 for b in byte_offsets if b is not None):
            return v
    return 1


def row_class(C, vec):
    lanes = -(-C // vec)
    if lanes > 32:
        return "wave1" if C <= 64 * vec else "wave2"
    return "g32" if lanes > 16 else "g16" if lanes > 8 else "g8"


def kernel_name(C, vec, n_rows, n_long):
    """What gnx_graph_last_kernel reports for an eval launch: the class, and "+chunks" where the hub rows' chunks ride in the row
    launch (sub-wave classes below SMALL_ROWS rows; there rows of up to 4 lanes run on 4-lane groups)."""
    lanes = -(-C // vec)
    if lanes > 32:
        return "spmm_wave"
    if n_long > 0 and n_rows < SMALL_ROWS:
        return "spmm_" + ("group32" if lanes > 16 else "group16" if lanes > 8 else "group4" if lanes <= 4 else "group8") + "+chunks"
    return "spmm_" + ("group32" if lanes > 16 else "group16" if lanes > 8 else "group8")


REACHABLE = sorted({(row_class(C, v), v) for C in WIDTHS for v in VECS if C % v == 0})


# ---- operand layouts -----------------------------------------------------------------------------------------------------------------
def window(values, pad, off, fill):
    """(buffer, view): ``values`` [r, C] as columns [off, off + C) of a buffer C + pad wide filled with ``fill``."""
    r, C = values.shape
    assert 0 <= off <= pad
    buf = np.full((r, C + pad), fill, dtype=np.float32)
    buf[:, off:off + C] = values
    return buf, buf[:, off:off + C]


def layouts_for(vec, C, breaker):
    """((pad, off) of X, of H0, of out) under which pick_vec must choose ``vec``: every window 4-aligned but for the one the
    ``breaker`` (0 .. 5: leading dimension or first byte of X, H0, out) pushes off by 2 (vec 2) or 1 (vec 1, even C)."""
    assert C % vec == 0
    lay = [[8, 4], [4, 0], [12, 8]]
    step = {4: 0, 2: 2, 1: 1}[vec]
    if step:
        which, what = breaker % 3, (breaker // 3) % 2
        if what == 0:
            lay[which][0] += step                    # the leading dimension
        else:
            lay[which][1] += step; lay[which][0] += 4    # the first byte (the leading dimension keeps its 4-alignment)
    return tuple(tuple(x) for x in lay)


# ---- the launch table ------------------------------------------------------------------------------------------------------------------
def _combos():
    out = [(C, v) for v in VECS for C in WIDTHS if C % v == 0]
    return out + [(40, 4), (64, 4)]                  # the 16-lane class is reached by these two alone: twice each, for the three H0 forms


def launch_table():
    """The fixed table: dicts(entry, C, vec, regime, kind, rect, h0, diag, relu, skip, lay, seed).  Per entry every (width, vector
    width) combination once (the two 16-lane ones twice); inside an (entry, class) the options cycle, so that every value meets
    every class; test_spmm_forms_cpu.py asserts the coverage."""
    table = []
    for e, entry in enumerate(ENTRIES):
        seen = dict.fromkeys(CLASSES, 0)
        for j, (C, vec) in enumerate(_combos()):
            cls = row_class(C, vec)
            k = seen[cls]
            seen[cls] += 1
            diag = entry in ACCEPTS_DIAG and (k // 2) % 2 == 1
            skip = entry in ACCEPTS_SKIP and (k + k // 2) % 2 == 1
            h0 = H0_FORMS[k % 3]
            breaker = j + e
            if breaker % 3 == 1 and (h0 == "none" or (h0 == "bias" and (breaker // 3) % 2 == 0)):
                breaker -= 1                         # no H0, or a bias row's ldh0 = 0, to push off: X takes it
            table.append(dict(entry=entry, C=C, vec=vec, cls=cls, regime="TS"[(j + e) % 2], kind=HUB_KIND[entry] if j % 5 != 4 else "ta"[HUB_KIND[entry] == "t"],
                              rect=(not diag) and (j + k) % 2 == 1, h0=h0, diag=diag, relu=k % 2 == 1, skip=skip,
                              lay=layouts_for(vec, C, breaker), seed=1000 * e + j))
    return table


def launch_id(s):
    return (f"{s['entry']}-{s['regime']}{s['kind']}{'r' if s['rect'] else 's'}-C{s['C']}v{s['vec']}-{s['h0']}" + ("-diag" if s["diag"] else "")
            + ("-relu" if s["relu"] else "") + ("-skip" if s["skip"] else ""))


# ---- operands, maps and the reference of one launch -------------------------------------------------------------------------------------
def row_maps(n_rows, seed):
    """(perm, rows, n_out): the scatter permutation, and an ascending map of the n_rows result rows into a buffer of n_out rows."""
    rng = np.random.default_rng([seed, 7])
    n_out = n_rows + ROWS_TALLER
    rows = np.sort(rng.choice(n_out, size=n_rows, replace=False))
    return rng.permutation(n_rows).astype(np.int32), rows.astype(np.int32), n_out


def reference(A, deg, L, x, h0_rows, d, beta=BETA, alpha=ALPHA, relu=False):
    """dict(pre, want, mag, bound) of one launch per RESULT row of the walked structure ``A`` (compact rows, before any map).
    ``h0_rows``: the mix term per result row as the launch must read it (a bias row broadcast, mapped rows selected) or None;
    ``d``: the diagonal weights or None (square structures)."""
    A = sp.csr_matrix(A, dtype=np.float64)
    b, a = float(np.float32(beta)), float(np.float32(alpha))
    xd = f64(x)
    S, M = A @ xd, abs(A) @ np.abs(xd)
    if d is not None:
        assert A.shape[0] == A.shape[1]
        S, M = S + f64(d)[:, None] * xd, M + np.abs(f64(d))[:, None] * np.abs(xd)
    pre, mag = b * S, abs(b) * M
    if h0_rows is not None:
        pre, mag = pre + a * f64(h0_rows), mag + np.abs(a * f64(h0_rows))
    terms = (deg + chunk_counts(deg, L) + 4 + (d is not None))[:, None]
    return dict(pre=pre, want=np.maximum(pre, 0.0) if relu else pre, mag=mag, bound=terms * U32 * mag)


def emulate_f32(A32, L, x, h0_rows, d, order, beta=BETA, alpha=ALPHA, relu=False):
    """The launch in float32 under ``order`` ("sequential" / "chunked" of spmm_f32): what the bound must admit."""
    acc = spmm_f32(A32, x, order, L)
    if d is not None:
        acc = acc + d.astype(np.float32)[:, None] * x.astype(np.float32)
    out = acc * np.float32(beta)
    if h0_rows is not None:
        out = out + np.float32(alpha) * h0_rows.astype(np.float32)
    return np.maximum(out, np.float32(0)) if relu else out


def operands(st, s):
    """The host side of launch ``s`` on structure ``st``: dict(x, h0, h0_rows, d, perm, rows, n_out, n_res, ref): x [n_in, C];
    h0 as stored ([n_res or n_out, C], [1, C] for a bias row, None); h0_rows as each compact result row reads it; ref = reference()."""
    entry, C = s["entry"], s["C"]
    A, deg, L = walked(st, entry)
    n_res, n_in = A.shape
    rng = np.random.default_rng([s["seed"], 3])
    x = rng.standard_normal((n_in, C)).astype(np.float32)
    perm, rows, n_out = row_maps(n_res, s["seed"])
    tall = n_out if entry == "rows" else n_res
    h0 = h0_rows = None
    if s["h0"] == "full":
        h0 = rng.standard_normal((tall, C)).astype(np.float32)
        h0_rows = h0[rows] if entry == "rows" else h0
    elif s["h0"] == "bias":
        h0 = rng.standard_normal((1, C)).astype(np.float32)
        h0_rows = np.broadcast_to(h0, (n_res, C))
    d = rng.uniform(0.5, 1.5, size=n_res).astype(np.float32) if s["diag"] else None
    ref = reference(A, deg, L, x, h0_rows, d, relu=s["relu"])
    return dict(x=x, h0=h0, h0_rows=h0_rows, d=d, perm=perm, rows=rows, n_out=n_out, n_res=n_res, tall=tall, ref=ref, deg=deg, L=L)


def expected_out(s, ops):
    """(want [tall, C] float64, written [tall] bool): the result buffer's window as the launch must leave it -- the reference at the
    rows the entry's map sends it to, the sentinel in every row outside the map and, under GNX_ACT_SKIP_EMPTY without a diagonal, in
    every row without entries."""
    entry, ref = s["entry"], ops["ref"]
    live = np.ones(ops["n_res"], dtype=bool)
    if s["skip"] and not s["diag"]:
        live = ops["deg"] > 0
    to = ops["perm"] if entry == "scatter" else ops["rows"] if entry == "rows" else np.arange(ops["n_res"])
    want = np.full((ops["tall"], s["C"]), float(SENTINEL))
    bound = np.zeros_like(want)
    written = np.zeros(ops["tall"], dtype=bool)
    want[to[live]], bound[to[live]], written[to[live]] = ref["want"][live], ref["bound"][live], True
    return want, bound, written

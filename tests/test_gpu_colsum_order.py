"""The summation order of the column sums (gnx_graph_colsum, gnx_graph_colsum_streams), pinned in float32: a numpy emulation of the
order csrc/gnx_prep.hip documents, asserted with torch.equal.

For column j the terms run in the order of the transposed structure: rows ascending.  A column of at most long_row entries: eight
partial sums a_s, each accumulated sequentially from 0.f over the positions b + s, b + s + 8, ..., then
((a0 + a4) + (a2 + a6)) + ((a1 + a5) + (a3 + a7)).  A longer column: 256 partial sums with stride 256, then red[i] += red[i + w] for
w = 128 ... 1.  A term is the raw value (p = 0), keep ? fl(v * 2) : 0 (p = 0.5), or, for a slot with duplicates, the sequential sum
from 0.f over its entries in input order of fl(e * 2) for the kept entries.  Only p = 0 and p = 0.5: the scale is then absent or 2,
exact, so the emulation does not depend on whether the compiler contracts the product into an fma.  All values are positive: adding
the 0.f of a dropped entry, of a lane without entries or of the emulation's padding changes no sum.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import gnntf_oracle as orc

pytestmark = pytest.mark.gpu

SEED, FIRST, STREAMS = 99, 7, 20
F0 = np.float32(0)


def columns_graph(n, counts, seed):
    """n x n COO with counts[j] entries in column j at distinct random rows, in shuffled order, values in [0.5, 1.5)"""
    rng = np.random.default_rng(seed)
    rows = np.concatenate([rng.choice(n, size=int(c), replace=False) for c in counts])
    cols = np.repeat(np.arange(n), counts)
    order = rng.permutation(len(rows))
    coo = np.stack([rows, cols], 1)[order].astype(np.int64)
    vals = (rng.random(len(coo)) + 0.5).astype(np.float32)
    return coo, vals, (n, n)


def graph_3000():
    """below TINY_ROWS: long_row = 512.  Columns of 0, 1, 7, 8, 9, 512, 513 and 1500 entries, the others random with every tenth of
    them empty (the list of non-empty columns is in use).  Four columns each of 512 and of 513 entries: the two walks give one
    such column the same float about every other time, and the emulation has to tell which side of long_row took which walk"""
    n, rng = 3000, np.random.default_rng(11)
    counts = rng.integers(1, 30, size=n)
    counts[::10] = 0
    counts[:14] = [0, 1, 7, 8, 9, 512, 513, 1500, 512, 513, 512, 513, 512, 513]
    return columns_graph(n, counts, 12), 512


def graph_64():
    """no empty column: the walk takes the columns as they are numbered"""
    counts = np.random.default_rng(21).integers(1, 20, size=64)
    return columns_graph(64, counts, 22), 512


def graph_40000():
    """between 2^15 and 2^20 rows: long_row = 128.  Four columns of 128 entries (short) and four of 129 (long)"""
    n, rng = 40000, np.random.default_rng(31)
    counts = rng.integers(0, 6, size=n)
    counts[[5, 200, 3000, 39999]], counts[[17, 201, 3001, 39998]] = 128, 129
    return columns_graph(n, counts, 32), 128


GRAPHS = {"n3000": graph_3000, "n64": graph_64, "n40000": graph_40000}
WAYS = ["as_is", "twice", "twice_entry_tables"]


def stored_twice(coo, vals):
    """every entry a second time behind the first copies; every third copy carries another value (a slot that is not uniform)"""
    again = vals.copy()
    again[::3] = (np.random.default_rng(41).random(len(again[::3])) + 0.5).astype(np.float32)
    return np.concatenate([coo, coo]), np.concatenate([vals, again])


def strided_sums(M, stride):
    """M[c, k]: term k of column c.  out[c, s] = the sequential float32 sum from 0.f of M[c, s], M[c, s + stride], ..."""
    acc = np.zeros((M.shape[0], stride), dtype=np.float32)
    for k in range(0, M.shape[1], stride):
        acc = acc + M[:, k:k + stride]
    return acc


def emulate(coo, terms, n, long_row):
    """column sums of the per-entry float32 ``terms`` (0 for a dropped entry) in the documented order"""
    assert terms.dtype == np.float32
    # slots: (col, row) ascending = the transposed structure; a slot's entries in input order (stable sort)
    order = np.lexsort((coo[:, 0], coo[:, 1]))
    c, r, t = coo[order, 1], coo[order, 0], terms[order]
    head = np.ones(len(c), dtype=bool)
    head[1:] = (c[1:] != c[:-1]) | (r[1:] != r[:-1])
    slot = np.cumsum(head) - 1
    rank = np.arange(len(c)) - np.flatnonzero(head)[slot]
    slot_val = np.zeros(int(head.sum()), dtype=np.float32)
    for k in range(int(rank.max()) + 1):                   # sequentially from 0.f over a slot's entries
        sel = rank == k
        slot_val[slot[sel]] = slot_val[slot[sel]] + t[sel]
    slot_col = c[head]
    counts = np.bincount(slot_col, minlength=n)
    begin = np.concatenate([[0], np.cumsum(counts)])
    pos = np.arange(len(slot_col)) - begin[slot_col]       # position inside the column, rows ascending
    out = np.zeros(n, dtype=np.float32)
    short = counts <= long_row
    width = -(-int(counts[short].max()) // 8) * 8
    M = np.zeros((n, width), dtype=np.float32)
    sel = short[slot_col]
    M[slot_col[sel], pos[sel]] = slot_val[sel]
    a = strided_sums(M, 8)
    out[:] = ((a[:, 0] + a[:, 4]) + (a[:, 2] + a[:, 6])) + ((a[:, 1] + a[:, 5]) + (a[:, 3] + a[:, 7]))
    for j in np.flatnonzero(~short):
        v = np.zeros(-(-int(counts[j]) // 256) * 256, dtype=np.float32)
        v[:counts[j]] = slot_val[begin[j]:begin[j + 1]]
        red = strided_sums(v[None, :], 256)[0]
        w = 128
        while w > 0:
            red[:w] = red[:w] + red[w:2 * w]
            w >>= 1
        out[j] = red[0]
    return out


@functools.lru_cache(maxsize=None)
def case(name, twice):
    """the graph and its expected sums: [0] without dropout, [1 + k] of stream FIRST + k at p = 0.5.  Computed once, read-only."""
    (coo, vals, shape), long_row = GRAPHS[name]()
    if twice:
        coo, vals = stored_twice(coo, vals)
    want = [emulate(coo, vals, shape[0], long_row)]
    for k in range(STREAMS):
        keep = orc.keep_mask(coo, 0.5, SEED, FIRST + k)
        want.append(emulate(coo, np.where(keep, vals * np.float32(2), F0).astype(np.float32), shape[0], long_row))
    want = np.stack(want)
    want.setflags(write=False)
    return coo, vals, shape, want


def assert_bits(got, want, counts, what):
    want = torch.tensor(want, device="cuda")
    if torch.equal(got, want):
        return
    bad = torch.nonzero(got != want)
    first = tuple(int(x) for x in bad[0])
    raise AssertionError(f"{what}: {len(bad)} sums differ, first at {first}: got {float(got[first])!r}, want {float(want[first])!r}, "
                         f"column of {int(counts[first[-1]])} entries")


@pytest.mark.parametrize("way", WAYS)
@pytest.mark.parametrize("name", list(GRAPHS))
def test_column_sums_in_the_documented_order(name, way):
    import gnntf
    from gnntf import _native as nat
    twice = way != "as_is"
    coo, vals, shape, want = case(name, twice)
    n = shape[0]
    counts = np.bincount(np.unique(coo, axis=0)[:, 1], minlength=n)
    g = gnntf.DeviceGraph(gnntf.SparseCOO(coo, vals, shape), device="cuda:0")
    if way == "twice_entry_tables":
        g.enable_entry_dropout()
        assert g.entry_dropout
    lib, stream = nat.lib(), nat.current_stream()
    one = torch.empty(n, device="cuda")
    if not twice:            # with duplicates the raw slot value is k_sum_slots' business (gnx_graph.hip), not this unit's
        nat.check(lib.gnx_graph_colsum(g.handle, 0.0, SEED, FIRST, nat.ptr(one), stream))
        assert_bits(one, want[0], counts, f"{name} {way}: gnx_graph_colsum, p = 0")
    for k in (0, 5):
        nat.check(lib.gnx_graph_colsum(g.handle, 0.5, SEED, FIRST + k, nat.ptr(one), stream))
        assert_bits(one, want[1 + k], counts, f"{name} {way}: gnx_graph_colsum, p = 0.5, stream {FIRST + k}")
    for K in (1, 2, 3, 20):
        got = torch.full((K, n), float("nan"), device="cuda")
        nat.check(lib.gnx_graph_colsum_streams(g.handle, 0.5, SEED, FIRST, K, nat.ptr(got), stream))
        assert_bits(got, want[1:1 + K], counts, f"{name} {way}: gnx_graph_colsum_streams, K = {K}")

"""Pendant elision (gnx_graph_set_pendant_elision): the rules restated in numpy, and the hand-built graph the tests walk.  No GPU
and no native code in here."""
import numpy as np


def elidable_rows(rowptr, colidx):
    """Row i is elidable iff it stores exactly one entry (i, h) with h != i, row h stores at least two entries, and no row other than
    h stores an entry in column i."""
    rowptr, colidx = np.asarray(rowptr, dtype=np.int64), np.asarray(colidx, dtype=np.int64)
    n = len(rowptr) - 1
    degree = np.diff(rowptr)
    rowidx = np.repeat(np.arange(n), degree)
    neighbour = np.full(n, -1, dtype=np.int64)
    one = degree == 1
    neighbour[one] = colidx[rowptr[:-1][one]]
    ok = one & (neighbour != np.arange(n))
    ok[ok] = degree[neighbour[ok]] >= 2
    foreign = rowidx != neighbour[colidx]            # entry (r, c) whose row is not the one neighbour of c
    ok[np.unique(colidx[foreign])] = False
    return ok


def hand_built_csr(n=1 << 20):
    """A sorted CSR over n vertices (most of them without entries; n >= 2^20: short rows and hub chunks in launches of their own).

    * a star: vertex 1000 with the 600 leaves 2000 .. 2599 (more than 512 entries: a hub row of two chunks); every leaf elides;
    * rows of 2, 4, 5 and 9 entries -- the edges of the batches of four -- that hold a pendant as their FIRST and as their LAST
      entry (leaves 3000 + 10 d and 5000 + 10 d of vertex 4000 + 10 d; the rest of the row are ring vertices);
    * a ring 4500 .. 4539 that supplies those other neighbours (two entries each at least: ordinary rows);
    * the isolated edge 6000 - 6001: two pendants that point at each other, neither elides;
    * pendant 6100 of ring vertex 4530, whose column row 4531 stores as well (a non-symmetric entry): does not elide;
    * pendant 6200 that points at ring vertex 4532, which does not point back: elides (nobody reads it).
    Returns rowptr, colidx, vals, shape and a dict of the named vertices."""
    edges = set()

    def both(u, v):
        edges.add((u, v)); edges.add((v, u))

    centre, leaves = 1000, np.arange(2000, 2600)
    for leaf in leaves:
        both(centre, int(leaf))
    ring = np.arange(4500, 4540)
    for k in range(len(ring)):
        both(int(ring[k]), int(ring[(k + 1) % len(ring)]))
    first, last, mid = {}, {}, {}
    for d in (2, 4, 5, 9):
        v = 4000 + 10 * d
        first[d], last[d], mid[d] = 3000 + 10 * d, 5000 + 10 * d, v
        both(v, first[d]); both(v, last[d])
        for k in range(d - 2):
            both(v, int(ring[3 * k + d]))
    both(6000, 6001)
    both(6100, 4530); edges.add((4531, 6100))
    edges.add((6200, 4532))
    e = np.array(sorted(edges), dtype=np.int64)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(e[:, 0], minlength=n))]).astype(np.int64)
    colidx = e[:, 1].astype(np.int32)
    vals = np.random.default_rng(7).uniform(0.25, 1.0, size=len(colidx)).astype(np.float32)
    named = dict(centre=centre, leaves=leaves, first=first, last=last, mid=mid, isolated=(6000, 6001), shared=6100, shared_reader=4531,
                 no_back=6200, no_back_target=4532, ring=ring)
    return rowptr, colidx, vals, (n, n), named


def expected_elidable(named, n):
    want = np.zeros(n, dtype=bool)
    want[named["leaves"]] = True
    for d in named["mid"]:
        want[named["first"][d]] = want[named["last"][d]] = True
    want[named["no_back"]] = True
    return want

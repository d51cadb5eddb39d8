"""The rules of pendant elision as tests/pendant_graphs.py restates them in numpy, on its hand-built graph: which rows elide and which
do not.  No GPU, no native code."""
import numpy as np

import pendant_graphs as pg


def test_hand_built_graph_elides_exactly_the_named_rows():
    rowptr, colidx, vals, shape, named = pg.hand_built_csr()
    n = shape[0]
    got = pg.elidable_rows(rowptr, colidx)
    assert got.shape == (n,) and np.array_equal(got, pg.expected_elidable(named, n))
    degree = np.diff(rowptr)
    assert degree[named["centre"]] == 600 and got[named["leaves"]].all()
    assert [int(degree[named["mid"][d]]) for d in (2, 4, 5, 9)] == [2, 4, 5, 9]
    for d in (2, 4, 5, 9):                                   # a pendant as the first and as the last entry of the row
        row = colidx[rowptr[named["mid"][d]]:rowptr[named["mid"][d] + 1]]
        assert row[0] == named["first"][d] and row[-1] == named["last"][d] and got[row[0]] and got[row[-1]] and not got[row[1:-1]].any()
    u, v = named["isolated"]
    assert degree[u] == degree[v] == 1 and not got[u] and not got[v]         # two pendants joined to each other
    assert degree[named["shared"]] == 1 and not got[named["shared"]]         # a third row stores its column
    assert named["shared"] in colidx[rowptr[named["shared_reader"]]:rowptr[named["shared_reader"] + 1]]
    target = named["no_back_target"]
    assert got[named["no_back"]] and named["no_back"] not in colidx[rowptr[target]:rowptr[target + 1]]
    assert len(vals) == len(colidx) == rowptr[-1]


def test_rules_one_by_one():
    def rows(*lists):
        rowptr = np.concatenate([[0], np.cumsum([len(l) for l in lists])])
        return pg.elidable_rows(rowptr, np.concatenate([np.asarray(l, dtype=np.int64) for l in lists]))

    assert rows([1], [0, 2], [1]).tolist() == [True, False, True]            # a path: both ends elide, the middle does not
    assert rows([1], [0]).tolist() == [False, False]                         # an isolated edge
    assert rows([0], [0, 1]).tolist() == [False, False]                      # a self loop is no pendant
    assert rows([1], [0, 2], [1, 0]).tolist() == [False, False, False]       # row 2 stores column 0 as well
    assert rows([1], [2, 3], [1], [1]).tolist() == [True, False, True, True]   # no back entry: still elidable
    assert rows([], [2], [1, 3], [2]).tolist() == [False, True, False, True]   # a row without entries
    assert rows([1], [0, 1]).tolist() == [True, False]                # the neighbour's second entry may be its own diagonal

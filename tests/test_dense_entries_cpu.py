"""What the dense and task-head entries refuse, without a device: gnx_dense, gnx_dense_wgrad, gnx_node_ce, gnx_node_ce_backward,
gnx_node_argmax, gnx_edge_scores and gnx_edge_scores_backward -- the return code and the gnx_last_error() text of every argument
check in them, in the order the entry makes them.  Pointers are fake and never dereferenced: each call fails (or returns for an empty
input) before anything is launched.  (gnx_dense_wgrad with n == 0 clears dW on the device: tests/test_gpu_dense.py's business.)"""
import ctypes

import pytest

X, W, B, OUT, G, DW, WORK, IDS, LABELS, LOSS, MEAN = (ctypes.c_void_p(0x1000 * (i + 1)) for i in range(11))
INVALID = -1
ACT_NONE, ACT_RELU = 0, 1


def lib():
    from gnntf import _native
    return _native.lib()


def refused(rc, text):
    assert rc == INVALID
    assert lib().gnx_last_error().decode() == text


def dense(n=100, F=8, O=4, ldx=None, ldw=None, ldo=None, act=ACT_RELU, x=X, w=W, out=OUT):
    return lib().gnx_dense(x, F if ldx is None else ldx, n, F, w, O if ldw is None else ldw, O, B, act, out, O if ldo is None else ldo, None)


@pytest.mark.parametrize("sizes", [dict(n=-1), dict(F=0), dict(O=0), dict(F=(1 << 24) + 1), dict(O=(1 << 20) + 1)],
                         ids=["n<0", "F=0", "O=0", "F>2^24", "O>2^20"])
def test_dense_bad_sizes(sizes):
    s = dict(dict(n=100, F=8, O=4), **sizes)
    refused(dense(**sizes), "gnx_dense: bad sizes (n=%d, F=%d, O=%d)" % (s["n"], s["F"], s["O"]))


@pytest.mark.parametrize("ld", [dict(ldx=7), dict(ldw=3), dict(ldo=3)], ids=["ldx", "ldw", "ldo"])
def test_dense_leading_dimension_below_the_row(ld):
    refused(dense(**ld), "gnx_dense: leading dimension smaller than the row")


@pytest.mark.parametrize("act", [-1, 2, 256])
def test_dense_invalid_activation(act):
    refused(dense(act=act), "gnx_dense: invalid activation %d" % act)
    refused(dense(n=0, act=act), "gnx_dense: invalid activation %d" % act)          # checked before the empty input returns


@pytest.mark.parametrize("null", ["x", "w", "out"])
def test_dense_null_pointer(null):
    refused(dense(**{null: None}), "gnx_dense: NULL pointer")


def test_dense_out_aliasing_x():
    refused(dense(out=X), "gnx_dense: out must not alias X")


def test_dense_no_rows_is_ok_without_pointers():
    assert dense(n=0, x=None, w=None, out=None) == 0
    assert dense(n=0, act=ACT_NONE) == 0


def wgrad(n=100, F=8, O=4, ldx=None, ldg=None, x=X, g=G, dw=DW, work=WORK, work_floats=1 << 20):
    return lib().gnx_dense_wgrad(x, F if ldx is None else ldx, g, O if ldg is None else ldg, n, F, O, dw, work, work_floats, None)


@pytest.mark.parametrize("sizes", [dict(n=-1), dict(F=0), dict(O=0), dict(F=(1 << 20) + 1), dict(O=(1 << 20) + 1)],
                         ids=["n<0", "F=0", "O=0", "F>2^20", "O>2^20"])
def test_dense_wgrad_bad_sizes(sizes):
    refused(wgrad(**sizes), "gnx_dense_wgrad: bad sizes")


@pytest.mark.parametrize("ld", [dict(ldx=7), dict(ldg=3)], ids=["ldx", "ldg"])
def test_dense_wgrad_leading_dimension_below_the_row(ld):
    refused(wgrad(**ld), "gnx_dense_wgrad: leading dimension smaller than the row")


def test_dense_wgrad_null_output():
    refused(wgrad(dw=None), "gnx_dense_wgrad: NULL output")
    refused(wgrad(n=0, dw=None), "gnx_dense_wgrad: NULL output")                    # before the empty input is looked at


@pytest.mark.parametrize("null", ["x", "g"])
def test_dense_wgrad_null_input(null):
    refused(wgrad(**{null: None}), "gnx_dense_wgrad: NULL input")


@pytest.mark.parametrize("scratch", [dict(work_floats=31), dict(work_floats=0), dict(work_floats=-5), dict(work=None)],
                         ids=["F*O-1", "0", "negative", "NULL"])
def test_dense_wgrad_scratch_smaller_than_one_partial(scratch):
    refused(wgrad(**scratch), "gnx_dense_wgrad: the scratch must hold at least F * O floats")


# the five task heads: (entry, call(sizes, pointers)); every call takes sizes m, C, n_rows and leading dimensions, then pointers
def node_ce(m=10, C=4, n_rows=50, ldl=None, ldg=None, p=(X, IDS, LABELS, LOSS, MEAN)):
    return lib().gnx_node_ce(p[0], C if ldl is None else ldl, n_rows, C, p[1], p[2], m, p[3], p[4], None)


def node_ce_backward(m=10, C=4, n_rows=50, ldl=None, ldg=None, p=(X, IDS, LABELS, MEAN, G)):
    return lib().gnx_node_ce_backward(p[0], C if ldl is None else ldl, n_rows, C, p[1], p[2], m, p[3], p[4], C if ldg is None else ldg, None)


def node_argmax(m=10, C=4, n_rows=50, ldl=None, ldg=None, p=(X, OUT)):
    return lib().gnx_node_argmax(p[0], C if ldl is None else ldl, n_rows, C, IDS, m, p[1], None)


def edge_scores(m=10, C=4, n_rows=50, ldl=None, ldg=None, p=(X, IDS, OUT)):
    return lib().gnx_edge_scores(p[0], C if ldl is None else ldl, n_rows, C, p[1], m, W, p[2], None)


def edge_scores_backward(m=10, C=4, n_rows=50, ldl=None, ldg=None, p=(X, IDS, G, DW)):
    return lib().gnx_edge_scores_backward(p[0], C if ldl is None else ldl, n_rows, C, p[1], m, W, p[2], p[3], C if ldg is None else ldg, None)


# entry -> the size arguments it refuses; m == 0 is an empty list (OK) for the last three, and gnx_edge_scores_backward never looks at n_rows
BAD_SIZES = {
    node_ce: [dict(m=0), dict(m=-1), dict(C=0), dict(n_rows=0), dict(ldl=3)],
    node_ce_backward: [dict(m=0), dict(m=-1), dict(C=0), dict(n_rows=0), dict(ldl=3), dict(ldg=3)],
    node_argmax: [dict(m=-1), dict(C=0), dict(n_rows=-1), dict(ldl=3)],
    edge_scores: [dict(m=-1), dict(C=0), dict(n_rows=-1), dict(ldl=3)],
    edge_scores_backward: [dict(m=-1), dict(C=0), dict(ldl=3), dict(ldg=3)],
}
HEADS = list(BAD_SIZES)
N_POINTERS = {node_ce: 5, node_ce_backward: 5, node_argmax: 2, edge_scores: 3, edge_scores_backward: 4}


@pytest.mark.parametrize("entry,sizes", [(e, s) for e in HEADS for s in BAD_SIZES[e]],
                         ids=["%s-%s=%d" % (e.__name__, *next(iter(s.items()))) for e in HEADS for s in BAD_SIZES[e]])
def test_head_bad_sizes(entry, sizes):
    refused(entry(**sizes), "gnx_%s: bad sizes" % entry.__name__)


@pytest.mark.parametrize("entry,which", [(e, i) for e in HEADS for i in range(N_POINTERS[e])],
                         ids=["%s-%d" % (e.__name__, i) for e in HEADS for i in range(N_POINTERS[e])])
def test_head_null_pointer(entry, which):
    p = list(entry.__defaults__[-1])
    p[which] = None
    refused(entry(p=tuple(p)), "gnx_%s: NULL pointer" % entry.__name__)


@pytest.mark.parametrize("entry", [node_argmax, edge_scores, edge_scores_backward], ids=lambda e: e.__name__)
def test_head_empty_list_is_ok_without_pointers(entry):
    assert entry(m=0, p=(None,) * N_POINTERS[entry]) == 0

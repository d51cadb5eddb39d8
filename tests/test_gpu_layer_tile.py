"""The 16-row tile frame of the fused layer kernels (csrc/gnx_layer_device.h; the kernels called here are in gnx_gcnii.hip and gnx_gcn.hip) on the MI355X at the sizes where only the frame can go wrong:
n = 1 (one partial tile), 15, 16 (a full tile), 17 (a tile plus one row) and 129 (a second block with a single live wave), each at
C = 16, 32, 64 (1, 2 and 4 passes over a tile).  Rows of 0 to 3 entries, row 0 without any (at n = 1 the only row); no hub rows -- their
path is that of tests/test_gpu_gcnii_shapes.py, test_gpu_gcnii_wgrad.py and test_gpu_gcn_fused.py.  Every handle runs as built and
after set_row_window(4), another row_order.

gnx_gcnii_step with d_mixed, gnx_gcnii_step_back with S_in / S_out, gnx_gcnii_wgrad and gnx_gcn_step (C_out = C_in and C_out = 7, with
d_agg) are called as those modules call them, over the handle's own values.  Two assertions per entry:
    values   against the float64 references of tests/gcnii_shapes_ref.py and tests/gcn_fused_ref.py with those modules' bounds for the
             same entry (the weight gradient's is test_gpu_gcnii_wgrad.py's): max |got - want| / bound <= 1
    nothing past row n   every output buffer has 16 more rows that hold a sentinel, bit-unchanged after the call: a frame that
             mishandles slot >= n_rows writes exactly there."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import gcn_fused_ref as gref
import gcnii_shapes_ref as ref

pytestmark = pytest.mark.gpu

A_MIX = 0.1
NS = (1, 15, 16, 17, 129)
WIDTHS = (16, 32, 64)
ORDERS = ("built", "window")
WINDOW = 4
PAD = 16                                                 # rows past n in every output buffer
SENTINEL = 1234.5


@pytest.fixture(scope="module")
def gnntf():
    import gnntf
    gnntf.set_default_device("cuda:0")
    yield gnntf
    gnntf.set_default_device(None)


def tile_graph(n):
    """(coo, vals, shape): row i holds min(i % 4, n) entries at distinct columns, values uniform in [0.5, 1.5)."""
    rng = np.random.default_rng(100 + n)
    deg = np.minimum(np.arange(n) % 4, n)
    rows = np.repeat(np.arange(n), deg)
    cols = np.concatenate([rng.choice(n, size=d, replace=False) for d in deg] + [np.empty(0, dtype=np.int64)])
    coo = np.stack([rows, cols], axis=1).astype(np.int64)
    return coo, rng.uniform(0.5, 1.5, size=len(coo)).astype(np.float32), (n, n)


class Handle:
    def __init__(self, gnntf, n, order):
        coo, vals, shape = tile_graph(n)
        self.n, self.order = n, order
        self.g = gnntf.DeviceGraph(gnntf.SparseCOO(coo, vals, shape), device="cuda:0")
        if order == "window":
            self.g.set_row_window(WINDOW)
        self.adj = gnntf.Adjacency(self.g)                # the handle's own values, in either structure
        rowptr, colidx, raw = (x.cpu().numpy() for x in self.g.csr_arrays())
        self.A = sp.csr_matrix((raw.astype(np.float64), colidx, rowptr), shape=shape)
        deg = np.diff(rowptr)
        assert deg[0] == 0 and deg.max() <= 3 and (n < 4 or deg.max() == 3) and self.g.n_hub_rows == 0


@pytest.fixture(scope="module")
def handles(gnntf):
    yield {(n, order): Handle(gnntf, n, order) for n in NS for order in ORDERS}
    for cached in (operands, gcn_operands, want_forward, want_backward, want_wgrad, want_gcn):
        cached.cache_clear()
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def operands(n, C):
    return ref.operands(n, C, seed=3000 + 100 * C + n)


@functools.lru_cache(maxsize=None)
def gcn_operands(n, C_in, C_out):
    return gref.operands(n, C_in, C_out, 4000 + 100 * C_in + 7 * C_out + n)


def graph_of(n):
    coo, vals, shape = tile_graph(n)
    return ref.csr_of(coo, vals, shape)


@functools.lru_cache(maxsize=None)
def want_forward(n, C, relu):
    op = operands(n, C)
    return ref.forward_ref(graph_of(n), op["H"], op["H0"], op["M"], A_MIX, relu)


@functools.lru_cache(maxsize=None)
def want_backward(n, C, s_alpha):
    op = operands(n, C)
    return ref.backward_ref(graph_of(n), op["G"], op["Mt"], A_MIX, op["S_in"], s_alpha)


@functools.lru_cache(maxsize=None)
def want_wgrad(n, C):
    """(want, bound) of dM = T^T G: the criterion of tests/test_gpu_gcnii_wgrad.py (want_wgrad there)."""
    op = operands(n, C)
    A = graph_of(n)
    fwd = ref.forward_ref(A, op["H"], op["H0"], op["M"], A_MIX, False)
    beta, alpha = ref.mix_constants(A_MIX)
    absT = beta * (abs(A) @ np.abs(ref.f64(op["H"]))) + alpha * np.abs(ref.f64(op["H0"]))
    absG = np.abs(ref.f64(op["G"]))
    terms = (n + 4) * ref.U32
    gamma = terms / (1.0 - terms)
    return fwd["T"].T @ ref.f64(op["G"]), gamma * (absT.T @ absG) + fwd["T_bound"].T @ absG


@functools.lru_cache(maxsize=None)
def want_gcn(n, C_in, C_out, relu):
    op = gcn_operands(n, C_in, C_out)
    return gref.forward_ref(graph_of(n), op["X"], op["W"], op["bias"], relu)


def dev(x):
    return torch.from_numpy(np.array(x, order="C")).cuda()            # (a copy: the shared operands are read-only)


def padded(rows, C):
    """A result buffer of ``rows`` + PAD rows, every element the sentinel."""
    return torch.full((rows + PAD, C), SENTINEL, dtype=torch.float32, device="cuda")


def written(buffer, rows, what):
    """The first ``rows`` rows on the host, after the PAD rows behind them were found bit-unchanged."""
    torch.cuda.synchronize()
    tail = buffer[rows:]
    assert torch.equal(tail.view(torch.int32), torch.full_like(tail, SENTINEL).view(torch.int32)), f"{what}: written past row {rows}"
    return buffer[:rows].cpu().numpy()


def within(what, got, want, bound):
    r = ref.ratio(got, want, bound)
    print(f"{what}: error / bound = {r:.3f}")
    assert r <= 1.0, f"{what}: error / bound = {r:.3f}"


def test_the_handles_hold_the_graph(handles):
    """The references are taken over tile_graph itself: the handle holds those entries, whichever row order it runs in."""
    for (n, order), h in handles.items():
        want = graph_of(n)
        assert np.array_equal(h.A.indptr, want.indptr) and np.array_equal(h.A.indices, want.indices) and np.array_equal(h.A.data, want.data)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("n", NS)
def test_forward(gnntf, handles, n, C, order):
    nat = gnntf.sparse.nat
    h = handles[n, order]
    d = {k: dev(v) for k, v in operands(n, C).items()}
    for relu in (True, False):
        where = f"gnx_gcnii_step n={n} C={C} {order} relu={relu}"
        out, mixed = padded(n, C), padded(n, C)
        nat.check(nat.lib().gnx_gcnii_step(h.g.handle, nat.ptr(h.adj.vals), nat.ptr(d["H"]), nat.ptr(d["H0"]), A_MIX, C, nat.ptr(d["M"]), C,
                                           nat.ACT_RELU if relu else nat.ACT_NONE, nat.ptr(out), nat.ptr(mixed), nat.current_stream()))
        assert h.g.last_kernel() == "spmm_gcnii_mfma"
        want = want_forward(n, C, relu)
        within(where + " out", written(out, n, where + " out"), want["out"], want["out_bound"])
        within(where + " T", written(mixed, n, where + " T"), want["T"], want["T_bound"])


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("n", NS)
def test_backward(gnntf, handles, n, C, order):
    nat = gnntf.sparse.nat
    h = handles[n, order]
    d = {k: dev(v) for k, v in operands(n, C).items()}
    for s_alpha in (1.0, 0.5):
        where = f"gnx_gcnii_step_back n={n} C={C} {order} s_alpha={s_alpha}"
        dH, S = padded(n, C), padded(n, C)
        nat.check(nat.lib().gnx_gcnii_step_back(h.g.handle, nat.ptr(h.adj.vals_t), nat.ptr(d["G"]), A_MIX, C, nat.ptr(d["Mt"]), C, nat.ptr(dH),
                                                nat.ptr(d["S_in"]), s_alpha, nat.ptr(S), None, nat.current_stream()))
        assert h.g.last_kernel() == "spmm_gcnii_back_mfma"
        want = want_backward(n, C, s_alpha)
        within(where + " dH", written(dH, n, where + " dH"), want["dH"], want["dH_bound"])
        within(where + " S", written(S, n, where + " S"), want["S"], want["S_bound"])


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("n", NS)
def test_weight_gradient(gnntf, handles, n, C, order):
    nat = gnntf.sparse.nat
    h = handles[n, order]
    d = {k: dev(v) for k, v in operands(n, C).items()}
    where = f"gnx_gcnii_wgrad n={n} C={C} {order}"
    dM, hub, work = padded(C, C), padded(n, C), padded(C, C)            # one slab (sparse._dense_wgrad's sizing at these n)
    nat.check(nat.lib().gnx_gcnii_wgrad(h.g.handle, nat.ptr(h.adj.vals), nat.ptr(d["H"]), nat.ptr(d["H0"]), A_MIX, C, nat.ptr(d["G"]), nat.ptr(dM),
                                        nat.ptr(hub), nat.ptr(work), C * C, nat.current_stream()))
    assert h.g.last_kernel() == "gcnii_wgrad_mfma"
    want, bound = want_wgrad(n, C)
    within(where, written(dM, C, where + " dM"), want, bound)
    written(work, C, where + " work")
    written(hub, 0, where + " hub rows (there are none)")


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("C_out", ["C_in", 7])
@pytest.mark.parametrize("C_in", WIDTHS)
@pytest.mark.parametrize("n", NS)
def test_gcn_layer(gnntf, handles, n, C_in, C_out, order):
    nat = gnntf.sparse.nat
    h = handles[n, order]
    C_out = C_in if C_out == "C_in" else C_out
    op = gcn_operands(n, C_in, C_out)
    Xd, Wd, bd = dev(op["X"]), dev(op["W"]), dev(op["bias"])
    for relu in (True, False):
        where = f"gnx_gcn_step n={n} {C_in}->{C_out} {order} relu={relu}"
        out, agg = padded(n, C_out), padded(n, C_in)
        nat.check(nat.lib().gnx_gcn_step(h.g.handle, nat.ptr(h.adj.vals), nat.ptr(Xd), C_in, C_in, nat.ptr(Wd), C_out, C_out, nat.ptr(bd),
                                         nat.ACT_RELU if relu else nat.ACT_NONE, 0.0, 0, 0, nat.ptr(out), C_out, nat.ptr(agg), None,
                                         nat.current_stream()))
        assert h.g.last_kernel() == f"k_spmm_gcn<{C_in}>"
        want = want_gcn(n, C_in, C_out, relu)
        within(where + " out", written(out, n, where + " out"), want["out"], want["out_bound"])
        within(where + " agg", written(agg, n, where + " agg"), want["agg"], want["agg_bound"])

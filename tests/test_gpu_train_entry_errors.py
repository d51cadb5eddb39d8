"""What the six loop entries of the fused training propagation (gnx_spmm_dropped_chained / _back and their _ord and _bf16 forms)
answer to a call with exactly one fault: the return code, the exact message, and result buffers left as they were.  Argument
refusals only: every refused call returns before anything is built or launched.

The expected messages are spelled out from the library's source.  One of them is not what one might expect: on a handle with
duplicate entries and no entry tables the _ord entries answer GNX_ERR_UNSUPPORTED like the others, but their message (it comes from
the gather order's own admission) says that the gather order exists for handles without duplicates and does not name
gnx_graph_enable_entry_dropout."""
import numpy as np
import pytest
import torch

import graphs

pytestmark = pytest.mark.gpu

C = 16
N = 64
SENTINEL = -77.5                       # 8 significant bits: exactly representable in bf16
SKIP_EMPTY = 256
ENTRIES = ["gnx_spmm_dropped_chained", "gnx_spmm_dropped_chained_ord", "gnx_spmm_dropped_chained_bf16",
           "gnx_spmm_dropped_back", "gnx_spmm_dropped_back_ord", "gnx_spmm_dropped_back_bf16"]


@pytest.fixture(scope="module")
def gnntf():
    import gnntf
    gnntf.set_default_device("cuda:0")
    yield gnntf
    gnntf.set_default_device(None)


@pytest.fixture(scope="module")
def handles(gnntf):
    """square: 64 vertices, no duplicates; block: 20 x 30 made a vertex block; dups: 64 vertices, duplicate entries, no entry
    tables; window: 64 vertices with a row window."""
    from gnntf import _native as nat
    coo, vals, shape = graphs.random_coo(N, N, 400, seed=2, dup_frac=0.3)
    dups = gnntf.DeviceGraph(gnntf.SparseCOO(coo, vals, shape), device="cuda:0")
    assert dups.nnz_entries > dups.nnz and not dups.entry_dropout
    once = np.unique(coo, axis=0)
    ones = np.ones(len(once), dtype=np.float32)
    square = gnntf.DeviceGraph(gnntf.SparseCOO(once, ones, shape), device="cuda:0")
    window = gnntf.DeviceGraph(gnntf.SparseCOO(once, ones, shape), device="cuda:0")
    window.set_row_window(16)
    rcoo = np.unique(graphs.random_coo(20, 30, 80, seed=1, dup_frac=0.0)[0], axis=0)
    block = gnntf.DeviceGraph(gnntf.SparseCOO(rcoo, np.ones(len(rcoo), dtype=np.float32), (20, 30)), device="cuda:0")
    gid = torch.arange(30, dtype=torch.int32, device="cuda")
    nat.check(nat.lib().gnx_graph_set_block(block.handle, 100, 5, nat.ptr(gid), nat.current_stream()))
    return dict(square=square, block=block, dups=dups, window=window, gid=gid)


class Buffers:
    """Operands of one call over a graph of n_rows x n_cols: X gathered ([n_cols, C], f32 or bf16), H0 / the running sum S and the
    results out / Y ([n_rows, C]), degree scales of n_cols.  The results hold the sentinel."""

    def __init__(self, n_rows, n_cols, bf16):
        rows = torch.bfloat16 if bf16 else torch.float32
        gen = torch.Generator(device="cuda").manual_seed(5)
        self.X = torch.randn((n_cols, C), device="cuda", generator=gen).to(rows)
        self.H0 = torch.randn((n_rows, C), device="cuda", generator=gen)
        self.D = torch.rand(n_cols, device="cuda", generator=gen) + 0.5
        self.D_next = torch.rand(n_cols, device="cuda", generator=gen) + 0.5
        self.out = torch.full((n_rows, C), SENTINEL, device="cuda")
        self.S = torch.full((n_rows, C), SENTINEL, device="cuda")
        self.S2 = torch.full((n_rows, C), SENTINEL, device="cuda")
        self.Y = torch.full((n_rows, C), SENTINEL, device="cuda", dtype=rows)

    def untouched(self):
        torch.cuda.synchronize()
        return all(bool((t.float() == SENTINEL).all()) for t in (self.out, self.S, self.S2, self.Y))


def call(name, handle, b, **over):
    """The valid call of entry ``name`` over ``handle`` with buffers ``b``, changed by ``over``; returns (code, message)."""
    from gnntf import _native as nat
    lib = nat.lib()
    P = lambda t: nat.ptr(t)
    if "chained" in name:
        a = dict(D=b.D, p=0.5, D_next=b.D_next, X=b.X, ldx=C, C=C, H0=b.H0, ldh0=C, act=0, out=b.out, out_bf16=0, ldo=C, order=3)
        a.update(over)
        args = [handle, P(a["D"]), a["p"], 1, 2, 0, P(a["D_next"]), P(a["X"]), a["ldx"], a["C"], P(a["H0"]), a["ldh0"], 0.9, 0.1, a["act"],
                P(a["out"])]
        args += [a["out_bf16"], a["ldo"]] if name.endswith("_bf16") else [a["ldo"], a["order"]] if name.endswith("_ord") else [a["ldo"]]
    else:
        a = dict(D=b.D, p=0.5, D_next=b.D_next, X=b.X, ldx=C, C=C, S_in=b.S, S_out=b.S, Y=b.Y, ldy=C, act=0, order=3)
        a.update(over)
        args = [handle, P(a["D"]), a["p"], 1, 2, 0, P(a["D_next"]), P(a["X"]), a["ldx"], a["C"], P(a["S_in"]), C, 1.0, 0.09, P(a["S_out"]), C,
                0.9, P(a["Y"]), a["ldy"], a["act"]]
        args += [a["order"]] if name.endswith("_ord") else []
    rc = getattr(lib, name)(*args, nat.current_stream())
    return rc, (lib.gnx_last_error() or b"").decode()


def single_faults(name, b):
    """(what, changed arguments, message) of every single-fault call the entry's arguments allow; all return -1."""
    rate = (name + ": " if name.endswith("_bf16") else "") + "dropout rate 1 outside [0, 1)"
    faults = [("width 0", dict(C=0), name + ": feature width 0 not in [1, 2^20]"),
              ("ldx < C", dict(ldx=C - 1), name + ": leading dimension smaller than C"),
              ("p = 1.0", dict(p=1.0), rate)]
    if "chained" in name:
        faults += [("out == X", dict(out=b.X), name + ": out must not alias X"),
                   ("bad act", dict(act=7), name + ": invalid activation 7"),
                   ("NULL D", dict(D=None), name + ": NULL degree scales")]
        if name.endswith("_bf16"):
            faults += [("out_bf16 = 2", dict(out_bf16=2), name + ": out_bf16 must be 0 or 1")]
    else:
        faults += [("out == X", dict(S_out=b.X), name + ": out must not alias X"),
                   ("bad act", dict(act=1), name + ": act must be GNX_ACT_NONE or GNX_ACT_SKIP_EMPTY"),
                   ("SKIP_EMPTY, S_in != S_out", dict(act=SKIP_EMPTY, S_in=b.S2), name + ": GNX_ACT_SKIP_EMPTY needs the sum updated in place"),
                   ("NULL D", dict(D=None), name + ": NULL degree scales / running sum"),
                   ("NULL S_in", dict(S_in=None), name + ": NULL degree scales / running sum"),
                   ("Y_out aliasing S_out", dict(Y=b.S), name + ": the pre-scaled output needs a buffer of its own"),
                   ("ldy < C", dict(ldy=C - 1), name + ": the pre-scaled output needs a buffer of its own")]
    if name.endswith("_ord"):
        faults += [("bad order bits", dict(order=4), name + ": invalid order flags 4")]
    return faults


@pytest.mark.parametrize("name", ENTRIES)
def test_single_faults(handles, name):
    b = Buffers(N, N, name.endswith("_bf16"))
    for what, over, message in single_faults(name, b):
        rc, got = call(name, handles["square"].handle, b, **over)
        print(f"{name}, {what}: {rc} {got!r}")
        assert (rc, got) == (-1, message), what
        assert b.untouched(), what
    assert call(name, handles["square"].handle, b)[0] == 0            # the call the faults were put into is a valid one
    torch.cuda.synchronize()


DUPLICATES = ": the graph holds duplicate COO entries: call gnx_graph_enable_entry_dropout on the handle first (or use gnx_graph_normalize + gnx_spmm)"
BF16_BLOCK = (": the handle is a vertex block (gnx_graph_set_block): bf16 training storage covers stand-alone graphs only -- "
              "use the f32 entry")
ORD_BLOCK = ": the handle is a vertex block (gnx_graph_set_block): the gather order exists for stand-alone graphs only"
ORD_DUPLICATES = ": the graph holds duplicate COO entries: the gather order exists for handles without duplicates only"
ORD_WINDOW = (": the handle has a row window (gnx_graph_set_row_window): its numbering carries locality already, the gather "
              "order is not built")
ADMISSION = {   # entry -> what a vertex block, duplicates without tables and a row window get: (code, message behind the name)
    "gnx_spmm_dropped_chained": ((0, None), (-4, DUPLICATES), (0, None)),
    "gnx_spmm_dropped_chained_ord": ((-4, ORD_BLOCK), (-4, ORD_DUPLICATES), (-4, ORD_WINDOW)),
    "gnx_spmm_dropped_chained_bf16": ((-4, BF16_BLOCK), (-4, DUPLICATES), (0, None)),
    "gnx_spmm_dropped_back": ((-1, ": needs a square stand-alone graph"), (-4, DUPLICATES), (0, None)),
    "gnx_spmm_dropped_back_ord": ((-4, ORD_BLOCK), (-4, ORD_DUPLICATES), (-4, ORD_WINDOW)),
    "gnx_spmm_dropped_back_bf16": ((-4, BF16_BLOCK), (-4, DUPLICATES), (0, None)),
}


@pytest.mark.parametrize("name", ENTRIES)
def test_handle_admission(handles, name):
    bf16 = name.endswith("_bf16")
    for kind, (code, tail) in zip(("block", "dups", "window"), ADMISSION[name]):
        b = Buffers(20, 30, bf16) if kind == "block" else Buffers(N, N, bf16)
        rc, got = call(name, handles[kind].handle, b)
        print(f"{name}, {kind}: {rc} {got!r}")
        assert rc == code, kind
        if code != 0:
            assert got == name + tail, kind
            assert b.untouched(), kind
    torch.cuda.synchronize()

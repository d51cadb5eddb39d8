"""What the GCNII layer's C entries refuse (gnx_gcnii_step, gnx_gcnii_step_drop, gnx_gcnii_step_bf16, gnx_gcnii_step_back), called straight
at the library: one table of calls with ONE thing wrong each, the return code and the words of the message (the entry's name and the
cause), and after every refusal the sentinel-filled result buffers untouched and last_kernel unchanged.  The three bf16 training
entries have their table in tests/test_gpu_gcnii_bf16_training.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

A_MIX = 0.1
N, HUB, N_HUB = 3000, 1500, 900
SEED, STREAM = 7, 2
INVALID, UNSUPPORTED = -1, -4
SENTINEL = 9.0
RESULTS = ("out", "out_b", "mixed", "work", "dH", "S")                     # the buffers an entry may write: sentinel-filled, never written here


@pytest.fixture(scope="module")
def gnntf():
    import gnntf
    gnntf.set_default_device("cuda:0")
    yield gnntf
    gnntf.set_default_device(None)


def directed_coo():
    """The graph of tests/test_gpu_gcnii_back.py: DIRECTED, 3 000 vertices, about 20 000 entries, no duplicates; sources below 2 900
    and targets from 100 up; column 1 500 holds 900 entries."""
    rng = np.random.default_rng(11)
    src, dst = rng.integers(0, N - 100, size=19100), rng.integers(100, N, size=19100)
    hub_src = rng.permutation(N - 100)[:N_HUB]
    key = np.unique(np.concatenate([src * N + dst, hub_src * N + HUB]))
    coo = np.stack([key // N, key % N], axis=1).astype(np.int64)
    coo = coo[rng.permutation(len(coo))]
    vals = rng.uniform(0.5, 1.5, size=len(coo)).astype(np.float32)
    return coo, vals, (N, N)


def buffers(C):
    """Operands (zeros, M = I), sentinel-filled results (``out_b``: a bf16 one) and a scratch buffer of width C, all [N, C] contiguous and
    of their own."""
    f32 = lambda: torch.full((N, C), SENTINEL, device="cuda")
    zeros = lambda: torch.zeros(N, C, device="cuda")
    return dict(H=zeros(), Hb=torch.zeros(N, C, device="cuda", dtype=torch.bfloat16), H0=zeros(), M=torch.eye(C, device="cuda"), G=zeros(),
                S_in=zeros(), out=f32(), out_b=f32().to(torch.bfloat16), mixed=f32(), work=f32(), dH=f32(), S=f32(), scratch=zeros())


@pytest.fixture(scope="module")
def shared(gnntf):
    """Made once, never changed: ``hub`` = the transpose of the directed graph (its forward structure has the hub row), ``flat`` = the
    graph itself (no hub row forward; the transposed structure, which the backward walks, has it), ``wide`` = the same entries in a
    3 000 x 3 001 shape; per handle its values in both orders; the buffers per width.  Every handle has run one launch, so that
    last_kernel has a name to keep."""
    coo, vals, shape = directed_coo()
    out = dict(buffers={C: buffers(C) for C in (16, 40, 260)})
    for name, idx, shp in (("hub", coo[:, ::-1].copy(), shape), ("flat", coo, shape), ("wide", coo, (N, N + 1))):
        g = gnntf.DeviceGraph(gnntf.SparseCOO(idx, vals, shp), device="cuda:0")
        deg = np.diff(g.csr_arrays()[0].cpu().numpy())
        adj = gnntf.Adjacency(g, g.csr_arrays()[2])
        gnntf.spmm(adj, torch.zeros(shp[1], 16, device="cuda"))
        out[name] = dict(g=g, vals=adj.vals, vals_t=adj.transposed_values() if name != "wide" else None, hubs=int((deg > 512).sum()))
    assert out["hub"]["hubs"] == 1 and out["flat"]["hubs"] == 0
    torch.cuda.synchronize()
    return out


# ---- the entries: argument names in the order of the C signature, and a good call's values (a str names a buffer) ----------------------
def good(entry, C):
    fwd = dict(vals="vals", H="H", H0="H0", a=A_MIX, C=C, M="M", ldm=C, act=1)
    if entry == "gnx_gcnii_step":
        return dict(fwd, out="out", mixed="mixed")
    if entry == "gnx_gcnii_step_drop":
        return dict(fwd, p=0.5, seed=SEED, stream_id=STREAM, out="out", mixed="mixed")
    if entry == "gnx_gcnii_step_bf16":
        return dict(fwd, H="Hb", out="out", out_bf16=0, work="work")
    assert entry == "gnx_gcnii_step_back"
    return dict(vals="vals_t", G="G", a=A_MIX, C=C, M="M", ldm=C, dH="dH", S_in="S_in", s_alpha=1.0, S="S", work="work")


F32_FORWARD = ("gnx_gcnii_step", "gnx_gcnii_step_drop")
FORWARD = F32_FORWARD + ("gnx_gcnii_step_bf16",)
BACK = "gnx_gcnii_step_back"
EVERY = FORWARD + (BACK,)


def rows():
    """(entries, graph, C, the one thing wrong, code, words of the message beside the entry's name[, False: the refusal follows a launch])"""
    t = [
        (FORWARD, "hub", 16, dict(act=7), INVALID, ["invalid activation"]),
        (EVERY, "wide", 16, dict(), INVALID, ["square graph"]),
        (FORWARD, "hub", 16, dict(H0=None), INVALID, ["NULL H0 / M"]),
        (FORWARD, "hub", 16, dict(M=None), INVALID, ["NULL H0 / M"]),
        (FORWARD, "hub", 16, dict(ldm=15), INVALID, ["ldm < C"]),
        ((BACK,), "flat", 16, dict(M=None), INVALID, ["NULL Mt"]),
        ((BACK,), "flat", 16, dict(ldm=15), INVALID, ["ldmt < C"]),
        # each aliasing rule
        (F32_FORWARD, "hub", 16, dict(out="H"), INVALID, ["out must not alias X"]),
        (("gnx_gcnii_step_bf16",), "hub", 16, dict(out="Hb"), INVALID, ["out must not alias X"]),
        ((BACK,), "flat", 16, dict(dH="G"), INVALID, ["out must not alias X"]),
    ]
    t += [(F32_FORWARD, "hub", 16, dict(mixed=other), INVALID, ["d_mixed must be a buffer of its own"]) for other in ("out", "H", "H0")]
    t += [(("gnx_gcnii_step_bf16",), "hub", 16, dict(out=other), INVALID, ["out must not alias H0 / M"]) for other in ("H0", "M")]
    t += [(("gnx_gcnii_step_bf16",), "hub", 16, dict(work=other), INVALID, ["d_work must be a buffer of its own"])
          for other in ("out", "Hb", "H0", "M", "vals")]
    t += [((BACK,), "flat", 16, dict(dH=other), INVALID, ["dH must not alias"]) for other in ("S_in", "S", "M")]
    t += [((BACK,), "flat", 16, dict(S=other), INVALID, ["S_out must not alias"]) for other in ("G", "M")]
    t += [((BACK,), "flat", 16, dict(work=other), INVALID, ["d_work must be a buffer of its own"]) for other in ("G", "dH", "S_in", "S", "M")]
    t += [
        # the buffers a width or a graph needs
        (F32_FORWARD, "flat", 40, dict(mixed=None), INVALID, ["width 40", "d_mixed"]),
        (("gnx_gcnii_step_bf16",), "hub", 16, dict(work=None), INVALID, ["d_work", "hub rows"]),
        (("gnx_gcnii_step_bf16",), "flat", 40, dict(work=None), INVALID, ["d_work", "two launches"]),
        ((BACK,), "flat", 40, dict(work=None), INVALID, ["width 40", "d_work"]),
        (("gnx_gcnii_step_drop",), "hub", 16, dict(p=1.0), INVALID, ["outside [0, 1)"]),
        ((BACK,), "flat", 16, dict(S=None), INVALID, ["S_in without S_out"]),
        (("gnx_gcnii_step_bf16",), "hub", 16, dict(out_bf16=2), INVALID, ["out_bf16 must be 0 or 1"]),
        # a bf16 result wider than one panel of the dense kernel.  The refusal belongs to the two-launch form, whose first launch fills
        # d_work: the scratch buffer stands there, every result stays untouched, and what last_kernel says afterwards is not pinned
        (("gnx_gcnii_step_bf16",), "flat", 260, dict(out="out_b", out_bf16=1, work="scratch"), UNSUPPORTED, ["C <= 256"], False),
    ]
    return [(entry, row[1], row[2], row[3], row[4], row[5], len(row) == 6) for row in t for entry in row[0]]


def row_id(row):
    entry, graph, C, wrong = row[:4]
    return "-".join([entry[4:], graph, str(C)] + [f"{k}={v}" for k, v in wrong.items()])


def call(lib, nat, shared, entry, graph, C, wrong):
    """The good call of ``entry`` at width C on handle ``graph`` with ``wrong`` laid over it."""
    h = shared[graph]
    named = dict(shared["buffers"][C], vals=h["vals"], vals_t=h["vals_t"])
    args = dict(good(entry, C), **wrong)
    values = [nat.ptr(named[v]) if isinstance(v, str) else v for v in args.values()]
    return getattr(lib, entry)(h["g"].handle, *values, nat.current_stream())


@pytest.mark.parametrize("row", rows(), ids=row_id)
def test_refusal_names_the_cause_and_launches_nothing(gnntf, shared, row):
    entry, graph, C, wrong, code, words, launches_nothing = row
    nat = gnntf.sparse.nat
    lib = nat.lib()
    g = shared[graph]["g"]
    before = g.last_kernel()
    assert before
    rc = call(lib, nat, shared, entry, graph, C, wrong)
    message = lib.gnx_last_error()
    assert rc == code and all(word.encode() in message for word in [entry + ":"] + words), (rc, message)
    torch.cuda.synchronize()
    assert all(bool((shared["buffers"][C][k] == SENTINEL).all()) for k in RESULTS)
    assert g.last_kernel() == before or not launches_nothing


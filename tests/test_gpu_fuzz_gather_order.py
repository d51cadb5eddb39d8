"""A seeded fuzz slice of its own, beside test_gpu_fuzz.py: kind ``gather_order`` -- the fused training loop of sparse.ppr_loop with
the iterate kept in the library's gather order against the same loop in the caller's order.  20 seeded random shapes (n 64 ... 20 000,
mean degree 2 ... 40, C 1 ... 140, K 1 ... 4); forward result and dH0 must be the same float32 bits."""
import numpy as np
import pytest
import torch

import graphs

pytestmark = pytest.mark.gpu

CASES, SEED, DROP_SEED, A = 20, 4242, 5, 0.1


def draw(case):
    rng = np.random.default_rng([SEED, case])
    n = int(round(np.exp(rng.uniform(np.log(64), np.log(20_000)))))
    degree = float(np.exp(rng.uniform(np.log(2), np.log(40))))
    C = int(rng.integers(1, 141))
    K = int(rng.integers(1, 5))
    p = float(rng.choice([0.1, 0.5, 0.9]))
    coo, _, shape = graphs.rmat_symmetric_coo(n, max(1, int(n * degree / 2)), seed=int(rng.integers(1 << 30)))
    vals = rng.uniform(0.25, 2.0, size=len(coo)).astype(np.float32)
    H0 = rng.standard_normal((n, C)).astype(np.float32)
    G = rng.standard_normal((n, C)).astype(np.float32)
    return dict(case=case, n=n, C=C, K=K, p=p, coo=coo, vals=vals, shape=shape, H0=H0, G=G)


@pytest.fixture(scope="module")
def gnntf():
    import gnntf
    gnntf.set_default_device("cuda:0")
    yield gnntf
    gnntf.set_default_device(None)


def run(gnntf, g, s, gather_order):
    sparse = gnntf.sparse
    scales = sparse.dropped_degree_scales(g, s["p"], DROP_SEED, s["case"], s["K"])
    make_adj = lambda k, bwd=False: sparse.dropped_adjacency(g, s["p"], DROP_SEED, s["case"] + k, D=scales[k])
    H0 = torch.from_numpy(s["H0"]).cuda().requires_grad_(True)
    out = sparse.ppr_loop(make_adj, H0, A, s["K"], gather_order=gather_order)
    out.backward(torch.from_numpy(s["G"]).cuda())
    return out.detach(), H0.grad.detach(), g.last_kernel()


def test_drawn_shapes_cover_the_ranges():
    shapes = [draw(case) for case in range(CASES)]
    assert all(64 <= s["n"] <= 20_000 and 1 <= s["C"] <= 140 and 1 <= s["K"] <= 4 for s in shapes)
    assert min(s["K"] for s in shapes) == 1 and max(s["K"] for s in shapes) == 4        # K = 1: no chained loop, today's path
    assert min(s["C"] for s in shapes) <= 16 and max(s["C"] for s in shapes) > 128     # sub-wave groups and one wave per row


@pytest.mark.parametrize("case", range(CASES))
def test_gather_order_fuzz(gnntf, case):
    s = draw(case)
    g = gnntf.DeviceGraph(gnntf.SparseCOO(s["coo"], s["vals"], s["shape"]), device="cuda:0")
    want = run(gnntf, g, s, "caller")
    got = run(gnntf, g, s, "relabelled")
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), {k: s[k] for k in ("case", "n", "C", "K", "p")}
    assert got[2].endswith("_ord") == (s["K"] > 1) and not want[2].endswith("_ord"), (got[2], want[2])
    assert torch.isfinite(want[0]).all() and torch.isfinite(want[1]).all()

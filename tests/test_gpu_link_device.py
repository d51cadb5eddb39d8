"""The device link task on the MI355X (csrc/gnx_link.hip): gnx_sample_negatives, gnx_edge_plan and gnx_edge_scores_backward_sorted through
gnntf._native, then device_negative_sampling + LinkPrediction under train(capture=False / True).

Criteria, none of them fitted to a kernel:
  * the sampler's buffer and fallback count: EQUAL to tests/link_device_ref.py, numpy over oracle.gnntf_oracle.hash_u24;
  * the plan: equal to the reference's stable sort and chunk list;
  * the sorted backward: bit for bit the float32 emulation of the summation order include/gnx.h states, and within the float64 bound
    1e-4 |want| + (k + 4) u sum |term| that tests/test_gpu_heads.py holds the atomic form to;
  * captured training: every parameter torch.equal to the eager run's.
Operands that are column slices of a wider tensor sit in NaN; buffers the entries write carry a sentinel wherever nothing may be written."""
import numpy as np
import pytest
import torch

import link_device_ref as ref

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
MARK = -77                           # sentinel of the integer buffers


@pytest.fixture(scope="module")
def gnntf():
    import gnntf
    gnntf.set_default_device("cuda:0")
    yield gnntf
    gnntf.set_default_device(None)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    return np.ascontiguousarray(t.detach().cpu().numpy())


def filled(shape, value, dtype=torch.float32):
    return torch.full(shape, value, dtype=dtype, device="cuda")


def untouched(t, value):
    return bool(torch.equal(t, torch.full_like(t, value)))


def place(x, pitch):
    """``x`` [n, C] on the device as it is ("dense"), or as a column slice of a wider tensor of NaNs: "odd" = columns 1 .. C of
    [n, C + 3] (a base 4 bytes past a row's start), "quad" = columns 4 .. C + 3 of a width that is a multiple of 4."""
    if pitch == "dense":
        return dev(x)
    n, C = x.shape
    left, ld = (1, C + 3) if pitch == "odd" else (4, (C + 11) // 4 * 4)
    view = filled((n, ld), float("nan"))[:, left:left + C]
    view.copy_(dev(x))
    assert view.stride(0) == ld > C and view.data_ptr() % 16 == (4 if pitch == "odd" else 0)
    return view


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float32).view(np.int32), np.asarray(b, dtype=np.float32).view(np.int32))


# ---- the sampler -----------------------------------------------------------------------------------------------------------------------
def symmetric_graph(gnntf, pairs, n):
    """(DeviceGraph, rowptr, colidx, set of stored (row, col)) of the undirected ``pairs`` stored in both directions."""
    coo = np.concatenate([pairs, pairs[:, ::-1]]).astype(np.int64)
    g = gnntf.DeviceGraph(gnntf.SparseCOO(coo, np.ones(len(coo), dtype=np.float32), (n, n)), device="cuda:0")
    rowptr, colidx = ref.csr_pattern(coo, n)
    return g, rowptr, colidx, set(map(tuple, coo.tolist()))


@pytest.fixture(scope="module")
def ordinary(gnntf):
    """300 nodes, about 1500 undirected pairs: degrees around 10."""
    rng = np.random.default_rng(17)
    pairs = rng.integers(0, 300, size=(1500, 2))
    pairs = np.unique(pairs[pairs[:, 0] != pairs[:, 1]], axis=0)
    return symmetric_graph(gnntf, pairs, 300) + (pairs,)


def raw_sample(gnntf, g, positives, samples, candidates, seed, stream, max_tries=32, expect=0):
    """gnx_sample_negatives itself into sentinel-filled buffers: (edges [m (1 + samples), 2], fallbacks); 8 rows past the buffer's end and
    the counter's neighbour must keep the sentinel.  ``expect`` != 0: the call must fail with that code and write nothing at all."""
    nat = gnntf._native
    m = len(positives)
    rows = m * (1 + max(samples, 0))
    out, count = filled((rows + 8, 2), MARK, torch.int64), filled((2,), 0, torch.int64)
    count[1] = MARK
    pos, cand = dev(np.asarray(positives, dtype=np.int64).reshape(-1, 2)), None if candidates is None else dev(np.asarray(candidates, dtype=np.int64))
    rc = nat.lib().gnx_sample_negatives(g.handle, nat.ptr(pos), m, samples, nat.ptr(cand), g.n_rows if candidates is None else len(candidates),
                                        max_tries, seed, stream, nat.ptr(out), nat.ptr(count), nat.current_stream())
    torch.cuda.synchronize()
    assert rc == expect, nat.lib().gnx_last_error()
    assert untouched(out[rows:], MARK) and int(count[1]) == MARK, "gnx_sample_negatives wrote past its outputs"
    if expect != 0:
        assert untouched(out, MARK) and int(count[0]) == 0
    return host(out[:rows]), int(count[0])


@pytest.mark.parametrize("listed", (False, True))
@pytest.mark.parametrize("samples", (1, 3))
def test_sampler_equals_the_reference(gnntf, ordinary, samples, listed):
    g, rowptr, colidx, entries, pairs = ordinary
    candidates = None if not listed else np.random.default_rng(3).choice(300, size=40, replace=False)
    for m in (0, 1, 257):
        positives = pairs[:m]
        seed, stream = 11, 40 + m
        want, fallbacks, _ = ref.sample_negatives(rowptr, colidx, 300, positives, samples, candidates, 32, seed, stream)
        assert fallbacks == 0 and want.shape == (m * (1 + samples), 2)
        for row, (u, w) in enumerate(want.tolist()):                     # the reference itself: the layout and the three conditions
            u0, v0 = positives[row // (1 + samples)]
            assert u == u0
            if row % (1 + samples) == 0:
                assert w == v0
            else:
                assert w != u0 and w != v0 and (u, w) not in entries and (w, u) not in entries
                assert candidates is None or w in candidates
        got, count = raw_sample(gnntf, g, positives, samples, candidates, seed, stream)
        assert np.array_equal(got, want) and count == 0
        again, _ = raw_sample(gnntf, g, positives, samples, candidates, seed, stream)
        assert np.array_equal(again, got)                                # one (seed, stream): the same bits
        if m == 257:                                                     # the handle's counter is added to the stream id
            counter = torch.tensor([5], dtype=torch.int64, device="cuda")
            g.set_dropout_counter(counter)
            try:
                shifted, _ = raw_sample(gnntf, g, positives, samples, candidates, seed, stream)
            finally:
                g.set_dropout_counter(None)
            want5, _, _ = ref.sample_negatives(rowptr, colidx, 300, positives, samples, candidates, 32, seed, stream + 5)
            assert np.array_equal(shifted, want5) and not np.array_equal(want5, want)


def test_sampler_saturated_sources(gnntf):
    """Source 0 is linked to 7 of the 8 candidates, source 1 to all 8.  The seed is picked on the CPU: the reference accepts source 0's
    negative after at least two tries and falls back for source 1 -- the launch returns (its loop is bounded by max_tries) with the
    reference's edges and count."""
    cands = np.arange(10, 18)
    pairs = np.array([(0, c) for c in cands[:7]] + [(1, c) for c in cands])
    g, rowptr, colidx, _ = symmetric_graph(gnntf, pairs, 20)
    positives = np.array([(0, 10), (1, 10)])
    for seed in range(200):
        want, fallbacks, tries = ref.sample_negatives(rowptr, colidx, 20, positives, 1, cands, 8, seed, 3)
        if fallbacks == 1 and 2 <= tries[0] and want[1, 1] == 17:
            break
    else:
        raise AssertionError("no seed below 200 shows both cases")
    assert tries[1] == 8 and want[3, 0] == 1 and want[3, 1] in cands
    got, count = raw_sample(gnntf, g, positives, 1, cands, seed, 3, max_tries=8)
    assert np.array_equal(got, want) and count == 1


def test_sampler_indices_past_2_to_24(gnntf):
    """2^24 + 3 rows: a candidate index takes more than the 24 bits of one hash.  The stream is searched on the CPU for a first draw at or
    past 2^24 (3 rows in 16 million: x K >= 2^72)."""
    n, m = 2 ** 24 + 3, 2000
    rng = np.random.default_rng(5)
    pairs = rng.integers(0, n, size=(500, 2))
    pairs[:4] = [(2 ** 24, 7), (2 ** 24 + 2, 2 ** 24 + 1), (n - 1, 0), (5, 2 ** 24)]
    g, rowptr, colidx, _ = symmetric_graph(gnntf, pairs, n)
    positives = pairs[np.arange(m) % len(pairs)]
    from oracle import gnntf_oracle as orc
    slots, threshold = np.arange(m), -(-2 ** 72 // n)
    for stream in range(20000):
        x = (orc.hash_u24(9, stream, slots, 0, 0).astype(np.uint64) << np.uint64(24)) | orc.hash_u24(9, stream, slots, 1, 0).astype(np.uint64)
        if (x >= np.uint64(threshold)).any():
            break
    else:
        raise AssertionError("no stream below 20000 draws an index past 2^24")
    want, fallbacks, _ = ref.sample_negatives(rowptr, colidx, n, positives, 1, None, 32, 9, stream)
    assert fallbacks == 0 and (want[1::2, 1] >= 2 ** 24).any() and (want[1::2, 1] < 2 ** 24).any()
    got, count = raw_sample(gnntf, g, positives, 1, None, 9, stream)
    assert np.array_equal(got, want) and count == 0


def test_sampler_range_and_refusals(gnntf, ordinary):
    g, rowptr, colidx, _, pairs = ordinary
    positives = pairs[:40].copy()
    positives[7], positives[21] = (300, 4), (9, -1)
    want, fallbacks, _ = ref.sample_negatives(rowptr, colidx, 300, positives, 2, None, 32, 4, 0)
    assert fallbacks == 0 and (want[[22, 23, 64, 65], 1] == -1).all() and (np.delete(want, [21, 22, 23, 63, 64, 65], axis=0) >= 0).all()
    assert want[21].tolist() == [300, 4] and want[63].tolist() == [9, -1]
    got, count = raw_sample(gnntf, g, positives, 2, None, 4, 0)
    assert np.array_equal(got, want) and count == 0
    F = dev(np.random.default_rng(1).standard_normal((300, 17)).astype(np.float32))
    scores = host(gnntf.edge_scores(F, dev(got)))
    bad = np.zeros(len(got), dtype=bool)
    bad[21:24], bad[63:66] = True, True                                  # the groups of positives 7 and 21: the positive row and both negatives
    assert np.array_equal(np.isnan(scores), bad)
    # refusals: the argument is named, nothing is written
    nat = gnntf._native
    for what, kwargs in (("K", dict(candidates=np.empty(0, dtype=np.int64))), ("samples", dict(samples=0)), ("max_tries", dict(max_tries=0))):
        args = dict(samples=1, candidates=None, max_tries=32)
        args.update(kwargs)
        raw_sample(gnntf, g, pairs[:5], args["samples"], args["candidates"], 4, 0, max_tries=args["max_tries"], expect=-1)
        assert what.encode() in nat.lib().gnx_last_error()
    out, count, pos = filled((16, 2), MARK, torch.int64), filled((1,), 0, torch.int64), dev(pairs[:5])
    lib, s = nat.lib(), nat.current_stream()
    for what, call in (("K", lambda: lib.gnx_sample_negatives(g.handle, nat.ptr(pos), 5, 1, nat.ptr(pos), 2 ** 31, 32, 4, 0, nat.ptr(out), nat.ptr(count), s)),
                       ("K", lambda: lib.gnx_sample_negatives(g.handle, nat.ptr(pos), 5, 1, None, 299, 32, 4, 0, nat.ptr(out), nat.ptr(count), s)),
                       ("m is negative", lambda: lib.gnx_sample_negatives(g.handle, nat.ptr(pos), -1, 1, None, 300, 32, 4, 0, nat.ptr(out), nat.ptr(count), s)),
                       ("NULL handle", lambda: lib.gnx_sample_negatives(None, nat.ptr(pos), 5, 1, None, 300, 32, 4, 0, nat.ptr(out), nat.ptr(count), s)),
                       ("d_positive", lambda: lib.gnx_sample_negatives(g.handle, None, 5, 1, None, 300, 32, 4, 0, nat.ptr(out), nat.ptr(count), s)),
                       ("d_edges", lambda: lib.gnx_sample_negatives(g.handle, nat.ptr(pos), 5, 1, None, 300, 32, 4, 0, None, nat.ptr(count), s)),
                       ("d_fallbacks", lambda: lib.gnx_sample_negatives(g.handle, nat.ptr(pos), 5, 1, None, 300, 32, 4, 0, nat.ptr(out), None, s))):
        assert call() == -1 and what.encode() in lib.gnx_last_error(), (what, lib.gnx_last_error())
    torch.cuda.synchronize()
    assert untouched(out, MARK) and int(count[0]) == 0


# ---- the plan and the sorted backward --------------------------------------------------------------------------------------------------
def raw_plan(gnntf, edges, n_rows):
    """gnx_edge_plan itself: (keys, pos, chunks) as device tensors, checked against the reference's stable sort and chunk list; 8
    elements past every stated size must keep the sentinel, and the workspace is exactly gnx_edge_plan_bytes(m) long."""
    nat = gnntf._native
    m = edges.shape[0]
    keys, pos, chunks = (filled((size + 8,), MARK, torch.int32) for size in (2 * m, 2 * m, 2 * m + 1))
    nbytes = int(nat.lib().gnx_edge_plan_bytes(m))
    assert nbytes >= 0, nat.lib().gnx_last_error()
    work = torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda")
    nat.check(nat.lib().gnx_edge_plan(nat.ptr(edges), m, n_rows, nat.ptr(keys), nat.ptr(pos), nat.ptr(chunks), nat.ptr(work), nbytes,
                                      nat.current_stream()))
    assert untouched(keys[2 * m:], MARK) and untouched(pos[2 * m:], MARK) and untouched(chunks[2 * m + 1:], MARK)
    want_keys, want_pos, want_chunks = ref.edge_plan(host(edges), n_rows)
    count = int(chunks[0])
    assert np.array_equal(host(keys[:2 * m]).astype(np.int64), want_keys) and np.array_equal(host(pos[:2 * m]).astype(np.int64), want_pos)
    assert count == len(want_chunks) and np.array_equal(host(chunks[1:1 + count]).astype(np.int64), want_chunks)
    assert untouched(chunks[1 + count:], MARK)
    return keys, pos, chunks


def raw_sorted_backward(gnntf, F, edges, r, g, pad=0, prefill=None, plan=None):
    """gnx_edge_plan + gnx_edge_scores_backward_sorted into d_grad_F [n, C + pad]: zeros (or ``prefill``) in the C columns, the sentinel
    in the padding, which must keep it.  Returns the C columns."""
    nat = gnntf._native
    n, C = F.shape
    m = edges.shape[0]
    keys, pos, chunks = raw_plan(gnntf, edges, n) if plan is None else plan
    grad = filled((n, C + pad), SENTINEL)
    grad[:, :C] = 0.0 if prefill is None else dev(prefill)
    floats = int(nat.lib().gnx_edge_sorted_work_floats(m, C))
    work = filled((floats + 8,), SENTINEL)
    nat.check(nat.lib().gnx_edge_scores_backward_sorted(nat.ptr(F), F.stride(0), n, C, nat.ptr(edges), m, nat.ptr(r), nat.ptr(g), nat.ptr(grad),
                                                        grad.stride(0), nat.ptr(keys), nat.ptr(pos), nat.ptr(chunks), nat.ptr(work), floats,
                                                        nat.current_stream()))
    assert untouched(grad[:, C:], SENTINEL), "gnx_edge_scores_backward_sorted wrote into the padding columns of d_grad_F"
    assert untouched(work[floats:], SENTINEL), "gnx_edge_scores_backward_sorted wrote past its workspace"
    return host(grad[:, :C])


def assert_within(what, got, want, bound):
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    exact = bound == 0
    assert (err[exact] == 0).all(), f"{what}: an element that no position names was written"
    ratio = float((err[~exact] / bound[~exact]).max()) if (~exact).any() else 0.0
    print(f"{what}: worst error / bound = {ratio:.4g}")
    assert ratio <= 1.0, f"{what}: worst error / bound = {ratio:.4g}"


def check_sorted(gnntf, what, F, edges, r, g, prefill=None, pitches=("dense",), pads=(5,)):
    """Every pitch of F and every gradient pitch against ONE emulation and ONE float64 reference of the case."""
    sums = ref.sorted_sums_f32(F, edges, r, g)
    start = np.zeros_like(F) if prefill is None else prefill
    want32 = ref.sorted_backward_f32(sums, start)
    want64, bound = ref.edge_grad_f64(F, edges, r, g, prefill)
    ed, gd, rd = dev(edges), dev(g), None if r is None else dev(r)
    for pitch in pitches:
        for pad in pads:
            got = raw_sorted_backward(gnntf, place(F, pitch), ed, rd, gd, pad=pad, prefill=prefill)
            assert same_bits(got, want32), f"{what}, {pitch}, pad {pad}: {np.count_nonzero(got.view(np.int32) != want32.view(np.int32))} elements differ from the emulation"
            assert same_bits(got[~sums[1]], start[~sums[1]])             # rows that no position names: not a bit moved
            assert_within(f"{what}, {pitch}, pad {pad}", got, want64, bound)


@pytest.mark.parametrize("C", (1, 15, 16, 17, 40, 64, 128))
def test_sorted_backward_widths_and_pitches(gnntf, C):
    """5000 drawn edges over 1000 rows, with and without the DistMult weights; the three pitches of F; gradient pitches C + 5 (never
    16-byte rows), C and C + 4 (16-byte rows where C % 4 == 0); into zeros and into a pre-filled d_grad_F."""
    rng = np.random.default_rng(1000 + C)
    F, r = rng.standard_normal((1000, C)).astype(np.float32), (rng.random(C) + 0.5).astype(np.float32)
    edges = rng.integers(0, 1000, size=(5000, 2))
    g, prefill = rng.standard_normal(5000).astype(np.float32), rng.standard_normal(F.shape).astype(np.float32)
    for weights in (None, r):
        check_sorted(gnntf, f"C = {C}, r = {weights is not None}", F, edges, weights, g, pitches=("dense", "odd", "quad"), pads=(5, 0, 4))
        check_sorted(gnntf, f"C = {C}, r = {weights is not None}, pre-filled", F, edges, weights, g, prefill=prefill)


def star(k, rng, n=200):
    """``k`` edges that all name node 0, on alternating sides; the spokes are other nodes."""
    spokes, zeros = rng.integers(1, n, size=k), np.zeros(k, dtype=np.int64)
    return np.where((np.arange(k) % 2 == 0)[:, None], np.stack([zeros, spokes], 1), np.stack([spokes, zeros], 1))


@pytest.mark.parametrize("C", (17, 64))
def test_sorted_backward_chunk_edges(gnntf, C):
    """Node 0 named exactly 255 ... 4097 times (one chunk, exactly one, one and a position, ..., 17 chunks); one edge 1000 times; self-loops
    only (both positions of a loop name its node); two endpoints out of range among good edges; m = 0 and 1."""
    rng = np.random.default_rng(C)
    F, r = rng.standard_normal((200, C)).astype(np.float32), (rng.random(C) + 0.5).astype(np.float32)
    cases = [(f"star {k}", star(k, rng)) for k in (255, 256, 257, 511, 512, 513, 4097)]
    cases.append(("one edge 1000 times", np.tile(np.array([[5, 9]]), (1000, 1))))
    cases.append(("self-loops", np.repeat(rng.integers(0, 200, size=(500, 1)) % 37, 2, axis=1)))
    mixed = rng.integers(0, 200, size=(60, 2))
    mixed[7], mixed[33] = (-1, 3), (5, 200)
    cases += [("out of range", mixed), ("m = 0", np.empty((0, 2), dtype=np.int64)), ("m = 1", np.array([[3, 8]]))]
    prefill = rng.standard_normal(F.shape).astype(np.float32)
    for what, edges in cases:
        g = rng.standard_normal(len(edges)).astype(np.float32)
        if what.startswith("star"):
            assert np.count_nonzero(edges == 0) == len(edges)
        for weights in (None, r):
            check_sorted(gnntf, f"{what}, C = {C}", F, edges, weights, g, pads=(5, 0))
        check_sorted(gnntf, f"{what}, C = {C}, pre-filled", F, edges, r, g, prefill=prefill)


def test_sorted_backward_repeats_and_agrees_with_the_atomic_form(gnntf):
    rng = np.random.default_rng(8)
    C = 40
    F, r = rng.standard_normal((200, C)).astype(np.float32), (rng.random(C) + 0.5).astype(np.float32)
    edges, g = star(4097, rng), rng.standard_normal(4097).astype(np.float32)
    Fd, ed, rd, gd = dev(F), dev(edges), dev(r), dev(g)
    plan = raw_plan(gnntf, ed, 200)
    first, second = (raw_sorted_backward(gnntf, Fd, ed, rd, gd, plan=plan) for _ in range(2))
    assert same_bits(first, second)
    nat = gnntf._native
    atomic = filled((200, C), 0.0)
    nat.check(nat.lib().gnx_edge_scores_backward(nat.ptr(Fd), C, 200, C, nat.ptr(ed), 4097, nat.ptr(rd), nat.ptr(gd), nat.ptr(atomic), C,
                                                 nat.current_stream()))
    want, bound = ref.edge_grad_f64(F, edges, r, g)
    assert_within("sorted", first, want, bound)
    assert_within("atomic", host(atomic), want, bound)


def test_edge_plan_alone(gnntf):
    """Keys ascending, positions ascending inside a key (stable), the out-of-range bucket last -- stated here on the reference's plan,
    which raw_plan holds the device's to."""
    rng = np.random.default_rng(2)
    edges = rng.integers(0, 50, size=(3000, 2))
    edges[[5, 900, 2999]] = [(50, 1), (2, -4), (77, 77)]
    keys, pos, chunks = ref.edge_plan(edges, 50)
    assert (np.diff(keys) >= 0).all() and (np.diff(pos)[np.diff(keys) == 0] > 0).all()
    assert (keys[-6:] == 50).all() and sorted(pos[-6:].tolist()) == [10, 11, 1800, 1801, 5998, 5999] and (keys[:-6] < 50).all()
    assert len(chunks) == 50                                             # about 120 positions per node: one chunk each
    raw_plan(gnntf, dev(edges), 50)
    raw_plan(gnntf, dev(star(600, rng)), 200)                            # node 0: chunks at 0, 256, 512


def test_edge_scores_sorted_through_the_package(gnntf):
    """gnntf.edge_scores(backward="sorted"): the gradient of F and of r; a DeviceIndex over a fixed list keeps its plan, a sampler's
    buffer does not."""
    rng = np.random.default_rng(4)
    F, r = rng.standard_normal((300, 16)).astype(np.float32), (rng.random(16) + 0.5).astype(np.float32)
    edges, g = rng.integers(0, 300, size=(700, 2)), rng.standard_normal(700).astype(np.float32)
    want32 = ref.sorted_backward_f32(ref.sorted_sums_f32(F, edges, r, g), np.zeros_like(F))
    sparse = gnntf.sparse
    for index in (sparse.DeviceIndex(edges, torch.device("cuda:0"), 300), sparse.DeviceIndex(edges, torch.device("cuda:0"), 300, fixed=False), dev(edges)):
        Fd, rd = dev(F).requires_grad_(), dev(r).reshape(16, 1).requires_grad_()
        z = gnntf.edge_scores(Fd, index, rd, backward="sorted")
        assert torch.equal(z, gnntf.edge_scores(Fd.detach(), index, rd.detach()))
        z.backward(dev(g))
        assert same_bits(host(Fd.grad), want32)
        np.testing.assert_allclose(host(rd.grad).reshape(-1), (g[:, None].astype(np.float64) * F[edges[:, 0]] * F[edges[:, 1]]).sum(0), rtol=1e-4, atol=1e-4)
        if isinstance(index, sparse.DeviceIndex):
            assert (index._edge_plan is not None) == index.fixed
    with pytest.raises(Exception, match="backward"):
        gnntf.edge_scores(dev(F), dev(edges), backward="other")


# ---- the model -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def two_sided():
    """300 users and 200 items, about 2 400 user-item pairs without duplicates, stored in both directions; 16-wide features."""
    rng = np.random.default_rng(31)
    n_u, n_i = 300, 200
    pairs = np.unique(np.stack([rng.integers(0, n_u, size=2400), n_u + rng.integers(0, n_i, size=2400)], axis=1), axis=0)
    coo = np.concatenate([pairs, pairs[:, ::-1]]).astype(np.int64)
    X = rng.standard_normal((n_u + n_i, 16)).astype(np.float32)
    return dict(coo=coo, vals=np.ones(len(coo), dtype=np.float32), shape=(n_u + n_i, n_u + n_i), X=X, pairs=pairs)


def run_training(gnntf, data, capture, batches=1, with_valid=False, epochs=3):
    """(parameters, _mask_calls, sampler calls, the sampler's buffer, the stream counts before training) of one run."""
    import random
    random.seed(0)
    np.random.seed(0)
    gnntf.set_seed(11)
    torch.manual_seed(3)
    model = gnntf.NGCF(gnntf.SparseCOO(data["coo"], data["vals"], data["shape"]), data["X"], num_classes=16, ngcf_layer="fused",
                       feature_dropout="fused", dropout=0.25)
    model.reset()
    calls = []

    class Counted(gnntf.device_negative_sampling):
        def __call__(self):
            calls.append(self.model._mask_calls)
            return super().__call__()

    positives = data["pairs"][::25]
    sampler = Counted(positives, model, negative_nodes=np.arange(300, 500))
    task = gnntf.LinkPrediction(sampler)
    assert task.edge_backward == "sorted" and len(task.edges) == 2 * len(positives) and task.edges is sampler.edges
    valid = None
    if with_valid:                                                       # a fixed list on the device: the held-out pairs and one drawn negative each
        fixed = ref.sample_negatives(*ref.csr_pattern(data["coo"], 500), 500, data["pairs"][5::50], 1, np.arange(300, 500), 32, 1, 0)[0]
        valid = gnntf.LinkPrediction(gnntf.sparse.DeviceIndex(fixed, torch.device("cuda:0")), np.tile([1, 0], len(fixed) // 2))
        assert valid.edge_backward == "atomic"
    before = (model._mask_calls, len(calls))
    torch.manual_seed(5)
    model.train(train=task, valid=valid, epochs=epochs, patience=50, capture=capture, batches=batches, verbose=False,
                optimizer=lambda params: torch.optim.Adam(params, lr=0.01, eps=1e-7, capturable=True))
    assert sampler.fallbacks() == 0
    return ([v.var.detach().clone() for v in model.vars()], model._mask_calls, calls, host(sampler.edges.tensor), before, positives)


@pytest.mark.parametrize("batches,with_valid", ((1, False), (2, True)))
def test_captured_training_equals_eager(gnntf, two_sided, batches, with_valid):
    """Three epochs of NGCF + LinkPrediction(device_negative_sampling): the replayed graphs draw the negatives the eager loop draws and
    give the same parameters, bit for bit.  Without a validation task the judge is the sampler task itself: it draws once more per epoch."""
    epochs = 3
    eager, eager_masks, eager_calls, eager_buffer, before, positives = run_training(gnntf, two_sided, False, batches, with_valid, epochs)
    captured, captured_masks, _, captured_buffer, _, _ = run_training(gnntf, two_sided, True, batches, with_valid, epochs)
    assert all(torch.equal(e, c) for e, c in zip(eager, captured))
    assert eager_masks == captured_masks
    # the eager run: the constructor's draw and LinkPrediction's, then one per step and -- as the judge -- one per epoch, each on a stream of its own
    assert before == (2, 2) and eager_calls[:2] == [0, 1]
    drawn = epochs * batches + (0 if with_valid else epochs)
    assert len(eager_calls) == 2 + drawn and len(set(eager_calls)) == len(eager_calls)
    layer_streams = eager_masks - 2 - drawn
    assert layer_streams > 0 and layer_streams % (epochs * batches) == 0
    # the buffer holds the draw of the LAST sampler call of the eager numbering, not the first step's
    rowptr, colidx = ref.csr_pattern(two_sided["coo"], 500)
    last, _, _ = ref.sample_negatives(rowptr, colidx, 500, positives, 1, np.arange(300, 500), 32, 11, eager_calls[-1])
    first, _, _ = ref.sample_negatives(rowptr, colidx, 500, positives, 1, np.arange(300, 500), 32, 11, eager_calls[2])
    assert np.array_equal(eager_buffer, last) and np.array_equal(captured_buffer, last) and not np.array_equal(first, last)


def test_eager_runs_repeat(gnntf, two_sided):
    """Two eager runs from one seed: the sorted backward leaves no order to chance."""
    a, b = run_training(gnntf, two_sided, False), run_training(gnntf, two_sided, False)
    assert a[1] == b[1] and all(torch.equal(x, y) for x, y in zip(a[0], b[0]))


def test_device_edges_in_link_prediction(gnntf, two_sided):
    """A DeviceIndex or a device tensor as ``edges`` stays on the device and keeps the atomic backward; a finite batch_size is refused."""
    edges = dev(two_sided["pairs"][:64])
    for given in (edges, gnntf.sparse.DeviceIndex(edges, torch.device("cuda:0"), 500)):
        task = gnntf.LinkPrediction(given, np.tile([1, 0], 32), loss="bce")
        assert task.edge_backward == "atomic" and len(task.edges) == 64 and task.edges.tensor.data_ptr() == edges.data_ptr()
        F = dev(two_sided["X"]).requires_grad_()
        task.loss(F).backward()
        assert F.grad.abs().sum() > 0 and task.predict(F.detach()).shape == (64,)
        assert 0.0 <= task.evaluate(F.detach()) <= 1.0
    with pytest.raises(Exception, match="batch_size"):
        gnntf.LinkPrediction(edges, batch_size=10)
    with pytest.raises(Exception, match="edge_backward"):
        gnntf.LinkPrediction(edges, edge_backward="other")

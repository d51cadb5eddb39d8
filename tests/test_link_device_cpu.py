"""The device link task without a GPU: the header declares the new entries and the library exports them, their argument checks run
before anything touches a device, the package exports the new names, and the numpy reference the GPU tests compare against
(tests/link_device_ref.py) agrees with a brute-force lookup and with float64."""
import ctypes

import numpy as np
import pytest

import abi_header
import link_device_ref as ref

ENTRIES = ("gnx_sample_negatives", "gnx_edge_plan_bytes", "gnx_edge_plan", "gnx_edge_sorted_work_floats", "gnx_edge_scores_backward_sorted")
FAKE = ctypes.c_void_p(4096)         # stands for a device pointer: every call below fails a check before anything would read it


def lib():
    from gnntf import _native
    return _native.lib()


def test_header_declares_and_library_exports_the_entries():
    from gnntf import _native
    declared = abi_header.declared()
    handle = ctypes.CDLL(_native.LIB_PATH)
    for name in ENTRIES:
        assert name in declared and hasattr(handle, name) and name in _native.SIGNATURES
    header = abi_header.text()
    assert "graph_predictor.py:52-98" in header and "graph_predictor.py:122-146" in header
    assert handle.gnx_version() == _native.ABI_VERSION == 900            # added within 0.9: callers probe for the symbols


def test_package_exports():
    import gnntf
    for name in ("device_negative_sampling", "sample_negatives", "DeviceIndex", "EdgePlan", "edge_scores", "negative_sampling"):
        assert hasattr(gnntf, name)
    assert gnntf.device_negative_sampling is gnntf.link_tasks.device_negative_sampling
    with pytest.raises(Exception, match="GPU only"):
        gnntf.edge_scores(__import__("torch").zeros(4, 4), [[0, 1]], backward="sorted")


def refused(rc, *words):
    message = lib().gnx_last_error()
    assert rc == -1 and all(w.encode() in message for w in words), message


def test_sampler_argument_errors():
    s = lib().gnx_sample_negatives
    refused(s(FAKE, FAKE, -1, 1, None, 10, 32, 0, 0, FAKE, FAKE, None), "gnx_sample_negatives", "m is negative")
    refused(s(FAKE, FAKE, 5, 0, None, 10, 32, 0, 0, FAKE, FAKE, None), "samples")
    refused(s(FAKE, FAKE, 5, 1, None, 10, 0, 0, 0, FAKE, FAKE, None), "max_tries")
    refused(s(FAKE, FAKE, 5, 1, FAKE, 0, 32, 0, 0, FAKE, FAKE, None), "K must be in [1, 2^31)")
    refused(s(FAKE, FAKE, 5, 1, FAKE, 2 ** 31, 32, 0, 0, FAKE, FAKE, None), "K must be in [1, 2^31)")
    refused(s(FAKE, FAKE, 2 ** 30, 2, FAKE, 10, 32, 0, 0, FAKE, FAKE, None), "m * samples")
    refused(s(None, FAKE, 5, 1, FAKE, 10, 32, 0, 0, FAKE, FAKE, None), "NULL handle")


def test_plan_argument_errors():
    p, nbytes = lib().gnx_edge_plan, lib().gnx_edge_plan_bytes
    assert nbytes(-1) == -1 and b"gnx_edge_plan_bytes: m" in lib().gnx_last_error()
    assert nbytes(2 ** 30) == -1
    refused(p(FAKE, -1, 10, FAKE, FAKE, FAKE, FAKE, 1 << 20, None), "gnx_edge_plan: m")
    refused(p(FAKE, 2 ** 30, 10, FAKE, FAKE, FAKE, FAKE, 1 << 20, None), "gnx_edge_plan: m")
    refused(p(FAKE, 5, -1, FAKE, FAKE, FAKE, FAKE, 1 << 20, None), "n_rows")
    refused(p(FAKE, 5, 2 ** 31, FAKE, FAKE, FAKE, FAKE, 1 << 20, None), "n_rows")
    refused(p(FAKE, 5, 10, FAKE, FAKE, None, FAKE, 1 << 20, None), "d_chunks")
    for args in ((None, 5, 10, FAKE, FAKE, FAKE, FAKE), (FAKE, 5, 10, None, FAKE, FAKE, FAKE), (FAKE, 5, 10, FAKE, None, FAKE, FAKE),
                 (FAKE, 5, 10, FAKE, FAKE, FAKE, None)):
        refused(p(*args, 1 << 20, None), "NULL pointer")
    refused(p(FAKE, 5, 10, FAKE, FAKE, FAKE, ctypes.c_void_p(4100), 1 << 20, None), "16-byte aligned")


def test_sorted_backward_argument_errors():
    b, floats = lib().gnx_edge_scores_backward_sorted, lib().gnx_edge_sorted_work_floats
    assert floats(1000, 64) == 2 * (2000 // 256 + 2) * 64 and floats(0, 1) == 4
    assert floats(-1, 4) == -1 and floats(5, 0) == -1 and b"gnx_edge_sorted_work_floats" in lib().gnx_last_error()
    good = dict(F=FAKE, ldf=8, n=50, C=8, edges=FAKE, m=10, r=None, g=FAKE, dF=FAKE, ldg=8, keys=FAKE, pos=FAKE, chunks=FAKE, work=FAKE,
                floats=floats(10, 8))

    def call(**change):
        a = dict(good, **change)
        return b(a["F"], a["ldf"], a["n"], a["C"], a["edges"], a["m"], a["r"], a["g"], a["dF"], a["ldg"], a["keys"], a["pos"], a["chunks"],
                 a["work"], a["floats"], None)

    for change in (dict(m=-1), dict(m=2 ** 30), dict(C=0), dict(ldf=7), dict(ldg=7), dict(n=-1), dict(n=2 ** 31)):
        refused(call(**change), "gnx_edge_scores_backward_sorted: bad sizes")
    for change in (dict(F=None), dict(edges=None), dict(g=None), dict(dF=None)):
        refused(call(**change), "NULL pointer")
    for change in (dict(keys=None), dict(pos=None), dict(chunks=None)):
        refused(call(**change), "NULL plan")
    refused(call(work=None), "d_work")
    refused(call(floats=good["floats"] - 1), "gnx_edge_sorted_work_floats")
    assert call(m=0, F=None, keys=None, work=None, floats=0) == 0        # no edges: nothing to do, nothing read


def test_link_prediction_refuses_what_the_device_cannot_follow():
    """The host paths are as they were (tests/test_link_tasks.py); the new keyword is checked without a device."""
    import gnntf
    edges = np.array([[0, 1], [0, 2]])
    assert gnntf.LinkPrediction(edges, [1, 0]).edge_backward == "atomic"
    assert gnntf.LinkPrediction(edges, [1, 0], edge_backward="sorted").edge_backward == "sorted"
    with pytest.raises(Exception, match="edge_backward"):
        gnntf.LinkPrediction(edges, [1, 0], edge_backward="fast")


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
def test_reference_sampler_against_a_set_lookup():
    """50 nodes: the binary search of the reference answers as a set of stored pairs does, draw for draw; saturated sources fall back."""
    rng = np.random.default_rng(0)
    coo = rng.integers(0, 50, size=(400, 2))
    coo[:49] = [(7, w) for w in range(50) if w != 30]                    # node 7 is linked to everything but node 30
    rowptr, colidx = ref.csr_pattern(coo, 50)
    entries = set(map(tuple, coo.tolist()))
    assert rowptr[-1] == len(entries) == len(colidx) and all((np.diff(colidx[rowptr[r]:rowptr[r + 1]]) > 0).all() for r in range(50))
    for r in range(50):
        for c in range(-1, 51):
            assert ref.stored(rowptr, colidx, r, c) == ((r, c) in entries)
    positives = np.concatenate([coo[100:160], [(7, 3), (50, 2)]])
    lookup = lambda u, w: (u, w) in entries or (w, u) in entries
    total = 0
    for samples, candidates, tries in ((1, None, 32), (3, np.arange(10, 45), 4)):
        a = ref.sample_negatives(rowptr, colidx, 50, positives, samples, candidates, tries, 5, 2)
        b = ref.sample_negatives(rowptr, colidx, 50, positives, samples, candidates, tries, 5, 2, linked=lookup)
        assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2])
        edges, fallbacks, used = a
        assert (edges[-samples:, 1] == -1).all() and (used[-samples:] == 0).all()            # the positive row (50, 2)
        group = 1 + samples
        ok = used < tries
        for e in np.flatnonzero(ok & (used > 0)):                        # accepted before the last try: the three conditions hold
            u, w = edges[(e // samples) * group + 1 + e % samples]
            v = positives[e // samples, 1]
            assert w != u and w != v and not lookup(u, w)
        assert (used.max() > 1) and (used <= tries).all()
        total += fallbacks
    assert total > 0                                                     # node 7 at 4 tries over 35 candidates
    assert ref.draw(5, 2, 0, 0, 50) != ref.draw(5, 3, 0, 0, 50) or ref.draw(5, 2, 1, 0, 50) != ref.draw(5, 3, 1, 0, 50)


def test_reference_draws_are_uniform_and_wide():
    """j = floor(x K / 2^48) stays below K and reaches past 2^24 for a K that needs more than one hash."""
    K = 80_000_000
    js = np.array([ref.draw(1, 0, e, 0, K) for e in range(2000)])
    assert 0 <= js.min() and js.max() < K and (js >= 2 ** 24).mean() > 0.7 and abs(js.mean() / K - 0.5) < 0.03


def test_reference_plan_and_summation_order():
    rng = np.random.default_rng(3)
    edges = rng.integers(0, 40, size=(700, 2))
    edges[:300, 0] = 0                                                   # node 0: more than one chunk
    edges[[4, 650]] = [(40, 1), (2, -1)]
    keys, pos, chunks = ref.edge_plan(edges, 40)
    flat = edges.reshape(-1)
    assert (np.diff(keys) >= 0).all() and (np.diff(pos)[np.diff(keys) == 0] > 0).all() and sorted(pos.tolist()) == list(range(1400))
    good = keys < 40
    assert np.array_equal(flat[pos[good]], keys[good]) and sorted(pos[~good].tolist()) == [8, 9, 1300, 1301]
    n0 = int((keys == 0).sum())
    assert n0 > 256 and chunks[:-(-n0 // 256)].tolist() == list(range(0, n0, 256))
    assert len(chunks) == -(-n0 // 256) + len(np.unique(keys[good])) - 1
    F, r = rng.standard_normal((40, 5)).astype(np.float32), rng.random(5).astype(np.float32) + 0.5
    g, prefill = rng.standard_normal(700).astype(np.float32), rng.standard_normal((40, 5)).astype(np.float32)
    for weights in (None, r):
        sums = ref.sorted_sums_f32(F, edges, weights, g)
        for start in (None, prefill):
            got = ref.sorted_backward_f32(sums, np.zeros_like(F) if start is None else start)
            want, bound = ref.edge_grad_f64(F, edges, weights, g, start)
            assert got.dtype == np.float32 and (np.abs(got - want) <= bound).all()
    # the order is what the emulation pins: a node named by 3 terms a, b, c gets fl(fl(a + b) + c), not another association
    F1 = np.array([[0.0], [1e8], [1.0], [-1e8]], dtype=np.float32)
    sums = ref.sorted_sums_f32(F1, np.array([[0, 1], [0, 2], [0, 3]]), None, np.ones(3, dtype=np.float32))
    assert sums[0][0, 0] == np.float32(np.float32(np.float32(1e8) + np.float32(1.0)) + np.float32(-1e8)) == 0.0

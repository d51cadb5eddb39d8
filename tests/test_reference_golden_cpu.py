"""The restatements of the reference project -- oracle/gnntf_oracle.py, tests/model_step_ref.py, tests/signal_ref.py, the eval halves of
the fused layers' *_ref.py files, gnntf/metrics.py -- against what the reference's OWN program text computes on the TensorFlow stand-in
(oracle/tf_standin), as tests/golden/make_reference_golden.py recorded it in tests/golden/reference_*.npz.

a. the stand-in's ops against plain numpy statements of the TensorFlow semantics they document;
b. the fixtures regenerated from the reference tree, array for array (skipped where GNX_REFERENCE_DIR does not exist);
c. every restatement against its fixture.  Both sides are float64 evaluations of the same real-valued expression that differ by the
   order of sums over at most a few thousand terms, about 1e-13 of the largest value: the bar is rtol 1e-9, atol 1e-9 max|want|
   (``ratio`` <= 1), integers and the recorded dropout calls equal.  Two restatements hold float32 CONSTANTS on purpose (they take the
   very operands the kernels read): gcnii_shapes_ref mixes with float32(1 - a) and float32(a), ngcf_fused_ref's leaky slope is
   float32(0.2).  Those differ from the reference by rounding, not meaning -- 2^-24 relative per constant and layer -- and are held
   to 1e-9 + layers * 2^-24 instead, as is signal_ref.ppr_ref over its ten steps (measured, printed by the tests: 4.1e-8 for the
   GCNII spectral chain, 4.1e-9 for the NGCF chain, 3.2e-8 for the sweep, against bars of 2.4e-7, 1.8e-7 and 6.0e-7; every other
   case is below 3e-15 of the largest value, NGCF's steps below 3e-12);
   GCNIIReg: signal_ref.gcniireg_reference is held to the reference's two steps with the reference's own projection vector (zeros);
   what this project's drawn vector changes is asserted as a named expected difference (test_fastreg_projection_is_a_named_deviation);
d. every planted mistake of model_step_ref.MISTAKES moves the restatement at least 10 x the float32 bar away from the fixture."""
import importlib.util
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import model_step_ref as ref
import reference_cases as cases
from oracle import gnntf_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = os.environ.get("GNX_REFERENCE_DIR", "/root/reference")
RTOL = ATOL = 1e-9
f64 = lambda x: np.asarray(x, dtype=np.float64)


def ratio(got, want, rtol=RTOL, atol=ATOL):
    """max |got - want| / (rtol |want| + atol max|want|): at most 1 where the bar holds."""
    got, want = f64(got), f64(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    if want.size == 0:
        return 0.0
    err, bar = np.abs(got - want), rtol * np.abs(want) + atol * np.abs(want).max()
    return float(np.where(err == 0, 0.0, err / np.where(bar == 0, np.finfo(np.float64).tiny, bar)).max())


# ======================================================================================================================================
# a. the stand-in's ops
# ======================================================================================================================================
@pytest.fixture(scope="module")
def tf():
    spec = importlib.util.spec_from_file_location("gnx_tf_standin", os.path.join(ROOT, "oracle", "tf_standin", "tensorflow", "__init__.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    module.standin_configure(dtype="float64")
    yield module
    module.standin_configure(dtype="float64")


def val(t):
    return t.numpy() if hasattr(t, "numpy") else np.asarray(t)


def test_standin_is_not_importable_by_accident():
    assert importlib.util.find_spec("tensorflow") is None or "tf_standin" not in (importlib.util.find_spec("tensorflow").origin or "")


def test_dense_ops(tf):
    rng = np.random.default_rng(0)
    a, b, c = rng.standard_normal((5, 4)), rng.standard_normal((4, 3)), rng.standard_normal((5, 4))
    assert val(tf.constant(a)).dtype == np.float64 and val(tf.constant(a.astype(np.float32))).dtype == np.float64
    np.testing.assert_allclose(val(tf.matmul(tf.constant(a), tf.constant(b))), a @ b, rtol=1e-14)
    assert np.array_equal(val(tf.concat([tf.constant(a), tf.constant(c)], axis=0)), np.concatenate([a, c], axis=0))
    assert np.array_equal(val(tf.concat([tf.constant(a), tf.constant(c)], axis=1)), np.concatenate([a, c], axis=1))
    assert np.array_equal(val(tf.reshape(tf.constant(a), (-1, 1))), a.reshape(-1, 1))
    assert np.array_equal(val(tf.multiply(tf.constant(a), tf.constant(c))), a * c)
    assert np.array_equal(val(tf.multiply(tf.constant(a), tf.constant(a[:1]))), a * a[:1])                    # broadcasting
    np.testing.assert_allclose(float(tf.reduce_sum(tf.constant(a))), a.sum(), rtol=1e-14)
    np.testing.assert_allclose(val(tf.reduce_sum(tf.constant(a), axis=1)), a.sum(axis=1), rtol=1e-14)
    np.testing.assert_allclose(val(tf.math.reduce_sum(tf.constant(a), axis=0)), a.sum(axis=0), rtol=1e-14)
    np.testing.assert_allclose(float(tf.reduce_mean(tf.constant(a))), a.mean(), rtol=1e-14)
    np.testing.assert_allclose(val(tf.exp(tf.constant(a))), np.exp(a), rtol=1e-14)
    wide = np.abs(rng.standard_normal(4000)) * 20 + 0.1
    assert np.array_equal(val(tf.sqrt(tf.constant(wide))), np.sqrt(wide))                                    # the correctly rounded root, bit for bit
    # the product as IEEE arithmetic alone decides it: the k-ascending sum of outer products (no BLAS, whose code path follows the processor)
    chain = np.zeros((5, 3))
    for k in range(4):
        chain = chain + a[:, k:k + 1] * b[k:k + 1, :]
    assert np.array_equal(val(tf.matmul(tf.constant(a), tf.constant(b))), chain)
    x = tf.Variable(tf.constant(wide[:50]))
    with tf.GradientTape() as tape:
        grads = tape.gradient(tf.reduce_sum(tf.sqrt(x) + tf.exp(-x) + tf.math.log(x) + tf.math.log1p(x) + tf.nn.tanh(x)), [x])
    w = wide[:50]
    np.testing.assert_allclose(val(grads[0]), 0.5 / np.sqrt(w) - np.exp(-w) + 1 / w + 1 / (1 + w) + 1 - np.tanh(w) ** 2, rtol=1e-13)
    assert val(tf.round(tf.constant([0.5, 1.5, 2.5, -0.5, 1.2]))).tolist() == [0.0, 2.0, 2.0, -0.0, 1.0]      # halves to even
    ties = np.zeros((3, 5)); ties[1, 2] = ties[1, 4] = 2.0
    assert val(tf.argmax(tf.constant(ties), axis=1)).tolist() == [0, 2, 0] and val(tf.argmax(tf.constant(ties), axis=1)).dtype == np.int64
    assert np.array_equal(val(tf.gather(tf.constant(a), [3, 0, 3], axis=0)), a[[3, 0, 3]])
    assert np.array_equal(val(tf.gather(tf.constant(a), np.array([1, 1]), axis=1)), a[:, [1, 1]])
    assert np.array_equal(val(tf.zeros((2, 3))), np.zeros((2, 3))) and np.array_equal(val(tf.ones((2, 3))), np.ones((2, 3)))
    assert np.array_equal(val(tf.eye(3)), np.eye(3))
    assert val(tf.constant([1.0, 0.0, 1.0], shape=(3, 1))).shape == (3, 1)
    assert val(tf.constant(np.arange(3))).dtype == np.int64                                                     # integers stay integers
    np.testing.assert_allclose(val(tf.sigmoid(tf.constant(a))), 1 / (1 + np.exp(-a)), rtol=1e-14)


def test_nn_and_math_ops(tf):
    rng = np.random.default_rng(1)
    a = rng.standard_normal((6, 5))
    assert np.array_equal(val(tf.nn.relu(tf.constant(a))), np.maximum(a, 0))
    np.testing.assert_allclose(val(tf.nn.leaky_relu(tf.constant(a))), np.where(a > 0, a, 0.2 * a), rtol=1e-15)      # the default alpha: 0.2
    np.testing.assert_allclose(val(tf.nn.leaky_relu(tf.constant(a), alpha=0.01)), np.where(a > 0, a, 0.01 * a), rtol=1e-15)
    np.testing.assert_allclose(val(tf.nn.tanh(tf.constant(a))), np.tanh(a), rtol=1e-14)
    np.testing.assert_allclose(val(tf.nn.sigmoid(tf.constant(a))), 1 / (1 + np.exp(-a)), rtol=1e-14)
    e = np.exp(a - a.max(axis=1, keepdims=True))
    np.testing.assert_allclose(val(tf.nn.softmax(tf.constant(a), axis=1)), e / e.sum(axis=1, keepdims=True), rtol=1e-13)
    np.testing.assert_allclose(val(tf.nn.log_softmax(tf.constant(a), axis=1)), np.log(e / e.sum(axis=1, keepdims=True)), rtol=1e-12)
    np.testing.assert_allclose(float(tf.nn.l2_loss(tf.constant(a))), (a ** 2).sum() / 2, rtol=1e-14)
    assert np.array_equal(val(tf.nn.embedding_lookup(tf.constant(a), np.array([5, 0, 5]))), a[[5, 0, 5]])
    np.testing.assert_allclose(val(tf.math.log(tf.constant(np.abs(a)))), np.log(np.abs(a)), rtol=1e-14)
    np.testing.assert_allclose(val(tf.math.log1p(tf.constant(np.abs(a)))), np.log1p(np.abs(a)), rtol=1e-14)
    np.testing.assert_allclose(float(tf.math.log1p(0.5)), math.log1p(0.5), rtol=1e-15)
    big = np.array([-800.0, -3.0, 0.0, 3.0, 800.0])
    np.testing.assert_allclose(val(tf.math.log_sigmoid(tf.constant(big))), [-800.0, -np.log1p(np.exp(3.0)), -np.log(2.0), -np.log1p(np.exp(-3.0)), 0.0],
                               rtol=1e-14)
    assert val(tf.math.count_nonzero(tf.constant(np.array([0, 3, 0, -1])))) == 2
    # l2_normalize: x * rsqrt(max(sum x^2, 1e-12)) -- a row below the epsilon is scaled by 1e6, a zero row stays zero
    x = np.array([[3.0, 4.0], [1e-8, 0.0], [0.0, 0.0]])
    want = x / np.sqrt(np.maximum((x * x).sum(axis=1, keepdims=True), 1e-12))
    assert want[1, 0] == pytest.approx(1e-2, rel=1e-12)
    for fn in (tf.math.l2_normalize, tf.nn.l2_normalize):
        np.testing.assert_allclose(val(fn(tf.constant(x), axis=1)), want, rtol=1e-14)
    # divide_no_nan: 0 where the divisor is 0, whatever the dividend
    np.testing.assert_array_equal(val(tf.math.divide_no_nan(1.0, tf.constant([2.0, 0.0, -4.0, -0.0]))), [0.5, 0.0, -0.25, 0.0])
    np.testing.assert_array_equal(val(tf.math.divide_no_nan(tf.constant([0.0, np.inf]), tf.constant([0.0, 0.0]))), [0.0, 0.0])


def test_dropout_asks_the_provider_and_scales(tf):
    asked = []

    def provider(ordinal, shape, rate):
        asked.append((ordinal, shape, rate))
        keep = (np.arange(int(np.prod(shape))).reshape(shape) % 3 != 0)
        return keep / (1.0 - rate)

    tf.standin_configure(dtype="float64", provider=provider)
    x = np.arange(1.0, 13.0).reshape(3, 4)
    out = val(tf.nn.dropout(tf.constant(x), 0.6))
    keep = np.arange(12).reshape(3, 4) % 3 != 0
    np.testing.assert_allclose(out, np.where(keep, x / 0.4, 0.0), rtol=1e-15)                                   # kept: times 1 / (1 - rate)
    assert np.array_equal(out == 0, ~keep)
    assert val(tf.nn.dropout(tf.constant(x), 0)) is not None and len(asked) == 1                               # rate 0: x, nobody asked
    val(tf.nn.dropout(tf.constant(x[0]), 0.25))
    assert asked == [(0, (3, 4), 0.6), (1, (4,), 0.25)]
    tf.standin_configure(provider=lambda ordinal, shape, rate: np.ones(shape))                                 # kept values not scaled: refused
    with pytest.raises(ValueError, match="scaled"):
        tf.nn.dropout(tf.constant(x), 0.5)
    tf.standin_configure(provider=None)
    with pytest.raises(RuntimeError, match="no mask provider"):
        tf.nn.dropout(tf.constant(x), 0.5)
    with pytest.raises(ValueError):
        tf.nn.dropout(tf.constant(x), 1.0)


def test_sparse_ops(tf):
    # unordered, with (1, 2) stored twice and an empty row 3 / column 0
    idx = np.array([[2, 1], [1, 2], [0, 3], [1, 2], [0, 1]])
    v = np.array([1.0, 2.0, 3.0, 0.5, 4.0])
    A = tf.SparseTensor(idx, v, (4, 4))
    dense = np.zeros((4, 4)); np.add.at(dense, (idx[:, 0], idx[:, 1]), v)
    assert tf.sparse.SparseTensor is tf.SparseTensor and A.shape == (4, 4) and A.dense_shape == (4, 4)
    np.testing.assert_array_equal(val(tf.sparse.reduce_sum(A, axis=0)), dense.sum(axis=0))                      # duplicates add up; column 0: 0
    np.testing.assert_array_equal(val(tf.sparse.reduce_sum(A, axis=1)), dense.sum(axis=1))
    assert float(tf.sparse.reduce_sum(A)) == v.sum()
    B = np.random.default_rng(2).standard_normal((4, 3))
    np.testing.assert_allclose(val(tf.sparse.sparse_dense_matmul(A, tf.constant(B))), dense @ B, rtol=1e-14)
    # dense * sparse and sparse * dense keep the index list (duplicates stay apart) and broadcast the dense side only
    d = np.array([2.0, 3.0, 5.0, 7.0])
    left = tf.reshape(tf.constant(d), (-1, 1)) * A
    assert isinstance(left, tf.SparseTensor) and np.array_equal(left.indices.numpy(), idx)
    np.testing.assert_array_equal(val(left.values), d[idx[:, 0]] * v)
    right = A * tf.constant(d)
    assert np.array_equal(right.indices.numpy(), idx)
    np.testing.assert_array_equal(val(right.values), v * d[idx[:, 1]])
    both = tf.reshape(tf.constant(d), (-1, 1)) * A * tf.constant(d)
    np.testing.assert_array_equal(val(both.values), d[idx[:, 0]] * v * d[idx[:, 1]])
    with pytest.raises(ValueError, match="only the dense side broadcasts"):
        A * tf.constant(np.ones((2, 4)))
    eye = tf.sparse.eye(4)
    assert eye.indices.numpy().tolist() == [[0, 0], [1, 1], [2, 2], [3, 3]] and val(eye.values).tolist() == [1.0] * 4
    # sparse.add on ordered duplicate-free input: the union, equal indices summed once
    P = tf.SparseTensor([[0, 0], [0, 2], [2, 2]], [1.0, 2.0, 3.0], (3, 3))
    S = tf.sparse.add(P, tf.sparse.eye(3))
    assert S.indices.numpy().tolist() == [[0, 0], [0, 2], [1, 1], [2, 2]] and val(S.values).tolist() == [2.0, 2.0, 1.0, 4.0]
    Z = tf.sparse.add(tf.SparseTensor([[1, 1]], [-1.0], (3, 3)), tf.sparse.eye(3))                            # a sum of 0 stays stored
    assert Z.indices.numpy().tolist() == [[0, 0], [1, 1], [2, 2]] and val(Z.values).tolist() == [1.0, 0.0, 1.0]
    # ... on unordered input with duplicates (the reading the op's docstring states): every entry once, the matrix is a + b
    S = tf.sparse.add(A, tf.sparse.eye(4))
    got = np.zeros((4, 4)); np.add.at(got, (S.indices.numpy()[:, 0], S.indices.numpy()[:, 1]), val(S.values))
    np.testing.assert_array_equal(got, dense + np.eye(4))
    assert len(val(S.values)) <= len(v) + 4
    with pytest.raises(ValueError):
        tf.sparse.add(A, tf.sparse.eye(3))


def test_variables_tape_and_float32_switch(tf):
    tf.standin_configure(dtype="float64")                                                                      # a fresh record of the tape's targets
    w = tf.Variable(tf.zeros((2, 2)), trainable=True)
    frozen = tf.Variable(tf.ones((2, 2)), trainable=False)
    w.assign(np.array([[1.0, 2.0], [3.0, 4.0]], dtype=np.float32))
    assert val(w).dtype == np.float64 and val(w).tolist() == [[1.0, 2.0], [3.0, 4.0]] and tuple(w.shape) == (2, 2)
    with pytest.raises(ValueError, match="shape"):
        w.assign(np.zeros((4,)))
    snapshot = tf.identity(w)
    w.assign(val(w) * 2)
    assert val(snapshot).tolist() == [[1.0, 2.0], [3.0, 4.0]] and val(w)[1, 1] == 8.0
    unused = tf.Variable(tf.zeros((1, 1)))
    with tf.GradientTape() as tape:
        loss = tf.reduce_sum(tf.matmul(w, frozen) * w) + 3.0 * tf.nn.l2_loss(w)
        grads = tape.gradient(loss, [w, unused])
    W, O = val(w), np.ones((2, 2))
    np.testing.assert_allclose(val(grads[0]), W @ O.T + W @ O + 3.0 * W, rtol=1e-14)                           # d sum((W O) * W) = W O^T + W O
    assert grads[1] is None and tf.standin_tape_targets() == [float(loss.numpy())]
    assert isinstance(loss.numpy(), np.ndarray)                                                                # numpy() of a watched tensor
    for name in ("models", "layers", "optimizers", "metrics"):
        with pytest.raises(NotImplementedError, match="tf.keras." + name):
            getattr(getattr(tf.keras, name), "Anything")
    with pytest.raises(NotImplementedError, match="tf.keras.losses.MeanSquaredError"):
        tf.keras.losses.MeanSquaredError
    with pytest.raises(NotImplementedError, match="from_logits"):
        tf.keras.losses.BinaryCrossentropy()
    with pytest.raises(NotImplementedError, match="tf.keras.Input"):
        tf.keras.Input(shape=(None, 3))
    z, y = np.array([-2.0, 0.5, 3.0, -0.1]), np.array([[0.0], [1.0], [1.0], [0.0]])
    want = np.mean(np.maximum(z, 0) - z * y[:, 0] + np.log1p(np.exp(-np.abs(z))))
    bce = tf.keras.losses.BinaryCrossentropy(from_logits=True)
    np.testing.assert_allclose(float(bce(tf.constant(y), tf.constant(z))), want, rtol=1e-14)                   # labels [m, 1], logits [m]
    np.testing.assert_allclose(float(bce(tf.constant(y), tf.constant(z.reshape(-1, 1)))), want, rtol=1e-14)
    logits, labels = np.random.default_rng(3).standard_normal((4, 3)), np.array([2, 0, 1, 1])
    lp = logits - np.log(np.exp(logits).sum(axis=1, keepdims=True))
    np.testing.assert_allclose(float(tf.keras.losses.SparseCategoricalCrossentropy(from_logits=True)(labels, tf.constant(logits))),
                               -lp[np.arange(4), labels].mean(), rtol=1e-14)
    for make, limit in ((tf.keras.initializers.RandomUniform(-0.3, 0.3), 0.3), (tf.keras.initializers.GlorotUniform(), math.sqrt(6 / 50)),
                        (tf.keras.initializers.HeUniform(), math.sqrt(6 / 20))):
        draw = val(make((20, 30)))
        assert draw.shape == (20, 30) and np.abs(draw).max() <= limit and np.abs(draw).max() > 0.8 * limit
    tf.standin_configure(dtype="float32")
    try:
        assert val(tf.constant(np.ones(2))).dtype == np.float32 and val(tf.eye(2)).dtype == np.float32
        v32 = tf.Variable(tf.zeros((1, 2)))
        v32.assign(np.array([[0.1, 0.2]]))
        assert val(v32).dtype == np.float32 and val(tf.matmul(tf.constant(np.ones((3, 1))), v32)).dtype == np.float32
    finally:
        tf.standin_configure(dtype="float64")


# ======================================================================================================================================
# b. the fixtures come out of the reference's text
# ======================================================================================================================================
def fixture_files(directory):
    return sorted(f for f in os.listdir(directory) if f.startswith("reference_") and f.endswith(".npz"))


def test_fixtures_are_within_the_size_limit():
    files = fixture_files(cases.GOLDEN)
    assert files and all(os.path.getsize(os.path.join(cases.GOLDEN, f)) <= cases.LARGEST_FIXTURE for f in files)


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "gnntf")), reason="no reference tree (GNX_REFERENCE_DIR)")
def test_fixtures_regenerate_from_the_reference(tmp_path):
    done = subprocess.run([sys.executable, os.path.join(cases.GOLDEN, "make_reference_golden.py"), str(tmp_path)], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-4000:]
    assert fixture_files(tmp_path) == fixture_files(cases.GOLDEN)
    for name in fixture_files(tmp_path):
        with np.load(os.path.join(tmp_path, name)) as new, np.load(os.path.join(cases.GOLDEN, name)) as old:
            assert sorted(new.files) == sorted(old.files), name
            for key in new.files:
                assert new[key].dtype == old[key].dtype and np.array_equal(new[key], old[key]), (name, key)


# ======================================================================================================================================
# c. the restatements against the fixtures
# ======================================================================================================================================
def dense_of(indices, values, n):
    return orc.to_dense(np.asarray(indices, dtype=np.int64), f64(values), (n, n))


@pytest.mark.parametrize("gname", ["full", "emptied"])
def test_get_adjacency(gname):
    z = cases.load("adjacency")
    coo, vals, shape = cases.adjacency_graphs()[gname]
    assert np.array_equal(z[gname + ".coo"], coo) and np.array_equal(z[gname + ".vals"].astype(np.float32), vals)
    worst, streams = 0.0, []
    for mode in ("eval", "train"):
        for normalized in cases.NORMALIZED:
            for add_eye in cases.ADD_EYE:
                key = f"{gname}.{mode}.{normalized}.{add_eye}"
                stream = int(z[key + ".stream"])
                ai, av = orc.get_adjacency(coo, vals, shape, graph_dropout=cases.ADJ_RATE, normalized=normalized, add_eye=add_eye,
                                           training=mode == "train", seed=cases.ADJ_SEED, stream=max(stream, 0), dtype=np.float64)
                want = dense_of(z[key + ".indices"], z[key + ".values"], shape[0])
                worst = max(worst, ratio(orc.to_dense(ai, av, shape), want))
                if mode == "train":
                    streams.append(stream)
                    # tf.nn.dropout on G.values keeps a dropped entry as an explicit zero in the index list (layered.py:50).  NAMED EXPECTED
                    # DIFFERENCE: sparse.DroppedAdjacency skips such an entry instead of multiplying by the stored 0 -- the same sum for
                    # finite features (its documented precondition), and it saves gathering about half of the rows.
                    keep = orc.keep_mask(coo, cases.ADJ_RATE, cases.ADJ_SEED, stream)
                    if add_eye == "none":
                        assert np.array_equal(z[key + ".indices"], coo) and (~keep).any() and np.all(z[key + ".values"][~keep] == 0)
                        if normalized == "none":            # (a kept entry may still be scaled by a D of 0)
                            assert np.array_equal(z[key + ".values"] == 0, ~keep)
                else:
                    assert stream == -1
                if add_eye == "none":                       # the index list is the graph's own, entry for entry
                    assert np.array_equal(z[key + ".indices"], coo) and ratio(av, z[key + ".values"]) <= 1
                if gname == "emptied" and normalized != "none" and add_eye != "before":
                    assert np.all(want[cases.EMPTIED_COLUMN, :][np.arange(shape[0]) != cases.EMPTIED_COLUMN] == 0)      # D = 0, no NaN
                assert np.isfinite(z[key + ".values"]).all()
    print(f"get_adjacency on the {gname} graph: worst ratio to the bar {worst:.3g}")
    assert worst <= 1
    # one edge mask per training call, numbered in call order: 1-D, of length nnz, at the rate
    assert streams == list(range(9))
    assert z[gname + ".calls"].tolist() == [[k, 0, len(coo), 0, int(cases.ADJ_RATE * 1e6), k] for k in range(9)]


def test_graph2adj():
    z = cases.load("container")
    for name, (nodes, edges, weights, _, directed) in cases.container_graphs().items():
        assert z[name + ".nodes"].tolist() == nodes                                                  # the graph iterates in insertion order
        idx, vals, shape = orc.graph2adj(z[name + ".nodes"].tolist(), [tuple(e) for e in z[name + ".edges"].tolist()],
                                         None if weights is None else z[name + ".weights"].astype(np.float64), directed=directed)
        assert np.array_equal(idx, z[name + ".indices"]) and np.array_equal(vals.astype(np.float64), z[name + ".values"]), name
        assert shape == (int(z[name + ".n"]),) * 2 and len(idx) == (1 if directed else 2) * len(edges)
    sym = z["directed-symmetrised.indices"]
    assert len(np.unique(sym[:, 0] * 7 + sym[:, 1])) < len(sym)                                       # arcs stored in both directions: twice


def eval_case(name):
    z = cases.load("eval")
    X, parameters = cases.eval_inputs(name)
    assert np.array_equal(z[name + ".X"].astype(np.float32), X) and len(z[name + ".calls"]) == 0                  # an eval forward draws nothing
    for k, p in enumerate(parameters):
        assert np.array_equal(z[f"{name}.p{k}"].astype(np.float32), p)
    return z, X, parameters, z[name + ".out"]


def pairs(parameters):
    return [(f64(parameters[i]), f64(parameters[i + 1])) for i in range(0, len(parameters), 2)]


def constant_csr(normalized="symmetric"):
    coo, vals, shape = ref.graph()
    ai, av = orc.get_adjacency(coo, vals, shape, normalized=normalized, training=False, dtype=np.float64)
    return sp.csr_matrix((av, (ai[:, 0], ai[:, 1])), shape=shape)


def test_eval_forwards_of_the_oracle():
    coo, vals, shape = ref.graph()
    assert np.array_equal(cases.load("eval")["graph"], cases.digest(coo, vals))
    seen = dict()
    for name in ("appnp", "appnpreg"):                      # APPNPReg is APPNP without the input Dropout: the same eval forward
        z, X, parameters, want = eval_case(name)
        got, _ = orc.appnp_forward_eval(coo, vals, shape, X, pairs(parameters), a=0.1, iterations=cases.APPNP_ITERATIONS, dtype=np.float64)
        seen[name] = ratio(got, want)
    z, X, parameters, want = eval_case("gcn")
    seen["gcn"] = ratio(orc.gcn_forward_eval(coo, vals, shape, X, pairs(parameters), dtype=np.float64), want)
    for name in ("gcnii", "gcniireg"):                      # GCNIIReg in eval mode: FastReg passes its input on, every dropout is the identity
        z, X, parameters, want = eval_case(name)
        got = orc.gcnii_forward_eval(coo, vals, shape, X, (f64(parameters[0]), f64(parameters[1])), [f64(p) for p in parameters[2:-2]],
                                     (f64(parameters[-2]), f64(parameters[-1])), a=0.1, l=0.5, dtype=np.float64)
        seen[name] = ratio(got, want)
    z, X, parameters, want = eval_case("ngcf")
    H, blocks = f64(X), []
    for k in range(3):
        W1, W2, b1, b2 = (f64(p) for p in parameters[4 * k:4 * k + 4])                               # gcn.py:120-123: the creation order
        H = orc.ngcf_layer_eval(coo, vals, shape, H, W1, b1, W2, b2, dtype=np.float64)
        blocks.append(H)
    seen["ngcf layer"] = ratio(blocks[0], z["ngcf.layer0"])
    assert want.shape == (3 * ref.N, 16)                                                              # Concatenate stacks along axis 0
    seen["ngcf"] = ratio(np.concatenate(blocks, axis=0), want)
    for name, r in seen.items():
        print(f"eval forward {name}: {r:.3g} x the bar")
    assert max(seen.values()) <= 1


@pytest.mark.parametrize("name", ["gcn", "gcn-spectral", "gcnii", "gcnii-spectral", "ngcf"])
def test_eval_forwards_of_the_step_reference(name):
    """model_step_ref.Reference.evaluate(): the restatement the training steps are judged against, in eval mode."""
    z, X, parameters, want = eval_case(name)
    coo, vals, shape = ref.graph()
    r = ref.Reference(cases.eval_layers(name), coo, vals, shape, X, parameters, ref.node_task(), ref.WEIGHT_DECAY, ref.SEED, fixed=ref.FixedMasks(23))
    got = r.evaluate()
    print(f"Reference.evaluate {name}: {ratio(got, want):.3g} x the bar")
    assert r.streams == 0 and ratio(got, want) <= 1


def test_eval_halves_of_the_fused_layer_references():
    """gcn_fused_ref.forward_ref, gcn_spectral_ref.spectral_ref, gcnii_spectral_ref.spectral_ref and ngcf_fused_ref.forward_ref, chained
    into the models' eval forwards over the float64 adjacency.  The last two hold float32 constants (the module docstring)."""
    import gcn_fused_ref
    import gcn_spectral_ref
    import gcnii_spectral_ref
    import ngcf_fused_ref
    A, B = constant_csr(), constant_csr("bipartite")
    seen = dict()
    for name, layer in (("gcn", gcn_fused_ref.forward_ref), ("gcn-spectral", gcn_spectral_ref.spectral_ref)):
        z, X, parameters, want = eval_case(name)
        H = f64(X)
        for W, b in pairs(parameters):
            H = layer(A, H, W, b, True)["out"]
        seen[name] = (ratio(H, want), 1.0)
    z, X, parameters, want = eval_case("gcnii-spectral")
    H0 = np.maximum(f64(X) @ f64(parameters[0]) + f64(parameters[1]), 0)
    H = H0
    for k in range(cases.EVAL_ITERATIONS):
        W, bias = f64(parameters[2 + 2 * k]), f64(parameters[3 + 2 * k])
        beta = math.log1p(0.5 / (k + 1))
        H = gcnii_spectral_ref.spectral_ref(A, H, H0, (1 - beta) * np.eye(W.shape[1]) + beta * W, bias.reshape(-1), 0.1, True)["out"]
    float32_constants = lambda layers: (RTOL + layers * 2.0 ** -24) / RTOL
    seen["gcnii-spectral"] = (ratio(H @ f64(parameters[-2]) + f64(parameters[-1]), want), float32_constants(cases.EVAL_ITERATIONS))
    z, X, parameters, want = eval_case("ngcf")
    H, blocks = f64(X), []
    for k in range(3):
        W1, W2, b1, b2 = (f64(p) for p in parameters[4 * k:4 * k + 4])
        H = ngcf_fused_ref.forward_ref(B, H, W1, b1, W2, b2, "leaky")["out"]
        blocks.append(H)
    seen["ngcf"] = (ratio(np.concatenate(blocks, axis=0), want), float32_constants(3))
    for name, (r, bar) in seen.items():
        print(f"fused-layer reference, eval half, {name}: {r:.3g} x the 1e-9 bar (held to {bar:.3g} x)")
    assert all(r <= bar for r, bar in seen.values())


def test_signal_and_structural_eval_forwards():
    import signal_ref
    z, X, _, want = eval_case("pprsweep")
    signal, _ = signal_ref.ppr_ref(constant_csr(), None, 0.1, signal_ref.PPR_ITERATIONS, 512)
    # ppr_ref mixes with float32(1 - a), float32(a) as the launch does: rounding, ten steps of 2^-24 relative (the module docstring)
    bar = (RTOL + signal_ref.PPR_ITERATIONS * 2.0 ** -24) / RTOL
    got = ratio(f64(X) / signal[:, None], want)
    print(f"PPRSweep: {got:.3g} x the 1e-9 bar (held to {bar:.3g} x: float32 mixing constants)")
    assert got <= bar
    # the same sweep with float64 constants: the meaning alone, at the bar itself
    A, h = constant_csr(), np.ones(ref.N)
    for _ in range(10):
        h = (A @ h) * (1 - 0.1) + 0.1
    assert ratio(f64(X) / h[:, None], want) <= 1
    for name in ("structural", "structural-l2"):
        z, X, parameters, want = eval_case(name)
        table = np.concatenate([f64(parameters[0]), f64(parameters[1])], axis=0)
        if name.endswith("l2"):
            table = orc.l2_normalize_rows(table)
        assert want.shape == (ref.N, 16) and ratio(table, want) <= 1                                  # zero-width features: the embeddings


# ---- the training steps ------------------------------------------------------------------------------------------------------------------
def expected_calls(layers, width, nnz, forwards, ordinal=0, stream=0):
    """The dropout calls the contract of tests/model_step_ref.py names for ``forwards`` training forwards: per layer its dropped adjacency
    first, then its feature mask; a counter mask and an edge mask take the next stream, a host-drawn mask none."""
    calls = []
    for _ in range(forwards):
        w = width
        for layer in layers:
            w = layer.get("outputs", w)
            if layer.get("graph_dropout", 0) != 0:
                calls.append([ordinal, 0, nnz, 0, int(round(layer["graph_dropout"] * 1e6)), stream])
                ordinal, stream = ordinal + 1, stream + 1
            if layer.get("rate", 0) != 0:
                counter = layer["mask"] == "counter"
                calls.append([ordinal, 1 if counter else 2, ref.N, w, int(round(layer["rate"] * 1e6)), stream if counter else -1])
                ordinal, stream = ordinal + 1, stream + (1 if counter else 0)
    return calls


def run_with_eval(reference):
    """Reference.run() keeping the eval forward's output."""
    results, counts = [], []
    results.append(reference.step()); reference.update(); counts.append(reference.streams)
    out = reference.evaluate(); counts.append(reference.streams)
    results.append(reference.step()); reference.update(); counts.append(reference.streams)
    return results, counts, out


def compare_steps(name, z, results, counts, out):
    worst = 0.0
    for step, (loss, grads) in enumerate(results):
        worst = max(worst, abs(loss - float(z["losses"][step])) / (RTOL * abs(float(z["losses"][step]))))
        for k, g in enumerate(grads):
            worst = max(worst, ratio(g, z[f"step{step}.g{k}"]))
        assert f"step{step}.g{len(grads)}" not in z
    if "eval" in z:
        worst = max(worst, ratio(out, z["eval"]))
    print(f"{name}: two steps and the eval forward between them, worst ratio to the bar {worst:.3g}")
    assert counts == z["streams_after"].tolist(), (counts, z["streams_after"].tolist())
    assert worst <= 1
    return worst


@pytest.mark.parametrize("name", cases.step_meanings())
def test_two_training_steps(name):
    case, z = ref.cases()[name], cases.load("step_" + name)
    coo, vals, shape = ref.graph()
    X, parameters = ref.features(case["width"]), ref.initial_parameters(case["layers"], case["width"], seed=31)
    assert np.array_equal(z["inputs"], cases.digest(coo, vals, X, *parameters))
    results, counts, out = run_with_eval(ref.reference_for(case, fixed_seed=23))
    # the reference's own call order yields the contract's numbering: two training forwards, none in the eval forward between them
    want_calls = expected_calls(case["layers"], case["width"], len(coo), forwards=2)
    assert z["calls"].tolist() == want_calls
    assert z["calls_after"].tolist() == [len(want_calls) // 2, len(want_calls) // 2, len(want_calls)]
    compare_steps(name, z, results, counts, out)


def gcniireg_inputs():
    import signal_ref
    g = cases.GCNIIREG_STEP
    layers = signal_ref.gcniireg_layers(ref.CLASSES, g["latent_dims"], g["iterations"])
    coo, vals, shape = ref.graph()
    X, parameters = ref.features(g["width"]), ref.initial_parameters(layers, g["width"], seed=31)
    make = lambda projection: signal_ref.gcniireg_reference(layers, coo, vals, shape, X, parameters, ref.node_task(), ref.WEIGHT_DECAY, ref.SEED,
                                                            ref.FixedMasks(23), projection=projection)
    return layers, coo, X, parameters, make


def test_two_gcniireg_training_steps():
    """signal_ref.gcniireg_reference with the reference's own projection vector -- the zeros a variable created inside the forward holds
    -- against the reference's two steps: everything else FastReg does (where its dropped adjacency's stream is drawn, the quotient,
    its sign, D as column sums of the dropped values) at the 1e-9 bar, and the reference's leak as it is."""
    layers, coo, X, parameters, make = gcniireg_inputs()
    z = cases.load("step_gcniireg")
    assert np.array_equal(z["inputs"], cases.digest(coo, ref.graph()[1], X, *parameters))
    results, counts, out = run_with_eval(make("zeros"))
    # per training forward: the four host-drawn feature masks in layer order, then -- when the objective is formed -- FastReg's adjacency
    forward = expected_calls(layers, cases.GCNIIREG_STEP["width"], len(coo), forwards=1)
    want_calls = []
    for k in range(2):
        want_calls += [[len(want_calls) + i] + c[1:] for i, c in enumerate(forward)]
        want_calls.append([len(want_calls), 0, len(coo), 0, 500000, k])
    assert z["calls"].tolist() == want_calls and z["calls_after"].tolist() == [5, 5, 10]
    # the leak: one more variable per forward (two steps and the eval forward after each), all zeros, never reached by the objective
    n = len(parameters)
    assert int(z["variables_after"]) == n + 4 and z["projections"].shape == (4, 64) and not z["projections"].any()
    assert "step0.g%d" % n not in z and not z["step1.g%d" % n].any() and not z["step1.g%d" % (n + 1)].any() and "step1.g%d" % (n + 2) not in z
    trimmed = {k: v for k, v in z.items() if k not in ("step1.g%d" % n, "step1.g%d" % (n + 1))}
    compare_steps("gcniireg (projection: zeros)", trimmed, results, counts, out)


def test_fastreg_projection_is_a_named_deviation():
    """NAMED EXPECTED DIFFERENCE.  The reference's FastReg projects on W = 0 in every forward (the module docstring of
    signal_ref.gcniireg_reference has the lines): f = 1/2 everywhere and -lambda has no gradient.  This project's FastReg -- the
    restatement's default, the HIP path -- draws W from U(+-1) per training forward, one mask stream AHEAD of the dropped adjacency's,
    because with zeros the layer regularises nothing.  What that changes against the reference's recorded steps, and what it does not:"""
    layers, coo, X, parameters, make = gcniireg_inputs()
    z = cases.load("step_gcniireg")
    first = make("uniform")
    loss, grads = first.step()
    assert first.streams == 2 and first.fastreg["w_stream"] == 0 and first.fastreg["g_stream"] == 1          # the reference: one stream, its number 0
    assert int(z["streams_after"][0]) == 1
    assert np.abs(first.fastreg["W"]).max() > 0.5
    ratios = [ref.ratio_to_bar(g, z[f"step0.g{k}"]) for k, g in enumerate(grads)]
    print(f"FastReg's drawn projection against the reference's zeros: loss {ref.loss_ratio_to_bar(loss, float(z['losses'][0])):.3g} x the float32 bar, "
          f"gradients {[float(f'{r:.3g}') for r in ratios]} x the bar")
    assert ref.loss_ratio_to_bar(loss, float(z["losses"][0])) >= 10
    assert min(ratios[:2]) >= 10                           # the pre-MLP Dense behind H0: -lambda now has a gradient
    assert max(ratio(g, z[f"step0.g{k}"]) for k, g in enumerate(grads) if k >= 2) <= 1                      # everything after FastReg: untouched


def test_gcniireg_eval_forward():
    import signal_ref
    z, X, parameters, want = eval_case("gcniireg")
    coo, vals, shape = ref.graph()
    layers = signal_ref.gcniireg_layers(ref.CLASSES, (cases.EVAL_LATENT,), cases.EVAL_ITERATIONS)
    for projection in ("uniform", "zeros"):                # an eval forward neither draws nor reads the projection
        r = signal_ref.gcniireg_reference(layers, coo, vals, shape, X, parameters, ref.node_task(), ref.WEIGHT_DECAY, ref.SEED,
                                          ref.FixedMasks(23), projection=projection)
        got = r.evaluate()
        print(f"gcniireg_reference.evaluate ({projection}): {ratio(got, want):.3g} x the bar")
        assert r.streams == 0 and ratio(got, want) <= 1


def appnp_restated(coo, vals, shape, X, nodes, labels, parameters, kinds, dtype=torch.float64):
    """tests/test_gpu_training.py's dense statement of an APPNP step (filter.py:27-35, trainable.py:69-79), twice with an eval forward
    between: Dropout(0.5), Dense(relu, dropout 0.6), Dense = H0, K x ((1 - a) A_k H + a H0) over a fresh dropped adjacency each."""
    c = cases.APPNP_STEP
    masks, state = ref.FixedMasks(c["mask_seed"]), dict(streams=0)
    W1, b1, W2, b2 = params = [torch.tensor(f64(p), requires_grad=True) for p in parameters]
    X64, rows, y = torch.from_numpy(f64(X)), torch.from_numpy(nodes), torch.from_numpy(labels)

    def draw():
        state["streams"] += 1
        return state["streams"] - 1

    def feature_mask(shape_, p, kind):
        return torch.from_numpy(ref.counter_mask(shape_, p, c["seed"], draw()) if kind == "counter" else masks.mask(shape_, p))

    def forward(training):
        H = X64 * feature_mask(tuple(X64.shape), 0.5, kinds[0]) if training else X64
        H = torch.relu(H @ W1 + b1)
        if training:
            H = H * feature_mask(tuple(H.shape), 0.6, kinds[1])
        H0 = H @ W2 + b2
        Hk = H0
        for _ in range(c["K"]):
            ai, av = orc.get_adjacency(coo, vals, shape, graph_dropout=0.5, training=training, seed=c["seed"],
                                       stream=draw() if training else 0, dtype=np.float64)
            Hk = (torch.from_numpy(orc.to_dense(ai, av, shape, dtype=np.float64)) @ Hk) * (1 - c["a"]) + H0 * c["a"]
        return Hk

    results, counts, out = [], [], None
    for phase in ("step", "eval", "step"):
        if phase == "eval":
            with torch.no_grad():
                out = forward(False).numpy()
        else:
            for p in params:
                p.grad = None
            loss = torch.nn.functional.cross_entropy(forward(True)[rows], y) + c["weight_decay"] * ((W1 ** 2).sum() / 2 + (b1 ** 2).sum() / 2)
            loss.backward()
            results.append((float(loss.detach()), [p.grad.numpy().copy() for p in params]))
            with torch.no_grad():
                for p in params:
                    p -= ref.STEP_SIZE * p.grad
        counts.append(state["streams"])
    return results, counts, out


@pytest.mark.parametrize("name", sorted(cases.APPNP_STEP_KINDS))
def test_two_appnp_training_steps(name):
    z, c = cases.load("step_" + name), cases.APPNP_STEP
    coo, vals, shape, X, nodes, labels, parameters = cases.appnp_step_inputs()
    assert np.array_equal(z["inputs"], cases.digest(coo, vals, X, nodes, labels, *parameters))
    kinds = cases.APPNP_STEP_KINDS[name]
    results, counts, out = appnp_restated(coo, vals, shape, X, nodes, labels, parameters, kinds)
    layers = [dict(rate=0.5, mask=kinds[0]), dict(rate=0.6, mask=kinds[1], outputs=c["hidden"])] + [dict(graph_dropout=0.5, outputs=c["classes"])] * c["K"]
    want_calls = [[o, k, c["n"] if k else r, w, p, s] for o, k, r, w, p, s in expected_calls(layers, c["F"], len(coo), forwards=2)]
    assert z["calls"].tolist() == want_calls
    compare_steps(name, z, results, counts, out)


def test_float32_evaluations_of_the_reference():
    """The reference's own text evaluated in float32 on the stand-in against itself in float64, in units of the gradient bar: the first
    float32 evaluations of the reference itself next to model_step_ref.FLOAT32_YARDSTICK (a float32 evaluation of the restatement).
    Both are float32 evaluations of one expression in different operation orders, so they agree in magnitude, not in digits: within 4 x
    either way for NGCF (the cancellation residue the yardstick's comment derives); every other model is within the bar itself.
    Measured, gradients in units of the bar, the reference's text | FLOAT32_YARDSTICK:  ngcf 6.080 | 2.857, ngcf-fused 15.190 | 18.453,
    ngcf-fused-drop 4.295 | 4.294, ngcf-wide 7.341 | 5.348, ngcf-wide-drop 25.774 | 22.504; GCN, GCNII and APPNP in all their forms
    0.003 ... 0.025; every loss at most 0.04 x its bar."""
    for name in cases.step_meanings() + sorted(cases.APPNP_STEP_KINDS) + ["gcniireg"]:
        z = cases.load("step_" + name)
        worst, step, k = 0.0, 0, 0
        while f"step{step}.g0" in z:
            if f"f32.step{step}.ratio" in z:               # the 128-wide cases keep the errors, not the float32 gradients
                worst = max(worst, float(z[f"f32.step{step}.ratio"].max()))
            while f"step{step}.g{k}" in z and f"f32.step{step}.g{k}" in z:
                if not z[f"step{step}.g{k}"].any():         # (GCNIIReg's leaked projection vectors: zero gradients on both sides)
                    assert not z[f"f32.step{step}.g{k}"].any()
                    k += 1
                    continue
                worst = max(worst, ref.ratio_to_bar(z[f"f32.step{step}.g{k}"], z[f"step{step}.g{k}"]))
                k += 1
            step, k = step + 1, 0
        loss = max(ref.loss_ratio_to_bar(float(a), float(b)) for a, b in zip(z["f32.losses"], z["losses"]))
        written = ref.FLOAT32_YARDSTICK.get(name)
        print(f"{name}: the reference in float32 against float64: gradients {worst:.3f} x the bar, loss {loss:.3g} x the bar"
              + (f" (FLOAT32_YARDSTICK: {written})" if written else ""))
        assert loss <= 1
        if written:
            assert written / 4 <= worst <= 4 * written
        else:
            assert worst <= 1


# ---- heads and measures ------------------------------------------------------------------------------------------------------------------
def test_node_head():
    z = cases.load("heads")
    for C in cases.NODE_WIDTHS:
        logits, nodes, labels = cases.node_head_inputs(C)
        key = f"node{C}."
        assert np.array_equal(z[key + "logits"].astype(np.float32), logits) and np.array_equal(z[key + "nodes"], nodes) and np.array_equal(z[key + "labels"], labels)
        loss = orc.node_loss(f64(logits), nodes, labels)
        print(f"node head C={C}: loss {abs(loss - float(z[key + 'loss'])) / (RTOL * max(abs(float(z[key + 'loss'])), 1e-300)):.3g} x the bar")
        assert abs(loss - float(z[key + "loss"])) <= RTOL * abs(float(z[key + "loss"])) + 1e-300
        assert np.array_equal(orc.node_predict(logits, nodes), z[key + "predict"])                    # the first of two equal maxima
        assert orc.node_evaluate(logits, nodes, labels) == float(z[key + "evaluate"])
    assert float(z["node1.loss"]) == 0.0


def test_link_head():
    z = cases.load("heads")
    worst = 0.0
    for C in cases.LINK_WIDTHS:
        F, edges, labels, r = cases.link_head_inputs(C)
        key = f"link{C}."
        assert np.array_equal(z[key + "F"].astype(np.float32), F) and np.array_equal(z[key + "edges"], edges) and np.array_equal(z[key + "r"].astype(np.float32), r)
        for similarity in ("dot", "cos"):
            for weights, tag in ((None, "plain"), (f64(r), "r")):
                at = f"{key}{similarity}."
                logits = orc.link_logits(f64(F), edges, weights, similarity)
                worst = max(worst, ratio(logits, z[f"{at}diff.{tag}.logits"]), ratio(1 / (1 + np.exp(-logits)), z[f"{at}diff.{tag}.predict"]))
                for form, got in (("diff", orc.link_loss_diff(f64(F), edges, weights, similarity)),
                                  ("bce", orc.link_loss_bce(f64(F), edges, labels, weights, similarity))):
                    want = float(z[f"{at}{form}.{tag}.loss"])
                    worst = max(worst, abs(got - want) / (RTOL * abs(want)))
    print(f"link head: worst ratio to the bar {worst:.3g}")
    assert worst <= 1


def test_measures():
    """gnntf/metrics.py is numpy and CPU torch: loaded from its file, without the package around it (whose import loads the library)."""
    spec = importlib.util.spec_from_file_location("gnx_metrics_alone", os.path.join(ROOT, "gnn-tf_amd", "gnntf", "metrics.py"))
    metrics = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(metrics)
    z = cases.load("measures")
    for k, (labels, scores) in enumerate(cases.measure_inputs()):
        assert np.array_equal(z[f"m{k}.labels"], labels) and np.array_equal(z[f"m{k}.scores"], scores)
        want = float(z[f"m{k}.auc"])
        assert abs(metrics.auc(labels, scores) - want) <= RTOL * want + 1e-12 and abs(orc.auc_by_pairs(labels, scores) - want) <= RTOL * want + 1e-12
        for name in ("avprec", "rec", "prec", "f1"):
            got = [float(getattr(metrics, name)(labels, scores, top)) for top in (1, 5, 10)]
            np.testing.assert_allclose(got, z[f"m{k}.{name}"], rtol=RTOL, atol=0, err_msg=f"{name} of pair {k}")
    assert float(z["m2.auc"]) == 1.0 and float(z["m3.auc"]) == 0.0 and 0 < float(z["m1.auc"]) < 1
    assert metrics.acc(z["acc.predictions"], z["acc.labels"]) == float(z["acc"])
    assert metrics.acc(torch.from_numpy(z["acc.predictions"]), z["acc.labels"]) == float(z["acc"])


# ======================================================================================================================================
# d. the fixtures would have caught every planted mistake
# ======================================================================================================================================
def meaning_of(name):
    from test_gpu_model_steps import key_of
    all_cases = ref.cases()
    return next(m for m in cases.step_meanings() if key_of(all_cases[m]) == key_of(all_cases[name]))


def planted():
    from test_model_step_ref_cpu import PLANTED
    return PLANTED


def test_every_mistake_is_planted():
    assert sorted({m for m, _ in planted()}) == sorted(ref.MISTAKES)


@pytest.mark.parametrize("mistake,name", planted())
def test_the_fixture_sees_the_mistake(mistake, name):
    """The first step of the mistaken restatement against the reference's own: some compared quantity is off by at least 10 x the
    float32 bar of tests/test_gpu_model_steps.py (the case's own: four times the yardstick for NGCF)."""
    case, z = ref.cases()[name], cases.load("step_" + meaning_of(name))
    loss, grads = ref.reference_for(case, mistake=mistake, fixed_seed=23).step()
    ratios = [ref.loss_ratio_to_bar(loss, float(z["losses"][0]))] + [ref.ratio_to_bar(g, z[f"step0.g{k}"]) / case["bar"] for k, g in enumerate(grads)]
    print(f"{mistake} in {name}: loss {ratios[0]:.3g} x the bar, worst gradient {max(ratios[1:]):.3g} x the case's bar")
    assert max(ratios) >= 10

"""A stand-in for the TensorFlow names the reference project's ``gnntf`` package uses, over CPU torch.

TEST INFRASTRUCTURE ONLY.  Nothing imports this package unless a runner puts ``oracle/tf_standin`` on ``sys.path``
(tests/golden/make_reference_golden.py does, inside a child process; tests/test_reference_golden_cpu.py loads it under a private
module name to check its ops).  It exists so that the reference's own program text can be executed: its composition, call order,
constants, axes and regularisation are then the reference's, and only the meaning of each op below is our reading of TensorFlow's
documentation.  Every op carries one line stating the TensorFlow semantics it implements.

Arithmetic: float64 on the CPU; ``standin_configure(dtype="float32")`` selects float32 (every float tensor made afterwards, every
``assign`` and every mask is cast to it).  A tensor is a ``torch.Tensor`` subclass whose ``numpy()`` detaches first, as an eager
TensorFlow tensor's does.

The same bits on every processor: the fixtures are regenerated and compared array for array, so nothing here may go through a library
that picks its code path by the processor.  torch's CPU sqrt, exp, log and tanh go through a vector math library that does (its
square root is not even the correctly rounded one) and its matmul through a BLAS that does; the stand-in takes neither: those unary
ops are evaluated one element at a time by the C library (``_Libm``) and the matrix product as the k-ascending sum of outer products
in plain element-wise multiplies and adds (``_MatMul``), both with their derivatives written out.  The runner also pins torch's own
kernels to their processor-independent build.

Dropout draws nothing here: ``tf.nn.dropout`` asks the mask provider that the runner installs (``standin_configure(provider=)``)
with the call's ordinal, the operand's shape and the rate, and multiplies by what it returns -- an array of the operand's shape
that is 0 at dropped elements and 1 / (1 - rate), to float32 rounding, at kept ones (checked).

Not supported, raising on first use with the op's name: keras.models, keras.layers, keras.optimizers, keras.metrics, keras.Input and
every keras.losses class but the two ``from_logits=True`` losses the reference's predictors call (without them no training step of
the reference can be evaluated)."""
import math as _math

import numpy as _np
import torch as _torch

_DTYPES = {"float64": _torch.float64, "float32": _torch.float32}
_state = dict(dtype=_torch.float64, provider=None, ordinal=0, generator=_torch.Generator().manual_seed(0), tape_targets=[])


def standin_configure(dtype=None, provider=None, reset_ordinal=True):
    """The constructor switch: the float type of everything made from here on, and the dropout mask provider."""
    if dtype is not None:
        _state["dtype"] = _DTYPES[str(dtype)]
    _state["provider"] = provider
    if reset_ordinal:
        _state["ordinal"] = 0
    _state["tape_targets"] = []


def standin_tape_targets():
    """The values GradientTape.gradient was asked to differentiate, in call order (the objective of each training step)."""
    return list(_state["tape_targets"])


class Tensor(_torch.Tensor):
    """tf.Tensor: an eager tensor; ``numpy()`` gives its value whether or not a tape watches it."""

    def numpy(self):
        return _torch.Tensor.numpy(self.detach().as_subclass(_torch.Tensor))


def _t(x, dtype=None):
    """Anything -> Tensor; floating values take the configured float type (as tf.constant and op inputs take the graph's)."""
    if isinstance(x, _torch.Tensor):
        out = x
    else:
        out = _torch.as_tensor(_np.asarray(x))
    if dtype is not None:
        out = out.to(dtype)
    elif out.is_floating_point() and out.dtype != _state["dtype"]:
        out = out.to(_state["dtype"])
    return out if isinstance(out, Tensor) else out.as_subclass(Tensor)


def _plain(x):
    return x.detach().as_subclass(_torch.Tensor)


def _libm(name, x):
    """``name`` of the C library element by element, in float64, rounded to x's type."""
    fn = getattr(_math, name)
    flat = _plain(x).to(_torch.float64).reshape(-1).tolist()
    return _torch.tensor([fn(v) for v in flat], dtype=_torch.float64).reshape(x.shape).to(x.dtype)


class _Libm(_torch.autograd.Function):
    """y = f(x) through the C library; the derivative in terms of x and y, in exact element-wise arithmetic."""
    DERIVATIVE = {"sqrt": lambda x, y: 0.5 / y, "exp": lambda x, y: y, "log": lambda x, y: 1.0 / x, "log1p": lambda x, y: 1.0 / (1.0 + x),
                  "tanh": lambda x, y: 1.0 - y * y}

    @staticmethod
    def forward(ctx, x, name):
        y = _libm(name, x)
        ctx.save_for_backward(_plain(x), y)
        ctx.name = name
        return y

    @staticmethod
    def backward(ctx, grad):
        x, y = ctx.saved_tensors
        return _plain(grad) * _Libm.DERIVATIVE[ctx.name](x, y), None


def _unary(name, x):
    return _t(_Libm.apply(_t(x).as_subclass(_torch.Tensor), name))


def _product(a, b):
    """a . b as sum over k ascending of a[:, k] b[k, :], each product and each add rounded once: IEEE arithmetic decides every bit."""
    out = _torch.zeros((a.shape[0], b.shape[1]), dtype=a.dtype)
    for k in range(a.shape[1]):
        out = out + a[:, k:k + 1] * b[k:k + 1, :]
    return out


class _MatMul(_torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        a, b = _plain(a), _plain(b)
        ctx.save_for_backward(a, b)
        return _product(a, b)

    @staticmethod
    def backward(ctx, grad):
        a, b = ctx.saved_tensors
        grad = _plain(grad)
        return _product(grad, b.t()), _product(a.t(), grad)


# ---- variables -----------------------------------------------------------------------------------------------------------------------
class Variable(Tensor):
    """tf.Variable(initial_value, trainable): a mutable tensor; ``assign`` overwrites it with a value of the same shape."""

    @staticmethod
    def __new__(cls, initial_value=None, trainable=True, **kwargs):
        data = _t(initial_value).detach().clone().as_subclass(_torch.Tensor)
        return _torch.Tensor._make_subclass(cls, data, bool(trainable))

    def __init__(self, initial_value=None, trainable=True, **kwargs):
        self.trainable = bool(trainable)

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        """An op on a variable gives a tensor, not a variable."""
        with _torch._C.DisableTorchFunctionSubclass():
            out = func(*args, **(kwargs or {}))
        if isinstance(out, _torch.Tensor) and not isinstance(out, Variable):
            return out.as_subclass(Tensor)
        return out

    def assign(self, value):
        """tf.Variable.assign(value): the variable takes ``value``; the shapes must agree."""
        value = _t(value)
        if tuple(value.shape) != tuple(self.shape):
            raise ValueError(f"tf.Variable.assign: shape {tuple(value.shape)} into {tuple(self.shape)}")
        with _torch.no_grad():
            self.copy_(value)
        return self


def identity(x):
    """tf.identity(x): a tensor with the shape and contents of x (of a variable: a snapshot of its value)."""
    return _t(x).detach().clone().as_subclass(Tensor)


# ---- constructors --------------------------------------------------------------------------------------------------------------------
def zeros(shape, dtype=None):
    """tf.zeros(shape): all elements 0."""
    return _t(_torch.zeros(tuple(shape), dtype=_state["dtype"]))


def ones(shape, dtype=None):
    """tf.ones(shape): all elements 1."""
    return _t(_torch.ones(tuple(shape), dtype=_state["dtype"]))


def eye(num_rows, num_columns=None, dtype=None):
    """tf.eye(n): the n x n identity."""
    return _t(_torch.eye(int(num_rows), int(num_rows if num_columns is None else num_columns), dtype=_state["dtype"]))


def constant(value, dtype=None, shape=None):
    """tf.constant(value, shape=): a tensor of ``value``, reshaped to ``shape`` where given."""
    out = _t(value)
    return out if shape is None else out.reshape(tuple(shape))


# ---- dense ops -------------------------------------------------------------------------------------------------------------------------
def matmul(a, b):
    """tf.matmul(a, b): the matrix product a . b."""
    a, b = _t(a), _t(b)
    if a.dim() != 2 or b.dim() != 2 or a.shape[1] != b.shape[0] or a.dtype != b.dtype:
        raise ValueError(f"tf.matmul: operands of shapes {tuple(a.shape)} and {tuple(b.shape)}, types {a.dtype} and {b.dtype}")
    return _t(_MatMul.apply(a.as_subclass(_torch.Tensor), b.as_subclass(_torch.Tensor)))


def concat(values, axis):
    """tf.concat(values, axis): the tensors joined along ``axis``."""
    return _torch.cat([_t(v) for v in values], dim=int(axis))


def reshape(tensor, shape):
    """tf.reshape(tensor, shape): the same elements in row-major order under a new shape; one -1 is inferred."""
    return _t(tensor).reshape(tuple(shape))


def multiply(x, y):
    """tf.multiply(x, y): the element-wise product, with broadcasting."""
    return _t(x) * _t(y)


def reduce_sum(input_tensor, axis=None, keepdims=False):
    """tf.reduce_sum(x, axis): the sum over ``axis`` (all elements where None)."""
    x = _t(input_tensor)
    return x.sum() if axis is None else x.sum(dim=axis, keepdim=keepdims)


def reduce_mean(input_tensor, axis=None, keepdims=False):
    """tf.reduce_mean(x, axis): the mean over ``axis`` (all elements where None)."""
    x = _t(input_tensor)
    return x.mean() if axis is None else x.mean(dim=axis, keepdim=keepdims)


def exp(x):
    """tf.exp(x): e^x element-wise."""
    return _unary("exp", x)


def sqrt(x):
    """tf.sqrt(x): the square root element-wise."""
    return _unary("sqrt", x)


def sigmoid(x):
    """tf.sigmoid(x) = tf.nn.sigmoid(x): 1 / (1 + e^-x) element-wise."""
    return _torch.sigmoid(_t(x))


def round(x):
    """tf.round(x): to the nearest integer, halves to the even one."""
    return _torch.round(_t(x))


def argmax(input, axis=None):
    """tf.argmax(x, axis): the index of the largest value along ``axis`` (0 where None), the smallest index among equal values, int64."""
    x = _t(input).detach().numpy()
    return _t(_np.argmax(x, axis=0 if axis is None else axis).astype(_np.int64))


def gather(params, indices, axis=0):
    """tf.gather(params, indices, axis): the slices of ``params`` along ``axis`` at ``indices``."""
    return _torch.index_select(_t(params), int(axis), _index(indices))


def _index(indices):
    return _torch.as_tensor(_np.asarray(indices.detach().numpy() if isinstance(indices, _torch.Tensor) else indices, dtype=_np.int64)).reshape(-1)


# ---- nn --------------------------------------------------------------------------------------------------------------------------------
class nn:
    @staticmethod
    def relu(features):
        """tf.nn.relu(x): max(x, 0)."""
        return _torch.relu(_t(features))

    @staticmethod
    def leaky_relu(features, alpha=0.2):
        """tf.nn.leaky_relu(x, alpha=0.2): x where x > 0, alpha x elsewhere; the default alpha is 0.2."""
        return _torch.nn.functional.leaky_relu(_t(features), negative_slope=float(alpha))

    @staticmethod
    def tanh(x):
        """tf.nn.tanh(x): the hyperbolic tangent element-wise."""
        return _unary("tanh", x)

    @staticmethod
    def sigmoid(x):
        """tf.nn.sigmoid(x): 1 / (1 + e^-x) element-wise."""
        return _torch.sigmoid(_t(x))

    @staticmethod
    def softmax(logits, axis=-1):
        """tf.nn.softmax(logits, axis): e^x / sum e^x along ``axis``."""
        return _torch.softmax(_t(logits), dim=int(axis))

    @staticmethod
    def log_softmax(logits, axis=-1):
        """tf.nn.log_softmax(logits, axis): x - log(sum e^x) along ``axis``."""
        return _torch.log_softmax(_t(logits), dim=int(axis))

    @staticmethod
    def l2_loss(t):
        """tf.nn.l2_loss(t): sum(t ** 2) / 2."""
        t = _t(t)
        return (t * t).sum() / 2

    @staticmethod
    def l2_normalize(x, axis=None, epsilon=1e-12):
        """tf.nn.l2_normalize(x, axis, epsilon=1e-12) = tf.math.l2_normalize: x * rsqrt(max(sum(x ** 2) along axis, epsilon))."""
        x = _t(x)
        squares = (x * x).sum() if axis is None else (x * x).sum(dim=axis, keepdim=True)
        return x * _torch.rsqrt(_torch.clamp(squares, min=float(epsilon)))

    @staticmethod
    def embedding_lookup(params, ids):
        """tf.nn.embedding_lookup(params, ids): the rows params[ids]."""
        return _torch.index_select(_t(params), 0, _index(ids))

    @staticmethod
    def dropout(x, rate):
        """tf.nn.dropout(x, rate): every element is kept with probability 1 - rate and scaled by 1 / (1 - rate), the others become 0;
        rate = 0 returns x.  Which elements are kept is the mask provider's decision (the module docstring)."""
        x = _t(x)
        rate = float(rate)
        if not 0 <= rate < 1:
            raise ValueError("tf.nn.dropout: rate must be in [0, 1)")
        if rate == 0:
            return x
        if _state["provider"] is None:
            raise RuntimeError("tf.nn.dropout: no mask provider installed (standin_configure(provider=...))")
        ordinal = _state["ordinal"]
        _state["ordinal"] += 1
        mask = _np.asarray(_state["provider"](ordinal, tuple(x.shape), rate), dtype=_np.float64)
        if mask.shape != tuple(x.shape):
            raise ValueError(f"tf.nn.dropout: a mask of shape {mask.shape} for an operand of shape {tuple(x.shape)}")
        kept = mask[mask != 0]
        if kept.size and _np.abs(kept * (1 - rate) - 1).max() > 2.0 ** -23:
            raise ValueError("tf.nn.dropout: kept elements are scaled by 1 / (1 - rate)")
        return x * _torch.from_numpy(mask).to(x.dtype)


# ---- math ------------------------------------------------------------------------------------------------------------------------------
class math:
    @staticmethod
    def log(x):
        """tf.math.log(x): the natural logarithm element-wise."""
        return _unary("log", x)

    @staticmethod
    def log1p(x):
        """tf.math.log1p(x): log(1 + x) element-wise."""
        return _unary("log1p", x)

    @staticmethod
    def log_sigmoid(x):
        """tf.math.log_sigmoid(x): log(1 / (1 + e^-x)) = -softplus(-x), computed without overflow."""
        return _torch.nn.functional.logsigmoid(_t(x))

    @staticmethod
    def divide_no_nan(x, y):
        """tf.math.divide_no_nan(x, y): x / y, and 0 where y is 0 (whatever x is)."""
        x, y = _t(x), _t(y)
        zero = y == 0
        return _torch.where(zero, _torch.zeros_like(y), x / _torch.where(zero, _torch.ones_like(y), y))

    @staticmethod
    def count_nonzero(input, axis=None):
        """tf.math.count_nonzero(x): the number of elements that are not 0, int64."""
        x = _t(input)
        return _torch.count_nonzero(x) if axis is None else _torch.count_nonzero(x, dim=axis)

    reduce_sum = staticmethod(reduce_sum)
    l2_normalize = staticmethod(nn.l2_normalize)


# ---- sparse ----------------------------------------------------------------------------------------------------------------------------
class SparseTensor:
    """tf.SparseTensor(indices, values, dense_shape): a COO list; nothing sorts it or merges equal indices.  ``sparse * dense`` and
    ``dense * sparse`` keep the sparse operand's index list and broadcast only the dense side to the sparse shape: each stored value
    is multiplied by the dense element at its index."""
    __array_priority__ = 1000

    def __init__(self, indices, values, dense_shape):
        self.indices = _torch.as_tensor(_np.asarray(indices, dtype=_np.int64).reshape(-1, 2))
        self.values = _t(values).reshape(-1)
        self.dense_shape = tuple(int(s) for s in dense_shape)
        if self.indices.shape[0] != self.values.shape[0]:
            raise ValueError("tf.SparseTensor: one value per index")

    @property
    def shape(self):
        return self.dense_shape

    def _cwise(self, dense):
        dense = _t(dense)
        if dense.dim() > 2 or any(d not in (1, s) for d, s in zip(reversed(dense.shape), reversed(self.dense_shape))):
            raise ValueError("SparseTensor * dense: only the dense side broadcasts, to the sparse operand's shape")
        spread = _torch.broadcast_to(dense, self.dense_shape)
        return SparseTensor(self.indices, self.values * spread[self.indices[:, 0], self.indices[:, 1]], self.dense_shape)

    __mul__ = _cwise
    __rmul__ = _cwise


class sparse:
    SparseTensor = SparseTensor

    @staticmethod
    def reduce_sum(sp_input, axis=None):
        """tf.sparse.reduce_sum(sp, axis): the sum of the stored values along ``axis`` as a dense tensor; entries with equal indices
        all add up; a row or column without entries sums to 0."""
        rows, cols = sp_input.indices[:, 0], sp_input.indices[:, 1]
        if axis is None:
            return sp_input.values.sum()
        axis = axis % 2
        out = _torch.zeros(sp_input.dense_shape[1 - axis], dtype=sp_input.values.dtype)
        return _t(out.index_add(0, cols if axis == 0 else rows, sp_input.values.as_subclass(_torch.Tensor)))

    @staticmethod
    def sparse_dense_matmul(sp_a, b):
        """tf.sparse.sparse_dense_matmul(A, B): out[i, :] = sum over the stored entries (i, j, v) of v B[j, :]; the index list may be
        unordered and entries with equal indices all add up."""
        b = _t(b)
        rows, cols = sp_a.indices[:, 0], sp_a.indices[:, 1]
        terms = (sp_a.values.to(b.dtype)[:, None] * b[cols]).as_subclass(_torch.Tensor)
        out = _torch.zeros((sp_a.dense_shape[0], b.shape[1]), dtype=b.dtype)
        return _t(out.index_add(0, rows, terms))

    @staticmethod
    def eye(num_rows, num_columns=None):
        """tf.sparse.eye(n): the n x n identity as a SparseTensor: the n diagonal entries, each 1, in order."""
        n = int(num_rows) if num_columns is None else min(int(num_rows), int(num_columns))
        diagonal = _np.arange(n, dtype=_np.int64)
        return SparseTensor(_np.stack([diagonal, diagonal], axis=1), ones((n,)), (int(num_rows), int(num_rows if num_columns is None else num_columns)))

    @staticmethod
    def add(a, b, threshold=0):
        """tf.sparse.add(a, b): the SparseTensor a + b.  The SparseAdd op states that it assumes both index lists in row-major order
        and merges them like two sorted lists: while both have entries left it compares the two front indices, emits the sum where
        they are equal (kept even where the sum is 0: threshold 0 drops nothing) and the smaller entry alone where they are not; what
        is left of either list follows.  THE READING CHOSEN for a list that is unordered or holds equal indices (the reference's
        graphs are both): the same merge runs over the lists as they are.  Every stored entry of a and of b is then emitted exactly
        once, alone or summed with ONE entry of the other list that has the same index -- an equal index may stay unmerged -- so the
        result, taken as a matrix (equal indices adding up, as every consumer in the reference does: reduce_sum,
        sparse_dense_matmul, the broadcast products), is a + b whatever the order.  Why this reading: it is the op's documented
        algorithm, it agrees with TensorFlow on ordered duplicate-free input, and on other input everything the reference computes
        from the result depends on the matrix alone; only the length and order of the index list are our reading."""
        if tuple(a.dense_shape) != tuple(b.dense_shape):
            raise ValueError("tf.sparse.add: operands of different shapes")
        ai, bi = a.indices.numpy(), b.indices.numpy()
        take_a, take_b, i, j = [], [], 0, 0
        while i < len(ai) and j < len(bi):
            ka, kb = (int(ai[i, 0]), int(ai[i, 1])), (int(bi[j, 0]), int(bi[j, 1]))
            if ka == kb:
                take_a.append(i); take_b.append(j); i += 1; j += 1
            elif ka < kb:
                take_a.append(i); take_b.append(-1); i += 1
            else:
                take_a.append(-1); take_b.append(j); j += 1
        take_a += list(range(i, len(ai))) + [-1] * (len(bi) - j)
        take_b += [-1] * (len(ai) - i) + list(range(j, len(bi)))
        take_a, take_b = _torch.as_tensor(take_a, dtype=_torch.int64), _torch.as_tensor(take_b, dtype=_torch.int64)
        zero = _torch.zeros(1, dtype=a.values.dtype)
        av, bv = _torch.cat([a.values, zero]), _torch.cat([b.values.to(a.values.dtype), zero])      # index -1: the appended 0
        indices = _torch.where((take_a >= 0)[:, None], a.indices[take_a.clamp(min=0)], b.indices[take_b.clamp(min=0)])
        return SparseTensor(indices, av[take_a] + bv[take_b], a.dense_shape)


# ---- training --------------------------------------------------------------------------------------------------------------------------
class GradientTape:
    """tf.GradientTape: records the ops on trainable variables inside its block; ``gradient(target, sources)`` gives d target / d
    source per source, None for a source the target does not depend on.  (torch autograd records always; the block is kept for form.)"""

    def __enter__(self):
        return self

    def __exit__(self, kind, value, traceback):
        return False

    def gradient(self, target, sources):
        sources = list(sources)
        _state["tape_targets"].append(float(target.detach()))
        grads = _torch.autograd.grad(target, sources, allow_unused=True)
        return [None if g is None else g.as_subclass(Tensor) for g in grads]


# ---- random and initialisers (no case depends on what they draw: every case assigns its parameters) ----------------------------------------
class random:
    @staticmethod
    def set_seed(seed):
        """tf.random.set_seed(seed): seeds the global generator."""
        _state["generator"].manual_seed(int(seed))

    @staticmethod
    def uniform(shape, minval=0, maxval=1):
        """tf.random.uniform(shape, minval=0, maxval=1): independent draws from U[minval, maxval)."""
        draw = _torch.rand(tuple(shape), generator=_state["generator"], dtype=_torch.float64)
        return _t(draw * (maxval - minval) + minval)


class _Unsupported:
    """A namespace of TensorFlow that the stand-in does not restate: any use raises, naming the op."""

    def __init__(self, name, supported=None):
        self._name, self._supported = name, dict(supported or {})

    def __getattr__(self, attribute):
        if attribute.startswith("__"):
            raise AttributeError(attribute)
        if attribute in self._supported:
            return self._supported[attribute]
        raise NotImplementedError(f"{self._name}.{attribute} is not supported by the TensorFlow stand-in")

    def __call__(self, *args, **kwargs):
        raise NotImplementedError(f"{self._name} is not supported by the TensorFlow stand-in")


def _fans(shape):
    shape = tuple(shape)
    return (shape[0], shape[0]) if len(shape) == 1 else (shape[-2], shape[-1])


class _initializers:
    class RandomUniform:
        """tf.keras.initializers.RandomUniform(minval, maxval)(shape): independent draws from U[minval, maxval)."""

        def __init__(self, minval=-0.05, maxval=0.05, seed=None):
            self.minval, self.maxval = float(minval), float(maxval)

        def __call__(self, shape, dtype=None):
            return random.uniform(shape, self.minval, self.maxval)

    class GlorotUniform:
        """tf.keras.initializers.GlorotUniform()(shape): U[-limit, limit), limit = sqrt(6 / (fan_in + fan_out))."""

        def __init__(self, seed=None):
            pass

        def __call__(self, shape, dtype=None):
            fan_in, fan_out = _fans(shape)
            limit = (6.0 / (fan_in + fan_out)) ** 0.5
            return random.uniform(shape, -limit, limit)

    class HeUniform:
        """tf.keras.initializers.HeUniform()(shape): U[-limit, limit), limit = sqrt(6 / fan_in)."""

        def __init__(self, seed=None):
            pass

        def __call__(self, shape, dtype=None):
            limit = (6.0 / _fans(shape)[0]) ** 0.5
            return random.uniform(shape, -limit, limit)


def _same_rank(y_true, y_pred):
    """Keras brings labels and predictions to one rank before a loss: where their ranks differ by one and the longer shape ends in 1,
    that axis is squeezed (labels [m, 1] against logits [m] become [m])."""
    y_true, y_pred = _t(y_true), _t(y_pred)
    if y_true.dim() == y_pred.dim() + 1 and y_true.shape[-1] == 1:
        y_true = y_true.squeeze(-1)
    elif y_pred.dim() == y_true.dim() + 1 and y_pred.shape[-1] == 1:
        y_pred = y_pred.squeeze(-1)
    return y_true, y_pred


class _SparseCategoricalCrossentropy:
    """tf.keras.losses.SparseCategoricalCrossentropy(from_logits=True)(labels, logits): the mean over the rows of
    -log_softmax(logits)[label]."""

    def __init__(self, from_logits=False, **kwargs):
        if not from_logits or kwargs:
            raise NotImplementedError("tf.keras.losses.SparseCategoricalCrossentropy: only from_logits=True is supported by the TensorFlow stand-in")

    def __call__(self, y_true, y_pred):
        y_pred = _t(y_pred)
        logp = _torch.log_softmax(y_pred, dim=-1)
        return -logp.gather(-1, _index(y_true).reshape(-1, 1)).mean()


class _BinaryCrossentropy:
    """tf.keras.losses.BinaryCrossentropy(from_logits=True)(labels, logits): the mean over all elements of
    max(z, 0) - z y + log(1 + e^-|z|) (tf.nn.sigmoid_cross_entropy_with_logits), labels and logits brought to one rank first."""

    def __init__(self, from_logits=False, **kwargs):
        if not from_logits or kwargs:
            raise NotImplementedError("tf.keras.losses.BinaryCrossentropy: only from_logits=True is supported by the TensorFlow stand-in")

    def __call__(self, y_true, y_pred):
        y, z = _same_rank(y_true, y_pred)
        y = y.to(z.dtype)
        return (_torch.clamp(z, min=0) - z * y + _unary("log1p", _unary("exp", -z.abs()))).mean()


class keras:
    initializers = _initializers
    models = _Unsupported("tf.keras.models")
    layers = _Unsupported("tf.keras.layers")
    optimizers = _Unsupported("tf.keras.optimizers")
    metrics = _Unsupported("tf.keras.metrics")
    losses = _Unsupported("tf.keras.losses", dict(SparseCategoricalCrossentropy=_SparseCategoricalCrossentropy,
                                                  BinaryCrossentropy=_BinaryCrossentropy))
    Input = _Unsupported("tf.keras.Input")

"""Sparse containers and the differentiable propagation ops over libgnx.so.

Stands where the reference uses tf.sparse.SparseTensor and tf.sparse.sparse_dense_matmul
(reference gnntf/core/gnn/graph_manipulation.py:31, gnntf/core/gnn/architectures/filter.py:19,
gnntf/core/gnn/architectures/gcn.py:88).
"""
from __future__ import annotations

import math
from collections import namedtuple
from ctypes import byref, c_float, c_int, c_int64, c_void_p

import numpy as np
import torch

from . import _native as nat


class SparseCOO:
    """What graph2adj returns: an UNSORTED COO that may hold duplicates, exactly like the
    tf.sparse.SparseTensor of the reference (graph_manipulation.py:31).
    ``indices`` int64 [nnz, 2], ``values`` float32 [nnz], ``dense_shape`` (rows, cols)."""

    def __init__(self, indices, values, dense_shape):
        if isinstance(indices, torch.Tensor):
            self.indices = indices.to(torch.int64).reshape(-1, 2)
            self.values = torch.as_tensor(values, dtype=torch.float32, device=self.indices.device).reshape(-1)
        else:
            self.indices = torch.from_numpy(np.ascontiguousarray(np.asarray(indices, dtype=np.int64).reshape(-1, 2)))
            self.values = torch.from_numpy(np.ascontiguousarray(np.asarray(values, dtype=np.float32).reshape(-1)))
        if self.indices.shape[0] != self.values.shape[0]:
            raise Exception("SparseCOO: indices and values disagree on the number of entries")
        self.dense_shape = (int(dense_shape[0]), int(dense_shape[1]))

    @property
    def shape(self):
        return self.dense_shape

    def to(self, device):
        return SparseCOO(self.indices.to(device), self.values.to(device), self.dense_shape)


def as_coo(graph) -> SparseCOO:
    """Accepts a SparseCOO, a torch sparse COO tensor, a scipy sparse matrix or an
    (indices, values, shape) triple."""
    if isinstance(graph, SparseCOO):
        return graph
    if isinstance(graph, torch.Tensor) and graph.is_sparse:
        return SparseCOO(graph._indices().t().contiguous(), graph._values(), graph.shape)
    if hasattr(graph, "tocoo"):
        m = graph.tocoo()
        return SparseCOO(np.stack([m.row, m.col], axis=1), m.data, m.shape)
    if isinstance(graph, (tuple, list)) and len(graph) == 3:
        return SparseCOO(*graph)
    raise Exception("Unsupported graph container: " + str(type(graph)))


class _BorrowedInt32:
    """A device array of ``n`` int32 the library owns, for torch.as_tensor (copied by the caller before the handle can change it)."""

    def __init__(self, pointer, n):
        self.__cuda_array_interface__ = dict(shape=(int(n),), typestr="<i4", data=(int(pointer or 0), False), version=2)


class DeviceGraph:
    """Owner of a gnx_graph_t (device CSR built from the COO)."""

    def __init__(self, coo: SparseCOO = None, device=None, csr=None):
        self._h = c_void_p()
        lib = nat.lib()
        if csr is not None:
            rowptr, colidx, vals, shape = csr
            nat.require_cuda(rowptr, colidx, vals)
            if (rowptr.dtype, colidx.dtype, vals.dtype) != (torch.int64, torch.int32, torch.float32):
                raise Exception("DeviceGraph: a CSR needs int64 rowptr, int32 colidx and float32 values")
            if not (rowptr.device == colidx.device == vals.device):
                raise Exception("DeviceGraph: the CSR arrays live on different devices")
            if rowptr.numel() != shape[0] + 1 or colidx.numel() != vals.numel():
                raise Exception("DeviceGraph: CSR array lengths do not match the shape")
            self.device = rowptr.device
            self._keep = (rowptr.contiguous(), colidx.contiguous(), vals.contiguous())
            with nat.on_device(self.device):    # (the creators take the stream mid-list: passed here, not appended)
                nat.launch(self.device, "gnx_graph_create_csr", shape[0], shape[1], self._keep[1].numel(), *self._keep, nat.current_stream(),
                           byref(self._h))
            self._keep = None
        else:
            device = torch.device(device if device is not None else "cuda")
            if device.type != "cuda":
                raise Exception("gnntf: graphs live on the GPU only; there is no CPU fallback")
            self.device = device
            idx = coo.indices.to(device).contiguous()
            val = coo.values.to(device).contiguous()
            self.device = idx.device                        # with its index ("cuda" -> "cuda:0")
            with nat.on_device(device):
                nat.launch(device, "gnx_graph_create_coo", *coo.dense_shape, idx.shape[0], idx, val, nat.current_stream(), byref(self._h))
        n_rows, n_cols, nnz_e, nnz_c = c_int64(), c_int64(), c_int64(), c_int64()
        nat.check(lib.gnx_graph_info(self._h, byref(n_rows), byref(n_cols), byref(nnz_e), byref(nnz_c)))
        self.n_rows, self.n_cols = n_rows.value, n_cols.value
        self.nnz_entries, self.nnz = nnz_e.value, nnz_c.value
        n_hub, threshold = c_int64(), c_int64()
        nat.check(lib.gnx_graph_hub_rows(self._h, byref(n_hub), byref(threshold)))
        # rows longer than ``long_row_threshold`` entries: the fused launches leave them to the long-row kernels (gnx_graph_hub_rows)
        self.n_hub_rows, self.long_row_threshold = n_hub.value, threshold.value
        self._entry_dropout = False

    @property
    def handle(self):
        return self._h

    @property
    def n_hub_rows_t(self) -> int:
        """``n_hub_rows`` of the TRANSPOSED structure: the columns with more than ``long_row_threshold`` entries, which the fused
        backward launches leave to the long-row kernels.  Counted once from a copy of the column indices and kept (it synchronises:
        the first use must not be under capture)."""
        if getattr(self, "_n_hub_rows_t", None) is None:
            if self.nnz == 0:
                self._n_hub_rows_t = 0
            else:
                counts = torch.bincount(self.csr_arrays()[1].long(), minlength=self.n_cols)
                self._n_hub_rows_t = int((counts > self.long_row_threshold).sum())
        return self._n_hub_rows_t

    @property
    def entry_dropout(self) -> bool:
        """Whether enable_entry_dropout() has run on this graph: the fused training kernels then accept its duplicate entries."""
        return getattr(self, "_entry_dropout", False)

    def enable_entry_dropout(self):
        """Builds NOW what the fused training kernels need on a graph whose COO holds duplicate entries (graph2adj of a graph that
        stores both directions: every entry twice): per coalesced slot its multiplicity and shared value, in CSR and transposed
        order (gnx_graph_enable_entry_dropout).  Edge dropout then stays per stored entry (layered.py:47-50), bit for bit what the
        materialised form gives, without writing a value array per iteration.  Allocates and synchronises: call before capturing.
        Does nothing on a graph without duplicates."""
        nat.launch(self.device, "gnx_graph_enable_entry_dropout", self._h)
        self._entry_dropout = True

    def csr_arrays(self, with_rows=False):
        """Copies of (rowptr int64, colidx int32, raw values float32[, rowidx int32])."""
        rowptr = torch.empty(self.n_rows + 1, dtype=torch.int64, device=self.device)
        colidx = torch.empty(self.nnz, dtype=torch.int32, device=self.device)
        vals = torch.empty(self.nnz, dtype=torch.float32, device=self.device)
        rows = torch.empty(self.nnz, dtype=torch.int32, device=self.device) if with_rows else None
        nat.launch(self.device, "gnx_graph_export", self._h, rowptr, colidx, vals, rows)
        return (rowptr, colidx, vals, rows) if with_rows else (rowptr, colidx, vals)

    def last_kernel(self) -> str:
        return (nat.lib().gnx_graph_last_kernel(self._h) or b"").decode()

    def reserve(self, C, transposed=False, k_loop=False, train_gather=False, gather_hints=False):
        """Builds NOW what the launches otherwise build on first use, sized for feature rows of up to ``C`` floats (the long-row
        slab; with ``transposed`` the transposed structure a backward needs; with ``k_loop`` the relabelled copy appnp_propagate
        runs narrow widths on; with ``train_gather`` the gather order and gather columns of the training loops' relabelled operand
        order, ppr_loop(gather_order="relabelled"), which implies ``transposed``; with ``gather_hints`` the hinted columns of
        set_gather_hints at this width, and with them the pendant plan of set_pendant_elision): those lazy builds allocate and synchronise, which
        a stream under hipGraph capture must not see (a launch that would have to grow something there raises instead).  Call
        before capturing (gnx_graph_reserve)."""
        flags = ((nat.RESERVE_TRANSPOSED if transposed else 0) | (nat.RESERVE_K_LOOP if k_loop else 0)
                 | (nat.RESERVE_TRAIN_GATHER if train_gather else 0) | (nat.RESERVE_GATHER_HINTS if gather_hints else 0))
        nat.launch(self.device, "gnx_graph_reserve", self._h, C, flags)

    def gather_order(self):
        """(order, rank), int32 [n] each, copies: the handle's gather order (gnx_graph_gather_order) -- ``order[i]`` = the vertex at
        position i, ``rank`` its inverse.  ``X[order.long()]`` is X stored in gather order.  Builds the order on first use
        (allocates and synchronises: not under capture)."""
        order, rank = c_void_p(), c_void_p()
        nat.launch(self.device, "gnx_graph_gather_order", self._h, byref(order), byref(rank))
        with nat.on_device(self.device):
            return tuple(torch.as_tensor(_BorrowedInt32(p.value, self.n_rows), device=self.device).clone() for p in (order, rank))

    def set_gather_hints(self, hot_rows=-1):
        """Gather hints of the wide float32 eval launches (gnx_graph_set_gather_hints): the ``hot_rows`` rows with the most entries
        are the ones worth keeping in the L2s; every other row is gathered with a non-temporal load.  -1 = automatic (large graphs,
        the rows that fill half an L2 at the width of the call), 0 = off, n > 0 = that many hot rows.  Same bits either way."""
        nat.launch(self.device, "gnx_graph_set_gather_hints", self._h, hot_rows)

    def gather_hints(self):
        """(hinted columns int32 [nnz] or None, hot_rows): a copy of the handle's hinted column array -- the column of every entry,
        bit 31 set where the column is not a hot row -- and the hot-row count it was built for (gnx_graph_gather_hints)."""
        cols, hot = c_void_p(), c_int64()
        with nat.on_device(self.device):
            nat.check(nat.lib().gnx_graph_gather_hints(self._h, byref(cols), byref(hot), None))
            if not cols.value:
                return None, 0
            torch.cuda.current_stream().synchronize()
            return torch.as_tensor(_BorrowedInt32(cols.value, self.nnz), device=self.device).clone(), hot.value

    def last_launch_hot_rows(self) -> int:
        """Hot rows the last SpMM launch over this graph gathered with; 0 = it took no gather hints (last_kernel() does not say)."""
        last = c_int64()
        nat.check(nat.lib().gnx_graph_gather_hints(self._h, None, None, byref(last)))
        return last.value

    def set_pendant_elision(self, mode=-1):
        """Pendant elision of appnp_propagate's K loop (gnx_graph_set_pendant_elision): a row whose one entry points at a row that
        alone points back is computed by the last iteration only; its neighbour forms the iterates between itself.  -1 = automatic
        (where the automatic gather hints are on), 0 = off, 1 = on wherever the launches take gather hints.  Same bits either way."""
        nat.launch(self.device, "gnx_graph_set_pendant_elision", self._h, mode)

    def pendant_elision(self):
        """(elidable rows as a bool tensor [n] or None when no plan is built, whether the last K loop elided them)
        (gnx_graph_pendant_elision)."""
        count, flags, last = c_int64(), c_void_p(), c_int()
        nat.launch(self.device, "gnx_graph_pendant_elision", self._h, byref(count), byref(flags), byref(last))
        with nat.on_device(self.device):
            if not flags.value:
                return None, bool(last.value)
            torch.cuda.current_stream().synchronize()
            borrowed = _BorrowedInt32(flags.value, self.n_rows)
            borrowed.__cuda_array_interface__["typestr"] = "|u1"
            rows = torch.as_tensor(borrowed, device=self.device).clone().bool()
            assert int(rows.sum()) == count.value
            return rows, bool(last.value)

    def set_row_window(self, window_rows):
        """Declares that the vertex numbering of THIS graph carries locality (a community / breadth-first order): launches take the
        rows in windows of ``window_rows`` consecutive ids (degree-binned inside a window) and narrow widths stay off the
        degree-relabelled copy; 0 = the default global degree bins (gnx_graph_set_row_window).  Same sums, other launch order."""
        nat.launch(self.device, "gnx_graph_set_row_window", self._h, window_rows)
        self.row_window = int(window_rows)

    def set_dropout_counter(self, counter):
        """``counter``: a one-element int64 device tensor added to every dropout stream id used with this graph (read by the
        kernels when they run), or None.  Lets a captured training step draw fresh masks on every replay."""
        if counter is not None and (counter.dtype != torch.int64 or counter.numel() != 1 or counter.device != self.device):
            raise Exception("set_dropout_counter: needs a one-element int64 tensor on the graph's device")
        self._counter = counter                                   # keep it alive while the handle points at it
        nat.check(nat.lib().gnx_graph_set_dropout_counter(self._h, nat.ptr(counter)))

    def __del__(self):
        try:
            if self._h:
                nat.lib().gnx_graph_destroy(self._h)
                self._h = c_void_p()
        except Exception:
            pass


class Adjacency:
    """What GNN.get_adjacency returns: a device graph + one set of (normalised, possibly
    dropped-out) values + the diagonal weight of an added identity.  Usable with
    ``gnntf.spmm(adj, H)`` wherever the reference calls tf.sparse.sparse_dense_matmul."""

    def __init__(self, graph: DeviceGraph, vals: torch.Tensor = None, diag: torch.Tensor = None, vals_t: torch.Tensor = None):
        self.graph = graph
        self.vals = vals          # values in coalesced-CSR order (None: the handle's raw values)
        self.diag = diag
        self.vals_t = vals_t      # the same values in the order of the transposed structure (backward), or None
        self.transposed_only = False   # normalize(..., transposed_only=True): ``vals`` is None because only ``vals_t`` was written, not because the values are the raw ones
        self.raw_dropout = None   # (p, seed, stream) when the values are the dropped RAW ones (normalize(..., "none", "none", p, ...)): signal_colsum

    def transposed_values(self):
        """Values in transposed order, permuted once and kept (a constant adjacency is reused by every backward)."""
        if self.vals_t is None:
            out = torch.empty(self.graph.nnz, dtype=torch.float32, device=self.graph.device)
            nat.launch(self.graph.device, "gnx_graph_permute_values_t", self.graph.handle, self.vals, out)
            self.vals_t = out
        return self.vals_t

    @property
    def shape(self):
        return (self.graph.n_rows, self.graph.n_cols)


class DroppedAdjacency(Adjacency):
    """The dropped + symmetrically re-normalised adjacency of one training iteration (layered.py:47-50 + gnn.py:41-42) WITHOUT
    its nnz-sized value array: only the N degree scales are computed up front; the SpMM kernels produce every entry's weight
    (D[row] * dropout(raw)) * D[col] from the counter RNG while they gather (gnx_spmm_dropped) -- forward and transposed, bit
    for bit the values gnx_graph_normalize would have written.  ``.vals`` materialises them on demand (custom layers).
    PRECONDITION: finite features and finite degree scales.  A dropped entry is SKIPPED here (its row is not gathered), whereas
    the reference keeps it as an explicit zero (tf.nn.dropout on G.values, layered.py:50), so 0 * inf or 0 * NaN in the
    gathered row -- or a NaN scale from a negative column sum -- makes a NaN there and not here.  For exact NaN propagation
    use the materialised form (``normalize(graph, "symmetric", "none", p, seed, stream)`` + ``spmm``), which multiplies every
    stored entry."""

    def __init__(self, graph: DeviceGraph, p, seed, stream_id, D=None):
        super().__init__(graph, None, None, None)
        self.p, self.seed, self.stream_id = float(p), int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream_id) & 0xFFFFFFFFFFFFFFFF
        self.D = D if D is not None else dropped_degree_scales(graph, self.p, self.seed, self.stream_id, 1)[0]
        self._vals = None

    @property
    def vals(self):
        if self._vals is None:
            self._vals = normalize(self.graph, "symmetric", "none", self.p, self.seed, self.stream_id).vals
        return self._vals

    @vals.setter
    def vals(self, value):
        self._vals = value

    def transposed_values(self):
        if self.vals_t is None:
            self.vals_t = normalize(self.graph, "symmetric", "none", self.p, self.seed, self.stream_id, transposed_only=True).vals_t
        return self.vals_t


def dropped_degree_scales(graph: DeviceGraph, p, seed, first_stream, n_streams) -> torch.Tensor:
    """D = divide_no_nan(1, sqrt(column sums of the dropped values)) (gnn.py:41) for ``n_streams`` consecutive dropout streams,
    [n_streams, n]: ONE pass over the structure for all of them (gnx_graph_colsum_streams)."""
    D = torch.empty((n_streams, graph.n_cols), dtype=torch.float32, device=graph.device)
    nat.launch(graph.device, "gnx_graph_colsum_streams", graph.handle, p, seed, first_stream, n_streams, D)
    nat.launch(graph.device, "gnx_degree_scale", D, D.numel(), nat.NORM["symmetric"], 0)
    return D


def can_fuse_dropout(graph: DeviceGraph, p) -> bool:
    return graph.n_rows == graph.n_cols and p > 0 and (graph.nnz_entries == graph.nnz or graph.entry_dropout)


def dropped_adjacency(graph: DeviceGraph, p, seed, stream_id, D=None) -> Adjacency:
    """A training iteration's adjacency: the fused form when the graph allows it (square; no duplicate COO entries, or
    enable_entry_dropout() called), else the materialised one.  ``D``: its degree scales if already known (dropped_degree_scales)."""
    if can_fuse_dropout(graph, p):
        return DroppedAdjacency(graph, p, seed, stream_id, D=D)
    return normalize(graph, "symmetric", "none", p, seed, stream_id)


def normalize(graph: DeviceGraph, normalized="symmetric", add_eye="none", dropout=0.0, seed=0, stream_id=0,
              transposed_only=False) -> Adjacency:
    """GNN.get_adjacency on the device (reference gnn.py:36-50).  ``transposed_only``: write the values in the
    order of the transposed structure only (all a backward pass needs)."""
    if normalized not in nat.NORM:
        raise Exception("Invalid matrix normalization")
    if add_eye not in nat.EYE:
        raise Exception("Invalid add_eye option")
    vals = torch.empty(graph.nnz, dtype=torch.float32, device=graph.device)
    diag = torch.empty(graph.n_rows, dtype=torch.float32, device=graph.device) if add_eye != "none" else None
    nat.launch(graph.device, "gnx_graph_normalize_t" if transposed_only else "gnx_graph_normalize", graph.handle, nat.NORM[normalized],
               nat.EYE[add_eye], dropout, seed, stream_id, vals, diag)
    adj = Adjacency(graph, None, diag, vals_t=vals) if transposed_only else Adjacency(graph, vals, diag)
    adj.transposed_only = bool(transposed_only)
    if normalized == "none" and add_eye == "none":
        adj.raw_dropout = (float(dropout), int(seed), int(stream_id))
    return adj


def _as_f32_rows(x: torch.Tensor) -> torch.Tensor:
    if x.dtype != torch.float32:
        x = x.float()
    if x.dim() != 2:
        raise Exception("propagation expects a 2-D feature matrix")
    if x.stride(1) != 1 or x.stride(0) < x.shape[1]:
        x = x.contiguous()
    return x


def _same_device(g, *tensors):
    """Raw pointers cross the C ABI: every operand must live on the graph's device."""
    for t in tensors:
        if t is not None and t.device != g.device:
            raise Exception(f"spmm: operand on {t.device}, the graph lives on {g.device}")


def _one_of(what, keyword, value, allowed):
    """Raises unless ``value`` is one of ``allowed``, the values the keyword ``keyword`` of ``what`` takes."""
    if value not in allowed:
        raise Exception(f"{what}: {keyword} must be one of " + ", ".join(repr(v) for v in allowed))


def _need_symbol(what, entry, keyword=None):
    """Raises where libgnx.so lacks ``entry``; ``keyword``: the opt-in of ``what`` that asked for it (it goes into the message)."""
    if not nat.has_symbol(entry):      # (a library without the entry raises: nothing falls back)
        asked = f"{what}:" if keyword is None else f"{what}: {keyword}=\"fused\""
        raise Exception(f"{asked} needs {entry}, which this libgnx.so does not export: rebuild the library")


def _bias_row(what, bias, width):
    """``bias`` ([width] / [1, width]) as the contiguous f32 row a launch of ``what`` reads; None stays None."""
    if bias is None:
        return None
    b = bias.to(torch.float32).reshape(-1).contiguous()
    if b.numel() != width:
        raise Exception(f"{what}: bias width mismatch")
    return b


def _row_stride(W):
    """The leading dimension of the weight matrix ``W`` (torch calls a one-row matrix contiguous whatever its row stride says)."""
    return W.stride(0) if W.shape[0] > 1 else W.shape[1]


def _mix_operand(H0, shape, bias=False):
    """(H0 as f32 rows, ldh0) of a launch whose result has ``shape``; (None, 0) without one.  ``bias``: one row serves every output
    row (ldh0 = 0)."""
    if H0 is None:
        return None, 0
    H0 = _as_f32_rows(H0)
    if bias and tuple(H0.shape) == (1, shape[1]) and shape[0] != 1:
        return H0.contiguous(), 0
    if tuple(H0.shape) != tuple(shape):
        raise Exception("spmm: H0 shape mismatch")
    return H0, H0.stride(0)


def _spmm_buffers(X, H0, rows_in, rows_out, out, new, bf16_out=False):
    """What _launch and _launch_bf16 check alike once ``X`` is in its stored format: (C, out, H0, ldh0) for ``rows_in`` gathered and
    ``rows_out`` result rows.  ``out`` None: a new tensor of dtype ``new``; else f32 rows of unit column stride -- with ``bf16_out`` f32 or
    bf16 rows whose leading dimension holds a row."""
    if X.shape[0] != rows_in:
        raise Exception(f"spmm: features have {X.shape[0]} rows, adjacency expects {rows_in}")
    C = X.shape[1]
    if out is None:
        out = torch.empty((rows_out, C), dtype=new, device=X.device)
    elif (tuple(out.shape) != (rows_out, C) or not (out.dtype == torch.float32 or (bf16_out and out.dtype == torch.bfloat16))
            or out.stride(1) != 1 or (bf16_out and out.stride(0) < C) or not out.is_cuda):
        raise Exception("spmm: bad output buffer")
    return (C, out) + _mix_operand(H0, (rows_out, C), bias=True)


def _launch(adj: Adjacency, X, H0, beta, alpha, act, transposed=False, out=None, out_rows=None):
    g = adj.graph
    nat.require_cuda(X, H0)
    _same_device(g, X, H0, out, out_rows, adj.diag)
    X = _as_f32_rows(X)
    rows_in, rows_out = (g.n_rows, g.n_cols) if transposed else (g.n_cols, g.n_rows)
    C, out, H0, ldh0 = _spmm_buffers(X, H0, rows_in, rows_out, out, torch.float32)
    if isinstance(adj, DroppedAdjacency) and out_rows is None:       # weights produced inside the kernel
        nat.launch(X.device, "gnx_spmm_dropped", g.handle, adj.D, adj.p, adj.seed, adj.stream_id, transposed, X, X.stride(0), C, H0, ldh0,
                   beta, alpha, act, out, out.stride(0))
        return out
    if transposed:
        entry, values = "gnx_spmm_tv", adj.transposed_values()
    else:
        if adj.vals is None and adj.vals_t is not None:
            raise Exception("spmm: this adjacency only holds transposed-order values")
        entry, values = "gnx_spmm", adj.vals
    if out_rows is not None:                                    # result row i -> out[out_rows[i]]
        if transposed or out_rows.dtype != torch.int32 or out_rows.numel() != rows_out or not out_rows.is_cuda:
            raise Exception("spmm: bad output row map")
        nat.launch(X.device, "gnx_spmm_scatter", g.handle, values, adj.diag, X, X.stride(0), C, H0, ldh0, beta, alpha, act, out_rows, out,
                   out.stride(0))
    else:
        nat.launch(X.device, entry, g.handle, values, adj.diag, X, X.stride(0), C, H0, ldh0, beta, alpha, act, out, out.stride(0))
    return out


def _launch_chained(adj: "DroppedAdjacency", X, H0, beta, alpha, prescaled, D_next, skip_empty=False, order=None, out_bf16=False):
    """One forward training iteration inside a loop (gnx_spmm_dropped_chained): X carries its column scale when ``prescaled``,
    the result carries ``D_next`` (the next iteration's column scale) unless that is None.  ``skip_empty``: rows without entries
    are left untouched (every iteration but the last: nobody gathers them; the library ignores it on graphs where somebody does).
    ``order`` (an OR of nat.ORD_X / nat.ORD_OUT, or None): the launch goes through gnx_spmm_dropped_chained_ord -- X stored in / the
    result written in the graph's gather order; same bits.
    A bf16 X: the gathered rows are stored as bf16 (gnx_spmm_dropped_chained_bf16); f32 H0; the result is f32, or bf16 (rounded once,
    after the D_next scale) with ``out_bf16``.  There is no gather-order entry for bf16 rows."""
    g = adj.graph
    bf16 = X.dtype == torch.bfloat16
    nat.require_cuda(X, H0)
    _same_device(g, X, H0, adj.D, D_next)
    C = X.shape[1]
    if (X.dtype not in (torch.float32, torch.bfloat16) or H0.dtype != torch.float32 or X.shape[0] != g.n_cols
            or tuple(H0.shape) != (g.n_rows, C) or not X.is_contiguous() or not H0.is_contiguous() or (out_bf16 and not bf16)):
        raise Exception("chained bf16 propagation: bad operands" if bf16 else "chained propagation: bad operand shapes")
    if bf16 and order is not None:
        raise Exception("chained bf16 propagation: bf16 rows have no gather-order entry")
    out = torch.empty((g.n_rows, C), dtype=torch.bfloat16 if out_bf16 else torch.float32, device=X.device)
    if bf16:
        entry, tail = "gnx_spmm_dropped_chained_bf16", (out_bf16, out.stride(0))
    elif order is not None:
        entry, tail = "gnx_spmm_dropped_chained_ord", (out.stride(0), order)
    else:
        entry, tail = "gnx_spmm_dropped_chained", (out.stride(0),)
    nat.launch(X.device, entry, g.handle, adj.D, adj.p, adj.seed, adj.stream_id, prescaled, D_next, X, X.stride(0), C, H0, H0.stride(0), beta,
               alpha, nat.ACT_NONE | (nat.ACT_SKIP_EMPTY if skip_empty else 0), out, *tail)
    return out


def _launch_back(adj: "DroppedAdjacency", X, prescaled, D_next, S_in, s_alpha, s_beta, S_out, y_beta, Y_out, skip_empty=False, order=None):
    """One backward training iteration inside a loop (gnx_spmm_dropped_back): acc = A_k^T X over the transposed structure, weights
    made in the kernel; S_out = s_beta acc + s_alpha S_in (S_in may be S_out), Y_out = y_beta acc * D_next (skipped when None).
    ``order`` (an OR of nat.ORD_X / nat.ORD_OUT, or None): through gnx_spmm_dropped_back_ord -- X stored in / Y_out written in the
    graph's gather order, the running sum in the caller's; same bits.
    A bf16 X: the gathered rows and the pre-scaled result Y_out are stored as bf16 (gnx_spmm_dropped_back_bf16); the running sum
    S_in / S_out is f32.  There is no gather-order entry for bf16 rows."""
    g = adj.graph
    bf16 = X.dtype == torch.bfloat16
    nat.require_cuda(X, S_in, S_out)
    _same_device(g, X, S_in, S_out, Y_out, adj.D, D_next)
    C = X.shape[1]
    rows = torch.bfloat16 if bf16 else torch.float32
    if any(t is not None and (tuple(t.shape) != (g.n_rows, C) or not t.is_contiguous() or t.dtype != dt)
           for t, dt in ((X, rows), (S_in, torch.float32), (S_out, torch.float32), (Y_out, rows))):
        raise Exception("chained bf16 backward: bad operands" if bf16 else "chained backward: bad operand shapes")
    if bf16 and order is not None:
        raise Exception("chained bf16 backward: bf16 rows have no gather-order entry")
    entry = "gnx_spmm_dropped_back_bf16" if bf16 else "gnx_spmm_dropped_back_ord" if order is not None else "gnx_spmm_dropped_back"
    tail = () if order is None else (order,)
    nat.launch(X.device, entry, g.handle, adj.D, adj.p, adj.seed, adj.stream_id, prescaled, D_next, X, C, C, S_in, C, s_alpha, s_beta, S_out, C,
               y_beta, Y_out, C, nat.ACT_SKIP_EMPTY if skip_empty else nat.ACT_NONE, *tail)


_launch_chained_bf16 = _launch_chained     # (the dtype of X picks the entry)
_launch_back_bf16 = _launch_back


def _forward_chained(adjs, H0, a, relabelled=False, bf16=False):
    """H_K of K >= 1 chained training iterations from f32 H0 ([n, C] contiguous), one gnx_spmm_dropped_chained each: the next
    iteration's column scale rides out with the rows, so from k = 1 on no per-entry scale gather is left.  ``relabelled``: the iterate
    is handed from launch to launch in the graph's gather order (gnx_spmm_dropped_chained_ord: H0 enters and H_K leaves in the caller's);
    same bits.  ``bf16``: the iterate is stored as bf16 between launches: X_0 = bf(H0); iteration k gathers X_k and writes
    bf(H_{k+1} * D_{k+1}), the last one f32 H_K."""
    K = len(adjs)
    X = to_bf16(H0) if bf16 else H0
    for k, adj in enumerate(adjs):
        last = k == K - 1
        order = ((nat.ORD_X if k > 0 else 0) | (0 if last else nat.ORD_OUT)) if relabelled else None
        # (rows without entries are a * H0 in the result and gathered by nobody: only the last iteration writes them)
        X = _launch_chained(adj, X, H0, 1.0 - a, a, prescaled=k > 0, D_next=None if last else adjs[k + 1].D, skip_empty=not last,
                            order=order, out_bf16=bf16 and not last)
    return X


def _backward_chained(adjs, g, a, relabelled=False, bf16=False):
    """dH0 of K chained training iterations for the upstream gradient ``g``: g_k = (1-a) A_k^T g_{k+1}, dH0 = g_0 + a (g_1 + ... +
    g_K), as K calls of gnx_spmm_dropped_back -- every call adds its g_k to the running sum in its epilogue and hands the next call
    its operand pre-scaled by that call's column scale, so no gradient of an iteration is kept, no per-entry scale is gathered
    and no separate summation pass exists.  ``relabelled`` (K > 1): the operand handed from call to call lives in the graph's gather
    order (gnx_spmm_dropped_back_ord: the first call gathers ``g`` as it is, the running sum stays in the caller's order); same bits.
    ``bf16``: the gathered gradient is stored as bf16: the first call gathers bf(g), every later one the bf((1-a) acc * D) its
    predecessor wrote; the running sum starts from f32 g and only ever adds f32 sums."""
    K = len(adjs)
    g = _as_f32_rows(g).contiguous()
    S = torch.empty_like(g)
    X = to_bf16(g) if bf16 else g
    for k in range(K - 1, -1, -1):
        first, last = k == K - 1, k == 0
        Y = None if last else torch.empty_like(X)
        order = ((0 if first else nat.ORD_X) | (0 if last else nat.ORD_OUT)) if relabelled else None
        # rows without entries: their g_k is 0 -- after the first call their sum is final and their Y row is never gathered
        _launch_back(adjs[k], X, not first, None if last else adjs[k - 1].D, g if first else S, a if first else 1.0,
                     (1.0 - a) if last else a * (1.0 - a), S, 1.0 - a, Y, skip_empty=not first, order=order)
        X = Y
    return S


def _forward_chained_bf16(adjs, H0, a):
    """_forward_chained with the iterate stored as bf16 between launches."""
    return _forward_chained(adjs, H0, a, bf16=True)


def _backward_chained_bf16(adjs, g, a):
    """_backward_chained with the gathered gradient stored as bf16."""
    return _backward_chained(adjs, g, a, bf16=True)


def _launch_rows(bf16, adj: Adjacency, X, H0, beta, alpha, rows, out, act):
    """gnx_spmm_rows over f32 rows ``X`` (anything else is widened) into an f32 ``out``, or with ``bf16`` gnx_spmm_rows_bf16 over bf16
    rows into an f32 or bf16 ``out`` of a leading dimension that holds a row: the checks and the call."""
    g = adj.graph
    nat.require_cuda(X, H0, rows, out)
    _same_device(g, X, H0, rows, out)
    if not bf16:
        X = _as_f32_rows(X)
    elif X.dim() != 2 or X.dtype != torch.bfloat16 or X.stride(1) != 1 or X.stride(0) < X.shape[1]:
        raise Exception("spmm: the bf16 row launch takes a bf16 feature matrix with unit column stride")
    if X.shape[0] != g.n_cols:
        raise Exception(f"spmm: features have {X.shape[0]} rows, adjacency expects {g.n_cols}")
    C = X.shape[1]
    if rows.dtype != torch.int32 or rows.numel() != g.n_rows or not rows.is_contiguous():
        raise Exception("spmm: bad row map")
    if (out.dtype not in ((torch.float32, torch.bfloat16) if bf16 else (torch.float32,)) or out.dim() != 2 or out.shape[1] != C
            or out.stride(1) != 1 or (bf16 and out.stride(0) < C)):
        raise Exception("spmm: bad output buffer")
    H0, ldh0 = _mix_operand(H0, out.shape)
    layer = (g.handle, adj.vals, X, X.stride(0), C, H0, ldh0, beta, alpha, act, rows, out)
    if bf16:
        nat.launch(X.device, "gnx_spmm_rows_bf16", *layer, out.dtype == torch.bfloat16, out.stride(0))
    else:
        nat.launch(X.device, "gnx_spmm_rows", *layer, out.stride(0))
    return out


def launch_rows(adj: Adjacency, X, H0, beta, alpha, rows, out, act=nat.ACT_NONE):
    """The fused step over a graph that holds a SUBSET of the output rows (the interior or the boundary rows of
    a vertex block): result row r is written to out[rows[r]] and mixes in H0[rows[r]] (gnx_spmm_rows)."""
    return _launch_rows(False, adj, X, H0, beta, alpha, rows, out, act)


def launch_rows_bf16(adj: Adjacency, X, H0, beta, alpha, rows, out, act=nat.ACT_NONE):
    """launch_rows with the gathered rows X stored as bf16 (gnx_spmm_rows_bf16): result row r is written to out[rows[r]] -- f32, or
    rounded once when ``out`` is bf16 -- and mixes in the f32 H0[rows[r]]."""
    return _launch_rows(True, adj, X, H0, beta, alpha, rows, out, act)


class _SpMM(torch.autograd.Function):
    """out = A . X ; backward dX = A^T . g (what tf.GradientTape derives for filter.py:19)."""

    @staticmethod
    def forward(ctx, X, adj):
        ctx.adj = adj
        return _launch(adj, X, None, 1.0, 0.0, nat.ACT_NONE)

    @staticmethod
    def backward(ctx, g):
        return _launch(ctx.adj, g.contiguous(), None, 1.0, 0.0, nat.ACT_NONE, transposed=True), None


class _PPRStep(torch.autograd.Function):
    """out = (A . H)*(1-a) + H0*a in one kernel (filter.py:19-21);
    backward dH = (1-a) A^T g, dH0 = a g."""

    @staticmethod
    def forward(ctx, H, H0, adj, a):
        ctx.adj, ctx.a = adj, a
        return _launch(adj, H, H0, 1.0 - a, a, nat.ACT_NONE)

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        gH = _launch(ctx.adj, g, None, 1.0 - ctx.a, 0.0, nat.ACT_NONE, transposed=True) if ctx.needs_input_grad[0] else None
        gH0 = g * ctx.a if ctx.needs_input_grad[1] else None
        return gH, gH0, None, None


PAD_WIDTHS = True      # tools flip this for A/B runs


PAD_MIN_ROWS = 1 << 16      # smaller graphs are launch-bound: the pad / slice launches would cost more than the loads save


def lines_per_row(C: int, elem_bytes: int = 4) -> float:
    """Average number of 128-byte lines a row of C floats (``elem_bytes`` = 2: bf16) touches when rows are stored back to back (row r
    starts at byte elem_bytes C r)."""
    size = elem_bytes * C
    step = math.gcd(size, 128)
    offsets = range(0, 128, step)
    return sum((off + size + 127) // 128 for off in offsets) / len(offsets)


def friendly_width(C: int, n_rows: int = PAD_MIN_ROWS) -> int:
    """The row width (floats) the K-iteration loops run at.  A gather moves whole 128-byte lines and the kernels load 16 bytes
    per lane when rows are 16-byte aligned: rows of 7 ... 31 floats are padded to the next power of two (a row then never
    straddles a line it does not fill: C = 9 ... 15 run 26 % faster as 16, 20 ... 24 as 32), wider ones to the next multiple of
    4 (C = 41 or 47 -- odd class counts -- would otherwise fall back to 4-byte loads) -- and on to the first multiple of 4 up to
    the next multiple of 32 at which a row touches no more lines than its size needs (round 6: C = 56, 224-byte rows, half of which
    span three lines: 4.50 ms per iteration on the config-4 graph against 3.75 as 64; 44 -> 48, 52 / 56 / 60 -> 64; 40 and 48
    stay, their rows never span a third line).  The pad columns are zero and stay zero."""
    if not PAD_WIDTHS or C <= 6 or n_rows < PAD_MIN_ROWS:     # up to 6 floats the pad / un-pad copies cost what the wider loads save
        return C
    if C <= 32:
        return 1 << (C - 1).bit_length()
    Cp = (C + 3) // 4 * 4
    best = Cp
    for wider in range(Cp + 4, (Cp + 31) // 32 * 32 + 1, 4):
        if lines_per_row(wider) < lines_per_row(best) - 1e-9:
            best = wider
    return best


def friendly_width_bf16(C: int, n_rows: int = PAD_MIN_ROWS) -> int:
    """friendly_width for bf16 rows (2-byte elements, 8 per 16-byte lane load): rows of 7 ... 63 elements are padded to the next
    power of two (C = 40: 80-byte rows, half of which span two lines, become one 128-byte line), wider ones to the next multiple of
    8 and on to the first multiple of 8 up to the next multiple of 64 at which a row touches no more lines than its size needs.
    The pad columns are zero and stay zero."""
    if not PAD_WIDTHS or C <= 6 or n_rows < PAD_MIN_ROWS:
        return C
    if C <= 64:
        return 1 << (C - 1).bit_length()
    Cp = (C + 7) // 8 * 8
    best = Cp
    for wider in range(Cp + 8, (Cp + 63) // 64 * 64 + 1, 8):
        if lines_per_row(wider, 2) < lines_per_row(best, 2) - 1e-9:
            best = wider
    return best


def _padded(H: torch.Tensor, Cp: int) -> torch.Tensor:
    if H.shape[1] == Cp:
        return H
    out = torch.zeros((H.shape[0], Cp), dtype=torch.float32, device=H.device)
    out[:, :H.shape[1]] = H
    return out


def _unpadded(H: torch.Tensor, C: int) -> torch.Tensor:
    return H if H.shape[1] == C else H[:, :C].contiguous()


def _one_fused_graph(adjs) -> bool:
    """Every iteration's adjacency makes its weights in the kernels, over one graph: what the chained loops need."""
    return all(isinstance(adj, DroppedAdjacency) and adj.graph is adjs[0].graph for adj in adjs)


class _PPRLoop(torch.autograd.Function):
    """K PPRIteration steps as ONE autograd node.  The step is linear in H, so the backward needs no
    stored activations: g_k = (1-a) A_k^T g_{k+1}, dH0 = g_0 + a * sum_k g_{k+1}.  In training mode
    every iteration has its own dropped + re-normalised adjacency A_k (filter.py:18 calls get_adjacency
    each time); the counter RNG lets the backward REGENERATE A_k from (seed, stream id) instead of
    keeping K value arrays alive.
    ``relu`` (the reference's per-iteration activation, filter.py:22): H_k = relu(Z_k) in every launch's epilogue; the backward then
    needs the sign of every Z_k, so the K outputs ARE kept (what the layer-by-layer form keeps anyway) and every gradient is
    masked by H_k > 0 before it goes through A_k^T: gz_k = g_k * (H_k > 0), g_{k-1} = (1-a) A_k^T gz_k, dH0 = g_0 + a sum_k gz_k."""

    @staticmethod
    def forward(ctx, H0, make_adj, a, K, relu=False, storage=torch.float32, gather_order="caller"):
        ctx.make_adj, ctx.a, ctx.K, ctx.relu = make_adj, a, K, relu
        act = nat.ACT_RELU if relu else nat.ACT_NONE
        H0 = _as_f32_rows(H0).contiguous()
        ctx.C = C = H0.shape[1]
        n = H0.shape[0]
        first = make_adj(0, False) if K > 0 else None
        adjs = None                     # the K adjacencies once a chained loop asked for them: make_adj is called once per iteration
        # which loop runs, decided once (the backward reads it): "bf16" / "caller" / "relabelled" = the chained loops, "layers" = one
        # launch per iteration through _launch
        ctx.loop = "layers"
        if _bf16(storage) and _bf16_training_applies(first, K, relu, C):
            # opt-in bf16 storage of the gathered operand (gnx_spmm_dropped_chained_bf16 / _back_bf16): the chained loop, on graphs
            # with duplicate entries too (there is no materialised bf16 form whose bits it would have to keep)
            adjs = [first] + [make_adj(k, False) for k in range(1, K)]
            if _one_fused_graph(adjs):
                ctx.loop = "bf16"
        if ctx.loop == "layers" and K > 1 and isinstance(first, DroppedAdjacency) and not relu and first.graph.nnz_entries == first.graph.nnz:
            # weights made in the kernels (only the K degree-scale vectors exist): the next iteration's column scale rides out with
            # the rows, so from k = 1 on no per-entry scale gather is left (gnx_spmm_dropped_chained).  Not on graphs with duplicate
            # entries: their fused form replaces the materialised one, whose results it keeps bit for bit (one gnx_spmm_dropped per
            # iteration, below), where the chained loop would round differently
            adjs = adjs if adjs is not None else [first] + [make_adj(k, False) for k in range(1, K)]
            if _one_fused_graph(adjs) and first.graph.n_rows == first.graph.n_cols:
                # the iterate handed from launch to launch in the graph's gather order (gnx_spmm_dropped_chained_ord): the same bits
                ctx.loop = "relabelled" if _train_gather_applies(gather_order, first.graph, friendly_width(C, n)) else "caller"
        if ctx.loop == "bf16":
            return _unpadded(_forward_chained_bf16(adjs, _padded(H0, friendly_width_bf16(C, n)), a), C)
        H0 = _padded(H0, friendly_width(C, n))
        if ctx.loop != "layers":
            return _unpadded(_forward_chained(adjs, H0, a, relabelled=ctx.loop == "relabelled"), C)
        H = H0
        kept = []
        for k in range(K):               # one adjacency alive at a time (a materialised one is an nnz-sized array)
            H = _launch(first if k == 0 else adjs[k] if adjs is not None else make_adj(k, False), H, H0, 1.0 - a, a, act)
            if relu:
                kept.append(H)
        if relu:
            ctx.save_for_backward(*kept)
        return _unpadded(H, C)

    @staticmethod
    def backward(ctx, g):
        gH0 = None
        if ctx.loop != "layers":
            adjs = [ctx.make_adj(k, True) for k in range(ctx.K)]
            fused = all(isinstance(adj, DroppedAdjacency) for adj in adjs)
            if ctx.loop == "bf16":
                if not fused:
                    raise Exception("ppr_loop: the bf16 forward ran on fused adjacencies, the backward was handed others")
                gH0 = _backward_chained_bf16(adjs, _padded(_as_f32_rows(g).contiguous(), friendly_width_bf16(ctx.C, g.shape[0])), ctx.a)
            elif fused:
                gH0 = _backward_chained(adjs, _padded(g.contiguous(), friendly_width(ctx.C, g.shape[0])), ctx.a,
                                        relabelled=ctx.loop == "relabelled")
        if gH0 is None:
            gH0 = _PPRLoop._backward_layers(ctx, _padded(g.contiguous(), friendly_width(ctx.C, g.shape[0])))
        return _unpadded(gH0, ctx.C), None, None, None, None, None, None

    @staticmethod
    def _backward_layers(ctx, g):
        # dH0 = g_0 + a (g_1 + ... + g_K): the gradients of the iterations are KEPT (as many as a tenth of the card's memory
        # holds, at most 15) and added up by one pass (gnx_linear_combination) instead of a read-modify-write of dH0 per iteration
        outs = ctx.saved_tensors if ctx.relu else None
        room = int(0.1 * torch.cuda.get_device_properties(g.device).total_memory) // max(g.numel() * 4, 1)
        limit = max(2, min(LINCOMB_TERMS - 1, room))
        pending, total = [], None
        for k in range(ctx.K - 1, -1, -1):
            if outs is not None:
                g = _relu_mask(g, outs[k])
            pending.append((g, ctx.a))
            if len(pending) >= limit:
                total, pending = linear_combination(([(total, 1.0)] if total is not None else []) + pending), []
            g = _launch(ctx.make_adj(k, True), g, None, 1.0 - ctx.a, 0.0, nat.ACT_NONE, transposed=True)
        pending.append((g, 1.0))
        return linear_combination(([(total, 1.0)] if total is not None else []) + pending)


LINCOMB_TERMS = 16


def linear_combination(terms) -> torch.Tensor:
    """sum_j coef_j * tensor_j for up to 16 equally shaped float32 device tensors, ``terms`` = [(tensor, coef), ...], in ONE pass
    (gnx_linear_combination; terms are added in list order).  Returns a new tensor."""
    if not 1 <= len(terms) <= LINCOMB_TERMS:
        raise Exception("linear_combination: 1 to %d terms" % LINCOMB_TERMS)
    # the kernel reads 16 bytes per lane: a contiguous VIEW with a storage offset (a row or column slice of a padded buffer)
    # need not be 16-byte aligned -- such a term is copied to a fresh allocation first
    tensors = [t if t.is_contiguous() and t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.contiguous_format) for t, _ in terms]
    first = tensors[0]
    nat.require_cuda(*tensors)
    for t in tensors:
        if t.shape != first.shape or t.dtype != torch.float32 or t.device != first.device:
            raise Exception("linear_combination: the terms must be float32 tensors of one shape on one device")
    out = torch.empty_like(first)
    k = len(tensors)
    ptrs = (c_void_p * k)(*[t.data_ptr() for t in tensors])
    coefs = (c_float * k)(*[float(c) for _, c in terms])
    nat.launch(first.device, "gnx_linear_combination", k, ptrs, coefs, first.numel(), out)
    return out


GATHER_ORDERS = ("caller", "relabelled", "auto")

# Training (ppr_loop gather_order="auto"): the allowance of the relabelled operand order, set from tools/train_gather_bench.py
# (profiles/NOTES.md "Gather order of the training loops"): a launch width (the padded row width the loop runs at) / graph size gets
# the relabelled order only where its K = 10 step measured faster than the caller-order step of the same run by more than the spread
# of the two medians (its upper quartile below the caller step's lower quartile).  Measured (R-MAT, 10 entries per vertex, C = 7, 8,
# 16, 32, 40, 64): NO width gains -- at 10^7 vertices the relabelled step is 4-14 % slower (C = 7 33.9 -> 37.3 ms, C = 32 35.6 ->
# 41.5, C = 64 55.8 -> 59.0), at 10^6 vertices 1-6 % slower: the scattered result write and the second index stream cost more than
# the shared hub lines save.  The allowance is therefore EMPTY (maximum width 0) and "auto" is "caller"; "relabelled" stays
# available explicitly (bitwise equal results)
TRAIN_GATHER_MAX_WIDTH = 0
TRAIN_GATHER_MIN_ROWS = 1_000_000


def _gather_order(gather_order) -> str:
    if gather_order not in GATHER_ORDERS:
        raise Exception(f"gather_order must be one of {GATHER_ORDERS}, not {gather_order!r}")
    return gather_order


def resolve_gather_order(gather_order, n_rows, width) -> str:
    """"caller" or "relabelled": what ``gather_order`` means for a graph of ``n_rows`` vertices at a launch width of ``width``
    floats -- "auto" takes the relabelled order only inside the measured allowance (TRAIN_GATHER_MAX_WIDTH / TRAIN_GATHER_MIN_ROWS)."""
    if _gather_order(gather_order) != "auto":
        return gather_order
    return "relabelled" if width <= TRAIN_GATHER_MAX_WIDTH and n_rows >= TRAIN_GATHER_MIN_ROWS else "caller"


def _train_gather_applies(gather_order, graph, width) -> bool:
    """Whether the chained f32 loop over ``graph`` hands its iterate on in the graph's gather order: asked for (or allowed) and the
    handle can have one (no row window: a numbering that carries locality keeps it)."""
    return resolve_gather_order(gather_order, graph.n_rows, width) == "relabelled" and not getattr(graph, "row_window", 0)


def may_use_train_gather(graph, gather_order) -> bool:
    """Whether a training loop over ``graph`` under ``gather_order`` can take the relabelled operand order at SOME width (what a
    captured training step reserves for: DeviceGraph.reserve(train_gather=True))."""
    if _gather_order(gather_order) == "caller" or graph.n_rows != graph.n_cols or graph.nnz_entries != graph.nnz \
            or getattr(graph, "row_window", 0):
        return False
    return gather_order == "relabelled" or (TRAIN_GATHER_MAX_WIDTH > 0 and graph.n_rows >= TRAIN_GATHER_MIN_ROWS)


def ppr_loop(make_adj, H0: torch.Tensor, a: float, iterations: int, relu: bool = False, storage=torch.float32,
             gather_order="caller") -> torch.Tensor:
    """``iterations`` fused PPR steps starting from H0; ``make_adj(k, for_backward)`` returns the Adjacency
    of iteration k (called again, with the same k and for_backward=True, during the backward, where only the
    transposed-order values are needed).  ``relu``: relu after every step (filter.py:22).
    ``storage=torch.bfloat16`` (opt-in): where every iteration's adjacency is a DroppedAdjacency of one square graph (training with
    edge dropout, weights made in the kernels) the rows the loop GATHERS are stored as bf16, forward and backward
    (gnx_spmm_dropped_chained_bf16 / gnx_spmm_dropped_back_bf16): X_0 = bf(H0), every later iterate leaves its launch as
    bf(H_{k+1} * D_{k+1}) -- one rounding, after the next iteration's column scale -- and the last iteration writes f32 H_K; the
    backward gathers bf(g), then bf((1-a) acc * D_{k-1}), while dH0 is summed in f32 from unrounded addends.  Masks, degree scales,
    weights, sums, H0 and the mix stay f32; two runs give the same bits.  bf16 is an allowance: the loop keeps f32 -- bit for bit
    the default -- with ``relu``, with any other adjacency, at K = 0, below BF16_TRAIN_MIN_WIDTH columns and on graphs of fewer than
    BF16_TRAIN_MIN_ROWS vertices (launch-bound steps, where bf16 measured slower).
    ``gather_order``: where the chained f32 loop applies (K > 1, every adjacency a DroppedAdjacency of one square graph without
    duplicate entries, no relu, f32 storage), ``"relabelled"`` keeps the iterate -- and, in the backward, the gradient handed from
    call to call -- in the graph's gather order between the launches (gnx_spmm_dropped_chained_ord / gnx_spmm_dropped_back_ord: hub
    rows share 128-byte lines): rows, entry order, masks, weights and sums stay the caller's, H0 enters and H_K / dH0 leave in the
    caller's order, and the result is bit for bit that of ``"caller"`` (today's path, the default here).  Everywhere else
    ``"relabelled"`` takes today's path.  ``"auto"`` takes the relabelled order inside the measured allowance only
    (TRAIN_GATHER_MAX_WIDTH, TRAIN_GATHER_MIN_ROWS)."""
    _bf16(storage)
    return _PPRLoop.apply(H0, make_adj, float(a), int(iterations), bool(relu), storage, _gather_order(gather_order))


class _SpMMBiasAct(torch.autograd.Function):
    """out = act(A . Y + bias) in one kernel (bias broadcast through the H0 operand, relu in the epilogue);
    backward: g' = g * (out > 0), dY = A^T g', dbias = column sums of g'."""

    @staticmethod
    def forward(ctx, Y, bias, adj, relu):
        out = _launch(adj, Y, bias, 1.0, 1.0, nat.ACT_RELU if relu else nat.ACT_NONE)
        ctx.adj, ctx.relu, ctx.has_bias = adj, relu, bias is not None
        ctx.save_for_backward(out if relu else None)
        return out

    @staticmethod
    def backward(ctx, g):
        (out,) = ctx.saved_tensors
        g = _relu_mask(g, out) if ctx.relu else g
        g = g.contiguous()
        gY = _launch(ctx.adj, g, None, 1.0, 0.0, nat.ACT_NONE, transposed=True) if ctx.needs_input_grad[0] else None
        gb = g.sum(dim=0, keepdim=True) if ctx.has_bias and ctx.needs_input_grad[1] else None
        return gY, gb, None, None


def spmm_bias_act(adj: Adjacency, Y: torch.Tensor, bias=None, relu=False, storage=torch.float32) -> torch.Tensor:
    """act(A . Y + bias) fused; ``bias`` is [1, C] or None.  ``storage=torch.bfloat16``: Y gathered as bf16 (inference only; the
    error bound of ``spmm``)."""
    if _bf16(storage):
        _no_grad_for_bf16("spmm_bias_act", Y, bias)
        return _launch_bf16(adj, Y, bias, 1.0, 1.0, nat.ACT_RELU if relu else nat.ACT_NONE)
    return _SpMMBiasAct.apply(Y, bias, adj, bool(relu))


def spmm(adj: Adjacency, X: torch.Tensor, storage=torch.float32) -> torch.Tensor:
    """Drop-in for tf.sparse.sparse_dense_matmul(adj, X); differentiable w.r.t. X.
    ``storage=torch.bfloat16`` (inference only: raises where autograd would need a gradient): X is gathered as bf16 -- a bf16 X as
    it is, an f32 X rounded once (gnx_cast_bf16) -- and summed in f32 (gnx_spmm_bf16); the f32 result is the exact sum over the
    rounded rows, i.e. |out - A.X| <= u |A| |X| elementwise (u = 2^-8) plus f32 rounding.  The default keeps the f32 path (a bf16
    X is widened to f32 there)."""
    if _bf16(storage):
        _no_grad_for_bf16("spmm", X)
        return _launch_bf16(adj, X, None, 1.0, 0.0, nat.ACT_NONE)
    return _SpMM.apply(X, adj)


def ppr_step(adj: Adjacency, H: torch.Tensor, H0: torch.Tensor, a) -> torch.Tensor:
    """One fused PPRIteration step.  ``a`` may be a float (fused kernel) or a tensor
    (a trainable teleport probability: un-fused so autograd reaches it)."""
    if isinstance(a, torch.Tensor):
        return spmm(adj, H) * (1 - a) + H0 * a
    return _PPRStep.apply(H, H0, adj, float(a))


def appnp_propagate(adj: Adjacency, H0: torch.Tensor, a: float = 0.1, iterations: int = 10, relu: bool = False,
                    storage=torch.float32) -> torch.Tensor:
    """The eval-mode K-iteration loop as ONE library call with two ping-pong buffers
    (no autograd, no per-layer .value caching) -- the measured hot path.  ``relu``: the reference's per-iteration activation
    (filter.py:22,28,35) in every iteration's epilogue (gnx_appnp_propagate_act).
    ``storage=torch.bfloat16``: the iterate is kept as bf16 between iterations (gnx_appnp_propagate_bf16): every gather moves half
    the bytes; sums, H0 and the mix stay f32 and the result is f32.  Error bound (u = 2^-8, symmetric normalisation of a
    symmetric pattern, no diagonal): per column ||H_bf16 - H_f32||_2 <= (u / a) max_k ||H_k||_2 to first order.  bf16 is an
    allowance: the library may keep f32 where bf16 does not pay (narrow widths on large graphs: BF16_MIN_WIDTH); the bound holds
    either way."""
    g = adj.graph
    nat.require_cuda(H0)
    H0 = _as_f32_rows(H0).contiguous()
    if g.n_rows != g.n_cols or H0.shape[0] != g.n_rows:
        raise Exception("appnp_propagate: needs a square graph matching H0")
    return _appnp_launch(_bf16(storage) and not (H0.shape[1] < BF16_MIN_WIDTH and g.n_rows >= BF16_F32_ROWS), adj, H0, a, iterations, relu)


def _appnp_launch(bf16, adj: Adjacency, H0, a, iterations, relu):
    """gnx_appnp_propagate_act, or with ``bf16`` gnx_appnp_propagate_bf16 (H0: f32 contiguous [n, C]), at the line-friendly width of the
    stored rows: the padding, the result, the ping-pong buffers (one f32 from two iterations on; two bf16 iterates) and the call."""
    C = H0.shape[1]
    H0 = _padded(H0, (friendly_width_bf16 if bf16 else friendly_width)(C, H0.shape[0]))
    out = torch.empty_like(H0)
    if bf16:
        work = torch.empty((2,) + tuple(H0.shape), dtype=torch.bfloat16, device=H0.device) if iterations > 0 else None
    else:
        work = torch.empty_like(H0) if iterations > 1 else None
    nat.launch(H0.device, "gnx_appnp_propagate_bf16" if bf16 else "gnx_appnp_propagate_act", adj.graph.handle, adj.vals, adj.diag, H0, a,
               iterations, H0.shape[1], nat.ACT_RELU if relu else nat.ACT_NONE, out, work)
    return _unpadded(out, C)


# ---- opt-in bf16 feature storage (inference only) ----------------------------------------------------------------------------
# bf16 is an allowance: appnp_propagate keeps f32 below BF16_MIN_WIDTH on graphs of at least BF16_F32_ROWS vertices -- there every
# gather is one 128-byte line whatever the element size and the f32 loop runs on the degree-relabelled copy (gnx_appnp_propagate),
# which the bf16 loop does not have (profiles/NOTES.md, bf16 storage)
BF16_MIN_WIDTH = 17
BF16_F32_ROWS = 1 << 20


# Training (ppr_loop storage=bf16): the allowance, set from tools/bf16_train_bench.py (profiles/NOTES.md "bf16 training storage"): a
# width / graph size gets bf16 only where its K = 10 step measured faster than the f32 step of the same run by more than the spread
# of the two medians.  Width: on the config-4 graph C = 33 ... 128 gain 1.18 - 1.53 x, C <= 16 lose 2 - 4 %, C = 17 ... 32 are a wash
# (up to 32 columns a gathered row is one 128-byte line in either format).  Rows: at 10^6 vertices C = 33 ... 128 gain 1.10 - 1.27 x,
# at 40 000 and at 2 708 vertices (launch-bound steps of under 1.5 ms) bf16 LOSES 1.2 - 1.9 x; nothing between was measured, so
# the smallest size that measured a gain is the threshold.  Outside the allowance the loop keeps f32
BF16_TRAIN_MIN_WIDTH = 33
BF16_TRAIN_MIN_ROWS = 1_000_000


def _bf16_training_applies(first, K, relu, C) -> bool:
    """Whether ppr_loop(storage=bf16) runs its bf16 loops: the chained fused form applies and width and graph size are inside the
    allowance."""
    return (K > 0 and not relu and isinstance(first, DroppedAdjacency) and first.graph.n_rows == first.graph.n_cols
            and C >= BF16_TRAIN_MIN_WIDTH and first.graph.n_rows >= BF16_TRAIN_MIN_ROWS)


def _bf16(storage) -> bool:
    if storage is torch.bfloat16:
        return True
    if storage is torch.float32:
        return False
    raise Exception(f"storage must be torch.float32 or torch.bfloat16, not {storage}")


def _no_grad_for_bf16(fn, *tensors):
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
        raise Exception(f"{fn}: bf16 storage is inference only (no backward); run it under torch.no_grad() or detach the inputs")


def to_bf16(X: torch.Tensor) -> torch.Tensor:
    """bf(X) on the device (gnx_cast_bf16: round to nearest even, NaN stays NaN), [n, C] contiguous bf16."""
    nat.require_cuda(X)
    X = _as_f32_rows(X)
    return _cast_bf16(X, torch.empty(X.shape, dtype=torch.bfloat16, device=X.device))


def _cast_bf16(X, dst):
    """The call of gnx_cast_bf16: f32 rows ``X`` into the bf16 rows ``dst`` of the same shape."""
    nat.launch(X.device, "gnx_cast_bf16", X, X.shape[0], X.shape[1], X.stride(0), dst, dst.stride(0))
    return dst


def _launch_bf16(adj: Adjacency, X, H0, beta, alpha, act, out_bf16=False, out=None):
    """_launch with X gathered as bf16 (gnx_spmm_bf16): f32 result, or bf16 with ``out_bf16``.  ``out``: the destination (f32 or
    bf16 rows, any leading dimension; its dtype decides the rounding)."""
    g = adj.graph
    nat.require_cuda(X, H0)
    _same_device(g, X, H0, adj.diag, out)
    if X.dim() != 2:
        raise Exception("propagation expects a 2-D feature matrix")
    if X.dtype == torch.bfloat16:
        Xb = X if X.stride(1) == 1 and X.stride(0) >= X.shape[1] else X.contiguous()
    else:
        Xb = to_bf16(X)
    if adj.vals is None and adj.vals_t is not None and Xb.shape[0] == g.n_cols:
        raise Exception("spmm: this adjacency only holds transposed-order values")
    C, out, H0, ldh0 = _spmm_buffers(Xb, H0, g.n_cols, g.n_rows, out, torch.bfloat16 if out_bf16 else torch.float32, bf16_out=True)
    nat.launch(Xb.device, "gnx_spmm_bf16", g.handle, adj.vals, adj.diag, Xb, Xb.stride(0), C, H0, ldh0, beta, alpha, act, out,
               out.dtype == torch.bfloat16, out.stride(0))
    return out


def cast_bf16_into(X: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
    """dst = bf(X) (gnx_cast_bf16) for a destination that exists already: f32 rows and bf16 rows of the same shape, any leading
    dimensions (a column range of a wider matrix into the local rows of a vertex block's buffer)."""
    nat.require_cuda(X, dst)
    X = _as_f32_rows(X)
    if dst.dtype != torch.bfloat16 or tuple(dst.shape) != tuple(X.shape) or dst.stride(1) != 1 or dst.stride(0) < dst.shape[1] or dst.device != X.device:
        raise Exception("cast_bf16_into: bad destination")
    return _cast_bf16(X, dst) if X.shape[0] and X.shape[1] else dst


def _appnp_propagate_bf16(adj: Adjacency, H0: torch.Tensor, a, iterations, relu):
    """appnp_propagate on gnx_appnp_propagate_bf16 (H0: f32 contiguous [n, C]) at every width: no f32 allowance."""
    return _appnp_launch(True, adj, H0, a, iterations, relu)


def gather_rows(X: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """out[r] = X[idx[r]] through the library's halo-packing kernel."""
    nat.require_cuda(X, idx)
    X = _as_f32_rows(X)
    idx = idx.to(torch.int64).contiguous()
    out = torch.empty((idx.numel(), X.shape[1]), dtype=torch.float32, device=X.device)
    nat.launch(X.device, "gnx_gather_rows", X, X.stride(0), idx, idx.numel(), X.shape[1], out, out.stride(0))
    return out


# ---- the dense ends of the path: libgnx.so's csrc/gnx_dense.hip, gnx_dense_wgrad.hip (matrix cores), gnx_heads.hip ---
def _dense_launch(X, W, bias, relu):
    nat.require_cuda(X, W, bias)
    X, W = _as_f32_rows(X), _as_f32_rows(W)
    if X.shape[1] != W.shape[0]:
        raise Exception(f"dense: features have {X.shape[1]} columns, the weights expect {W.shape[0]}")
    out = torch.empty((X.shape[0], W.shape[1]), dtype=torch.float32, device=X.device)
    b = _bias_row("dense", bias, W.shape[1])
    nat.launch(X.device, "gnx_dense", X, X.stride(0), X.shape[0], X.shape[1], W, W.stride(0), W.shape[1], b, nat.ACT_RELU if relu else nat.ACT_NONE,
               out, out.stride(0))
    return out


def _relu_mask(g, out):
    """g * (out > 0) in one pass (relu's backward; ``out`` is a relu output, never NaN)."""
    return torch.ops.aten.threshold_backward(g.contiguous(), out, 0.0)


def _wgrad_slabs(n, floats):
    """Row slabs of a weight gradient over ``n`` rows whose partial sums hold ``floats`` floats each: one per 256 rows, at most 2048,
    the scratch capped at 1 GiB (include/gnx.h, gnx_dense_wgrad)."""
    return max(1, min(2048, (n + 255) // 256, (1 << 28) // max(floats, 1)))


def _dense_wgrad_launch(entry, X, G, graph=(), din=()):
    """The scratch, dW and the call of gnx_dense_wgrad or, with the graph handle and the input mask's triple, of gnx_dense_wgrad_drop:
    the same slabs and the same summation order.  ``X`` / ``G`` are f32 rows."""
    n, F = X.shape
    O = G.shape[1]
    work = torch.empty(_wgrad_slabs(n, F * O) * F * O, dtype=torch.float32, device=X.device)
    dW = torch.empty((F, O), dtype=torch.float32, device=X.device)
    nat.launch(X.device, entry, *graph, X, X.stride(0), G, G.stride(0), n, F, O, *din, dW, work, work.numel())
    return dW


def _dense_wgrad(X, G):
    """dW = X^T . G on the matrix cores (gnx_dense_wgrad): row slabs, partial sums added in a fixed order."""
    return _dense_wgrad_launch("gnx_dense_wgrad", _as_f32_rows(X), _as_f32_rows(G))


class _DenseAct(torch.autograd.Function):
    """out = act(X . W + b) on the matrix cores (layers.py:135-136; the transform of gcn.py:89).
    backward: g' = g * (out > 0); dX = g' . W^T through the same kernel; dW = X^T . g' through gnx_dense_wgrad (MFMA over row
    slabs); db = column sums of g' (a torch reduction)."""

    @staticmethod
    def forward(ctx, X, W, bias, relu):
        out = _dense_launch(X, W, bias, relu)
        ctx.relu, ctx.has_bias = relu, bias is not None
        ctx.bias_shape = None if bias is None else tuple(bias.shape)
        ctx.save_for_backward(X, W, out if relu else None)
        return out

    @staticmethod
    def backward(ctx, g):
        X, W, out = ctx.saved_tensors
        g = _relu_mask(g, out) if ctx.relu else g
        g = g.contiguous()
        gX = _dense_launch(g, W.t().contiguous(), None, False) if ctx.needs_input_grad[0] else None
        gW = _dense_wgrad(X, g) if ctx.needs_input_grad[1] else None
        gb = g.sum(dim=0).reshape(ctx.bias_shape) if ctx.has_bias and ctx.needs_input_grad[2] else None
        return gX, gW, gb, None


def dense(X: torch.Tensor, W: torch.Tensor, bias=None, relu=False) -> torch.Tensor:
    """act(X . W + bias) for device tensors, through gnx_dense (float32 MFMA).  ``bias`` [1, O] / [O] or None."""
    return _DenseAct.apply(X, W, bias, bool(relu))


def _dropout_triple(dropout, what):
    """(p, seed, stream) of a counter-RNG feature dropout as (float, uint64, uint64), or None for ``None`` / a rate of 0."""
    if dropout is None:
        return None
    p, seed, stream = dropout
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise Exception(f"{what}: dropout rate {p} outside [0, 1)")
    return (p, int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream) & 0xFFFFFFFFFFFFFFFF) if p > 0 else None


def _feature_dropout_launch(graph: DeviceGraph, X, p, seed, stream, rows=None, out=None):
    """gnx_feature_dropout: drop(X) into ``out`` (None: a new tensor; X itself: in place), over the row ids ``rows`` (int32) or all rows."""
    nat.require_cuda(X, rows, out)
    _same_device(graph, X, rows, out)
    if X.dtype != torch.float32 or X.dim() != 2 or X.stride(1) != 1 or X.stride(0) < X.shape[1]:
        raise Exception("feature_dropout: needs float32 rows")
    if out is None:
        out = torch.empty_like(X, memory_format=torch.contiguous_format)
        if rows is not None:
            out.copy_(X)
    elif tuple(out.shape) != tuple(X.shape) or out.dtype != torch.float32 or out.stride(1) != 1 or out.stride(0) < out.shape[1]:
        raise Exception("feature_dropout: bad output buffer")
    if rows is not None and (rows.dtype != torch.int32 or rows.dim() != 1 or not rows.is_contiguous()):
        raise Exception("feature_dropout: the row list must be a contiguous int32 vector")
    n = X.shape[0] if rows is None else rows.numel()
    if X.shape[1] == 0:
        return out
    nat.launch(X.device, "gnx_feature_dropout", graph.handle, X, X.stride(0), n, X.shape[1], rows, p, seed, stream, out, out.stride(0))
    return out


def _padded_rows(n, C, device):
    """An uninitialised f32 [n, C] view of rows of stride roundup4(C): every row starts 16-byte aligned and can be read in whole 16-byte
    pieces (what the fused GCN backward gathers; the padding columns are never written and their content does not matter)."""
    return torch.empty((n, (C + 3) // 4 * 4), dtype=torch.float32, device=device)[:, :C]


def _gate_launch(graph: DeviceGraph, g, y, p, seed, stream, relu, bf16, padded=False):
    """The backward's gate, gnx_feature_dropout_back or (``bf16``: y is the stored bf16 output) gnx_feature_dropout_back_bf16: returns
    (G, Gb) with G = kept ? g * s : 0 -- with ``relu`` also 0 where ``y`` <= 0 -- and Gb = bf(G), None without ``bf16``.
    ``padded``: G is written into rows of stride roundup4(C) (_padded_rows; the pass takes the stride as its ldG)."""
    g = _as_f32_rows(g).contiguous()
    nat.require_cuda(g, y)
    _same_device(graph, g, y)
    G = _padded_rows(g.shape[0], g.shape[1], g.device) if padded else torch.empty_like(g)
    Gb = torch.empty(g.shape, dtype=torch.bfloat16, device=g.device) if bf16 else None
    if g.numel() == 0:
        return G, Gb
    y = y if relu else None
    args = (graph.handle, g, g.stride(0), y, 0 if y is None else y.stride(0), g.shape[0], g.shape[1], p, seed, stream,
            nat.ACT_RELU if relu else nat.ACT_NONE, G, G.stride(0))
    if bf16:
        nat.launch(g.device, "gnx_feature_dropout_back_bf16", *args, Gb, Gb.stride(0))
    else:
        nat.launch(g.device, "gnx_feature_dropout_back", *args)
    return G, Gb


def _feature_dropout_back(graph: DeviceGraph, g, y, p, seed, stream, relu, padded=False):
    """gnx_feature_dropout_back: G = kept ? g * s : 0, with ``relu`` also 0 where the dropped forward output ``y`` is <= 0."""
    return _gate_launch(graph, g, y, p, seed, stream, relu, bf16=False, padded=padded)[0]


class _FeatureDropout(torch.autograd.Function):
    """out = drop(X) with the counter RNG's mask of (seed, stream); backward G = kept ? g * s : 0, the mask made again from the triple."""

    @staticmethod
    def forward(ctx, X, graph, p, seed, stream):
        ctx.graph, ctx.triple = graph, (p, seed, stream)
        return _feature_dropout_launch(graph, _as_f32_rows(X), p, seed, stream)

    @staticmethod
    def backward(ctx, g):
        return _feature_dropout_back(ctx.graph, g, None, *ctx.triple, relu=False), None, None, None, None


def feature_dropout(graph: DeviceGraph, X: torch.Tensor, p, seed, stream) -> torch.Tensor:
    """tf.nn.dropout(X, p) (layered.py:44-45) with the mask of the counter RNG instead of torch's generator (gnx_feature_dropout):
    element (i, c) is kept iff hash_u24(seed, stream + counter, i, c, 0) >= int(p * 2^24), kept values are scaled by the f32
    1 / (1 - p), dropped ones are +0.  ``graph`` lends its dropout counter (DeviceGraph.set_dropout_counter: a replayed hipGraph then
    draws fresh masks) and is otherwise not read.  Reproducible from (seed, stream); differentiable w.r.t. X; device tensors only."""
    triple = _dropout_triple((p, seed, stream), "feature_dropout")
    nat.require_cuda(X)
    if triple is None:
        return X
    return _FeatureDropout.apply(X, graph, *triple)


def _dropout_args(dropout):
    """The (p, seed, stream) an entry takes for ``dropout`` = the checked triple or None (rate 0: nothing is hashed)."""
    return dropout or (0.0, 0, 0)


def _gated_gradient(graph: DeviceGraph, g, out, relu, dropout):
    """g' of a fused layer from the upstream gradient ``g`` and the saved ``out``: with a fused mask one pass (gnx_feature_dropout_back:
    kept ? g * s : 0, gated by out > 0 under ``relu``), else the relu mask; contiguous."""
    if dropout is not None:
        return _feature_dropout_back(graph, g, out, *dropout, relu=relu)
    return (_relu_mask(g, out) if relu else g).contiguous()


DENSE_DROPOUTS = ("torch", "fused")


def _dense_drop_launch(graph: DeviceGraph, X, W, bias, relu, din, dout):
    """gnx_dense_drop: drop_out(act(drop_in(X) . W + bias)) in the dense kernels' launch; ``din`` / ``dout`` = checked triples or None."""
    _need_symbol("dense_step", "gnx_dense_drop")
    nat.require_cuda(X, W, bias)
    _same_device(graph, X, W, bias)
    if X.shape[1] != W.shape[0]:
        raise Exception(f"dense_step: features have {X.shape[1]} columns, the weights expect {W.shape[0]}")
    out = torch.empty((X.shape[0], W.shape[1]), dtype=torch.float32, device=X.device)
    b = _bias_row("dense_step", bias, W.shape[1])
    nat.launch(X.device, "gnx_dense_drop", graph.handle, X, X.stride(0), X.shape[0], X.shape[1], W, W.stride(0), W.shape[1], b,
               nat.ACT_RELU if relu else nat.ACT_NONE, *_dropout_args(din), *_dropout_args(dout), out, out.stride(0))
    return out


def _dense_wgrad_drop(graph: DeviceGraph, X, G, din):
    """dW = drop_in(X)^T . G with the mask made again in the weight-gradient kernels (gnx_dense_wgrad_drop): _dense_wgrad's slabs and
    summation order, no dropped copy of X.  ``din`` None: _dense_wgrad itself."""
    if din is None:
        return _dense_wgrad(X, G)
    _need_symbol("dense_step", "gnx_dense_wgrad_drop")
    X, G = _as_f32_rows(X), _as_f32_rows(G)
    _same_device(graph, X, G)
    return _dense_wgrad_launch("gnx_dense_wgrad_drop", X, G, (graph.handle,), din)


class _DenseStep(torch.autograd.Function):
    """out = drop_out(act(drop_in(X) . W + b)) as one launch (gnx_dense_drop).  Saves (X, W, out): X is the caller's tensor, no dropped
    copy and no mask exist.  backward: G' = the gate over out (gnx_feature_dropout_back: output mask, scale and relu in one pass; the
    relu mask without an output dropout); dW = drop_in(X)^T . G' with the mask made again (gnx_dense_wgrad_drop); db = column sums;
    dX, where wanted, = drop_in's backward over G' . W^T (gnx_dense, then gnx_feature_dropout_back with the input triple)."""

    @staticmethod
    def forward(ctx, X, W, bias, graph, relu, din, dout):
        out = _dense_drop_launch(graph, X, W, bias, relu, din, dout)
        ctx.graph, ctx.relu, ctx.din, ctx.dout = graph, relu, din, dout
        ctx.has_bias, ctx.bias_shape = bias is not None, None if bias is None else tuple(bias.shape)
        ctx.save_for_backward(X, W, out)
        return out

    @staticmethod
    def backward(ctx, g):
        X, W, out = ctx.saved_tensors
        G = _gated_gradient(ctx.graph, g, out, ctx.relu, ctx.dout)
        gW = _dense_wgrad_drop(ctx.graph, X, G, ctx.din) if ctx.needs_input_grad[1] else None
        gb = G.sum(dim=0).reshape(ctx.bias_shape) if ctx.has_bias and ctx.needs_input_grad[2] else None
        gX = None
        if ctx.needs_input_grad[0]:
            gX = _dense_launch(G, W.t().contiguous(), None, False)
            if ctx.din is not None:
                gX = _feature_dropout_back(ctx.graph, gX, None, *ctx.din, relu=False)
        return gX, gW, gb, None, None, None, None


def dense_step(graph: DeviceGraph, X: torch.Tensor, W: torch.Tensor, bias=None, relu=False, in_dropout=None, out_dropout=None) -> torch.Tensor:
    """drop_out(act(drop_in(X) . W + bias)) -- a Dropout layer, a Dense layer and the Dense's own dropout (layers.py:125-136, 175-181;
    filter.py:30-33) -- as ONE launch of the dense kernels (gnx_dense_drop) and one autograd node.  ``in_dropout`` / ``out_dropout`` =
    ``(p, seed, stream)`` or None, as ``gcnii_step(dropout=)`` takes them: the masks are ``feature_dropout``'s -- element (i, c) is
    kept iff hash_u24(seed, stream + counter, i, c, 0) >= int(p * 2^24), kept values times the f32 1 / (1 - p) -- made where the
    kernels pick up a row of X and where they finish a row of the result, so the result is bit for bit
    ``feature_dropout(dense(feature_dropout(X, in), W, bias, relu), out)`` while no dropped copy of X and no mask reach memory.  The node
    saves X itself, W and the result; its weight gradient makes the input mask again (gnx_dense_wgrad_drop).  ``graph`` lends its
    dropout counter and is otherwise not read.  Without either triple (or with rates of 0) it is ``dense``.  float32 device tensors."""
    din, dout = _dropout_triple(in_dropout, "dense_step"), _dropout_triple(out_dropout, "dense_step")
    if din is None and dout is None:
        return dense(X, W, bias, relu)
    nat.require_cuda(X, W, bias)
    X, W = _as_f32_rows(X), _as_f32_rows(W)
    return _DenseStep.apply(X, W, bias, graph, bool(relu), din, dout)


def _gcnii_input_grads(adj, G, a, M, want_H, want_H0, fused_backward, fused_edge=False):
    """(dH, dH0) of a GCNII layer from its gated gradient ``G``; None where not wanted.  ``fused_backward``: one launch
    (gcnii_step_back: dH = ((1-a) A^T G) M^T, dH0 = (a G) M^T -- it always makes dH; a caller that wants dH0 alone is not what a GCNII
    stack asks for); else dT = G M^T (gnx_dense), dH = (1-a) A^T dT, dH0 = a dT."""
    if not (want_H or want_H0):
        return None, None
    Mt = M.t().contiguous()
    if fused_backward:
        gH, gH0 = gcnii_step_back(adj, G, a, Mt, want_S=want_H0, edge_dropout="fused" if fused_edge else "composed")
        return (gH if want_H else None), gH0
    gT = _dense_launch(G, Mt, None, False)
    gH = _launch(adj, gT, None, 1.0 - a, 0.0, nat.ACT_NONE, transposed=True) if want_H else None
    return gH, (gT * a if want_H0 else None)


def _gcnii_operands(what, adj, rows, f32=(), M=None, constant=None, device=True):
    """The checks the GCNII launches share: a square adjacency without a diagonal -- with ``constant`` (what it is that needs one) no
    DroppedAdjacency either -- with ``device`` device tensors on its device, ``rows`` (bf16 or f32, [n, C]), every ``f32`` matrix of
    that shape (float32, contiguous; None passes) and ``M`` [C, C]; returns (graph, C).  (It sits on every launch of launch-bound
    steps: nothing is looked at twice, and the f32 forward, which never compared devices, passes ``device=False``.)"""
    if constant is not None and isinstance(adj, DroppedAdjacency):
        raise Exception(f"{what}: {constant} needs a constant adjacency (a DroppedAdjacency makes its weights in the SpMM)")
    if adj.diag is not None:
        raise Exception(f"{what}: add_eye adjacencies are not supported by the fused step")
    g, shape = adj.graph, rows.shape
    if device:
        nat.require_cuda(rows, M, *f32)
        _same_device(g, rows, M, *f32)
    if len(shape) != 2 or g.n_rows != g.n_cols or shape[0] != g.n_rows or (M is not None and M.shape != (shape[1], shape[1])):
        raise Exception(f"{what}: shape mismatch")
    for t in f32:
        if t is not None and (t.shape != shape or t.dtype != torch.float32 or not t.is_contiguous()):
            raise Exception(f"{what}: shape mismatch")
    return g, shape[1]


def _gcnii_launch(adj: Adjacency, H, H0, a, M, relu, keep_mixed, dropout=None, fused_edge=False):
    """gnx_gcnii_step; returns (out, T or None).  T = the mixed rows (A.H)(1-a) + H0 a, written by the same launch when kept.
    ``dropout`` = (p, seed, stream): gnx_gcnii_step_drop, out = drop(act(T . M)); T stays undropped.
    ``fused_edge`` (``adj`` is a DroppedAdjacency): gnx_gcnii_step_dropped -- the weights are made in the launch's gather loop from the
    adjacency's (D, p, seed, stream) and ``adj.vals`` is never materialised."""
    nat.require_cuda(H, H0, M)
    H, H0, M = _as_f32_rows(H).contiguous(), _as_f32_rows(H0).contiguous(), _as_f32_rows(M)
    g, C = _gcnii_operands("gcnii_step", adj, H, (H0,), M, device=fused_edge)
    out = torch.empty_like(H)
    mixed = torch.empty_like(H) if keep_mixed or C not in (16, 32, 64) else None
    act = nat.ACT_RELU if relu else nat.ACT_NONE
    if fused_edge:
        _same_device(g, adj.D)
        nat.launch(H.device, "gnx_gcnii_step_dropped", g.handle, adj.D, adj.p, adj.seed, adj.stream_id, H, H0, a, C, M, M.stride(0), act,
                   *_dropout_args(dropout), out, mixed)
        return out, mixed
    layer = (g.handle, adj.vals, H, H0, a, C, M, M.stride(0), act)
    if dropout is not None:
        nat.launch(H.device, "gnx_gcnii_step_drop", *layer, *dropout, out, mixed)
    else:
        nat.launch(H.device, "gnx_gcnii_step", *layer, out, mixed)
    return out, mixed


GCNII_BACKWARDS = ("composed", "fused")
GCNII_WEIGHT_GRADIENTS = ("stored", "recomputed")
GCNII_EDGE_DROPOUTS = ("composed", "fused")
GCNII_FUSED_WIDTHS = (16, 32, 64)


def _edge_dropout(what, edge_dropout) -> bool:
    """Whether ``edge_dropout`` asks for the fused form; raises on anything but the two names."""
    _one_of(what, "edge_dropout", edge_dropout, GCNII_EDGE_DROPOUTS)
    return edge_dropout == "fused"


def _weight_gradient(what, weight_gradient) -> bool:
    """Whether ``weight_gradient`` asks for the recomputed form; raises on anything but the two names."""
    _one_of(what, "weight_gradient", weight_gradient, GCNII_WEIGHT_GRADIENTS)
    return weight_gradient == "recomputed"


def gcnii_wgrad(adj: Adjacency, H: torch.Tensor, H0: torch.Tensor, a: float, G: torch.Tensor, hub_rows=None) -> torch.Tensor:
    """dM = T^T . G of one GCNII layer with the mixed rows T = (1-a) A.H + a H0 made again inside the launch and never stored
    (gnx_gcnii_wgrad; a bf16 ``H`` -- the rows a bf16 training layer gathered -- takes gnx_gcnii_wgrad_bf16; no autograd).  ``H``, ``H0``
    and the gated gradient ``G`` (f32) are contiguous [n, C], C in {16, 32, 64}, on a constant square adjacency without a diagonal; a row
    of T has the bits the forward stores, the sum over the rows is ordered differently from gnx_dense_wgrad's (float32 rounding).
    ``hub_rows``: an f32 [n, C] scratch the caller owns (a backward shares one among its layers); None allocates one, and only when the
    graph has hub rows (DeviceGraph.n_hub_rows).  The slabs of the partial sums are sized as gnx_dense_wgrad's."""
    g, C = _gcnii_operands("gcnii_wgrad", adj, H, (H0, G, hub_rows) if H.dtype == torch.bfloat16 else (H, H0, G, hub_rows), None,
                           "the recomputed weight gradient")
    bf16 = H.dtype == torch.bfloat16
    if C not in GCNII_FUSED_WIDTHS or (bf16 and not H.is_contiguous()):
        raise Exception("gcnii_wgrad: needs contiguous f32 or bf16 rows of width 16, 32 or 64")
    n = H.shape[0]
    if hub_rows is None and g.n_hub_rows > 0:
        hub_rows = torch.empty((n, C), dtype=torch.float32, device=H.device)
    work = torch.empty(_wgrad_slabs(n, C * C) * C * C, dtype=torch.float32, device=H.device)
    dM = torch.empty((C, C), dtype=torch.float32, device=H.device)
    nat.launch(H.device, "gnx_gcnii_wgrad_bf16" if bf16 else "gnx_gcnii_wgrad", g.handle, adj.vals, H, H0, a, C, G, dM, hub_rows, work,
               work.numel())
    return dM


def gcnii_step_back(adj: Adjacency, G: torch.Tensor, a: float, Mt: torch.Tensor, S_in=None, s_alpha=1.0, want_S=True, edge_dropout="composed"):
    """The backward of gcnii_step past the relu gate as ONE launch for C in {16, 32, 64} (gnx_gcnii_step_back; no autograd):
    with ``G`` = g * (out > 0) and ``Mt`` = M^T,  dH = ((1-a) A^T G) . Mt  and  S = s_alpha S_in + (a G) . Mt  -- the gradient of H and
    the layer's term of dH0 on top of a running sum ``S_in`` (None: no such term).  Returns (dH, S); ``want_S=False`` skips the
    second product and returns (dH, None).  G is gathered over the transposed structure itself: G . Mt never reaches memory.
    Other widths run gnx_dense, the transposed SpMM and one linear combination, through a work buffer allocated here.
    ``edge_dropout="fused"`` with a DroppedAdjacency (which is refused otherwise): gnx_gcnii_step_back_dropped, the same launch with
    the weights of the transposed walk made from the adjacency's (D, p, seed, stream) -- bit for bit the results over the materialised
    adjacency ``normalize(graph, "symmetric", "none", p, seed, stream)``."""
    fused_edge = _edge_dropout("gcnii_step_back", edge_dropout) and isinstance(adj, DroppedAdjacency)
    G, S_in = _as_f32_rows(G).contiguous(), None if S_in is None else _as_f32_rows(S_in).contiguous()
    return _gcnii_back_launch(False, adj, G, None, a, Mt, S_in, s_alpha, want_S, False, fused_edge=fused_edge)


def _gcnii_back_launch(bf16, adj, X, G, a, Mt, S_in, s_alpha, want_S, in_place, fused_edge=False):
    """gnx_gcnii_step_back over the f32 rows ``X`` (the gated gradient itself; ``G`` is None), or with ``bf16``
    gnx_gcnii_step_back_bf16 over its bf16 copy ``X`` beside the f32 ``G``: the checks, the buffers -- dH, S (``in_place``: S_in itself;
    None without ``want_S``), and for f32 rows of the other widths the work buffer of the composed form -- and the call.
    Returns (dH, S)."""
    Mt = _as_f32_rows(Mt)
    if bf16:
        g, C = _gcnii_operands("gcnii_step_back_bf16", adj, X, (G, S_in), Mt, "bf16 training storage")
        if X.dtype != torch.bfloat16 or not X.is_contiguous():
            raise Exception("gcnii_step_back_bf16: needs contiguous bf16 rows [n, C] and Mt [C, C]")
        if want_S == (G is None) or (S_in is not None and not want_S) or (in_place and S_in is None):
            raise Exception("gcnii_step_back_bf16: the f32 G goes with want_S, S_in needs want_S, in_place needs S_in")
    else:
        g, C = _gcnii_operands("gcnii_step", adj, X, (S_in,), Mt, None if fused_edge else "the fused backward")
        if S_in is not None and not want_S:
            raise Exception("gcnii_step: S_in without want_S")
    dH = torch.empty_like(X, dtype=torch.float32) if bf16 else torch.empty_like(X)
    S = (S_in if in_place else torch.empty_like(dH)) if want_S else None
    work = torch.empty_like(dH) if not bf16 and C not in (16, 32, 64) else None
    if fused_edge:      # (f32 rows: gnx_gcnii_step_back_dropped makes the transposed weights itself; no value array is written)
        _same_device(g, adj.D)
        nat.launch(X.device, "gnx_gcnii_step_back_dropped", g.handle, adj.D, adj.p, adj.seed, adj.stream_id, X, a, C, Mt, Mt.stride(0), dH, S_in,
                   s_alpha, S, work)
        return dH, S
    values = adj.transposed_values()
    if bf16:
        nat.launch(X.device, "gnx_gcnii_step_back_bf16", g.handle, values, X, G, a, C, Mt, Mt.stride(0), dH, S_in, s_alpha, S, None)
    else:
        nat.launch(X.device, "gnx_gcnii_step_back", g.handle, values, X, a, C, Mt, Mt.stride(0), dH, S_in, s_alpha, S, work)
    return dH, S


class _GCNIIStep(torch.autograd.Function):
    """out = act(T . M), T = (A . H)(1-a) + H0 a, as ONE launch that also leaves T in memory for the backward (gcn.py:22-27 under
    tf.GradientTape): with g' = g * (out > 0):  dM = T^T g' (gnx_dense_wgrad), dT = g' M^T (gnx_dense), dH = (1-a) A^T dT, dH0 = a dT.
    ``backward="fused"``: dH = ((1-a) A^T g') M^T and dH0 = (a g') M^T from ONE launch (gcnii_step_back), dT never written.
    ``dropout`` = (p, seed, stream): out = drop(act(T . M)) from the same launch (gnx_gcnii_step_drop); the dropped out is what is
    saved, and g' = kept ? g * s : 0 gated by out > 0 comes from one pass (gnx_feature_dropout_back) in place of the relu mask.
    ``recompute``: T is neither written nor saved -- (H, H0, M, out) are saved instead of (T, M, out), where H is the previous layer's
    saved output and H0 the stack's -- and dM comes from gcnii_wgrad, which makes T again (widths 16, 32, 64 only).
    ``fused_edge``: ``adj`` is a DroppedAdjacency and stays one (it keeps its D; no value array): the forward is
    gnx_gcnii_step_dropped with T written, the fused backward gnx_gcnii_step_back_dropped, the composed one the transposed dropped SpMM."""

    @staticmethod
    def forward(ctx, H, H0, M, adj, a, relu, backward="composed", dropout=None, recompute=False, fused_edge=False):
        ctx.adj, ctx.a, ctx.relu, ctx.fused_backward, ctx.dropout, ctx.recompute = adj, a, relu, backward == "fused", dropout, recompute
        ctx.fused_edge = fused_edge
        if recompute:   # T is not written: the backward makes it again from H and H0 (gcnii_wgrad), which are saved in its place
            H, H0 = _as_f32_rows(H).contiguous(), _as_f32_rows(H0).contiguous()
            out, _ = _gcnii_launch(adj, H, H0, a, M, relu, keep_mixed=False, dropout=dropout)
            ctx.save_for_backward(H, H0, M, out if relu or dropout is not None else None)
            return out
        out, T = _gcnii_launch(adj, H, H0, a, M, relu, keep_mixed=True, dropout=dropout, fused_edge=fused_edge)
        ctx.save_for_backward(T, M, out if relu or dropout is not None else None)
        return out

    @staticmethod
    def backward(ctx, g):
        if ctx.recompute:
            H, H0, M, out = ctx.saved_tensors
        else:
            T, M, out = ctx.saved_tensors
        g = _gated_gradient(ctx.adj.graph, g, out, ctx.relu, ctx.dropout)
        if not ctx.needs_input_grad[2]:
            gM = None
        elif ctx.recompute:
            gM = gcnii_wgrad(ctx.adj, H, H0, ctx.a, _as_f32_rows(g).contiguous())
        else:
            gM = _dense_wgrad(T, g)
        gH, gH0 = _gcnii_input_grads(ctx.adj, g, ctx.a, M, ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.fused_backward, ctx.fused_edge)
        return gH, gH0, gM, None, None, None, None, None, None, None


def gcnii_step(adj: Adjacency, H: torch.Tensor, H0: torch.Tensor, a: float, M: torch.Tensor, relu=True, storage=torch.float32,
               out_storage=torch.float32, backward="composed", dropout=None, weight_gradient="stored", edge_dropout="composed") -> torch.Tensor:
    """act(((A . H)(1-a) + H0 a) . M), M = (1-b) I + b W (gcn.py:22-27) -- ONE fused launch for C in {16, 32, 64}: the mixed
    rows stay in LDS and meet M on the matrix cores (gnx_gcnii_step).  Without autograd they never reach HBM; when gradients are
    needed the same launch also writes them (dM = T^T g needs them), once, and the transform does not read them back.  Other
    widths run the fused SpMM+mix and then the matrix-core transform.
    ``storage=torch.bfloat16`` (inference only: raises where autograd would need a gradient): the rows the launch GATHERS are bf16
    (gnx_gcnii_step_bf16) -- a bf16 H as it is, an f32 H rounded once (gnx_cast_bf16) -- widened exactly; sums, H0, the mix and the
    transform stay f32.  The result is f32, or with ``out_storage=torch.bfloat16`` rounded once as it is stored (what the next layer
    of a stack gathers).  Over a bf16-representable H the f32 result is bit for bit the default path's.
    ``backward``: ``"composed"`` (the default: gnx_dense, the transposed SpMM and a scaling, today's bits) or ``"fused"`` (opt-in:
    after the relu mask and gnx_dense_wgrad, dH and dH0 come from one launch, gcnii_step_back; the forward and dM keep their bits,
    dH and dH0 agree to float32 rounding -- the products associate differently).  A DroppedAdjacency keeps the generic composition.
    ``dropout`` = ``(p, seed, stream)`` (opt-in; None, the default, is today's call): the layer's feature dropout (gcn.py:27) leaves
    the same launch, out = drop(act(...)) (gnx_gcnii_step_drop) with the mask of ``feature_dropout`` -- the counter RNG of the edge
    dropout, not torch's generator; the mixed rows kept for dM stay undropped, and the backward starts with one pass
    (gnx_feature_dropout_back) instead of torch's dropout backward and the relu mask.  Behind the generic composition of a
    DroppedAdjacency the mask is ``feature_dropout``'s pass.  Training only: raises together with ``storage=torch.bfloat16``.
    ``weight_gradient``: ``"stored"`` (the default: the launch writes T, it is saved, dM = T^T g comes from gnx_dense_wgrad -- today's
    bits) or ``"recomputed"`` (opt-in, C in {16, 32, 64} on a constant adjacency, device tensors): the launch writes no T and the layer
    saves (H, H0, M, out) instead of (T, M, out) -- in a stack H is the previous layer's saved output, so a layer keeps 4 bytes per
    element less -- and dM comes from ``gcnii_wgrad``, which makes T again.  out, dH and dH0 keep their bits; dM agrees to float32
    rounding (another summation order).  Other widths, a DroppedAdjacency and the inference paths ignore it.
    ``edge_dropout``: ``"composed"`` (the default: a DroppedAdjacency under autograd is the generic composition -- the dropped SpMM + mix,
    gnx_dense, the mask as a pass of its own -- today's calls and bits) or ``"fused"`` (opt-in): with a DroppedAdjacency, float32
    device tensors and gradients needed the step is the one autograd node of a constant adjacency -- gnx_gcnii_step_dropped makes
    every entry's weight in the gather loop of the fused launch and writes T, ``dropout`` leaves the same launch, and the backward
    honours ``backward`` (``"fused"``: gnx_gcnii_step_back_dropped; ``"composed"``: gnx_dense, the transposed dropped SpMM and a
    scaling).  out, dH, dH0 and dM are bit for bit those of the same call over the materialised adjacency
    ``normalize(graph, "symmetric", "none", p, seed, stream)``; against ``"composed"`` the forward keeps its bits at the other widths
    and agrees to float32 rounding at 16 / 32 / 64 (matrix-core transform order).  A dropped entry is skipped, not multiplied by 0
    (the DroppedAdjacency precondition of finite features).  Constant adjacencies, calls without autograd, bf16 storage and
    ``weight_gradient="recomputed"`` keep today's path whatever it says."""
    _one_of("gcnii_step", "backward", backward, GCNII_BACKWARDS)
    recompute = _weight_gradient("gcnii_step", weight_gradient)
    fused_edge = _edge_dropout("gcnii_step", edge_dropout) and not recompute and _fused_edge_applies(adj, H, H0, M)
    if dropout is not None:
        if _bf16(storage) or _bf16(out_storage):
            raise Exception("gcnii_step: dropout belongs to training, bf16 storage is inference only")
        dropout = _dropout_triple(dropout, "gcnii_step")            # (None again for a rate of 0)
    if _bf16(storage):
        _no_grad_for_bf16("gcnii_step", H, H0, M)
        return _gcnii_launch_bf16(adj, H, H0, a, M, relu, _bf16(out_storage))
    if _bf16(out_storage):
        raise Exception("gcnii_step: a bf16 result needs storage=torch.bfloat16")
    if torch.is_grad_enabled() and (H.requires_grad or H0.requires_grad or M.requires_grad):
        if fused_edge:                                              # weights made inside the fused launch itself (gnx_gcnii_step_dropped)
            return _GCNIIStep.apply(H, H0, M, adj, float(a), bool(relu), backward, dropout, False, True)
        if isinstance(adj, DroppedAdjacency):                       # weights made inside the SpMM: the generic composition knows how
            out = dense(ppr_step(adj, H, H0, a), M, None, relu)
            return out if dropout is None else feature_dropout(adj.graph, out, *dropout)
        return _GCNIIStep.apply(H, H0, M, adj, float(a), bool(relu), backward, dropout, recompute and H.shape[-1] in GCNII_FUSED_WIDTHS)
    return _gcnii_launch(adj, H, H0, a, M, relu, keep_mixed=False, dropout=dropout)[0]


def _fused_edge_applies(adj, H, H0, M) -> bool:
    """Whether gcnii_step(edge_dropout="fused") can take the fused launch: a DroppedAdjacency and float32 device tensors."""
    return isinstance(adj, DroppedAdjacency) and all(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 for t in (H, H0, M))


GCN_LAYERS = ("composed", "fused")
GCN_BACKWARDS = ("composed", "fused")
GCN_FUSED_WIDTHS = (16, 32, 64)       # C_in of the one-launch form of gnx_gcn_step; its C_out is any width up to C_in


def _gcn_launch(adj: Adjacency, X, W, bias, relu, keep_agg, dropout=None, fused_edge=False, spectral=False):
    """gnx_gcn_step, or with ``fused_edge`` (``adj`` is a DroppedAdjacency) gnx_gcn_step_dropped; returns (out, agg or None).
    ``spectral``: gnx_step_spectral_gcn / gnx_step_spectral_gcn_dropped -- out = 2 drop(act(P') - bias) -- and a third result, the gate
    words (int32 [n, ceil(C_out / 32)]: one bit per element, P' > 0) with ``keep_agg`` and ``relu``, else None.
    ``keep_agg`` (training): the launch also writes the aggregated rows A . X, which dW needs.  Without it the rows that have to pass
    through memory -- hub rows, and every row of the widths the one launch does not take -- go through a scratch buffer.
    ``dropout`` = the checked (p, seed, stream) or None."""
    nat.require_cuda(X, W, bias)
    X, W = _as_f32_rows(X), _as_f32_rows(W)
    g = adj.graph
    if not fused_edge and adj.vals is None and adj.vals_t is not None:
        raise Exception("gcn_step: this adjacency only holds transposed-order values")
    _same_device(g, X, W, bias, adj.vals if not fused_edge else adj.D)
    n, C_in = X.shape
    C_out = W.shape[1]
    if g.n_rows != g.n_cols or n != g.n_rows or W.shape[0] != C_in or C_in < 1 or C_out < 1:
        raise Exception("gcn_step: shape mismatch")
    b = _bias_row("gcn_step", bias, C_out)
    one_launch = C_in in GCN_FUSED_WIDTHS and C_out <= C_in and X.stride(0) % 4 == 0 and X.data_ptr() % 16 == 0
    out = torch.empty((n, C_out), dtype=torch.float32, device=X.device)
    rows = torch.empty((n, C_in), dtype=torch.float32, device=X.device) if keep_agg or not one_launch or g.n_hub_rows > 0 else None
    agg, work = (rows, None) if keep_agg else (None, rows)
    p, seed, stream = _dropout_args(dropout)
    layer = (X, X.stride(0), C_in, W, W.stride(0), C_out, b, nat.ACT_RELU if relu else nat.ACT_NONE, p, seed, stream, out, out.stride(0), agg)
    if spectral:
        _need_symbol("gcn_step_spectral", "gnx_step_spectral_gcn_dropped" if fused_edge else "gnx_step_spectral_gcn")
        gate = torch.empty((n, _gate_words(C_out)), dtype=torch.int32, device=X.device) if keep_agg and relu else None
        layer = layer + (gate,)
        plain, dropped = "gnx_step_spectral_gcn", "gnx_step_spectral_gcn_dropped"
    else:
        plain, dropped = "gnx_gcn_step", "gnx_gcn_step_dropped"
    if fused_edge:
        nat.launch(X.device, dropped, g.handle, adj.D, adj.p, adj.seed, adj.stream_id, *layer, work)
    else:
        nat.launch(X.device, plain, g.handle, adj.vals, *layer, work)
    return (out, agg, gate) if spectral else (out, agg)


class _GCNStep(torch.autograd.Function):
    """out = drop(act((A . X) . W + b)) as ONE launch that also leaves agg = A . X for the backward (gcn.py:88-89 under
    tf.GradientTape); (agg, W, out) is what is saved.  backward, composed from what exists: g' = g * (out > 0), or with a fused mask
    one pass (gnx_feature_dropout_back); dW = agg^T g' (gnx_dense_wgrad); db = column sums of g'; dX = A^T (g' W^T) -- gnx_dense, then
    the transposed SpMM, the dropped one under ``fused_edge`` (``adj`` stays a DroppedAdjacency: no value array).
    ``backward="fused"``: the gate writes g' into rows of stride roundup4(C_out) and dX = (A^T g') W^T comes from ONE launch that gathers
    g' at the output width (gcn_step_back); g' W^T is never written.  dW and db read the same g' and keep their bits.  The node then
    keeps agg itself (``ctx.agg``; (W, out) are what is saved) and lets it go as soon as dW is made, BEFORE dX is allocated: the
    backward never holds agg beside dX.  The price: such a node runs its backward once -- a second one (``retain_graph=True``) raises
    and asks for a new forward."""

    @staticmethod
    def forward(ctx, X, W, bias, adj, relu, dropout, fused_edge, backward="composed"):
        return _gcn_node_forward(ctx, X, W, bias, adj, relu, dropout, fused_edge, backward, spectral=False)

    @staticmethod
    def backward(ctx, g):
        return _gcn_node_backward(ctx, g) + (None, None, None, None, None)


def _gcn_node_forward(ctx, X, W, bias, adj, relu, dropout, fused_edge, backward, spectral):
    """The forward of _GCNStep and, with ``spectral``, of _GCNSpectralStep: the launch with agg = A . X kept, and what the backward
    reads -- (agg, W, third) with third = the output where a gate needs it, the spectral layer's gate words instead."""
    ctx.adj, ctx.relu, ctx.dropout, ctx.fused_edge, ctx.fused_backward = adj, relu, dropout, fused_edge, backward == "fused"
    ctx.spectral, ctx.bias_shape = spectral, None if bias is None else tuple(bias.shape)
    how = dict(spectral=True) if spectral else dict()      # (named only where it is not the default: gcn_step's call otherwise)
    out, agg, *gate = _gcn_launch(adj, X, W, bias, relu, keep_agg=True, dropout=dropout, fused_edge=fused_edge, **how)
    third = gate[0] if spectral else out if relu or dropout is not None else None
    if ctx.fused_backward:      # (agg is neither an input nor an output of the node: it may live on ctx, which can let it go early)
        ctx.agg = agg
        ctx.save_for_backward(W, third)
        return out
    ctx.save_for_backward(agg, W, third)
    return out


def _gcn_node_backward(ctx, g):
    """(dX, dW, db) of _GCNStep and _GCNSpectralStep: the gate, dW = agg^T G' (gnx_dense_wgrad), then dX from G' -- composed (gnx_dense,
    then the transposed SpMM, which runs with G' already let go) or, with ``backward="fused"``, ONE launch (gcn_step_back).  Under
    ``backward="fused"`` the node hands over the agg it kept on ``ctx`` -- once: a second backward raises -- and the rows are released
    once dW is made, before dX [n, C_in] is allocated; where dX is wanted G' then lives in rows of stride roundup4(C_out), which
    gnx_dense_wgrad reads as an [n, C_out] view.  The spectral gate pass writes them there and makes db itself.  _GCNStep's gate pass
    writes them there too, while its relu mask and its ungated gradient take one narrow copy when C_out is no multiple of 4; its
    column sums run over contiguous rows whichever backward it is (torch picks its reduction by the strides)."""
    saved = ctx.saved_tensors
    if ctx.fused_backward:
        agg, ctx.agg = ctx.agg, None
        if agg is None:
            what = "gcn_step_spectral" if ctx.spectral else "gcn_step"
            raise Exception(f"{what}(backward=\"fused\"): the node let its aggregated rows go in its first backward; run the forward again "
                            "(or use backward=\"composed\" where a graph is retained)")
        W, third = saved
    else:
        agg, W, third = saved
    del saved
    want_X = ctx.needs_input_grad[0]
    want_b = ctx.bias_shape is not None and ctx.needs_input_grad[2]
    gb = None
    if ctx.spectral:
        G, gb = _gcnii_spectral_gate(ctx.adj.graph, g, third, ctx.relu, ctx.dropout, padded=ctx.fused_backward and want_X)
        gb = gb if want_b else None
    else:
        C_out = g.shape[1]
        padded = ctx.fused_backward and want_X and C_out % 4 != 0
        if ctx.dropout is not None:
            G = _feature_dropout_back(ctx.adj.graph, g, third, *ctx.dropout, relu=ctx.relu, padded=padded)
            if want_b:
                gb = G.contiguous().sum(dim=0)
        else:
            G = (_relu_mask(g, third) if ctx.relu else g).contiguous()
            if want_b:
                gb = G.sum(dim=0)
            if padded:
                narrow, G = G, _padded_rows(G.shape[0], C_out, G.device)
                G.copy_(narrow)
                del narrow
    gW = _dense_wgrad(agg, G) if ctx.needs_input_grad[1] else None
    del agg                                                 # (under backward="fused" the last reference: the rows are free before dX is made)
    gX = None
    if want_X and ctx.fused_backward:
        gX = _gcn_back_launch(ctx.adj, G, W.t().contiguous(), ctx.fused_edge)
    elif want_X:
        gT = _dense_launch(G, W.t().contiguous(), None, False)
        del G                                               # (the gated gradient is done with: the transposed SpMM runs without it)
        gX = _launch(ctx.adj, gT, None, 1.0, 0.0, nat.ACT_NONE, transposed=True)
    return gX, gW, None if gb is None else gb.reshape(ctx.bias_shape)


def _gcn_back_launch(adj: Adjacency, G, Wt, fused_edge=False):
    """gnx_gcn_step_back over the gated gradient ``G`` [n, C_out] (f32 rows of any stride) and ``Wt`` = W^T [C_out, C_in], or with
    ``fused_edge`` (``adj`` is a DroppedAdjacency) gnx_gcn_step_back_dropped: the checks, dX, the work buffer -- [n, C_out] where the one
    launch applies and the transposed structure has hub rows, [n, C_in] where the entry runs gnx_dense and the transposed SpMM, none
    otherwise -- and the call.  Returns dX [n, C_in]."""
    nat.require_cuda(G, Wt)
    G, Wt = _as_f32_rows(G), _as_f32_rows(Wt)
    g = adj.graph
    _same_device(g, G, Wt, adj.D if fused_edge else None)
    n, C_out = G.shape
    C_in = Wt.shape[1]
    if g.n_rows != g.n_cols or n != g.n_rows or Wt.shape[0] != C_out or C_in < 1 or C_out < 1:
        raise Exception("gcn_step_back: shape mismatch")
    one_launch = (C_in in GCN_FUSED_WIDTHS and C_out <= C_in and G.stride(0) % 4 == 0 and G.stride(0) >= (C_out + 3) // 4 * 4
                  and G.data_ptr() % 16 == 0)
    dX = torch.empty((n, C_in), dtype=torch.float32, device=G.device)
    if not one_launch:
        work = torch.empty((n, C_in), dtype=torch.float32, device=G.device)
    elif g.n_hub_rows_t > 0:
        work = torch.empty((n, C_out), dtype=torch.float32, device=G.device)
    else:
        work = None
    tail = (G, G.stride(0), C_out, Wt, _row_stride(Wt), C_in, dX, dX.stride(0), work, 0 if work is None else work.numel())
    if fused_edge:
        nat.launch(G.device, "gnx_gcn_step_back_dropped", g.handle, adj.D, adj.p, adj.seed, adj.stream_id, *tail)
    else:
        nat.launch(G.device, "gnx_gcn_step_back", g.handle, adj.transposed_values(), *tail)
    return dX


def gcn_step_back(adj: Adjacency, G: torch.Tensor, W: torch.Tensor, edge_dropout="composed") -> torch.Tensor:
    """The gradient of X of gcn_step past the gate as ONE launch (gnx_gcn_step_back; no autograd): with ``G`` [n, C_out] the gated
    gradient and ``W`` [C_in, C_out] the layer's weights,  dX = (A^T G) . W^T  -- G is gathered over the transposed structure at the
    OUTPUT width and G . W^T never reaches memory -- for C_in in {16, 32, 64} and C_out <= C_in.  A ``G`` whose rows are not whole
    16-byte pieces (C_out no multiple of 4 in contiguous rows) is copied once into padded rows.  Other widths run gnx_dense and the
    transposed SpMM inside the entry, through a work buffer allocated here.  Hub rows of the transposed structure pass through an
    [n, C_out] buffer.  ``edge_dropout="fused"`` with a DroppedAdjacency: gnx_gcn_step_back_dropped, the weights of the transposed walk
    made from the adjacency's (D, p, seed, stream) -- bit for bit the result over the materialised adjacency; a DroppedAdjacency
    without it uses its materialised transposed values."""
    fused_edge = _edge_dropout("gcn_step_back", edge_dropout) and isinstance(adj, DroppedAdjacency)
    G, W = _as_f32_rows(G), _as_f32_rows(W)
    if G.dim() != 2 or W.dim() != 2 or W.shape[1] != G.shape[1]:
        raise Exception("gcn_step_back: shape mismatch")
    C_in, C_out = W.shape
    if C_in in GCN_FUSED_WIDTHS and C_out <= C_in and (G.stride(0) % 4 != 0 or G.data_ptr() % 16 != 0):
        padded = _padded_rows(G.shape[0], C_out, G.device)
        padded.copy_(G)
        G = padded
    return _gcn_back_launch(adj, G, W.t().contiguous(), fused_edge)


def _dense_or_torch(X, W, bias, relu):
    """act(X . W + bias), the transform of a composed layer: the dense kernel on device tensors, torch's ops on CPU tensors."""
    if X.is_cuda:
        return dense(X, W, bias, relu)
    out = torch.matmul(X, W) + (bias if bias is not None else 0)
    return torch.relu(out) if relu else out


def _spectral_tail(activated, bias, dropout):
    """2 * dropout(activated - bias), the elementwise tail of a composed spectral layer, with TORCH's dropout at the rate of ``dropout``
    = (p, seed, stream) or None."""
    y = activated - bias
    p = 0.0 if dropout is None else float(dropout[0])
    return 2 * (torch.nn.functional.dropout(y, p=p, training=True) if p != 0 else y)


def _gcn_composed(adj, X, W, bias, relu, dropout):
    """The layer as today's ops: spmm, then the dense kernel with bias and relu (CPU tensors: torch), then the mask as a pass of its own."""
    out = _dense_or_torch(spmm(adj, X), W, bias, relu)
    if dropout is None or float(dropout[0]) == 0:
        return out
    if out.is_cuda:
        return feature_dropout(adj.graph, out, *dropout)
    return torch.nn.functional.dropout(out, p=float(dropout[0]), training=True)


def gcn_step(adj: Adjacency, X: torch.Tensor, W: torch.Tensor, bias=None, relu=True, dropout=None, edge_dropout="composed",
             backward="composed") -> torch.Tensor:
    """GCNLayer (gcn.py:77-89) as one launch (gnx_gcn_step; opt-in, GNN(gcn_layer="fused")): drop(act((A . X) . W + bias)) with
    ``X`` [n, C_in], ``W`` [C_in, C_out] and ``bias`` [C_out] / [1, C_out] or None.  For C_in in {16, 32, 64} and C_out <= C_in the
    aggregated rows stay in LDS and meet W on the matrix cores: A . X, which ``spmm`` + ``dense`` write and read back, never reaches
    memory without autograd.  Other widths run the SpMM, the dense kernel and the mask pass inside the same call.
    ``dropout`` = ``(p, seed, stream)`` or None: the mask of ``feature_dropout`` (the counter RNG of the edge dropout, not torch's
    generator) over the finished rows, from the same launch.
    Under autograd it is one node that saves (A . X, W, out) -- the launch writes A . X once, for dW -- and returns the gradients of X,
    W and bias from today's kernels: the relu gate (or gnx_feature_dropout_back), gnx_dense_wgrad, the column sums, gnx_dense and
    the transposed SpMM.
    ``backward``: ``"composed"`` (the default: those calls, today's bits) or ``"fused"`` (opt-in): the gate writes G' into rows of
    stride roundup4(C_out) and dX = (A^T G') W^T comes from ONE launch that gathers G' at the output width (gcn_step_back,
    gnx_gcn_step_back; under ``edge_dropout="fused"`` gnx_gcn_step_back_dropped) -- neither G' W^T [n, C_in] nor gnx_dense appears;
    out, dW and db keep their bits, dX agrees to float32 rounding (the products associate differently).  It acts under autograd only.
    The node then lets A . X go once dW is made, before dX is allocated, and therefore runs its backward once: a second backward over
    a retained graph raises and asks for a new forward.
    ``edge_dropout``: ``"composed"`` (the default) or ``"fused"``: with a DroppedAdjacency the launch makes every entry's weight in
    its gather loop (gnx_gcn_step_dropped) -- out and A . X bit for bit those over the materialised adjacency
    ``normalize(graph, "symmetric", "none", p, seed, stream)`` -- and the backward's transposed SpMM is the dropped one.
    CPU tensors, an adjacency with a diagonal and a DroppedAdjacency without ``edge_dropout="fused"`` run ``spmm`` + ``dense``:
    today's calls and bits."""
    fused_edge = _edge_dropout("gcn_step", edge_dropout)
    _one_of("gcn_step", "backward", backward, GCN_BACKWARDS)
    tensors = (X, W) if bias is None else (X, W, bias)
    if (not all(isinstance(t, torch.Tensor) and t.is_cuda for t in tensors) or adj.diag is not None
            or (isinstance(adj, DroppedAdjacency) and not fused_edge)):
        return _gcn_composed(adj, X, W, bias, bool(relu), dropout)
    dropout = _dropout_triple(dropout, "gcn_step")
    fused_edge = fused_edge and isinstance(adj, DroppedAdjacency)
    if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
        return _GCNStep.apply(X, W, bias, adj, bool(relu), dropout, fused_edge, backward)
    return _gcn_launch(adj, X, W, bias, bool(relu), keep_agg=False, dropout=dropout, fused_edge=fused_edge)[0]


NGCF_LAYERS = ("composed", "fused")
NGCF_BACKWARDS = ("composed", "fused")
NGCF_FUSED_WIDTHS = (16, 32, 64)      # C_in of the one-launch form of gnx_ngcf_step; its C_out is any width up to C_in
NGCF_WIDES = ("composed", "fused")
NGCF_WIDE_WIDTHS = (128,)             # C_in of gnx_step_wide_ngcf (the SpMM, then one row-local launch); C_out any width up to C_in
NGCF_WIDE_BACKWARDS = ("composed", "fused")      # the backward at those widths: today's calls, or gnx_step_back_wide_ngcf
NGCF_ACTIVATIONS = {"none": nat.ACT_NONE, "relu": nat.ACT_RELU, "leaky": nat.ACT_LEAKY}
NGCF_SLOPES = {"none": 1.0, "relu": 0.0, "leaky": 0.2}


def _ngcf_work_floats(n, C_in, C_out, composed_rows, has_agg):
    """include/gnx.h, gnx_ngcf_step: the scratch of ``composed_rows`` rows that pass through memory (the hub rows of the one launch,
    every row otherwise) -- an [n, C_in] share for their aggregated rows where d_agg does not hold them, then their products with X
    and their first pre-activations as compact rows."""
    if composed_rows == 0:
        return 0
    up4 = lambda x: (x + 3) // 4 * 4
    return (0 if has_agg else up4(n * C_in)) + up4(composed_rows * C_in) + composed_rows * C_out


def _ngcf_rows_fit(widths, C_in, C_out, X, A=None):
    """What every fused NGCF launch asks: C_in in ``widths``, C_out <= C_in, 16-byte aligned rows of X and, where given, of a contiguous A."""
    return (C_in in widths and C_out <= C_in and X.stride(0) % 4 == 0 and X.data_ptr() % 16 == 0
            and (A is None or (A.is_contiguous() and A.data_ptr() % 16 == 0)))


def _ngcf_check_saved(n, C_out, activation, gate, y, rnorm):
    """What the backward reads of the forward's: the gate words, and the reciprocal norms with the output they go with."""
    if activation != "none" and (gate is None or gate.dtype != torch.int32 or tuple(gate.shape) != (n, 2 * _gate_words(C_out)) or not gate.is_contiguous()):
        raise Exception("ngcf_step: the gate words must be a contiguous int32 [n, 2 ceil(C_out / 32)]")
    if rnorm is not None and (y is None or tuple(y.shape) != (n, C_out) or rnorm.numel() != n or not rnorm.is_contiguous()):
        raise Exception("ngcf_step: the reciprocal norms go with the forward's output")


def _ngcf_wide_fusable(wide, X, C_in, C_out):
    """Where ``wide="fused"`` has a launch (gnx_step_wide_ngcf): C_in = 128, C_out <= C_in, 16-byte aligned rows of X."""
    return wide == "fused" and _ngcf_rows_fit(NGCF_WIDE_WIDTHS, C_in, C_out, X)


def _ngcf_launch(adj: Adjacency, X, W1, b1, W2, b2, activation, keep, dropout=None, normalize=True, wide="composed"):
    """gnx_ngcf_step; returns (out, agg, gate, rnorm).  ``keep`` (training): the launch also writes the aggregated rows A . X, the gate
    words (int32 [n, 2 ceil(C_out / 32)]: the P1 words, then the P2 words; none for the identity) and, with ``normalize``, the rows'
    reciprocal norms (negative where the clamp acted); all None otherwise.  ``dropout`` = the checked (p, seed, stream) or None.
    ``wide="fused"``: where _ngcf_wide_fusable says so the call is gnx_step_wide_ngcf -- the same arguments, outputs and formats, and a
    scratch of the aggregated rows alone where they are not kept; everything else is gnx_ngcf_step with today's arguments."""
    nat.require_cuda(X, W1, W2, b1, b2)
    X, W1, W2 = _as_f32_rows(X), _as_f32_rows(W1), _as_f32_rows(W2)
    g = adj.graph
    if adj.vals is None and adj.vals_t is not None:
        raise Exception("ngcf_step: this adjacency only holds transposed-order values")
    _same_device(g, X, W1, W2, b1, b2, adj.vals)
    n, C_in = X.shape
    C_out = W1.shape[1]
    if g.n_rows != g.n_cols or n != g.n_rows or tuple(W1.shape) != (C_in, C_out) or tuple(W2.shape) != (C_in, C_out) or C_in < 1 or C_out < 1:
        raise Exception("ngcf_step: shape mismatch")
    biases = [_bias_row("ngcf_step", b, C_out) for b in (b1, b2)]
    one_launch = _ngcf_rows_fit(NGCF_FUSED_WIDTHS, C_in, C_out, X)
    out = torch.empty((n, C_out), dtype=torch.float32, device=X.device)
    agg = torch.empty((n, C_in), dtype=torch.float32, device=X.device) if keep else None
    gated = keep and activation != "none"
    gate = torch.empty((n, 2 * _gate_words(C_out)), dtype=torch.int32, device=X.device) if gated else None
    rnorm = torch.empty(n, dtype=torch.float32, device=X.device) if keep and normalize else None
    rows_launch = _ngcf_wide_fusable(wide, X, C_in, C_out)
    if rows_launch:
        _need_symbol("ngcf_step", "gnx_step_wide_ngcf", keyword="wide")
        floats = 0 if keep else (n * C_in + 3) // 4 * 4
    else:
        floats = _ngcf_work_floats(n, C_in, C_out, g.n_hub_rows if one_launch else n, keep)
    work = torch.empty(floats, dtype=torch.float32, device=X.device) if floats else None
    p, seed, stream = _dropout_args(dropout)
    nat.launch(X.device, "gnx_step_wide_ngcf" if rows_launch else "gnx_ngcf_step", g.handle, adj.vals, X, X.stride(0), C_in, W1, _row_stride(W1),
               W2, _row_stride(W2), C_out, biases[0], biases[1], NGCF_ACTIVATIONS[activation], p, seed, stream, normalize, out, out.stride(0),
               agg, gate, rnorm, work, floats)
    return out, agg, gate, rnorm


def _ngcf_back_gate(graph: DeviceGraph, g, y, rnorm, gate, activation, dropout=None):
    """gnx_ngcf_back_gate: (G1, G2), [n, C_out] views of rows of stride roundup4(C_out) whose padding is zero, from the upstream gradient
    ``g``, the forward's output ``y``, its reciprocal norms (None: no norm was applied) and gate words, and its dropout triple."""
    g = _as_f32_rows(g)
    nat.require_cuda(g, y, rnorm, gate)
    _same_device(graph, g, y, rnorm, gate)
    n, C = g.shape
    _ngcf_check_saved(n, C, activation, gate, y, rnorm)
    y = None if rnorm is None else _as_f32_rows(y)
    G1, G2 = _padded_rows(n, C, g.device), _padded_rows(n, C, g.device)
    p, seed, stream = _dropout_args(dropout)
    nat.launch(g.device, "gnx_ngcf_back_gate", graph.handle, g, g.stride(0), y, 0 if y is None else y.stride(0), rnorm,
               gate if activation != "none" else None, n, C, NGCF_ACTIVATIONS[activation], p, seed, stream, G1, G2, G1.stride(0))
    return G1, G2


def _ngcf_back_work_floats(n, C_out):
    """include/gnx.h, gnx_step_back_ngcf: the bias slabs -- one per block of the launch, at most 8192, and one per group of 64 of them, 2 C_out
    floats each."""
    slabs = max(1, min(8192, ((n + 15) // 16 + 3) // 4))
    return (slabs + (slabs + 63) // 64) * 2 * C_out


def _ngcf_back_fusable(X, A, W1):
    """Where gnx_step_back_ngcf has a launch: C_in in {16, 32, 64}, C_out <= C_in, 16-byte aligned rows of X and A."""
    return _ngcf_rows_fit(NGCF_FUSED_WIDTHS, *W1.shape, X, A)


def _ngcf_back_launch(adj: Adjacency, g, y, rnorm, gate, activation, dropout, X, A, W1, W2, want_P=True, want_db=(True, True), want_dX=True,
                      entry="gnx_step_back_ngcf", work_floats=_ngcf_back_work_floats):
    """gnx_step_back_ngcf (or ``entry``, an entry of the same parameter list, with its ``work_floats(n, C_out)``), one call: returns
    dict(G1, G2, P, db1, db2, dA, R, dX).  G1 / G2 are [n, C_out] views of rows of stride roundup4(C_out) whose padding is zero;
    P = X * A only with ``want_P`` (dW1 needs it), db1 / db2 [C_out] with ``want_db``, and with ``want_dX`` the products dA = (G1 W1^T) * X + G2 W2^T and R = (G1 W1^T) * A and dX = A_hat^T dA + R (None each otherwise: no products
    and no transposed SpMM).  W1 / W2 are read as stored: no transposed copy.  ``dropout`` = the checked (p, seed, stream) or None."""
    g, X, A, W1, W2 = _as_f32_rows(g), _as_f32_rows(X), _as_f32_rows(A), _as_f32_rows(W1), _as_f32_rows(W2)
    nat.require_cuda(g, y, rnorm, gate, X, A, W1, W2)
    graph = adj.graph
    _same_device(graph, g, y, rnorm, gate, X, A, W1, W2)
    n, C_out = g.shape
    C_in = X.shape[1]
    if (graph.n_rows != graph.n_cols or n != graph.n_rows or tuple(X.shape) != (n, C_in) or tuple(A.shape) != (n, C_in) or not A.is_contiguous()
            or tuple(W1.shape) != (C_in, C_out) or tuple(W2.shape) != (C_in, C_out)):
        raise Exception("ngcf_step: shape mismatch in the backward")
    _ngcf_check_saved(n, C_out, activation, gate, y, rnorm)
    y = None if rnorm is None else _as_f32_rows(y)
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=g.device)
    G1, G2 = _padded_rows(n, C_out, g.device), _padded_rows(n, C_out, g.device)
    P = new(n, C_in) if want_P else None
    db1, db2 = (new(C_out) if w else None for w in want_db)
    dA, R, dX = (new(n, C_in), new(n, C_in), new(n, C_in)) if want_dX else (None, None, None)
    floats = work_floats(n, C_out) if any(want_db) else 0
    work = new(floats) if floats else None
    p, seed, stream = _dropout_args(dropout)
    nat.launch(g.device, entry, graph.handle, adj.transposed_values() if want_dX else None, g, g.stride(0), y, 0 if y is None else y.stride(0),
               rnorm, gate if activation != "none" else None, C_out, NGCF_ACTIVATIONS[activation], p, seed, stream, X, X.stride(0), A, C_in,
               W1, _row_stride(W1), W2, _row_stride(W2), G1, G2, G1.stride(0), P, db1, db2, dA, R, dX, C_in, work, floats)
    return dict(G1=G1, G2=G2, P=P, db1=db1, db2=db2, dA=dA, R=R, dX=dX)


def _ngcf_wide_back_work_floats(n, C_out):
    """include/gnx.h, gnx_step_back_wide_ngcf: the bias slabs -- one per 512 rows, at most 1024, 2 C_out floats each."""
    return max(1, min(1024, (n + 511) // 512)) * 2 * C_out


def _ngcf_wide_back_fusable(wide_backward, X, A, W1):
    """Where ``wide_backward="fused"`` has a launch (gnx_step_back_wide_ngcf): C_in = 128, C_out <= C_in, 16-byte aligned rows of X and A."""
    return wide_backward == "fused" and _ngcf_rows_fit(NGCF_WIDE_WIDTHS, *W1.shape, X, A)


def _ngcf_wide_back_launch(adj: Adjacency, g, y, rnorm, gate, activation, dropout, X, A, W1, W2, want_P=True, want_db=(True, True), want_dX=True):
    """gnx_step_back_wide_ngcf, one call: what _ngcf_back_launch returns, from the gate pass, one row-local launch and the transposed SpMM
    at C_in = 128.  A library without the entry raises: nothing falls back."""
    _need_symbol("ngcf_step", "gnx_step_back_wide_ngcf", keyword="wide_backward")
    return _ngcf_back_launch(adj, g, y, rnorm, gate, activation, dropout, X, A, W1, W2, want_P=want_P, want_db=want_db, want_dX=want_dX,
                             entry="gnx_step_back_wide_ngcf", work_floats=_ngcf_wide_back_work_floats)


class _NGCFStep(torch.autograd.Function):
    """out = l2_normalize(drop(act((X * A) . W1 + b1) + act(A . W2 + b2))), A = A_hat . X, as ONE launch (gnx_ngcf_step) that leaves A,
    two gate bits per element (P1 > 0, P2 > 0) and the rows' reciprocal norms; (A, gate, rnorm, out, W1, W2) and the input X are what
    is saved.  backward, composed from today's kernels around one gate pass (gnx_ngcf_back_gate -> G1, G2): db = the column sums,
    dW1 = (X * A)^T G1 and dW2 = A^T G2 (gnx_dense_wgrad), Q1 = G1 W1^T and Q2 = G2 W2^T (gnx_dense), dA = Q1 * X + Q2 and
    dX = Q1 * A + A_hat^T dA (the transposed SpMM); the elementwise products in torch.
    ``backward="fused"``, where gnx_step_back_ngcf has a launch (_ngcf_back_fusable): that entry once -- the gate, the column sums, X * A,
    both products, dA and Q1 * A from one launch, then the transposed SpMM with Q1 * A mixed in -- and gnx_dense_wgrad twice.  The saved
    tensors stay: a second backward over a retained graph gives the same bits.
    ``wide_backward="fused"``, where gnx_step_back_wide_ngcf has a launch (_ngcf_wide_back_fusable: C_in = 128): the same route through
    that entry.  What is saved has one format from gnx_ngcf_step and from gnx_step_wide_ngcf, so the route does not depend on ``wide``."""

    @staticmethod
    def forward(ctx, X, W1, b1, W2, b2, adj, activation, dropout, normalize, backward="composed", wide="composed", wide_backward="composed"):
        ctx.adj, ctx.activation, ctx.dropout, ctx.backward, ctx.wide_backward = adj, activation, dropout, backward, wide_backward
        ctx.bias_shapes = tuple(None if b is None else tuple(b.shape) for b in (b1, b2))
        how = dict() if wide == "composed" else dict(wide=wide)      # (named only where it is not the default: today's call otherwise)
        out, agg, gate, rnorm = _ngcf_launch(adj, X, W1, b1, W2, b2, activation, keep=True, dropout=dropout, normalize=normalize, **how)
        ctx.save_for_backward(X, agg, gate, rnorm, out if normalize else None, W1, W2)
        return out

    @staticmethod
    def backward(ctx, g):
        X, A, gate, rnorm, out, W1, W2 = ctx.saved_tensors
        X = _as_f32_rows(X)
        need = ctx.needs_input_grad
        launch = (_ngcf_wide_back_launch if _ngcf_wide_back_fusable(ctx.wide_backward, X, A, W1)
                  else _ngcf_back_launch if ctx.backward == "fused" and _ngcf_back_fusable(X, A, W1) else None)
        if launch is not None:
            want_db = tuple(ctx.bias_shapes[k] is not None and need[2 + 2 * k] for k in (0, 1))
            made = launch(ctx.adj, g, out, rnorm, gate, ctx.activation, ctx.dropout, X, A, W1, W2, want_P=need[1], want_db=want_db, want_dX=need[0])
            del made["dA"], made["R"]                      # (the transposed SpMM inside the call was their last reader)
            gW1 = _dense_wgrad(made["P"], made["G1"]) if need[1] else None
            gW2 = _dense_wgrad(A, made["G2"]) if need[3] else None
            gb1, gb2 = (None if made[k] is None else made[k].reshape(shape) for k, shape in zip(("db1", "db2"), ctx.bias_shapes))
            gX = made["dX"]
            del made                                       # (P, G1, G2, dA and R are free before the caller allocates anything)
            return gX, gW1, gb1, gW2, gb2, None, None, None, None, None, None, None
        G1, G2 = _ngcf_back_gate(ctx.adj.graph, g, out, rnorm, gate, ctx.activation, ctx.dropout)
        gb1 = G1.contiguous().sum(dim=0).reshape(ctx.bias_shapes[0]) if ctx.bias_shapes[0] is not None and need[2] else None
        gb2 = G2.contiguous().sum(dim=0).reshape(ctx.bias_shapes[1]) if ctx.bias_shapes[1] is not None and need[4] else None
        gW1 = _dense_wgrad(X * A, G1) if need[1] else None
        gW2 = _dense_wgrad(A, G2) if need[3] else None
        gX = None
        if need[0]:
            Q1 = _dense_launch(G1, W1.t().contiguous(), None, False)
            Q2 = _dense_launch(G2, W2.t().contiguous(), None, False)
            del G1, G2
            dA = torch.addcmul(Q2, Q1, X)                   # Q1 * X + Q2
            del Q2
            gX = torch.addcmul(_launch(ctx.adj, dA, None, 1.0, 0.0, nat.ACT_NONE, transposed=True), Q1, A)
        return gX, gW1, gb1, gW2, gb2, None, None, None, None, None, None, None


def _ngcf_act(x, activation):
    if activation == "leaky":
        return torch.nn.functional.leaky_relu(x, 0.2)
    return torch.relu(x) if activation == "relu" else x


def _ngcf_composed(adj, X, W1, b1, W2, b2, activation, dropout, normalize):
    """The layer as today's ops: spmm, a torch multiply, two transforms (the dense kernel on the device), torch's activations and sum,
    the mask as a pass of its own (torch's dropout on CPU tensors), torch's normalize."""
    agg = spmm(adj, X)
    P1, P2 = _dense_or_torch(X * agg, W1, b1, False), _dense_or_torch(agg, W2, b2, False)
    u = _ngcf_act(P1, activation) + _ngcf_act(P2, activation)
    if dropout is not None and float(dropout[0]) != 0:
        u = feature_dropout(adj.graph, u, *dropout) if u.is_cuda else torch.nn.functional.dropout(u, p=float(dropout[0]), training=True)
    return torch.nn.functional.normalize(u, dim=1, eps=1e-12) if normalize else u


def ngcf_step(adj: Adjacency, X: torch.Tensor, W1: torch.Tensor, b1, W2: torch.Tensor, b2, activation="leaky", dropout=None,
              normalize=True, backward="composed", wide="composed", wide_backward="composed") -> torch.Tensor:
    """NGCFLayer (gcn.py:116-135) as one launch (gnx_ngcf_step; opt-in, GNN(ngcf_layer="fused")):
    l2_normalize(drop(act((X * (A . X)) . W1 + b1) + act((A . X) . W2 + b2))) with ``X`` [n, C_in], ``W1`` / ``W2`` [C_in, C_out], ``b1`` /
    ``b2`` [C_out] / [1, C_out] or None and ``activation`` ``"leaky"`` (tf.nn.leaky_relu's slope 0.2), ``"relu"`` or ``"none"``.  For
    C_in in {16, 32, 64} and C_out <= C_in the aggregated rows stay in LDS, meet W2 and -- multiplied in place by the row's own X -- W1
    on the matrix cores, and leave masked and normalised; other widths run the SpMM, the dense kernel and the row passes inside the call.
    ``dropout`` = ``(p, seed, stream)`` or None: the mask of ``feature_dropout`` (the counter RNG, not torch's generator), applied
    before the norm in the same launch.  ``normalize=False`` stops before the norm (what a caller with torch's dropout needs).
    Under autograd it is one node that saves (A . X, the gate bits, the reciprocal norms, out, W1, W2) beside its input X; the backward
    is one gate pass (gnx_ngcf_back_gate) and today's kernels: the column sums, gnx_dense_wgrad, gnx_dense and the transposed SpMM.
    ``backward``: ``"composed"`` (the default: those calls, today's bits) or ``"fused"`` (opt-in; GNN(ngcf_backward="fused")): for
    C_in in {16, 32, 64}, C_out <= C_in and aligned rows ONE launch (gnx_step_back_ngcf) makes the gated gradients, both bias sums,
    X * A, G1 W1^T and G2 W2^T on the matrix cores (W1 / W2 read as stored), dA and Q1 * A; the transposed SpMM mixes Q1 * A in, and
    gnx_dense_wgrad runs twice.  out, dW1 and dW2 keep their bits; dX and the bias gradients agree to float32 rounding (one fused
    multiply-add where torch rounds twice; slab-ordered sums).  P and dX are made only where W1 and X need a gradient.  A second
    backward over a retained graph works and gives the same bits.  It acts under autograd only; other widths keep the composed calls.
    ``wide``: ``"composed"`` (the default: today's call) or ``"fused"`` (opt-in; GNN(ngcf_wide="fused")): for C_in = 128, C_out <= C_in
    and aligned rows the call is gnx_step_wide_ngcf -- gnx_spmm into A . X, then ONE row-local launch that reads X and A . X once and
    writes the finished rows, the gate words and the reciprocal norms in gnx_ngcf_step's formats -- instead of the SpMM, a product pass,
    the dense kernel twice and a row pass inside gnx_ngcf_step.  The node and its composed backward are unchanged (``backward="fused"``
    stays inert at this width); the results agree with the composed call to float32 rounding.  Other widths make today's call.
    ``wide_backward``: ``"composed"`` (the default: today's backward) or ``"fused"`` (opt-in; GNN(ngcf_wide_backward="fused")): for
    C_in = 128, C_out <= C_in and aligned rows the backward is ONE call of gnx_step_back_wide_ngcf -- the gate pass and the slab-ordered
    bias sums, one row-local launch that forms G1 W1^T and G2 W2^T on the matrix cores (W1 / W2 read as stored) and writes dA, Q1 * A
    and X * A, then the transposed SpMM with Q1 * A mixed in -- and gnx_dense_wgrad twice, whichever call made the forward.  out, dW1
    and dW2 keep their bits; dX and the bias gradients agree with the composed backward to float32 rounding.  A second backward over a
    retained graph gives the same bits.  It acts under autograd only; other widths and misaligned rows keep the composed backward.
    CPU tensors, an adjacency with a diagonal and a DroppedAdjacency run today's ops."""
    _one_of("ngcf_step", "activation", activation, NGCF_ACTIVATIONS)
    _one_of("ngcf_step", "backward", backward, NGCF_BACKWARDS)
    _one_of("ngcf_step", "wide", wide, NGCF_WIDES)
    _one_of("ngcf_step", "wide_backward", wide_backward, NGCF_WIDE_BACKWARDS)
    tensors = tuple(t for t in (X, W1, b1, W2, b2) if t is not None)
    if not all(isinstance(t, torch.Tensor) and t.is_cuda for t in tensors) or adj.diag is not None or isinstance(adj, DroppedAdjacency):
        return _ngcf_composed(adj, X, W1, b1, W2, b2, activation, dropout, bool(normalize))
    dropout = _dropout_triple(dropout, "ngcf_step")
    if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
        return _NGCFStep.apply(X, W1, b1, W2, b2, adj, activation, dropout, bool(normalize), backward, wide, wide_backward)
    how = dict() if wide == "composed" else dict(wide=wide)
    return _ngcf_launch(adj, X, W1, b1, W2, b2, activation, keep=False, dropout=dropout, normalize=bool(normalize), **how)[0]


GCNII_SPECTRALS = ("composed", "fused")


def _gate_words(C: int) -> int:
    """Words per row of the spectral layer's gate bits (include/gnx.h: bit c & 31 of word row * ceil(C / 32) + (c >> 5))."""
    return (C + 31) // 32


def _gcnii_spectral_launch(adj: Adjacency, H, H0, a, M, bias, relu, keep, dropout=None):
    """gnx_gcnii_step_spectral; returns (out, T, gate).  ``keep`` (training): the launch also writes the undropped mixed rows T and, with
    ``relu``, the gate words (int32 [n, ceil(C / 32)]: one bit per element, P' > 0); both None otherwise, except that the widths
    other than 16 / 32 / 64 pass their mixed rows through memory in any case.  ``dropout`` = the checked (p, seed, stream) or None."""
    nat.require_cuda(H, H0, M, bias)
    H, H0, M = _as_f32_rows(H).contiguous(), _as_f32_rows(H0).contiguous(), _as_f32_rows(M)
    g, C = _gcnii_operands("gcnii_step_spectral", adj, H, (H0,), M, "the fused spectral layer")
    b = bias.to(torch.float32).reshape(-1).contiguous()
    if b.numel() != C or b.device != H.device:
        raise Exception("gcnii_step_spectral: the bias must hold one value per column, on the rows' device")
    out = torch.empty_like(H)
    mixed = torch.empty_like(H) if keep or C not in GCNII_FUSED_WIDTHS else None
    gate = torch.empty((H.shape[0], _gate_words(C)), dtype=torch.int32, device=H.device) if keep and relu else None
    p, seed, stream = _dropout_args(dropout)
    nat.launch(H.device, "gnx_gcnii_step_spectral", g.handle, adj.vals, H, H0, a, C, M, M.stride(0), b, nat.ACT_RELU if relu else nat.ACT_NONE,
               p, seed, stream, out, mixed, gate)
    return out, mixed if keep else None, gate


def _gcnii_spectral_gate(graph: DeviceGraph, g, gate, relu, dropout=None, padded=False):
    """gnx_gcnii_spectral_back: (G', dbias) from the upstream gradient ``g``, the forward's gate words and its dropout triple:
    u = 2 drop(g), G' = gate ? u : 0, dbias[c] = -sum_i (gate ? 0 : u[i, c]); without ``relu`` G' = u and dbias = 0.
    ``padded``: G' is written into rows of stride roundup4(C) (_padded_rows; the pass takes the stride as its ldG)."""
    g = _as_f32_rows(g).contiguous()
    nat.require_cuda(g, gate)
    _same_device(graph, g, gate)
    n, C = g.shape
    if relu and (gate is None or gate.dtype != torch.int32 or tuple(gate.shape) != (n, _gate_words(C)) or not gate.is_contiguous()):
        raise Exception("gcnii_step_spectral: the gate words must be a contiguous int32 [n, ceil(C / 32)]")
    G = _padded_rows(n, C, g.device) if padded else torch.empty_like(g)
    dbias = torch.empty(C, dtype=torch.float32, device=g.device)
    if C == 0:
        return G, dbias
    slabs = max(1, min(2048, (n + 255) // 256))                      # include/gnx.h: a function of n alone
    work = torch.empty(slabs * C, dtype=torch.float32, device=g.device) if relu else None
    p, seed, stream = _dropout_args(dropout)
    nat.launch(g.device, "gnx_gcnii_spectral_back", graph.handle, g, g.stride(0), gate if relu else None, n, C,
               nat.ACT_RELU if relu else nat.ACT_NONE, p, seed, stream, G, G.stride(0), dbias, work, 0 if work is None else work.numel())
    return G, dbias


class _GCNIISpectralStep(torch.autograd.Function):
    """out = 2 drop(act(T . M + bias) - bias), T = (A . H)(1-a) + H0 a, as ONE launch (gnx_gcnii_step_spectral) that leaves T and one
    gate bit per element (P' > 0) for the backward: (T, M, gate) is all that is saved -- neither act(P') nor out.  backward: the gate
    pass (gnx_gcnii_spectral_back: u = 2 drop(g), G' = gate ? u : 0, dbias = -sum of the gated-off u), dM = T^T G' (gnx_dense_wgrad),
    then dH and dH0 from G' as in _GCNIIStep: composed (gnx_dense + the transposed SpMM) or ``backward="fused"`` (gcnii_step_back)."""

    @staticmethod
    def forward(ctx, H, H0, M, bias, adj, a, relu, backward, dropout):
        ctx.adj, ctx.a, ctx.relu, ctx.fused_backward, ctx.dropout, ctx.bias_shape = adj, a, relu, backward == "fused", dropout, tuple(bias.shape)
        out, T, gate = _gcnii_spectral_launch(adj, H, H0, a, M, bias, relu, keep=True, dropout=dropout)
        ctx.save_for_backward(T, M, gate)
        return out

    @staticmethod
    def backward(ctx, g):
        T, M, gate = ctx.saved_tensors
        G, gbias = _gcnii_spectral_gate(ctx.adj.graph, g, gate, ctx.relu, ctx.dropout)
        gM = _dense_wgrad(T, G) if ctx.needs_input_grad[2] else None
        gH, gH0 = _gcnii_input_grads(ctx.adj, G, ctx.a, M, ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.fused_backward)
        gbias = gbias.reshape(ctx.bias_shape) if ctx.needs_input_grad[3] else None
        return gH, gH0, gM, gbias, None, None, None, None, None


def _spectral_composed(adj, H, H0, a, M, bias, relu, dropout):
    """The layer as today's ops: ppr_step, the dense kernel with bias and relu, then torch's elementwise tail (torch's dropout)."""
    return _spectral_tail(_dense_or_torch(ppr_step(adj, H, H0, a), M, bias, relu), bias, dropout)


def gcnii_step_spectral(adj: Adjacency, H: torch.Tensor, H0: torch.Tensor, a: float, M: torch.Tensor, bias: torch.Tensor, relu=True,
                        dropout=None, backward="composed") -> torch.Tensor:
    """GCNIISpectralPreservingLayer (gcn.py:30-51) as one launch (gnx_gcnii_step_spectral; opt-in, GNN(gcnii_spectral="fused")):
    2 * drop(act(T . M + bias) - bias) with T = (A . H)(1-a) + H0 a, M = (1-b) I + b W and ``bias`` [C] / [1, C].  The bias joins the
    product on the matrix cores before the activation; - bias, the mask and the doubling happen as the rows are stored.  C in
    {16, 32, 64} is ONE launch; other widths run the SpMM+mix, the dense kernel and one row pass.
    ``dropout`` = ``(p, seed, stream)`` or None: the mask of ``feature_dropout`` -- the counter RNG of the edge dropout, NOT torch's
    generator: element (i, c) is kept iff hash_u24(seed, stream + counter, i, c, 0) >= int(p * 2^24), kept values times the f32 1 / (1 - p).
    Without autograd nothing but the result is written.  Under autograd it is one node that saves (T, M, gate) -- the mixed rows for
    dM = T^T G', and ONE BIT per element (P' > 0) packed into int32 words [n, ceil(C / 32)] instead of the activated rows, the result and
    a byte mask -- and returns the gradients of H, H0, M and bias: first one gate pass (gnx_gcnii_spectral_back: G' = gate ? 2 drop(g) : 0
    and dbias, a fixed-order sum without atomics), then gnx_dense_wgrad, then by ``backward`` the composed gnx_dense + transposed SpMM or
    ``gcnii_step_back`` (gcnii_step's ``backward``).
    The composed path -- ppr_step, the dense kernel, torch's elementwise tail with TORCH's dropout at rate p -- is kept for a
    DroppedAdjacency, an adjacency with a diagonal, CPU tensors and a rate outside [0, 1).  (``weight_gradient="recomputed"`` is not
    offered: the layer would save its input in place of T, the same 4 bytes per element.)"""
    _one_of("gcnii_step_spectral", "backward", backward, GCNII_BACKWARDS)
    rate = 0.0 if dropout is None else float(dropout[0])
    if (isinstance(adj, DroppedAdjacency) or adj.diag is not None or not (H.is_cuda and H0.is_cuda and M.is_cuda and bias.is_cuda)
            or not 0.0 <= rate < 1.0):
        return _spectral_composed(adj, H, H0, a, M, bias, bool(relu), dropout)
    dropout = _dropout_triple(dropout, "gcnii_step_spectral")
    if torch.is_grad_enabled() and (H.requires_grad or H0.requires_grad or M.requires_grad or bias.requires_grad):
        return _GCNIISpectralStep.apply(H, H0, M, bias, adj, float(a), bool(relu), backward, dropout)
    return _gcnii_spectral_launch(adj, H, H0, a, M, bias, bool(relu), keep=False, dropout=dropout)[0]


GCN_SPECTRALS = ("composed", "fused")


class _GCNSpectralStep(torch.autograd.Function):
    """out = 2 drop(act((A . X) . W + bias) - bias) as ONE launch (gnx_step_spectral_gcn; under ``fused_edge`` gnx_step_spectral_gcn_dropped)
    that leaves agg = A . X and one gate bit per element (P' > 0) for the backward: (agg, W, gate) is all that is saved -- neither
    act(P') nor out nor a byte mask.  backward: the gate pass (gnx_gcnii_spectral_back at width C_out: u = 2 drop(g), G' = gate ? u : 0,
    dbias = -sum of the gated-off u), dW = agg^T G' (gnx_dense_wgrad), then dX from G' as in _GCNStep: composed (gnx_dense + the
    transposed SpMM) or ``backward="fused"`` -- the gate pass writes G' into rows of stride roundup4(C_out), dX = (A^T G') W^T is ONE launch
    (gcn_step_back), and the node keeps agg itself (``ctx.agg``; (W, gate) are what is saved), lets it go once dW is made, before dX is
    allocated, and therefore runs its backward once."""

    @staticmethod
    def forward(ctx, X, W, bias, adj, relu, dropout, fused_edge, backward):
        return _gcn_node_forward(ctx, X, W, bias, adj, relu, dropout, fused_edge, backward, spectral=True)

    @staticmethod
    def backward(ctx, g):
        return _gcn_node_backward(ctx, g) + (None, None, None, None, None)


def _gcn_spectral_composed(adj, X, W, bias, relu, dropout):
    """The layer as today's ops (_gcn_composed's shape): spmm, the dense kernel with bias and relu (CPU tensors: torch), then torch's
    elementwise tail with TORCH's dropout."""
    return _spectral_tail(_dense_or_torch(spmm(adj, X), W, bias, relu), bias if bias is not None else 0, dropout)


def gcn_step_spectral(adj: Adjacency, X: torch.Tensor, W: torch.Tensor, bias=None, relu=True, dropout=None, edge_dropout="composed",
                      backward="composed") -> torch.Tensor:
    """GCNSpectralPreservingLayer (gcn.py:92-105) as one launch (gnx_step_spectral_gcn; opt-in, GNN(gcn_spectral="fused")):
    2 * drop(act((A . X) . W + bias) - bias) with ``X`` [n, C_in], ``W`` [C_in, C_out] and ``bias`` [C_out] / [1, C_out] or None (zeros).
    For C_in in {16, 32, 64} and C_out <= C_in the aggregated rows stay in LDS and meet W on the matrix cores, the bias joins the
    product there before the activation, and - bias, the mask and the doubling happen as the rows are stored; other widths run the
    SpMM, the dense kernel and one row pass inside the same call.
    ``dropout`` = ``(p, seed, stream)`` or None: the mask of ``feature_dropout`` -- the counter RNG of the edge dropout, NOT torch's
    generator: element (i, c) is kept iff hash_u24(seed, stream + counter, i, c, 0) >= int(p * 2^24), kept values times the f32 1 / (1 - p).
    Without autograd nothing but the result is written.  Under autograd it is one node that saves (A . X, W, gate) -- the aggregated rows
    for dW, and ONE BIT per element (P' > 0) packed into int32 words [n, ceil(C_out / 32)] instead of the activated rows, the result
    and a byte mask -- and returns the gradients of X, W and bias: one gate pass (gnx_gcnii_spectral_back: G' = gate ? 2 drop(g) : 0
    and dbias, a fixed-order sum without atomics), gnx_dense_wgrad, then dX by ``backward`` exactly as in ``gcn_step``: ``"composed"``
    (gnx_dense + the transposed SpMM) or ``"fused"`` (G' in rows of stride roundup4(C_out), ONE launch gcn_step_back, A . X let go once
    dW is made: such a node runs its backward once).
    ``edge_dropout="fused"`` with a DroppedAdjacency: gnx_step_spectral_gcn_dropped makes every entry's weight in its gather loop -- bit
    for bit the result over ``normalize(graph, "symmetric", "none", p, seed, stream)`` -- and the backward's transposed SpMM is the
    dropped one.
    CPU tensors, an adjacency with a diagonal, a DroppedAdjacency without ``edge_dropout="fused"`` and a rate outside [0, 1) run
    ``spmm`` + ``dense`` and torch's elementwise tail with TORCH's dropout: today's calls and bits."""
    fused_edge = _edge_dropout("gcn_step_spectral", edge_dropout)
    _one_of("gcn_step_spectral", "backward", backward, GCN_BACKWARDS)
    tensors = (X, W) if bias is None else (X, W, bias)
    rate = 0.0 if dropout is None else float(dropout[0])
    if (not all(isinstance(t, torch.Tensor) and t.is_cuda for t in tensors) or adj.diag is not None
            or (isinstance(adj, DroppedAdjacency) and not fused_edge) or not 0.0 <= rate < 1.0):
        return _gcn_spectral_composed(adj, X, W, bias, bool(relu), dropout)
    dropout = _dropout_triple(dropout, "gcn_step_spectral")
    fused_edge = fused_edge and isinstance(adj, DroppedAdjacency)
    if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
        return _GCNSpectralStep.apply(X, W, bias, adj, bool(relu), dropout, fused_edge, backward)
    return _gcn_launch(adj, X, W, bias, bool(relu), keep_agg=False, dropout=dropout, fused_edge=fused_edge, spectral=True)[0]


# the model-level bf16 path of GCNIILayer (graph_model.py) keeps f32 below this width.  tools/gcnii_bf16_bench.py is the measurement
# it is to be set from (profiles/NOTES.md "bf16 storage in the GCNII layer": no table recorded yet); until then it stands where the
# plain SpMM's measurements put it: up to 32 columns a gathered row is one 128-byte line in either format (a wash at C = 17 ... 32,
# a loss at C <= 16).  The C entry and gcnii_step(storage=) themselves are not gated.
GCNII_BF16_MIN_WIDTH = 33
GCNII_BF16_MAX_WIDTH = 256      # a bf16 result of gnx_gcnii_step_bf16 is one column panel of the dense kernel


def _gcnii_launch_bf16(adj: Adjacency, H, H0, a, M, relu, out_bf16, out=None, work=None):
    """gnx_gcnii_step_bf16.  ``out`` / ``work``: buffers a stack of layers shares (contiguous [n, C]: bf16 or f32 / f32)."""
    nat.require_cuda(H)
    if H.dim() != 2:
        raise Exception("gcnii_step: shape mismatch")
    Hb = (H if H.is_contiguous() else H.contiguous()) if H.dtype == torch.bfloat16 else to_bf16(H)
    H0, M = _as_f32_rows(H0).contiguous(), _as_f32_rows(M)
    g, C = _gcnii_operands("gcnii_step", adj, Hb, (H0,), M)
    if out_bf16 and C > GCNII_BF16_MAX_WIDTH:                       # wider than one panel: the f32 result, rounded by gnx_cast_bf16
        return to_bf16(_gcnii_launch_bf16(adj, Hb, H0, a, M, relu, False, work=work))
    want = torch.bfloat16 if out_bf16 else torch.float32
    if out is None:
        out = torch.empty(Hb.shape, dtype=want, device=Hb.device)
    if work is None:
        work = torch.empty(Hb.shape, dtype=torch.float32, device=Hb.device)
    if out.dtype != want or tuple(out.shape) != tuple(Hb.shape) or not out.is_contiguous() or work.dtype != torch.float32 \
            or tuple(work.shape) != tuple(Hb.shape) or not work.is_contiguous() or out.device != Hb.device or work.device != Hb.device:
        raise Exception("gcnii_step: bad output / work buffer")
    nat.launch(Hb.device, "gnx_gcnii_step_bf16", g.handle, adj.vals, Hb, H0, a, C, M, M.stride(0), nat.ACT_RELU if relu else nat.ACT_NONE, out,
               out_bf16, work)
    return out


def gcnii_chain_bf16(adj: Adjacency, H: torch.Tensor, steps, widen_last=False) -> torch.Tensor:
    """A stack of GCNII layers with the rows handed from layer to layer stored as bf16 (inference only).  ``steps``: per layer
    (H0, a, M, relu).  The input is rounded once (a bf16 H is used as it is), every layer but the last stores bf(out), the last one
    f32 -- bit for bit gcnii_step(storage=bf16, out_storage=bf16 ... f32) layer by layer; H0 stays f32.  One f32 work buffer and two
    bf16 buffers serve the whole stack.  ``widen_last``: the last layer stores bf16 too and the exact widening of that row is returned
    (the value an INNER layer of a longer stack hands on)."""
    steps = list(steps)
    _no_grad_for_bf16("gcnii_chain_bf16", H, *[t for H0, _, M, _ in steps for t in (H0, M)])
    if not steps:
        raise Exception("gcnii_chain_bf16: no layers")
    X = H if H.dtype == torch.bfloat16 else to_bf16(H)
    work = torch.empty(X.shape, dtype=torch.float32, device=X.device)
    ping = [torch.empty(X.shape, dtype=torch.bfloat16, device=X.device) for _ in range(min(2, len(steps) - (0 if widen_last else 1)))]
    for k, (H0, a, M, relu) in enumerate(steps):
        last = k == len(steps) - 1 and not widen_last
        X = _gcnii_launch_bf16(adj, X, H0, a, M, relu, not last, out=None if last else ping[k % 2], work=work)
    return X.float() if widen_last else X


# ---- bf16 row storage for GCNII training (opt-in): gnx_gcnii_step_train_bf16, gnx_feature_dropout_back_bf16, gnx_gcnii_step_back_bf16 ----
# the model-level path (GCNIILayer.__run__, GNN(gcnii_training_dtype=torch.bfloat16)) keeps f32 below this width and on graphs of fewer
# rows: the allowance, set from tools/gcnii_bf16_train_bench.py (profiles/NOTES.md "bf16 storage in GCNII training"; the training step of
# an 8-layer stack, f32 "fused" against bf16 interleaved): a width / graph size gets bf16 only where its step measured faster with the
# quartile ranges apart.  At 10^7 vertices / 10^8 entries C = 32 and C = 64 gain 1.04 x and C = 16 loses 9 %; at 10^6 vertices every
# width loses 4 - 8 %, on the Cora-shaped graph 1 - 4 %; nothing between 10^6 and 10^7 was measured, so the smallest size that measured a
# gain is the threshold.  The functions below are not gated.
GCNII_BF16_TRAIN_MIN_WIDTH = 32
GCNII_BF16_TRAIN_MIN_ROWS = 10_000_000
GCNII_BF16_TRAIN_WIDTHS = (16, 32, 64)


def _gcnii_bf16_operands(what, adj, rows, *f32):
    """_gcnii_operands as the bf16 training pieces call it (the name it had while only they used it): a constant adjacency."""
    return _gcnii_operands(what, adj, rows, f32, None, "bf16 training storage")


def gcnii_step_train_bf16(adj: Adjacency, Hb: torch.Tensor, H0: torch.Tensor, a: float, M: torch.Tensor, relu=True, dropout=None,
                          out_bf16=True, work=None, keep_mixed=True):
    """The training forward of one GCNII layer over bf16 gathered rows (gnx_gcnii_step_train_bf16; no autograd): returns (out, T) with
    T = (1-a) A.H~ + a H0 in f32, undropped, and out = drop(act(T . M)) as bf16 (``out_bf16``) or f32.  ``Hb``: bf16 [n, C] contiguous,
    C in {16, 32, 64}; ``dropout`` = (p, seed, stream) or None; ``work``: an f32 [n, C] buffer a run of layers shares (graphs with hub
    rows need one; None allocates it).  ``keep_mixed=False``: T is not written (gnx_gcnii_step_drop_bf16: the layer's weight gradient
    makes it again, gcnii_wgrad) and (out, None) is returned, out with the same bits; ``work`` is then allocated only for hub rows."""
    H0, M = _as_f32_rows(H0).contiguous(), _as_f32_rows(M)
    g, C = _gcnii_operands("gcnii_step_train_bf16", adj, Hb, (H0, work), M, "bf16 training storage")
    if Hb.dtype != torch.bfloat16 or not Hb.is_contiguous():
        raise Exception("gcnii_step_train_bf16: needs contiguous bf16 rows [n, C] and M [C, C]")
    p, seed, stream = _dropout_triple(dropout, "gcnii_step_train_bf16") or (0.0, 0, 0)
    out = torch.empty(Hb.shape, dtype=torch.bfloat16 if out_bf16 else torch.float32, device=Hb.device)
    T = torch.empty(Hb.shape, dtype=torch.float32, device=Hb.device) if keep_mixed else None
    if work is None and (keep_mixed or g.n_hub_rows > 0):
        work = torch.empty(Hb.shape, dtype=torch.float32, device=Hb.device)
    layer = (g.handle, adj.vals, Hb, H0, a, C, M, M.stride(0), nat.ACT_RELU if relu else nat.ACT_NONE, p, seed, stream, out, out_bf16)
    if keep_mixed:
        nat.launch(Hb.device, "gnx_gcnii_step_train_bf16", *layer, T, work)
    else:
        nat.launch(Hb.device, "gnx_gcnii_step_drop_bf16", *layer, work)
    return out, T


def feature_dropout_back_bf16(graph: DeviceGraph, g: torch.Tensor, yb, dropout=None, relu=True):
    """The backward's gate over the STORED bf16 output ``yb`` of a layer (gnx_feature_dropout_back_bf16): returns (G, Gb) with
    G = kept ? g * s : 0 in f32 -- with ``relu`` also 0 where the stored y <= 0 -- and Gb = bf(G).  ``dropout`` = (p, seed, stream) or
    None (the relu gate plus the cast); any width."""
    nat.require_cuda(g, yb)
    if relu and (yb is None or yb.dtype != torch.bfloat16 or tuple(yb.shape) != tuple(g.shape) or not yb.is_contiguous()):
        raise Exception("feature_dropout_back_bf16: relu needs the stored bf16 output, contiguous, in the gradient's shape")
    return _gate_launch(graph, g, yb, *(_dropout_triple(dropout, "feature_dropout_back_bf16") or (0.0, 0, 0)), relu, bf16=True)


def gcnii_step_back_bf16(adj: Adjacency, Gb: torch.Tensor, G, a: float, Mt: torch.Tensor, S_in=None, s_alpha=1.0, want_S=True, in_place=False):
    """gcnii_step_back with the gathered operand in bf16 (gnx_gcnii_step_back_bf16; no autograd): dH = ((1-a) A^T Gb~) . Mt in f32 and
    S = s_alpha S_in + (a G) . Mt from the f32 ``G`` (None with ``want_S=False``).  Returns (dH, S); ``in_place``: S is S_in itself."""
    return _gcnii_back_launch(True, adj, Gb, G, a, Mt, S_in, s_alpha, want_S, in_place)


class _GCNIITrainRunBf16(torch.autograd.Function):
    """A run of GCNII training layers over bf16 rows as ONE autograd node (as _PPRLoop is for K iterations).  forward: the f32 input is
    rounded once, layer l gathers the stored rows of layer l - 1, every layer but the last stores bf(out), the last f32; saved per layer:
    the f32 T and the stored out.  backward, last layer first: the gate (G, Gb) -> dM = T^T G (gnx_dense_wgrad, f32) -> one launch for
    dH (the next upstream gradient) and the layer's term of dH0; consecutive layers that share one H0 tensor add their terms into one
    running sum (S_in = S_out, s_alpha = 1), another H0 starts a new sum.  Tensor arguments: H, then (H0, M) per layer.
    ``recompute``: no T is written or saved -- per layer (M, stored out) only, beside the run's input and the H0 tensors, which their
    producers hold anyway -- and dM comes from gcnii_wgrad over the rows the layer gathered: layer k - 1's stored out, and for the first
    layer the input rounded again (the same bits; a saved copy would cost the run 2 bytes per element).  One hub-row scratch serves
    the whole backward."""

    @staticmethod
    def forward(ctx, adj, meta, same_H0, stored, recompute, H, *tensors):
        X = to_bf16(H)
        hubs = adj.graph.n_hub_rows > 0
        work = torch.empty(H.shape, dtype=torch.float32, device=H.device) if hubs or not recompute else None
        saved, n = [], len(meta)
        for k, (a, relu, dropout) in enumerate(meta):
            H0, M = tensors[2 * k], tensors[2 * k + 1]
            X, T = gcnii_step_train_bf16(adj, X, H0, a, M, relu, dropout, out_bf16=k < n - 1, work=work, keep_mixed=not recompute)
            saved += [M, X] if recompute else [T, M, X]
            if stored is not None and k < n - 1:
                stored.append(X)
        ctx.adj, ctx.meta, ctx.same_H0, ctx.recompute = adj, meta, same_H0, recompute
        if recompute:
            saved = [H] + [tensors[2 * k] for k in range(n)] + saved
        ctx.save_for_backward(*saved)
        return X

    @staticmethod
    def backward(ctx, g):
        adj, meta, saved = ctx.adj, ctx.meta, ctx.saved_tensors
        n = len(meta)
        need = ctx.needs_input_grad[6:]
        grads = [None] * (2 * n)
        S = None                                                    # the running dH0 sum of the layers k .. that share one H0
        if ctx.recompute:
            H, H0s, saved = saved[0], saved[1:n + 1], saved[n + 1:]
            hub = torch.empty(H.shape, dtype=torch.float32, device=H.device) if adj.graph.n_hub_rows > 0 else None
        for k in range(n - 1, -1, -1):
            a, relu, dropout = meta[k]
            if ctx.recompute:
                M, out = saved[2 * k:2 * k + 2]
            else:
                T, M, out = saved[3 * k:3 * k + 3]
            if k == n - 1:                                          # the run's f32 output: the existing gate, then the cast
                G = _feature_dropout_back(adj.graph, g, out, *(dropout or (0.0, 0, 0)), relu=relu)
                Gb = to_bf16(G)
            else:
                G, Gb = feature_dropout_back_bf16(adj.graph, g, out, dropout, relu)
            if need[2 * k + 1] and ctx.recompute:                   # the rows layer k gathered: layer k - 1's stored out / the rounded input
                grads[2 * k + 1] = gcnii_wgrad(adj, saved[2 * k - 1] if k > 0 else to_bf16(H), H0s[k], a, G, hub_rows=hub)
            elif need[2 * k + 1]:
                grads[2 * k + 1] = _dense_wgrad(T, G)
            want_S = need[2 * k]
            continues = want_S and S is not None                    # (S is not None: layer k + 1 shares this layer's H0 and wanted its sum)
            g, S = gcnii_step_back_bf16(adj, Gb, G if want_S else None, a, M.t().contiguous(), S_in=S if continues else None,
                                        want_S=want_S, in_place=continues)
            if not ctx.same_H0[k]:                                  # the sum ends with the first layer of its H0: one gradient per sum
                grads[2 * k], S = S, None
        return (None, None, None, None, None, g if ctx.needs_input_grad[5] else None) + tuple(grads)


def gcnii_train_run_bf16(adj: Adjacency, H: torch.Tensor, steps, stored=None, weight_gradient="stored") -> torch.Tensor:
    """A run of GCNII layers in TRAINING with the rows handed from layer to layer -- and the gated gradient on the way back -- stored as
    bf16 (opt-in; one autograd node for the whole run).  ``steps``: per layer (H0, a, M, relu, dropout) with dropout = (p, seed, stream)
    of the fused feature dropout or None.  The run's f32 input is rounded once (its gradient passes straight through), every layer but
    the last stores bf(out), the last writes f32; sums, H0, T, the mix, the transform, dM and the running dH0 sums stay f32.  Widths 16,
    32 and 64 on a constant square adjacency without a diagonal; device tensors.  ``stored``: a list that receives the bf16 rows of
    every layer but the last (what an inner layer's ``.value`` widens).  The backward is the fused one (gcnii_step_back_bf16).
    ``weight_gradient="recomputed"`` (opt-in): the forward goes through gnx_gcnii_step_drop_bf16, which writes no T; a layer then saves
    its M and its stored out alone -- 2 bytes per element for an inner layer instead of 6 -- and its dM comes from gnx_gcnii_wgrad_bf16
    over the rows it gathered (``gcnii_wgrad``).  The run's output, dH, dH0 and the input's gradient keep their bits; every dM agrees
    to float32 rounding."""
    recompute = _weight_gradient("gcnii_train_run_bf16", weight_gradient)
    steps = [(H0, float(a), M, bool(relu), _dropout_triple(dropout, "gcnii_train_run_bf16")) for H0, a, M, relu, dropout in steps]
    if not steps:
        raise Exception("gcnii_train_run_bf16: no layers")
    g, C = _gcnii_bf16_operands("gcnii_train_run_bf16", adj, H, *[H0 for H0, *_ in steps])
    if H.dtype != torch.float32 or C not in GCNII_BF16_TRAIN_WIDTHS:
        raise Exception("gcnii_train_run_bf16: needs f32 rows of width 16, 32 or 64")
    tensors = [t for H0, _, M, _, _ in steps for t in (H0, M)]
    same_H0 = tuple(k > 0 and steps[k][0] is steps[k - 1][0] for k in range(len(steps)))          # layer k shares its H0 tensor with layer k - 1
    return _GCNIITrainRunBf16.apply(adj, tuple((a, relu, dropout) for _, a, _, relu, dropout in steps), same_H0, stored, recompute,
                                    H.contiguous(), *tensors)


class DeviceIndex:
    """Node ids / labels / edges of a task, checked ONCE on the host (range) and kept on the device: a task evaluates the same
    index lists every epoch, and on small graphs an upload + a device-side check per call would dominate the epoch.
    The kernels themselves never dereference an out-of-range id (NaN / -1 instead); device tensors handed in directly skip the
    host check."""

    def __init__(self, values, device, upper=None, what="node id", fixed=True):
        """``fixed=False``: the tensor is a buffer that its owner rewrites between uses (device_negative_sampling); nothing derived
        from its contents -- the plan of the sorted edge-score backward -- is then kept."""
        if isinstance(values, torch.Tensor):
            self.tensor = values.to(device=device, dtype=torch.int64).contiguous()
        else:
            host = np.ascontiguousarray(np.asarray(values, dtype=np.int64))
            if upper is not None and host.size and (int(host.min()) < 0 or int(host.max()) >= upper):
                raise Exception(f"{what} out of range [0, {upper})")
            self.tensor = torch.from_numpy(host).to(device)
        self.upper, self.fixed = upper, bool(fixed)
        self._edge_plan = None                  # (n_rows, EdgePlan) of a fixed edge list: edge_scores(backward="sorted") sorts it once

    def __len__(self):
        return self.tensor.shape[0]


def _as_index(x, device, upper, what):
    if isinstance(x, DeviceIndex):
        if x.tensor.device != device or (x.upper is not None and upper is not None and x.upper != upper):
            raise Exception("DeviceIndex built for another device / size")
        return x.tensor
    return DeviceIndex(x, device, upper, what).tensor


class _NodeCE(torch.autograd.Function):
    """mean_i CE(log_softmax(logits[nodes_i]), labels_i) fused over the listed nodes (graph_predictor.py:19-25)."""

    @staticmethod
    def forward(ctx, logits, nodes, labels):
        logits = _as_f32_rows(logits)
        m = nodes.numel()
        per_node = torch.empty(m + 256, dtype=torch.float32, device=logits.device)       # + scratch of the two-level mean
        mean = torch.empty(1, dtype=torch.float32, device=logits.device)
        nat.launch(logits.device, "gnx_node_ce", logits, logits.stride(0), logits.shape[0], logits.shape[1], nodes, labels, m, per_node, mean)
        ctx.save_for_backward(logits, nodes, labels)
        return mean.reshape(())

    @staticmethod
    def backward(ctx, g):
        logits, nodes, labels = ctx.saved_tensors
        grad = torch.zeros((logits.shape[0], logits.shape[1]), dtype=torch.float32, device=logits.device)
        g = g.to(torch.float32).reshape(1).contiguous()
        nat.launch(logits.device, "gnx_node_ce_backward", logits, logits.stride(0), logits.shape[0], logits.shape[1], nodes, labels, nodes.numel(),
                   g, grad, grad.stride(0))
        return grad, None, None


def node_ce(logits: torch.Tensor, nodes, labels) -> torch.Tensor:
    """The NodeClassification loss on the device in two small launches (gather + log-softmax + CE, then the mean).
    ``nodes`` / ``labels``: host sequences (range-checked here), DeviceIndex objects (checked when built) or device tensors."""
    nat.require_cuda(logits)
    nodes = _as_index(nodes, logits.device, logits.shape[0], "node id")
    labels = _as_index(labels, logits.device, logits.shape[1], "label")
    if nodes.numel() != labels.numel() or nodes.numel() == 0:
        raise Exception("node_ce: nodes and labels must be equally long and non-empty")
    return _NodeCE.apply(logits, nodes, labels)


def node_argmax(logits: torch.Tensor, nodes=None) -> torch.Tensor:
    """argmax over the rows of ``nodes`` (all rows when None) in one launch; ties go to the lowest class."""
    nat.require_cuda(logits)
    logits = _as_f32_rows(logits.detach())
    idx = None if nodes is None else _as_index(nodes, logits.device, logits.shape[0], "node id")
    m = logits.shape[0] if idx is None else idx.numel()
    out = torch.empty(m, dtype=torch.int64, device=logits.device)
    nat.launch(logits.device, "gnx_node_argmax", logits, logits.stride(0), logits.shape[0], logits.shape[1], idx, m, out)
    return out


# ---- sparse input features: the first Dense of the pre-MLP as an SpMM over the rows of W ---------------------------------
class SparseRows:
    """A feature matrix that is mostly zeros (Cora: 1433 columns, 1.3 % non-zero), held as a device CSR.  It flows through
    the layer stack in place of the dense tensor until the first Dense consumes it: Dropout on it drops stored entries
    (tf.nn.dropout leaves zeros zero, layers.py:180-181), Dense on it is X . W computed as an SpMM whose "dense operand" is
    W -- 4F bytes of X per row become 8 bytes per stored entry, and W (F x 64 floats) stays cache resident."""

    def __init__(self, graph: DeviceGraph, dropout=0.0, seed=0, stream_id=0):
        self.graph, self.p, self.seed, self.stream_id = graph, float(dropout), int(seed), int(stream_id)
        self.shape = (graph.n_rows, graph.n_cols)

    @classmethod
    def from_dense(cls, X: torch.Tensor):
        idx = torch.nonzero(X)
        return cls(DeviceGraph(SparseCOO(idx, X[idx[:, 0], idx[:, 1]], tuple(X.shape)), device=X.device))

    def with_dropout(self, p, seed, stream_id):
        if self.p != 0:
            raise Exception("SparseRows: dropout applied twice before a Dense layer")
        return SparseRows(self.graph, p, seed, stream_id)

    def adjacency(self) -> Adjacency:
        """The stored values (dropped per entry and rescaled while a dropout is pending) as an Adjacency over X."""
        if self.p == 0:
            return Adjacency(self.graph, None)
        return normalize(self.graph, "none", "none", self.p, self.seed, self.stream_id)


class _SparseDense(torch.autograd.Function):
    """out = act(X . W + b), X sparse: forward = fused SpMM (bias through the H0 operand, relu in the epilogue);
    backward dW = X^T . g' = the transposed SpMM; X is an input and gets no gradient."""

    @staticmethod
    def forward(ctx, W, bias, adj, relu):
        out = _launch(adj, W, bias, 1.0, 1.0, nat.ACT_RELU if relu else nat.ACT_NONE)
        ctx.adj, ctx.relu, ctx.has_bias = adj, relu, bias is not None
        ctx.save_for_backward(out if relu else None)
        return out

    @staticmethod
    def backward(ctx, g):
        (out,) = ctx.saved_tensors
        g = (_relu_mask(g, out) if ctx.relu else g).contiguous()
        gW = _launch(ctx.adj, g, None, 1.0, 0.0, nat.ACT_NONE, transposed=True) if ctx.needs_input_grad[0] else None
        gb = g.sum(dim=0, keepdim=True) if ctx.has_bias and ctx.needs_input_grad[1] else None
        return gW, gb, None, None


def sparse_dense(rows: SparseRows, W: torch.Tensor, bias=None, relu=False) -> torch.Tensor:
    """act(X . W + bias) for sparse X (``bias`` [1, O] or None)."""
    return _SparseDense.apply(W, bias, rows.adjacency(), bool(relu))


# ---- link head: the logit of every listed edge in one launch -------------------------------------------------------------
class _EdgeScores(torch.autograd.Function):
    """logit_i = sum_c F[u_i, c] F[v_i, c] (r[c] or 1)  (graph_predictor.py:122-126); backward scatters into dF with atomics;
    the DistMult weights' gradient (C numbers) is a reduction over the edges, done with torch on the gathered rows."""

    @staticmethod
    def forward(ctx, F, edges, r):
        F = _as_f32_rows(F)
        rr = None if r is None else r.to(torch.float32).reshape(-1).contiguous()
        out = torch.empty(edges.shape[0], dtype=torch.float32, device=F.device)
        nat.launch(F.device, "gnx_edge_scores", F, F.stride(0), F.shape[0], F.shape[1], edges, edges.shape[0], rr, out)
        ctx.save_for_backward(F, edges, rr)
        ctx.r_shape = None if r is None else tuple(r.shape)
        return out

    @staticmethod
    def backward(ctx, g):
        F, edges, rr = ctx.saved_tensors
        g = g.to(torch.float32).contiguous()
        gF = gr = None
        if ctx.needs_input_grad[0]:
            gF = torch.zeros((F.shape[0], F.shape[1]), dtype=torch.float32, device=F.device)
            nat.launch(F.device, "gnx_edge_scores_backward", F, F.stride(0), F.shape[0], F.shape[1], edges, edges.shape[0], rr, g, gF, gF.stride(0))
        if rr is not None and ctx.needs_input_grad[2]:
            gr = (g[:, None] * F[edges[:, 0]] * F[edges[:, 1]]).sum(0).reshape(ctx.r_shape)
        return gF, None, gr


class EdgePlan:
    """gnx_edge_plan of one [m, 2] edge list over ``n_rows`` nodes: the positions of the flattened list stably sorted by the node they
    name (keys, pos) and the sorted index at which every chunk of 256 positions of a node begins (chunks[0] = their number)."""

    _bytes = dict()                             # gnx_edge_plan_bytes by m (a host query; the same for every list of that length)

    def __init__(self, edges: torch.Tensor, n_rows: int):
        m = edges.shape[0]
        self.m, self.n_rows = m, int(n_rows)
        self.keys = torch.empty(2 * m, dtype=torch.int32, device=edges.device)              # uint32 in the library
        self.pos = torch.empty(2 * m, dtype=torch.int32, device=edges.device)
        self.chunks = torch.empty(2 * m + 1, dtype=torch.int32, device=edges.device)
        if m not in EdgePlan._bytes:
            EdgePlan._bytes[m] = int(nat.lib().gnx_edge_plan_bytes(m))
            if EdgePlan._bytes[m] < 0:
                del EdgePlan._bytes[m]
                nat.check(-1)
        workspace = torch.empty(max(EdgePlan._bytes[m], 16), dtype=torch.uint8, device=edges.device)
        nat.launch(edges.device, "gnx_edge_plan", edges, m, self.n_rows, self.keys, self.pos, self.chunks, workspace, workspace.numel())


def _edge_plan_of(index, edges: torch.Tensor, n_rows: int) -> EdgePlan:
    """The plan of ``edges``: kept on ``index`` when that is a DeviceIndex over a fixed list, built anew otherwise."""
    if not (isinstance(index, DeviceIndex) and index.fixed):
        return EdgePlan(edges, n_rows)
    if index._edge_plan is None or index._edge_plan[0] != n_rows:
        index._edge_plan = (n_rows, EdgePlan(edges, n_rows))
    return index._edge_plan[1]


class _EdgeScoresSorted(torch.autograd.Function):
    """_EdgeScores with the backward of gnx_edge_scores_backward_sorted: every row of dF is summed in the fixed order of the plan
    (made in the forward), so two runs give the same bits."""

    @staticmethod
    def forward(ctx, F, edges, r, index):
        out = _EdgeScores.forward(ctx, F, edges, r)
        ctx.plan = _edge_plan_of(index, edges, F.shape[0]) if ctx.needs_input_grad[0] else None
        return out

    @staticmethod
    def backward(ctx, g):
        F, edges, rr = ctx.saved_tensors
        g = g.to(torch.float32).contiguous()
        gF = gr = None
        if ctx.needs_input_grad[0]:
            m, C, plan = edges.shape[0], F.shape[1], ctx.plan
            gF = torch.zeros((F.shape[0], C), dtype=torch.float32, device=F.device)
            work = torch.empty(max(int(nat.lib().gnx_edge_sorted_work_floats(m, C)), 4), dtype=torch.float32, device=F.device)
            nat.launch(F.device, "gnx_edge_scores_backward_sorted", F, F.stride(0), F.shape[0], C, edges, m, rr, g, gF, gF.stride(0), plan.keys,
                       plan.pos, plan.chunks, work, work.numel())
        if rr is not None and ctx.needs_input_grad[2]:
            gr = (g[:, None] * F[edges[:, 0]] * F[edges[:, 1]]).sum(0).reshape(ctx.r_shape)
        return gF, None, gr, None


def edge_scores(F: torch.Tensor, edges, r=None, backward="atomic") -> torch.Tensor:
    """Logits of the listed edges ([m, 2] node ids): <F[u], F[v]> or, with DistMult weights r [C, 1], <F[u] * F[v], r>.
    ``backward``: "atomic" adds the gradient into the endpoint rows with float atomics (gnx_edge_scores_backward: the sum of a row
    depends on scheduling); "sorted" sorts the endpoints once per call -- once per list for a DeviceIndex over a fixed list -- and sums
    every row in that fixed order (gnx_edge_plan + gnx_edge_scores_backward_sorted)."""
    if backward not in ("atomic", "sorted"):
        raise Exception('edge_scores: backward must be "atomic" or "sorted"')
    nat.require_cuda(F, r)
    e = _as_index(edges, F.device, F.shape[0], "edge endpoint").reshape(-1, 2)
    if backward == "sorted":
        return _EdgeScoresSorted.apply(F, e, r, edges)
    return _EdgeScores.apply(F, e, r)


def sample_negatives(graph: DeviceGraph, positives: torch.Tensor, samples, candidates, seed, stream, out=None, max_tries=32,
                     fallbacks=None) -> torch.Tensor:
    """negative_sampling's draw (graph_predictor.py:52-98) as one launch of gnx_sample_negatives: ``out`` [m (1 + samples), 2] (made when
    None) receives every pair of ``positives`` [m, 2] followed by ``samples`` pairs (u, w), w drawn from ``candidates`` (device ids; None:
    every node of ``graph``) by the counter RNG at (seed, stream + the graph's dropout counter) until it is neither u, v nor linked to u
    in ``graph``, at most ``max_tries`` times.  ``fallbacks``: an int64 device counter of the slots that kept a rejected draw."""
    nat.require_cuda(positives, candidates, out)
    positives = positives.to(torch.int64).reshape(-1, 2).contiguous()
    m, samples = positives.shape[0], int(samples)
    if candidates is not None:
        candidates = candidates.to(torch.int64).reshape(-1).contiguous()
    if samples < 1:
        raise Exception("sample_negatives: samples must be at least 1")
    if out is None:
        out = torch.empty((m * (1 + samples), 2), dtype=torch.int64, device=positives.device)
    if out.dtype != torch.int64 or not out.is_contiguous() or out.numel() != 2 * m * (1 + samples):
        raise Exception("sample_negatives: out must be a contiguous int64 [m (1 + samples), 2] tensor")
    if fallbacks is None:
        fallbacks = torch.zeros(1, dtype=torch.int64, device=positives.device)
    _same_device(graph, positives, candidates, out, fallbacks)
    nat.launch(graph.device, "gnx_sample_negatives", graph.handle, positives, m, samples, candidates,
               graph.n_rows if candidates is None else candidates.numel(), max_tries, seed, stream, out, fallbacks)
    return out


# ---- ranking evaluation: every candidate of every source in one call ------------------------------------------------------
RANK_MAX_K = 32          # GNX_RANK_MAX_K
RANK_POS_PASS = 32       # GNX_RANK_POS_PASS: positive scores of a source the tile kernel keeps in LDS; further ones are read from memory

RankResult = namedtuple("RankResult", "n_pos n_neg less equal top_ids top_scores top_is_pos scores")


def rank_candidates(graph: DeviceGraph, F: torch.Tensor, sources, positives, candidates, k, r=None, scores=False, splits=0) -> RankResult:
    """MeanLinkPrediction.evaluate's ranking (graph_predictor.py:154-203) for all ``sources`` in one call of gnx_rank_candidates: the list
    of a source is its held-out neighbours (``positives`` = (ptr [S + 1], ids [P]), a CSR list, or None) followed by every id of
    ``candidates`` -- STRICTLY ASCENDING -- that is neither the source nor linked to it in ``graph`` in either direction.  Returns device
    tensors: ``n_pos``, ``n_neg`` (-1: the source or one of its held-out ids is out of range), ``less`` / ``equal`` (over the positives,
    the strangers that score below / equal: AUC = (less + equal / 2) / (n_pos n_neg)), and the ``k`` best entries of the list,
    ``top_ids`` (-1 where the list is shorter), ``top_scores`` (-inf there), ``top_is_pos``: higher score first, on a tie the entry later in
    the list.  ``scores=True`` adds the raw [S, K] scores of every in-range pair (cells of out-of-range ids are NaN).  ``r``: DistMult
    weights [C].  ``splits``: candidate parts, 0 = the library's choice; no output depends on it.  Finite ``F`` is a precondition."""
    nat.require_cuda(F, r)
    F = _as_f32_rows(F.detach())
    device = F.device
    sources = _as_index(sources, device, None, "source node").reshape(-1)
    candidates = _as_index(candidates, device, None, "candidate node").reshape(-1)
    S, K, k = sources.numel(), candidates.numel(), int(k)
    if positives is None:
        ptr, ids = torch.zeros(S + 1, dtype=torch.int64, device=device), torch.zeros(0, dtype=torch.int64, device=device)
    else:
        ptr, ids = (_as_index(x, device, None, "held-out node").reshape(-1) for x in positives)
    if ptr.numel() != S + 1:
        raise Exception("rank_candidates: positives = (ptr, ids) needs one more pointer than there are sources")
    if not 1 <= k <= RANK_MAX_K:
        raise Exception(f"rank_candidates: k must be in [1, {RANK_MAX_K}]")
    rr = None if r is None else r.detach().to(torch.float32).reshape(-1).contiguous()
    if rr is not None and rr.numel() != F.shape[1]:
        raise Exception("rank_candidates: r must hold one weight per column of F")
    _same_device(graph, F, rr, sources, ptr, ids, candidates)
    counts = torch.empty((4, S), dtype=torch.int64, device=device)
    top_ids = torch.empty((S, k), dtype=torch.int64, device=device)
    top_scores = torch.empty((S, k), dtype=torch.float32, device=device)
    top_is_pos = torch.empty((S, k), dtype=torch.uint8, device=device)
    raw = torch.full((S, K), float("nan"), dtype=torch.float32, device=device) if scores else None
    nbytes = int(nat.lib().gnx_rank_candidates_bytes(S, ids.numel(), K, k, int(splits)))
    if nbytes < 0:
        nat.check(-1)
    workspace = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=device)
    nat.launch(device, "gnx_rank_candidates", graph.handle, F, F.stride(0), F.shape[0], F.shape[1], rr, sources, S, ptr, ids, ids.numel(),
               candidates, K, k, splits, *counts, top_ids, top_scores, top_is_pos, raw, workspace, workspace.numel())
    return RankResult(counts[0], counts[1], counts[2], counts[3], top_ids, top_scores, top_is_pos, raw)


# ---- node signals at width 1: libgnx.so's csrc/gnx_signal.hip (experimental_filter.py:7-43 of the reference) ------------------------
def _signal_adjacency(what, adj: Adjacency, transposed=False):
    """(graph, values in the order of the structure walked or None for the raw values) of a width-1 launch.  A DroppedAdjacency is
    used through its materialised values: one array, shared by every launch over it."""
    for entry in ("gnx_signal_project", "gnx_signal_spmv", "gnx_signal_ppr", "gnx_signal_smoothness", "gnx_signal_smoothness_back"):
        _need_symbol(what, entry)
    if adj.diag is not None:
        raise Exception(f"{what}: an adjacency with an added identity is not supported at width 1")
    if not transposed:
        if adj.transposed_only:
            raise Exception(f"{what}: this adjacency only holds transposed-order values")
        return adj.graph, adj.vals
    raw = not isinstance(adj, DroppedAdjacency) and adj.vals is None and not adj.transposed_only
    return adj.graph, (None if raw else adj.transposed_values())


def _signal_vector(what, g: DeviceGraph, x, n, name):
    """``x`` as a contiguous float32 [n] tensor on the graph's device (None stays None); no gradient flows through a signal launch."""
    if x is None:
        return None
    nat.require_cuda(x)
    _same_device(g, x)
    x = x.detach().to(torch.float32).reshape(-1).contiguous()
    if x.numel() != n:
        raise Exception(f"{what}: {name} holds {x.numel()} values, the adjacency expects {n}")
    return x


def signal_project(X: torch.Tensor, w: torch.Tensor, sigmoid=True) -> torch.Tensor:
    """f = sigmoid(X . w) as an [n] tensor (``sigmoid=False``: the dot product), one launch of gnx_signal_project; X may be a column
    slice of a wider matrix.  No autograd node: smoothness() differentiates through it."""
    nat.require_cuda(X, w)
    _need_symbol("signal_project", "gnx_signal_project")
    X = _as_f32_rows(X.detach())
    w = w.detach().to(torch.float32).reshape(-1).contiguous()
    if w.numel() != X.shape[1] or w.device != X.device:
        raise Exception("signal_project: w must hold one weight per column of X, on X's device")
    out = torch.empty(X.shape[0], dtype=torch.float32, device=X.device)
    nat.launch(X.device, "gnx_signal_project", X, X.stride(0), X.shape[0], X.shape[1], w, sigmoid, out)
    return out


def signal_spmv(adj: Adjacency, x: torch.Tensor, h0=None, beta=1.0, alpha=0.0, transposed=False) -> torch.Tensor:
    """beta * (A . x) + alpha * h0 for ONE scalar per node, [n] tensors throughout (``transposed``: A^T; ``h0=None``: the constant 1,
    bit for bit a vector of ones).  The lanes of a group split a row's entries (gnx_signal_spmv): fixed summation order, no float
    atomics, a row without entries gives alpha * h0.  Not differentiable."""
    g, vals = _signal_adjacency("signal_spmv", adj, transposed)
    n_in, n_out = (g.n_rows, g.n_cols) if transposed else (g.n_cols, g.n_rows)
    x = _signal_vector("signal_spmv", g, x, n_in, "x")
    h0 = _signal_vector("signal_spmv", g, h0, n_out, "h0")
    out = torch.empty(n_out, dtype=torch.float32, device=g.device)
    nat.launch(g.device, "gnx_signal_spmv", g.handle, vals, transposed, x, h0, beta, alpha, out)
    return out


def signal_ppr(adj: Adjacency, h0=None, a: float = 0.1, iterations: int = 10) -> torch.Tensor:
    """``iterations`` steps x <- (1-a) A x + a h0 from x = h0 (None: the constant 1) on one scalar per node: an [n] tensor, bit for bit
    ``iterations`` signal_spmv calls (gnx_signal_ppr).  What PPRSweep propagates: every column of its operand is the same."""
    g, vals = _signal_adjacency("signal_ppr", adj)
    if g.n_rows != g.n_cols:
        raise Exception("signal_ppr: needs a square adjacency")
    h0 = _signal_vector("signal_ppr", g, h0, g.n_rows, "h0")
    out = torch.empty(g.n_rows, dtype=torch.float32, device=g.device)
    work = torch.empty(g.n_rows, dtype=torch.float32, device=g.device)
    nat.launch(g.device, "gnx_signal_ppr", g.handle, vals, h0, a, iterations, out, work)
    return out


def sweep(adj: Adjacency, X: torch.Tensor, a: float = 0.1, iterations: int = 10, signal=None) -> torch.Tensor:
    """PPRSweep.__forward__ (experimental_filter.py:12-19): X / HN with HN the ``iterations``-step PPR of a matrix of ones -- whose
    columns are all the same, so HN is signal_ppr(adj) and the division one torch pass.  The signal has no parameters: under autograd
    dX = g / HN.  ``signal``: HN if the caller holds it already (a constant adjacency's).
    Where the composition measured faster it is taken: at up to SWEEP_COMPOSED_MAX_WIDTH columns on graphs of at least
    SWEEP_COMPOSED_MIN_ROWS vertices appnp_propagate runs on the handle's degree-relabelled copy, which the width-1 loop does not have
    (R-MAT 10M / 100M, ten iterations, composed against width-1: C = 7 15.6 / 19.3 ms, C = 8 15.1 / 18.9, C = 16 17.9 / 19.0 -- and
    from the first width without the relabelled copy on the other way round: C = 17 22.3 / 19.0, C = 32 21.0 / 19.2, C = 48 37.4 / 19.4,
    C = 64 38.3 / 19.6; profiles/NOTES.md, "Width-1 node signals")."""
    if signal is None and X.shape[1] <= SWEEP_COMPOSED_MAX_WIDTH and adj.graph.n_rows >= SWEEP_COMPOSED_MIN_ROWS and adj.diag is None:
        return X / appnp_propagate(adj, torch.ones_like(X.detach()), a, iterations)
    HN = signal_ppr(adj, None, a, iterations) if signal is None else signal
    return X / HN[:, None]


SWEEP_COMPOSED_MAX_WIDTH = 16           # = the widest rows gnx_appnp_propagate runs on the relabelled copy (RELABEL_MAX_C) ...
SWEEP_COMPOSED_MIN_ROWS = 1 << 20       # ... and the smallest graph it builds that copy for


def signal_colsum(adj: Adjacency) -> torch.Tensor:
    """D_j = sum_i A_ij of the adjacency's own values (tf.sparse.reduce_sum(G, axis=0), experimental_filter.py:39), in a fixed order:
    gnx_graph_colsum with the dropout triple of a ``normalized="none"`` adjacency (or of the raw values), else A^T . 1 at width 1."""
    g = adj.graph
    triple = getattr(adj, "raw_dropout", None)
    if triple is None and adj.vals is None and not adj.transposed_only and not isinstance(adj, DroppedAdjacency):
        triple = (0.0, 0, 0)
    if triple is None:
        return signal_spmv(adj, torch.ones(g.n_rows, dtype=torch.float32, device=g.device), None, 1.0, 0.0, transposed=True)
    D = torch.empty(g.n_cols, dtype=torch.float32, device=g.device)
    nat.launch(g.device, "gnx_graph_colsum", g.handle, *triple, D)
    return D


def smoothness_work_floats(n: int) -> int:
    """Floats of scratch gnx_signal_smoothness needs for n rows (include/gnx.h)."""
    return n // 64 + 64


class _Smoothness(torch.autograd.Function):
    """lambda = sum (f - A f)^2 / sum D f^2, f = sigmoid(X . w), as ONE node: the projection, one width-1 gather with the two global
    sums behind it; backward one gather over the transposed structure (gnx_signal_smoothness_back), dX = gz w^T as one broadcast and,
    where w needs it, dw = X^T gz through gnx_dense_wgrad at one output column.  No value is read back: the node records into a hipGraph."""

    @staticmethod
    def forward(ctx, X, w, adj, colsum):
        g, vals = _signal_adjacency("smoothness", adj)
        n = g.n_rows
        f = signal_project(X, w)
        d = torch.empty(n, dtype=torch.float32, device=g.device)
        sums = torch.empty(3, dtype=torch.float32, device=g.device)
        work = torch.empty(smoothness_work_floats(n), dtype=torch.float32, device=g.device)
        nat.launch(g.device, "gnx_signal_smoothness", g.handle, vals, f, colsum, d, sums, work)
        ctx.adj, ctx.colsum = adj, colsum
        ctx.save_for_backward(X, w, f, d, sums)
        return sums[2].clone()

    @staticmethod
    def backward(ctx, upstream):
        X, w, f, d, sums = ctx.saved_tensors
        g, vals_t = _signal_adjacency("smoothness", ctx.adj, transposed=True)
        upstream = upstream.detach().to(torch.float32).reshape(1).contiguous()
        gz = torch.empty(g.n_rows, dtype=torch.float32, device=g.device)
        nat.launch(g.device, "gnx_signal_smoothness_back", g.handle, vals_t, f, d, ctx.colsum, sums, upstream, gz)
        dX = gz[:, None] * w.detach().reshape(1, -1) if ctx.needs_input_grad[0] else None
        dw = _dense_wgrad(X.detach(), gz[:, None]).reshape(w.shape) if ctx.needs_input_grad[1] else None
        return dX, dw, None, None


def smoothness(adj: Adjacency, X: torch.Tensor, w: torch.Tensor, colsum=None, fused=True) -> torch.Tensor:
    """FastReg's Rayleigh quotient (experimental_filter.py:34-43, without its sign): the 0-dim device tensor
    lambda = sum_i (f_i - (A f)_i)^2 / sum_i D_i f_i^2 with f = sigmoid(X . w), w [C, 1] or [C], differentiable w.r.t. X and w.
    ``colsum``: D; by default the column sums of ``adj``'s own values (signal_colsum).  The division is plain: a graph without
    entries gives what IEEE gives.  ``fused=True``: one autograd node over the width-1 kernels (_Smoothness).  ``fused=False``: the
    same mathematics composed from spmm at width 1 (whose backward is gnx_spmm_tv) and torch sums -- the baseline of
    tools/signal_bench.py, and the path of what the width-1 entries refuse: an adjacency with an added identity (``adj.diag``) takes it
    whatever ``fused`` says, its D the column sums of the values plus the diagonal.  Square adjacency; device tensors: a graph handle
    lives on the GPU, so neither form has a CPU path (CPU tensors raise, as they do in spmm)."""
    g = adj.graph
    if g.n_rows != g.n_cols:
        raise Exception("smoothness: needs a square adjacency")
    if X.dim() != 2 or X.shape[0] != g.n_rows or w.numel() != X.shape[1]:
        raise Exception("smoothness: X must be [n, C] and w hold C weights")
    nat.require_cuda(X, w, colsum)
    _same_device(g, X, w, colsum)
    if colsum is not None:
        D = _signal_vector("smoothness", g, colsum, g.n_cols, "colsum")
    elif adj.diag is not None:
        if adj.transposed_only:
            raise Exception("smoothness: this adjacency only holds transposed-order values")
        D = signal_colsum(Adjacency(g, adj.vals)) + adj.diag
    else:
        D = signal_colsum(adj)
    if fused and adj.diag is None:
        return _Smoothness.apply(_as_f32_rows(X), w, adj, D)
    f = torch.sigmoid(torch.matmul(X, w.reshape(-1, 1)))
    diffs = f - spmm(adj, f)
    return (diffs * diffs).sum() / (D[:, None] * f * f).sum()


def signal_uniform(graph: DeviceGraph, n: int, bound: float, seed, stream) -> torch.Tensor:
    """[n] draws of U(-bound, bound) from the counter RNG of the edge dropout (gnx_signal_uniform): reproducible from (seed, stream),
    and -- the handle's dropout counter is added to the stream on the device -- fresh on every replay of a captured step."""
    _need_symbol("signal_uniform", "gnx_signal_uniform")
    out = torch.empty(int(n), dtype=torch.float32, device=graph.device)
    nat.launch(graph.device, "gnx_signal_uniform", graph.handle, n, bound, seed, stream, out)
    return out

"""Graph architectures over the HIP propagation path: GNN (adjacency owner), PPRIteration,
APPNP, GCNLayer, GCN.

Mirrors reference gnntf/core/gnn/gnn.py:29-50, gnntf/core/gnn/architectures/filter.py:6-35
and gnntf/core/gnn/architectures/gcn.py:77-113.  Where the reference calls
tf.sparse.sparse_dense_matmul on a freshly re-normalised tf.sparse tensor, these layers call
the fused gfx950 kernels through gnntf.sparse; the eval-mode normalised adjacency is
computed once per (normalized, add_eye) and cached, because it is constant.
"""
from __future__ import annotations

import math

import torch

from . import ordering, sparse
from .blocks import Concatenate, Dense, Dropout, affine, is_relu, linear, relu
from .params import default_device
from .protocol import Layer
from .training import Trainable


class Structural(Layer):
    """gnn.py:5-26: trainable per-node embeddings (``bipartite`` rows in one variable, the rest in another), optionally
    l2-normalised, prepended to the incoming features; with zero-width features the embeddings ARE the features."""

    def __build__(self, architecture, dims: int = 16, l2_contraint: bool = False, bipartite: int = 0, **kwargs):
        rows, width = architecture.top_shape()
        self.l2_contraint = l2_contraint
        self.embeddings = architecture.create_var((bipartite, dims), **kwargs)
        self.embeddings2 = architecture.create_var((rows - bipartite, dims), **kwargs)
        return rows, dims + width

    def __forward__(self, architecture, features):
        table = self.embeddings2 if self.embeddings.shape[0] == 0 else torch.cat([self.embeddings, self.embeddings2], dim=0)
        if self.l2_contraint:
            table = torch.nn.functional.normalize(table, dim=1, eps=1e-12)
        return table if features.shape[1] == 0 else torch.cat([table, features], dim=1)


FEATURE_DROPOUTS = ("torch", "fused")
STORAGE_DTYPES = (torch.float32, torch.bfloat16)

# the opt-in keywords of GNN.__init__ with the values each takes, in the order __init__ checks them (a call with two bad ones names the
# first).  The first value is today's path: what a layer reads on an architecture that does not carry the attribute (_switch)
SWITCHES = (
    ("dense_dropout", sparse.DENSE_DROPOUTS), ("gcn_spectral", sparse.GCN_SPECTRALS), ("ngcf_layer", sparse.NGCF_LAYERS),
    ("ngcf_backward", sparse.NGCF_BACKWARDS), ("ngcf_wide", sparse.NGCF_WIDES), ("ngcf_wide_backward", sparse.NGCF_WIDE_BACKWARDS),
    ("gcn_backward", sparse.GCN_BACKWARDS), ("gcn_layer", sparse.GCN_LAYERS), ("gcnii_edge_dropout", sparse.GCNII_EDGE_DROPOUTS),
    ("gcnii_spectral", sparse.GCNII_SPECTRALS), ("feature_dropout", FEATURE_DROPOUTS), ("gcnii_backward", sparse.GCNII_BACKWARDS),
    ("train_gather_order", sparse.GATHER_ORDERS), ("inference_dtype", STORAGE_DTYPES), ("training_dtype", STORAGE_DTYPES),
    ("gcnii_training_dtype", STORAGE_DTYPES), ("gcnii_weight_gradient", sparse.GCNII_WEIGHT_GRADIENTS),
)
_TODAYS_PATH = {keyword: allowed[0] for keyword, allowed in SWITCHES}


def _switch(architecture, keyword):
    """What ``architecture`` says about the GNN keyword ``keyword``; today's path where it is no GNN and does not say."""
    return getattr(architecture, keyword, _TODAYS_PATH[keyword])


class GNN(Trainable):
    """gnn.py:29-50."""

    # a graph whose COO holds duplicate entries (graph2adj of a both-direction graph) gets its entry tables the first time it
    # propagates in training mode with edge dropout (DeviceGraph.enable_entry_dropout): the fused training kernels then run on it,
    # same masks and values as the materialised form.  False: such graphs stay on the materialised form (A/B comparisons)
    fuse_entry_dropout = True

    def __init__(self, graph, features, preprocessor: Layer = None, reorder=None, inference_dtype=torch.float32,
                 training_dtype=torch.float32, train_gather_order="auto", gcnii_backward="composed", feature_dropout="torch",
                 gcnii_training_dtype=torch.float32, gcnii_weight_gradient="stored", gcnii_spectral="composed",
                 gcnii_edge_dropout="composed", gcn_layer="composed", gcn_backward="composed", ngcf_layer="composed",
                 ngcf_backward="composed", ngcf_wide="composed", ngcf_wide_backward="composed", gcn_spectral="composed",
                 dense_dropout="torch"):
        """``reorder`` (opt-in, not in the reference): store the graph and the feature rows with the vertices relabelled; every
        [N, .] tensor inside the model then lives in that order, and the model's OUTPUT is put back into the caller's order, so
        tasks, labels and node ids are unaffected.  Results agree with the unordered model to float32 rounding.
        ``"degree"``: stable order of descending entry count (5-20 % faster propagation at C <= 128: rows sharing a wave, their
        H0/out rows and the hub rows become neighbours in memory).
        ``"locality"``: community by community (gnntf.ordering.locality_order: label propagation) with the library told so
        (row windows, one window of the numbering per XCD at a time) -- for graphs that HAVE communities, as the reference's
        citation datasets do: -16 ... -31 % per propagation at C = 7 ... 256 on a planted-partition x power-law graph of 10M
        vertices.  On a graph without communities (R-MAT) the order finds none (``locality_share`` fails
        ordering.found_communities) and the model keeps the default order (``reorder_used`` is then None); so do graphs of
        a few windows, which fit the caches in any order.
        Measurements: profiles/NOTES.md round 5.
        ``inference_dtype=torch.bfloat16`` (opt-in, not in the reference): eval-mode forwards without autograd (``predict()``, the
        validation forwards inside ``train()``) gather the propagated features as bf16 with f32 sums (sparse.appnp_propagate /
        sparse.spmm ``storage``); every forward with grad enabled -- every training step -- runs the f32 path unchanged (``training_dtype`` is the
        separate switch for those).  Error:
        the APPNP loop is within (2^-8 / a) max_k ||H_k||_2 per column of the f32 result (first order), a GCN SpMM within
        2^-8 |A| |X| elementwise.  In GCNII a run of plain GCNIILayer layers runs as one bf16 chain (gnx_gcnii_step_bf16): the run's
        input is rounded once, every layer but the run's last stores its rows rounded once to bf16, the last writes f32; sums, H0
        (f32), the mix and the transform stay f32.  Elementwise the result is within E_L of the f32 stack to first order,
        E_0 = 2^-8 |H|, E_{l+1} = ((1-a) |A| E_l) |M_l| + 2^-8 |out_l| (layers that store bf16).  GCNIISpectralPreservingLayer,
        activations other than relu / the identity, add_eye and widths outside sparse.GCNII_BF16_MIN_WIDTH ...
        GCNII_BF16_MAX_WIDTH keep f32 and its bits.
        ``training_dtype=torch.bfloat16`` (opt-in, not in the reference; separate from ``inference_dtype``, which keeps meaning eval
        only): training-mode PPR propagation with edge dropout (PPRLoop, fused runs of PPRIteration layers) gathers its iterate and
        its back-propagated gradient as bf16 (sparse.ppr_loop ``storage``): masks, degree scales, weights, sums, H0, the mix and
        both results of the step stay f32, a row is rounded once as it is handed to the next iteration.  It is an allowance: the
        loop keeps f32 -- today's bits -- where the fused chained form does not apply (relu, no edge dropout, a graph that cannot
        fuse its dropout), below sparse.BF16_TRAIN_MIN_WIDTH columns and on graphs of fewer than sparse.BF16_TRAIN_MIN_ROWS vertices
        (where it measured slower).  It is ignored by GCNLayer / GCNIILayer training (GCNII training has a switch of its own,
        ``gcnii_training_dtype`` below) and by the vertex-partitioned path (sharded.py), which keep f32 whatever it says.
        ``train_gather_order`` (not in the reference): ``"caller"``, ``"relabelled"`` or ``"auto"`` (sparse.ppr_loop
        ``gather_order``).  ``"relabelled"``: the fused f32 training loops (PPRLoop, fused runs of PPRIteration layers, with edge
        dropout) keep the iterate and the back-propagated gradient in the library's hub-adjacent gather order BETWEEN their launches;
        the model, its rows, masks and sums stay in the caller's numbering and every result is bit for bit that of ``"caller"``
        (unlike ``reorder="degree"``, which renumbers the model and rounds differently).  Where the chained f32 loop does not apply
        (relu, bf16 training storage, graphs with duplicate entries, ``reorder="locality"`` row windows, the vertex-partitioned path)
        it is today's path.  ``"auto"`` (the default) takes the relabelled order only at the widths and graph sizes where it
        measured faster (sparse.TRAIN_GATHER_MAX_WIDTH / TRAIN_GATHER_MIN_ROWS; profiles/NOTES.md).
        ``gcnii_backward`` (not in the reference): ``"composed"`` (the default) or ``"fused"`` (sparse.gcnii_step ``backward``).
        ``"fused"``: the backward of every plain GCNIILayer on the device with a constant adjacency is the relu mask, the weight
        gradient and ONE launch for dH and dH0 (gnx_gcnii_step_back) instead of the dense kernel, the transposed SpMM and a scaling;
        the forward and the weight gradients keep their bits, dH and dH0 agree to float32 rounding.  GCNIISpectralPreservingLayer,
        dropped adjacencies, add_eye and the CPU path keep their code whatever it says.  The default stays ``"composed"``: the other
        order moves the roundings of existing gradients (measurement: profiles/NOTES.md "Fused GCNII backward").
        ``feature_dropout`` (not in the reference): ``"torch"`` (the default: torch.nn.functional.dropout behind every layer, today's
        calls and bits) or ``"fused"``.  ``"fused"``: the feature dropout of every plain GCNIILayer (this class itself, relu or the
        identity as activation, 0 < ``dropout`` < 1, device tensors, no add_eye) in training mode leaves the layer's launch
        (sparse.gcnii_step ``dropout``, gnx_gcnii_step_drop) with a mask of the counter RNG the edge dropout uses: element (i, c) of
        the layer's ``_next_mask_stream()`` stream is kept iff hash_u24(seed, stream, i, c, 0) >= int(p * 2^24), kept values times the
        f32 1 / (1 - p).  The masks differ from torch's, which is why it is opt-in; a training step is then reproducible from
        (seed, stream) alone, and ``train(capture=True)`` equals the eager run bit for bit.  GCNIISpectralPreservingLayer, other
        activations, CPU tensors, Dense / Dropout layers and the vertex-partitioned path keep torch's dropout whatever it says
        (measurement: profiles/NOTES.md "Fused GCNII feature dropout").
        ``gcnii_training_dtype=torch.bfloat16`` (opt-in, not in the reference; a keyword of its own, so that ``training_dtype`` on an
        existing GCNII model keeps today's bits): in training mode with grad enabled a RUN of at least two consecutive plain GCNIILayer
        layers (the class itself, relu or the identity as activation, a float ``a``, no add_eye, ``graph_dropout`` 0 -- a constant
        adjacency --, and ``dropout`` 0 or ``feature_dropout="fused"`` with 0 < dropout < 1, so that nothing sits between two layers)
        executes as ONE autograd node over bf16 rows (sparse.gcnii_train_run_bf16): the run's input is rounded once, every layer but
        the run's last stores its (dropped) output rounded once to bf16 -- what the next layer gathers and what is saved for the
        backward --, the last writes f32; on the way back the gated gradient is gathered as bf16.  Sums, H0, the mixed rows T, the
        mix, the transform, the weight gradients and the running dH0 sums stay f32.  The layers draw their mask streams in layer
        order, so the masks are those of the f32 ``"fused"`` path under the same seed; the backward is always the fused one.  The
        ``.value`` of an inner layer is the detached exact widening of its stored rows, made on first read.  It is an allowance:
        widths outside {16, 32, 64} or below sparse.GCNII_BF16_TRAIN_MIN_WIDTH, graphs of fewer than
        sparse.GCNII_BF16_TRAIN_MIN_ROWS rows (where the step measured slower: profiles/NOTES.md "bf16 storage in GCNII training" --
        4 % faster at C = 32 / 64 on 10^7 vertices, slower at C = 16 and at 10^6 vertices and below), GCNIISpectralPreservingLayer,
        torch dropout, eval mode, the vertex-partitioned path and ``fuse_runs = False`` keep today's path and today's bits.
        ``gcnii_weight_gradient`` (not in the reference): ``"stored"`` (the default) or ``"recomputed"`` (sparse.gcnii_step /
        sparse.gcnii_train_run_bf16 ``weight_gradient``).  A training GCNII layer saves two [n, C] matrices for its backward: its output
        and the mixed rows T = (1-a) A.H + a H0, the latter for dW alone.  ``"recomputed"``: every plain GCNIILayer (this class itself,
        relu or the identity as activation, width 16, 32 or 64, device tensors, a constant adjacency without add_eye), on the f32 path
        and in a ``gcnii_training_dtype=torch.bfloat16`` run alike, writes no T in its forward and saves its input and H0 in T's place;
        dW then comes from one launch that makes T again in LDS and multiplies T^T G on the matrix cores (gnx_gcnii_wgrad).  Where it
        saves memory: with ``feature_dropout="fused"`` or a layer ``dropout`` of 0 the layer's input IS the previous layer's saved
        output and H0 is saved by the layer that made it, so a layer keeps 4 bytes per element and layer less -- 8 -> 4 in f32,
        6 -> 2 with bf16 rows; with torch's dropout the input is a tensor of its own (the dropout's result) and the saving is nil.  The
        logits, the loss, dH, dH0 and the gradient of the run's input keep their bits, every dW agrees to float32 rounding (another
        summation order: why it is opt-in); works with either ``gcnii_backward``; ``train(capture=True)`` equals the eager run bit for
        bit under fused dropout, as before.  GCNIISpectralPreservingLayer, other activations, add_eye, other widths, dropped
        adjacencies, CPU tensors and the vertex-partitioned path keep today's path whatever it says (measurement: profiles/NOTES.md
        "GCNII weight gradient without stored rows").
        ``gcnii_spectral`` (not in the reference): ``"composed"`` (the default: today's calls and bits) or ``"fused"``
        (sparse.gcnii_step_spectral).  ``"fused"``: every GCNIISpectralPreservingLayer (that class itself, relu or the identity as
        activation, float32 device tensors, a constant adjacency without add_eye) runs 2 * dropout(act(T . M + bias) - bias) as ONE
        launch (gnx_gcnii_step_spectral) instead of the SpMM+mix, the dense kernel and three elementwise passes, in eval mode and in
        training mode alike.  In training mode with 0 < ``dropout`` < 1 the mask leaves the same launch and is the COUNTER RNG's, not
        torch's: element (i, c) of the layer's ``_next_mask_stream()`` stream is kept iff hash_u24(seed, stream, i, c, 0) >= int(p * 2^24),
        kept values times the f32 1 / (1 - p), as for ``feature_dropout="fused"`` -- the masks differ from torch's, which is why the
        switch is opt-in; a training step is then reproducible from (seed, stream) alone and ``train(capture=True)`` equals the eager
        run bit for bit.  For its backward the layer saves the mixed rows T and ONE BIT per element (the sign of the pre-activation) --
        4 bytes and a bit per element instead of 9 bytes -- and starts it with one gate pass (gnx_gcnii_spectral_back) that also makes
        the bias gradient; it honours ``gcnii_backward``.  The eval-mode result agrees with the composed one to float32 rounding (the
        same sums; the bias is added inside the matrix-core epilogue either way).  Plain GCNIILayer stacks and every other keyword on
        them, ``feature_dropout="fused"`` on a spectral stack (which that switch never touched), the bf16 switches, other activations,
        a rate of 1 or more, dropped adjacencies, add_eye, CPU tensors, GCNSpectralPreservingLayer and the vertex-partitioned path keep
        today's path and bits whatever it says (measurement: profiles/NOTES.md "Fused spectral-preserving GCNII layer").
        ``gcnii_edge_dropout`` (not in the reference): ``"composed"`` (the default: today's calls and bits) or ``"fused"``
        (sparse.gcnii_step ``edge_dropout``).  ``"fused"``: a plain GCNIILayer (the class itself, relu or the identity as activation, a
        float ``a``, float32 device tensors, no add_eye) in training mode with ``graph_dropout`` != 0 on a graph that can fuse its
        dropout -- the reference's default, ``GCNIILayer(..., graph_dropout=0.5)`` -- runs as the ONE launch of a constant adjacency
        (gnx_gcnii_step_dropped): every entry's weight (D[row] * drop(raw)) * D[col] is made in the gather loop, the mixed rows are
        written once, and with ``feature_dropout="fused"`` and 0 < ``dropout`` < 1 the feature mask leaves the same launch (otherwise
        torch's dropout follows as today).  The backward is the existing gate, gnx_dense_wgrad and, with ``gcnii_backward="fused"``, one
        launch over the transposed structure (gnx_gcnii_step_back_dropped); with ``"composed"`` gnx_dense, the transposed dropped SpMM and
        a scaling.  The layer draws its mask streams in today's order and number (the adjacency's first, then the feature mask's), so a
        seed means the masks it means under ``"composed"``; every tensor has the bits of the same layer over the materialised adjacency,
        and against ``"composed"`` agrees to float32 rounding (the transform runs in the fused launch's order).  Eval mode, constant
        adjacencies, GCNIISpectralPreservingLayer, other activations, ``gcnii_weight_gradient="recomputed"``,
        ``gcnii_training_dtype=torch.bfloat16``, add_eye, graphs that cannot fuse their dropout, CPU tensors and the vertex-partitioned
        path keep today's path whatever it says (measurement: profiles/NOTES.md "Fused GCNII layer under edge dropout").
        ``gcn_layer`` (not in the reference): ``"composed"`` (the default: today's calls and bits) or ``"fused"`` (sparse.gcn_step).
        ``"fused"``: a GCNLayer (the class itself, no ``transform_first``, relu or the identity as activation, float32 device rows of
        width 16, 32 or 64, at most as many outputs, no add_eye, not a bf16 ``inference_dtype`` forward) runs
        act((A . X) . W + b) as ONE launch (gnx_gcn_step) instead of the SpMM and the dense kernel with A . X written and read back
        between them, in eval mode and in training mode alike; in training mode over a DroppedAdjacency the launch makes the weights
        itself (gnx_gcn_step_dropped), and with ``feature_dropout="fused"`` and 0 < ``dropout`` < 1 the mask leaves the same launch
        (otherwise torch's dropout follows as today).  The layer draws its mask streams in today's order and number: the adjacency's,
        then the mask's.  In ``GCN(latent_dims=[64])`` this is the 64 -> num_classes layer (the first layer gathers at the feature
        width); in ``[64, 64, 64]`` every layer but the first.  The backward is composed from today's kernels.  The result agrees with
        the composed one to float32 rounding.  GCNSpectralPreservingLayer and other subclasses, ``transform_first``, other
        activations, other widths, add_eye, CPU tensors and the vertex-partitioned path keep today's path and bits whatever it says
        (measurement: profiles/NOTES.md "Fused GCN layer").
        ``gcn_backward`` (not in the reference): ``"composed"`` (the default: today's calls and bits) or ``"fused"`` (sparse.gcn_step
        ``backward``).  It acts on the layers that run as the one autograd node of ``gcn_layer="fused"`` and is inert otherwise.
        ``"fused"``: after the gate, gnx_dense_wgrad and the column sums, the gradient of the layer's input is ONE launch over the
        transposed structure (gnx_gcn_step_back, under edge dropout gnx_gcn_step_back_dropped) that gathers the gated gradient at the
        OUTPUT width and multiplies by W^T on the matrix cores -- dX = (A^T G') W^T -- instead of gnx_dense and the transposed SpMM with
        the [n, C_in] matrix G' W^T written, read back and gathered at the input width.  The forward, dW and db keep their bits; dX
        agrees to float32 rounding (the products associate differently: why the default stays ``"composed"``; measurement:
        profiles/NOTES.md "Fused GCN backward").  Such a layer lets its saved A . X go once dW is made, before dX is allocated, so
        its backward never holds the two side by side; in return it runs its backward once (a second backward over a retained
        graph raises and asks for a new forward).
        ``ngcf_layer`` (not in the reference): ``"composed"`` (the default: today's calls and bits) or ``"fused"`` (sparse.ngcf_step).
        Every layer whose class is NGCFLayer itself -- leaky_relu, relu or the identity, both biases or none, f32 rows on the device,
        an input width of 16, 32 or 64 that the layer does not widen, an adjacency without a diagonal -- then runs
        l2_normalize(dropout(act((X * (A . X)) . W1 + b1) + act((A . X) . W2 + b2))) as ONE launch (gnx_ngcf_step) instead of one SpMM, a
        multiply, two transforms, two activations, an add, the dropout and the normalisation as passes of their own.  In training
        with 0 < ``dropout`` < 1 the mask leaves the same launch under ``feature_dropout="fused"`` (the counter RNG; a
        ``_next_mask_stream()`` stream per layer); with torch's dropout the launch stops before the norm and torch's dropout and
        normalize follow as today.  The backward is one gate pass (gnx_ngcf_back_gate) and today's kernels (``ngcf_backward``, below, folds
        it into one launch around the transposed SpMM).  The results agree with
        the composed layer to float32 rounding.  Subclasses, CPU tensors, bf16 rows, other widths (128, the width of the
        library_recommendation demo, among them) and the sharded layers keep today's path and bits.
        ``ngcf_backward`` (not in the reference): ``"composed"`` (the default: today's calls and bits) or ``"fused"`` (sparse.ngcf_step
        ``backward``).  It acts on the layers that run as the one autograd node of ``ngcf_layer="fused"`` and is inert otherwise.
        ``"fused"``: the gate pass, both bias sums, X * A, G1 W1^T and G2 W2^T, dA = Q1 * X + Q2 and Q1 * A come from ONE row-local
        launch (gnx_step_back_ngcf: the products on the matrix cores, the weights read as stored), the transposed SpMM mixes Q1 * A
        in, and gnx_dense_wgrad runs twice -- instead of the column sums, a torch multiply, gnx_dense twice and two addcmul passes.
        It works with the mask in the launch and with torch's dropout and normalize alike.  The forward, dW1 and dW2 keep their
        bits; dX and the bias gradients agree to float32 rounding (why the default stays ``"composed"``; measurement:
        profiles/NOTES.md "Fused NGCF backward").  The node keeps its saved tensors: a second backward over a retained graph works.
        ``ngcf_wide`` (not in the reference): ``"composed"`` (the default: today's calls and bits) or ``"fused"`` (sparse.ngcf_step
        ``wide``).  It acts together with ``ngcf_layer="fused"`` and is inert otherwise: a layer of input width 128 -- the width of the
        library_recommendation demo -- that meets every other condition of ``ngcf_layer`` then runs as the SpMM and ONE row-local launch
        (gnx_step_wide_ngcf: both transforms on the matrix cores with the weights in LDS, the gate words, the activations' sum, the mask
        and the norm over rows read once) instead of the SpMM and the sixteen torch passes around it, in the same three forms: eval mode
        or a dropout of 0, the mask in the launch under ``feature_dropout="fused"``, or the launch without the norm followed by
        torch's dropout and normalize.  The backward is the composed one of ``ngcf_layer`` (``ngcf_backward="fused"`` has no launch at
        this width).  The results agree with the composed layer to float32 rounding (measurement: profiles/NOTES.md "NGCF layer at
        width 128").  A model built without the keyword makes today's calls at every width.
        ``ngcf_wide_backward`` (not in the reference): ``"composed"`` (the default: today's calls and bits) or ``"fused"``
        (sparse.ngcf_step ``wide_backward``).  It acts on the layers that ``ngcf_layer="fused"`` and ``ngcf_wide="fused"`` together run
        at input width 128 and is inert otherwise: their backward is then ONE call of gnx_step_back_wide_ngcf -- the gate pass with the
        slab-ordered bias sums, one row-local launch (G1 W1^T and G2 W2^T on the matrix cores with the weights in LDS, read as stored;
        dA, Q1 * A and X * A written once) and the transposed SpMM with Q1 * A mixed in -- and gnx_dense_wgrad twice, instead of the
        column sums, a torch multiply, two transposed weight copies, gnx_dense twice and two addcmul passes.  The forward, dW1 and dW2
        keep their bits; dX and the bias gradients agree to float32 rounding (why the default stays ``"composed"``; measurement:
        profiles/NOTES.md "NGCF backward at width 128").  A second backward over a retained graph works.
        ``gcn_spectral`` (not in the reference): ``"composed"`` (the default: today's calls and bits) or ``"fused"``
        (sparse.gcn_step_spectral).  ``"fused"``: a GCNSpectralPreservingLayer (the class itself, no ``transform_first``, relu or the
        identity as activation, float32 device rows of width 16, 32 or 64, at most as many outputs, no add_eye, not a bf16
        ``inference_dtype`` forward) runs 2 * dropout(act((A . X) . W + b) - b) as ONE launch (gnx_step_spectral_gcn) instead of the
        SpMM, the dense kernel and three elementwise passes, in eval mode and in training mode alike; in training mode over a
        DroppedAdjacency the launch makes the weights itself (gnx_step_spectral_gcn_dropped).  In training mode with 0 < ``dropout`` < 1
        the mask leaves the same launch and is the COUNTER RNG's, not torch's: element (i, c) of the layer's ``_next_mask_stream()``
        stream -- drawn after the adjacency's, in today's order -- is kept iff hash_u24(seed, stream, i, c, 0) >= int(p * 2^24), kept
        values times the f32 1 / (1 - p), as for ``gcnii_spectral="fused"``: the masks differ from torch's, which is why the switch is
        opt-in; a training step is then reproducible from (seed, stream) alone and ``train(capture=True)`` equals the eager run bit
        for bit.  For its backward the layer saves A . X and ONE BIT per element (the sign of the pre-activation) instead of A . X, the
        activated rows, the subtraction's result and a byte mask, and starts it with one gate pass (gnx_gcnii_spectral_back) that also
        makes the bias gradient; it honours ``gcn_backward``.  In ``GCN(latent_dims=[64], layer_type=GCNSpectralPreservingLayer)`` this
        is the 64 -> num_classes layer (the first layer gathers at the feature width); in ``[64, 64, 64]`` every layer but the first.
        The eval-mode result agrees with the composed one to float32 rounding.  GCNLayer and ``gcn_layer="fused"`` (which keeps
        ignoring this class), other subclasses, ``transform_first``, other activations, other widths, a rate of 1 or more, add_eye, CPU
        tensors and the vertex-partitioned path keep today's path and bits whatever it says (measurement: profiles/NOTES.md "Fused
        spectral-preserving GCN layer").
        ``dense_dropout`` (not in the reference): ``"torch"`` (the default: torch.nn.functional.dropout behind every Dense and in every
        Dropout layer, today's calls and bits) or ``"fused"`` (sparse.dense_step).  A keyword of its own: ``feature_dropout="fused"``
        keeps leaving these layers to torch.  ``"fused"`` acts in training mode on Dropout and Dense layers (the classes themselves) over
        float32 device rows, for rates in (0, 1) and relu or the identity as the Dense's activation.  A Dropout directly followed by a
        Dense -- the front of APPNP (filter.py:30-33) and of GCNII (gcn.py:68-70) -- executes as ONE launch of the dense kernels
        (gnx_dense_drop): the mask is applied to a row's values as the matrix cores pick them up, the Dense's own dropout in the
        epilogue, and neither a dropped copy of the feature matrix nor a mask is written; the backward makes the input mask again
        inside the weight-gradient kernels (gnx_dense_wgrad_drop) and saves the feature matrix itself.  The Dropout layer's ``.value``
        is made on first read (sparse.feature_dropout with the same triple: the bits the launch consumed).  A Dense with a rate and no
        Dropout in front runs the same launch with its output mask alone; a Dropout followed by anything else is the pass
        sparse.feature_dropout.  The masks are the COUNTER RNG's, not torch's: element (i, c) of a layer's ``_next_mask_stream()``
        stream -- drawn in layer order, the Dropout's, then the Dense's -- is kept iff hash_u24(seed, stream, i, c, 0) >= int(p * 2^24),
        kept values times the f32 1 / (1 - p); that is why the switch is opt-in.  Every mask of an APPNP or GCNII training step (with
        ``feature_dropout="fused"`` for the GCNII layers) is then the counter RNG's: a step is reproducible from its seed and
        ``train(capture=True)`` equals the eager run.  Eval mode, SparseRows features (they have masks of their own), CPU tensors, a
        Layered without a graph handle (MLP), other activations, subclasses, rates of 0 and of 1 or more, and the vertex-partitioned
        path keep today's path and bits whatever it says; ``fuse_runs = False`` keeps the layers apart, each with the counter RNG's pass
        (measurement: profiles/NOTES.md "Fused dropout around Dense")."""
        given = locals()
        for keyword, allowed in SWITCHES:
            if allowed is STORAGE_DTYPES:
                if given[keyword] not in allowed:
                    raise Exception(f"GNN: {keyword} must be torch.float32 or torch.bfloat16")
            else:
                sparse._one_of("GNN", keyword, given[keyword], allowed)
        super().__init__(features)
        for keyword, _ in SWITCHES:
            setattr(self, keyword, given[keyword])
        self._order = self._newid = None
        self.reorder_used, self.locality_share = None, None
        if isinstance(graph, sparse.DeviceGraph):
            if reorder is not None:
                raise Exception("GNN: reorder needs the COO adjacency, not a ready DeviceGraph")
            self.graph = graph
        else:
            coo = sparse.as_coo(graph).to(default_device())
            if reorder not in (None, "degree", "locality"):
                raise Exception("Invalid reorder option")
            n = coo.dense_shape[0]
            order = None
            if reorder == "degree":
                order = torch.argsort(torch.bincount(coo.indices[:, 0], minlength=n), descending=True, stable=True)    # new id -> old id
            elif reorder == "locality":
                if coo.dense_shape[0] != coo.dense_shape[1]:
                    raise Exception("GNN: reorder=\"locality\" needs a square adjacency")
                order = ordering.locality_order(coo.indices, n)
            if order is not None:
                newid = torch.empty_like(order)
                newid[order] = torch.arange(n, device=order.device)
                if reorder == "locality":
                    # did the order find communities?  On a graph without them (R-MAT) it is a loss against the default: keep that
                    self.locality_share = ordering.share_within(coo.indices, newid, ordering.LOCALITY_WINDOW)
                    baseline = ordering.degree_order_share(coo.indices, n, ordering.LOCALITY_WINDOW)
                    if not ordering.found_communities(self.locality_share, n, ordering.LOCALITY_WINDOW, baseline):
                        order, reorder = None, None
            self.reorder_used = reorder
            if order is not None:
                if isinstance(self.features, sparse.SparseRows):
                    raise Exception("GNN: reorder needs dense input features")
                self._order, self._newid = order, newid
                coo = sparse.SparseCOO(newid[coo.indices], coo.values, coo.dense_shape)
                self.features = self.features.index_select(0, order)
            self.graph = sparse.DeviceGraph(coo, device=default_device())
            if reorder == "locality":
                self.graph.set_row_window(ordering.LOCALITY_WINDOW)
        self._adjacency_cache = dict()
        self._signal_cache = dict()              # eval-mode node signals of the constant adjacency (PPRSweep): constants of the graph
        if preprocessor is not None:
            self.add(preprocessor)

    def __call__(self, features):
        if self._order is None:
            return super().__call__(features)
        if features is not self.features:                  # rows given in the caller's order
            features = features.index_select(0, self._order)
        return super().__call__(features).index_select(0, self._newid)

    def get_adjacency(self, graph_dropout=0.5, normalized="symmetric", add_eye="none"):
        """Edge dropout (training mode only) -> optional +I -> D^-1/2 A D^-1/2 by column sums
        (gnn.py:36-50), as one device call.  Returns an Adjacency for gnntf.spmm."""
        if normalized not in ("symmetric", "bipartite", "none"):
            raise Exception("Invalid matrix normalization")
        if graph_dropout != 0 and self.is_training():
            seed, stream = self._next_mask_stream()
            if normalized == "symmetric" and add_eye == "none":          # the values are produced inside the SpMM kernels
                self._enable_entry_dropout()
                return sparse.dropped_adjacency(self.graph, graph_dropout, seed, stream)
            return sparse.normalize(self.graph, normalized, add_eye, graph_dropout, seed, stream)
        key = (normalized, add_eye)
        if key not in self._adjacency_cache:
            self._adjacency_cache[key] = sparse.normalize(self.graph, normalized, add_eye)
        return self._adjacency_cache[key]

    def _mask_triple(self, rate):
        """(rate, seed, stream) of a layer's counter-RNG feature mask: draws the layer's next mask stream (_next_mask_stream)."""
        return (rate,) + tuple(self._next_mask_stream())

    def _enable_entry_dropout(self):
        """The entry tables of a graph with duplicate entries, once, before its first fused training propagation (fuse_entry_dropout)."""
        g = self.graph
        if self.fuse_entry_dropout and g.nnz_entries != g.nnz and g.n_rows == g.n_cols and not g.entry_dropout:
            g.enable_entry_dropout()


def _eval_storage(architecture) -> torch.dtype:
    """The feature storage of a propagation: GNN.inference_dtype in an eval-mode forward without autograd, else float32."""
    if torch.is_grad_enabled() or not isinstance(architecture, GNN) or architecture.is_training():
        return torch.float32
    return architecture.inference_dtype


def _propagation_run(architecture: "GNN", H0_value, a, iterations, graph_dropout, with_relu=False):
    """``iterations`` PPR steps from H0 through the fused loop (what PPRLoop and a run of plain PPRIteration layers execute).
    ``with_relu``: relu after every step (the reference's ``activation`` argument, filter.py:22,28,35), in the kernels' epilogue.
    Returns (result, run) with run(k) = the value after the first k iterations (for the intermediate layers' lazy ``.value``)."""
    training = graph_dropout != 0 and architecture.is_training()
    cheap = True                                                # asking make_adj for an iteration's adjacency again costs nothing
    if training:
        seed, first = architecture._next_mask_stream(iterations)
        graph, p = architecture.graph, graph_dropout
        if isinstance(architecture, GNN):
            architecture._enable_entry_dropout()
        if sparse.can_fuse_dropout(graph, p):
            # the degree scales of all K iterations in one pass over the structure; kept (K x N floats) for the backward
            scales = sparse.dropped_degree_scales(graph, p, seed, first, iterations)
            make_adj = lambda k, bwd=False: sparse.dropped_adjacency(graph, p, seed, first + k, D=scales[k])
        elif graph.nnz * iterations * 4 <= (64 << 20):
            # small graph (launch-latency regime): keep the K materialised adjacencies for the backward (one permute launch
            # there instead of three launches to regenerate); large graphs regenerate to save K nnz-sized arrays
            kept = dict()

            def make_adj(k, bwd=False):
                if k not in kept:
                    kept[k] = sparse.normalize(graph, "symmetric", "none", p, seed, first + k)
                return kept.pop(k) if bwd else kept[k]
        else:
            cheap = False                                       # every call materialises an nnz-sized value array
            make_adj = lambda k, bwd=False: sparse.normalize(graph, "symmetric", "none", p, seed, first + k, transposed_only=bwd)
    else:
        adj = architecture.get_adjacency(graph_dropout)
        make_adj = lambda k, bwd=False: adj
    if not torch.is_grad_enabled() and not training:
        storage = _eval_storage(architecture)
        run = lambda k: sparse.appnp_propagate(make_adj(0, False), H0_value, a, k, relu=with_relu, storage=storage)
    else:
        storage = _switch(architecture, "training_dtype") if training else torch.float32
        # (the argument is passed only where it can change the path: outside the allowance "auto" is today's call, argument for argument)
        gather_order = _switch(architecture, "train_gather_order") if training else "caller"
        ordered = dict(gather_order=gather_order) if training and sparse.may_use_train_gather(architecture.graph, gather_order) else dict()
        run = lambda k: sparse.ppr_loop(make_adj, H0_value, a, k, relu=with_relu, storage=storage, **ordered)
    return run(iterations), run, (make_adj if cheap else None)


class PPRIteration(Layer):
    """One APPNP power-iteration step (filter.py:6-22): activation(dropout((A.H)(1-a) + H0 a)).

    A RUN of such layers as user code builds it (reference demos/custom_layers.py:8-13: ``for _ in range(10):
    gnn.add(PPRIteration(H0, 0.1))``) executes as one fused loop when the layers are plain -- the same H0 layer, one float restart
    probability, the identity or relu as the activation of ALL of them (relu runs in the kernels' epilogue, gnx_appnp_propagate_act),
    identity restart transform, no feature dropout (in eval mode, where it does not act, any), one graph_dropout -- and the run starts from
    H0's own value: the same arithmetic and the same sequence of edge-dropout masks as layer by layer (bitwise on graphs below
    2^20 vertices; above, narrow widths run on the relabelled copy: float32 rounding), at the cost of the PPRLoop layer.  The last
    layer of the run holds the result; the ``.value`` of an intermediate layer is computed when somebody reads it.
    ``architecture.fuse_runs = False`` switches this off."""

    def __build__(self, architecture: GNN, H0: Layer, restart_probability: float = 0.1, activation=linear,
                  dropout: float = 0, graph_dropout: float = 0.5, restart_transform=linear):
        self.restart_probability = restart_probability
        self.H0 = H0
        self.dropout = dropout
        self.graph_dropout = graph_dropout
        self.activation = activation
        self.restart_transform = restart_transform
        return architecture.top_shape()  # preserves the feature shape

    def __forward__(self, architecture: GNN, features):
        self.G = architecture.get_adjacency(self.graph_dropout)
        a = self.restart_transform(self.restart_probability)
        mixed = sparse.ppr_step(self.G, features, self.H0.value, a)
        return self.activation(architecture.dropout(mixed, self.dropout))

    # ``.value`` (layered.py:79-81) may be pending after a fused run: computed on first read
    @property
    def value(self):
        pending = self.__dict__.get("_pending_value")
        if pending is not None:
            self.__dict__["_value"], self.__dict__["_pending_value"] = pending(), None
        return self.__dict__.get("_value")

    @value.setter
    def value(self, v):
        self.__dict__["_value"], self.__dict__["_pending_value"] = v, None

    def _plain(self, training=True):
        """Whether this layer can be one step of a fused run.  Feature dropout (filter.py:22) only acts in training mode
        (layered.py:44-45): an eval-mode run fuses whatever the layers' ``dropout`` says."""
        a = self.restart_probability
        return (type(self) is PPRIteration and isinstance(a, (int, float)) and not isinstance(a, bool)
                and (self.activation is linear or is_relu(self.activation))
                and self.restart_transform is linear and (self.dropout == 0 or not training) and self.output_regularize == 0)

    def __run__(self, architecture: GNN, features, stack, at):
        training = not isinstance(architecture, GNN) or architecture.is_training()
        if not self._plain(training) or not isinstance(architecture, GNN) or features is not getattr(self.H0, "value", None) \
                or not isinstance(features, torch.Tensor) or not features.is_cuda:
            return None
        run = [self]
        for layer in stack[at + 1:]:
            if not (isinstance(layer, PPRIteration) and layer._plain(training) and layer.H0 is self.H0 and layer is not self
                    and layer.restart_probability == self.restart_probability and layer.graph_dropout == self.graph_dropout
                    and (layer.activation is self.activation or (is_relu(layer.activation) and is_relu(self.activation)))
                    and all(layer is not seen for seen in run)):
                break
            run.append(layer)
        if len(run) < 2:
            return None
        out, upto, make_adj = _propagation_run(architecture, features, float(self.restart_probability), len(run), self.graph_dropout,
                                               with_relu=is_relu(self.activation))
        for k, layer in enumerate(run[:-1]):
            layer.__dict__["_value"], layer.__dict__["_pending_value"] = None, (lambda k=k: upto(k + 1))
        run[-1].value = out
        for k, layer in enumerate(run):                         # filter.py:18 leaves the iteration's adjacency in self.G
            layer.G = make_adj(k, False) if make_adj is not None else None
        return len(run), out


class PPRLoop(Layer):
    """``iterations`` PPRIteration layers (filter.py:34-35) collapsed into one layer and one autograd node:
    same arithmetic and the same sequence of edge-dropout masks as the layer-by-layer form, but no
    per-iteration ``.value`` tensors and no stored activations for the backward (they are not needed: the
    step is linear in H, and dropped adjacencies are regenerated from the counter RNG).  What ``APPNP(..., fused=True)`` builds (an
    explicit opt-in: the default keeps the reference's layer list and fuses at execution, PPRIteration.__run__); only the default
    identity activation / zero feature dropout can be collapsed."""

    def __build__(self, architecture: GNN, H0: Layer, restart_probability: float = 0.1, iterations: int = 10,
                  graph_dropout: float = 0.5):
        self.restart_probability = restart_probability
        self.H0 = H0
        self.iterations = iterations
        self.graph_dropout = graph_dropout
        return architecture.top_shape()

    def __forward__(self, architecture: GNN, features):
        return _propagation_run(architecture, self.H0.value, self.restart_probability, self.iterations, self.graph_dropout)[0]


class APPNP(GNN):
    """filter.py:25-35 -- https://arxiv.org/pdf/1810.05997.pdf"""

    def __init__(self, G, features, num_classes: int, a: float = 0.1, latent_dims=[64], iterations=10,
                 dropout=0.6, graph_dropout=0.5, activation=linear, fused=False, **kwargs):
        """Builds filter.py:30-35's layer list as it stands there: Dropout(0.5), one Dense per latent width, the output Dense (= H0),
        then ``iterations`` PPRIteration layers -- ``layers()`` has the reference's length, order and types, every iteration its own
        ``.value`` / ``.G``.  The container EXECUTES the run of plain PPRIteration layers as one fused loop (PPRIteration.__run__:
        same arithmetic, same sequence of edge-dropout masks, one autograd node in training mode; settled rows skipped, the relabelled
        copy at narrow widths, line-friendly padded widths), so the list costs what the collapsed form costs.
        ``fused=True`` (not in the reference) collapses the iterations into ONE PPRLoop layer explicitly: no per-iteration layer
        objects at all; needs a float restart probability and the identity activation."""
        super().__init__(G, features, **kwargs)
        self.add(Dropout(0.5))
        for latent_dim in latent_dims:
            self.add(Dense(latent_dim, activation=relu, dropout=dropout))
        H0 = self.add(Dense(num_classes, regularize=False))
        if fused:
            if a is None or isinstance(a, torch.Tensor) or activation is not linear:
                raise Exception("APPNP(fused=True) needs a float restart probability and the identity activation")
            self.add(PPRLoop(H0, a, iterations, graph_dropout=graph_dropout))
            return
        for _ in range(iterations):
            self.add(PPRIteration(H0, self.create_var() if a is None else a, graph_dropout=graph_dropout, activation=activation))


class PPRSweep(Layer):
    """experimental_filter.py:7-19: features / HN, HN = ten PPR iterations of ``features * 0 + 1``.  Every column of that operand is
    the same, so HN is ONE scalar per node (sparse.signal_ppr over the width-1 kernels) and the layer one division.  ``get_adjacency()``
    is asked once per forward, with the reference's default ``graph_dropout = 0.5``: in training mode one dropped adjacency serves all
    ten iterations (its values materialised once); in eval mode the signal is a constant of the graph and is kept on the model.
    Where the composition measured faster -- up to 16 feature columns on graphs of at least 2^20 vertices, where appnp_propagate over
    the matrix of ones runs on the relabelled copy -- a training-mode forward takes it (sparse.sweep)."""

    ITERATIONS = 10                             # experimental_filter.py:16

    def __build__(self, architecture: GNN, restart_probability: float = 0.1):
        self.restart_probability = restart_probability
        return architecture.top_shape()  # preserves the feature shape

    def __forward__(self, architecture: GNN, features):
        self.G = architecture.get_adjacency()
        a = float(self.restart_probability)
        cache = getattr(architecture, "_signal_cache", None)
        if cache is None or self.G is not getattr(architecture, "_adjacency_cache", {}).get(("symmetric", "none")):
            return sparse.sweep(self.G, features, a, self.ITERATIONS)
        key = ("ppr", a, self.ITERATIONS)
        if key not in cache:
            cache[key] = sparse.signal_ppr(self.G, None, a, self.ITERATIONS)
        return sparse.sweep(self.G, features, a, self.ITERATIONS, signal=cache[key])


class FastReg(Layer):
    """experimental_filter.py:22-43: passes its input on unchanged and adds -lambda to the objective, lambda the Rayleigh quotient
    sum (f - G f)^2 / sum D f^2 of the one-column signal f = sigmoid(features . W) over the un-normalised adjacency
    (sparse.smoothness: one autograd node over the width-1 kernels).  In training mode that adjacency is dropped at the reference's
    default 0.5 and D is the column sums of those same dropped values (same seed and stream).
    NAMED DEVIATION.  The reference calls ``create_var`` inside ``__forward__``: W is a new [C, 1] variable on every forward, is never
    trained, and the model's variable list grows by one per forward.  A new variable holds zeros (variables.py:6) and only reset()
    initialises it, which train() calls once, ahead of every forward: in the reference as it stands W = 0 in every forward, f = 1/2
    everywhere and -lambda is a constant without a gradient (tests/golden/reference_step_gcniireg.npz records it;
    tests/test_reference_golden_cpu.py holds the restatement with W = 0 to it and asserts what the draw changes).  Here W is instead
    drawn afresh per training-mode forward with the initialiser create_var names as its default, U(+-1/sqrt(shape[1])) = U(+-1) --
    the random projection the layer is evidently written for; with zeros it regularises nothing --, from the counter RNG of the edge
    dropout (one mask stream, drawn AHEAD of the dropped adjacency's: reproducible from the seed, fresh on every replay of a captured
    step), and is NOT registered among the model's variables.  An eval-mode forward keeps the last draw and draws none itself (zeros where there
    has been no training-mode forward yet): nothing reads it, and eval forwards leave the numbering of the mask streams alone.
    On CPU tensors the forward still runs (W from torch's generator), but ``loss()`` needs the device: the adjacency is a GPU handle
    and sparse.smoothness has no CPU form."""

    def __build__(self, architecture: GNN):
        self.output_regularize = 1
        self.internal_shape = (architecture.top_shape()[1], 1)
        self.W = None
        return architecture.top_shape()

    def __forward__(self, architecture: GNN, features):
        self.features = features
        self.architecture = architecture
        if not architecture.is_training():
            # an eval-mode forward draws no mask stream, as in the reference, where no eval forward asks for anything random: ahead of
            # the first training-mode forward W is what the reference's freshly created variable holds, zeros (variables.py:6)
            if self.W is None:
                self.W = torch.zeros(self.internal_shape, dtype=torch.float32, device=features.device)
        else:
            width, bound = self.internal_shape[0], self.internal_shape[1] ** -0.5
            if isinstance(features, torch.Tensor) and features.is_cuda:
                seed, stream = architecture._next_mask_stream()
                self.W = sparse.signal_uniform(architecture.graph, width, bound, seed, stream).reshape(width, 1)
            else:                                   # CPU tensors: torch's generator, as create_var's initialisers draw
                self.W = (torch.rand(self.internal_shape, device=features.device) * 2 - 1) * bound
        return features

    def loss(self):
        G = self.architecture.get_adjacency(normalized="none")
        return -sparse.smoothness(G, self.features, self.W)


class APPNPReg(GNN):
    """experimental_filter.py:46-55: APPNP without the leading Dropout (its FastReg is commented out in the reference)."""

    def __init__(self, G, features, num_classes: int, a: float = 0.1, latent_dims=[64], iterations=10,
                 dropout=0.6, graph_dropout=0.5, activation=linear, **kwargs):
        super().__init__(G, features, **kwargs)
        for latent_dim in latent_dims:
            self.add(Dense(latent_dim, activation=relu, dropout=dropout))
        H0 = self.add(Dense(num_classes, regularize=False))
        for _ in range(iterations):
            self.add(PPRIteration(H0, self.create_var() if a is None else a, graph_dropout=graph_dropout, activation=activation))


class GCNLayer(Layer):
    """gcn.py:77-89: dropout(activation((A.X).W + b)) -- aggregation first, at the input width, as the
    reference computes it.  ``transform_first=True`` opts into the algebraically equal A.(X.W) when the layer
    narrows the features (outputs < inputs): the SpMM then runs at the output width with bias + relu in its
    epilogue (half the gather traffic for 128 -> 64); float32 rounding differs by a few ulp."""

    def __build__(self, gcn, outputs: int, activation=relu, bias: bool = True, dropout: float = 0, graph_dropout: float = 0,
                  transform_first: bool = False):
        self.W = gcn.create_var((gcn.top_shape()[1], outputs))
        self.b = gcn.create_var((1, outputs), "zero") if bias else 0
        self.activation = activation
        self.dropout = dropout
        self.graph_dropout = graph_dropout
        self.transform_first = bool(transform_first) and outputs < gcn.top_shape()[1]
        return (gcn.top_shape()[0], outputs)

    def _fused_gcn(self, gcn, features, adjacency) -> bool:
        """Whether GNN(gcn_layer="fused") applies to this forward (no tensor is read, no mask stream is drawn)."""
        return (_switch(gcn, "gcn_layer") == "fused" and type(self) is GCNLayer and not self.transform_first
                and (self.activation is relu or self.activation is linear)
                and isinstance(features, torch.Tensor) and features.is_cuda and features.dtype == torch.float32
                and features.shape[1] in sparse.GCN_FUSED_WIDTHS and self.W.shape[1] <= features.shape[1]
                and adjacency.diag is None and _eval_storage(gcn) is not torch.bfloat16)

    def __forward__(self, gcn, features):
        adjacency = gcn.get_adjacency(self.graph_dropout)
        if self._fused_gcn(gcn, features, adjacency):
            # GNN(gcn_layer="fused"): the aggregation and the transform in one launch; with feature_dropout="fused" the mask too
            triple = None
            if _switch(gcn, "feature_dropout") == "fused" and gcn.is_training() and 0 < self.dropout < 1:
                triple = gcn._mask_triple(self.dropout)
            out = sparse.gcn_step(adjacency, features, self.W, self.b if isinstance(self.b, torch.Tensor) else None,
                                  relu=self.activation is relu, dropout=triple, edge_dropout="fused",
                                  backward=_switch(gcn, "gcn_backward"))
            return out if triple is not None else gcn.dropout(out, self.dropout)
        if self.transform_first:
            bias = self.b if isinstance(self.b, torch.Tensor) else None
            projected = affine(features, self.W, 0)
            storage = _eval_storage(gcn)
            if self.activation is relu or self.activation is linear:
                out = sparse.spmm_bias_act(adjacency, projected, bias, relu=self.activation is relu, storage=storage)
            else:
                out = self.activation(sparse.spmm_bias_act(adjacency, projected, bias, storage=storage))
            return gcn.dropout(out, self.dropout)
        aggregated_features = sparse.spmm(adjacency, features, storage=_eval_storage(gcn))
        return gcn.dropout(affine(aggregated_features, self.W, self.b, self.activation), self.dropout)


class GCNSpectralPreservingLayer(GCNLayer):
    """gcn.py:92-105: the GCN layer with its bias taken back out after the activation and the surviving half of the dropout
    doubled -- 2 * dropout(act((A.X).W + b) - b).  Same kernels as GCNLayer (the SpMM, then the matrix-core transform with the
    bias and a relu fused); the correction is an elementwise tail.
    On a GNN with ``gcn_spectral="fused"`` the whole layer is ONE launch (gnx_step_spectral_gcn), in training mode with the counter RNG's
    dropout mask instead of torch's, and its backward keeps A . X and one gate bit per element (GNN.__init__)."""

    def _fused_spectral(self, gcn, features, adjacency) -> bool:
        """Whether GNN(gcn_spectral="fused") applies to this forward (no tensor is read, no mask stream is drawn)."""
        return (_switch(gcn, "gcn_spectral") == "fused" and type(self) is GCNSpectralPreservingLayer and not self.transform_first
                and (self.activation is relu or self.activation is linear)
                and isinstance(features, torch.Tensor) and features.is_cuda and features.dtype == torch.float32
                and features.shape[1] in sparse.GCN_FUSED_WIDTHS and self.W.shape[1] <= features.shape[1]
                and adjacency.diag is None and _eval_storage(gcn) is not torch.bfloat16
                and (not gcn.is_training() or 0 <= self.dropout < 1))       # (a rate of 1 or more stays with torch and what it makes of it)

    def __forward__(self, gcn, features):
        adjacency = gcn.get_adjacency(self.graph_dropout)
        if self._fused_spectral(gcn, features, adjacency):
            triple = gcn._mask_triple(self.dropout) if gcn.is_training() and self.dropout != 0 else None
            return sparse.gcn_step_spectral(adjacency, features, self.W, self.b if isinstance(self.b, torch.Tensor) else None,
                                            relu=self.activation is relu, dropout=triple, edge_dropout="fused",
                                            backward=_switch(gcn, "gcn_backward"))
        activated = affine(sparse.spmm(adjacency, features), self.W, self.b, self.activation)
        return 2 * gcn.dropout(activated - self.b, self.dropout)


class GCN(GNN):
    """gcn.py:108-113 (the last layer keeps the default relu, as in the reference)."""

    def __init__(self, G, features, num_classes, latent_dims=[64], layer_type=GCNLayer, transform_first=False, **kwargs):
        super().__init__(G, features, **kwargs)
        extra = dict(transform_first=True) if transform_first else dict()
        for latent_dim in latent_dims:
            self.add(layer_type(latent_dim, graph_dropout=0.5, dropout=0.5, **extra))
        self.add(layer_type(num_classes, **extra))


class GCNIILayer(Layer):
    """gcn.py:7-27: dropout(act(((1-a) A.H + a H0) . ((1-b) I + b W))), b = beta_transformer(l / (k+1)).
    ONE launch per layer for C in {16, 32, 64} -- the mixed rows stay in LDS and meet (1-b) I + b W on the matrix cores
    (gnx_gcnii_step); in training the same launch also writes the mixed rows once (dW needs them) instead of a second launch
    reading them back.  On a GNN with ``feature_dropout="fused"`` the training-mode dropout is part of that launch too
    (gnx_gcnii_step_drop; GNN.__init__).

    On a GNN with ``inference_dtype=torch.bfloat16`` a RUN of consecutive plain GCNIILayer layers (this class itself, relu or the
    identity as activation, no add_eye) in an eval-mode forward without autograd executes as one bf16 chain
    (sparse.gcnii_chain_bf16 over gnx_gcnii_step_bf16): the run's input is rounded to bf16 once, every layer but the run's last
    stores its rows rounded once to bf16 -- what the next layer gathers -- and the last one writes f32; sums, each layer's f32 H0,
    the mix and the transform stay f32 (dropout is the identity in eval mode, so nothing sits between the layers).  The ``.value``
    of an inner layer of the run is the exact widening of its bf16 rows, computed when somebody reads it.  Widths outside
    sparse.GCNII_BF16_MIN_WIDTH ... GCNII_BF16_MAX_WIDTH, every forward under autograd or in training mode, and
    GCNIISpectralPreservingLayer keep the f32 path and its bits.  ``architecture.fuse_runs = False`` switches the chain off.

    On a GNN with ``gcnii_training_dtype=torch.bfloat16`` a run of such layers in TRAINING mode executes as one autograd node over
    bf16 rows (sparse.gcnii_train_run_bf16; the conditions and the rounding points: GNN.__init__)."""

    # ``.value`` may be pending after a bf16 run: computed on first read (as PPRIteration's)
    @property
    def value(self):
        pending = self.__dict__.get("_pending_value")
        if pending is not None:
            self.__dict__["_value"], self.__dict__["_pending_value"] = pending(), None
        return self.__dict__.get("_value")

    @value.setter
    def value(self, v):
        self.__dict__["_value"], self.__dict__["_pending_value"] = v, None

    def _transform(self):
        b = self.beta_transformer(self.l / (self.k + 1))
        eye = torch.eye(self.W.shape[1], device=self.W.device, dtype=self.W.dtype)
        return (1 - b) * eye + b * self.W

    def _bf16_plain(self, gcn) -> bool:
        """Whether this layer can be one step of a bf16 run (the caller has established eval mode without autograd)."""
        width = self.W.shape[1]
        return (type(self) is GCNIILayer and (self.activation is relu or self.activation is linear)
                and isinstance(self.a, (int, float)) and not isinstance(self.a, bool)
                and sparse.GCNII_BF16_MIN_WIDTH <= width <= sparse.GCNII_BF16_MAX_WIDTH
                and isinstance(getattr(self.H0, "value", None), torch.Tensor)
                and gcn.get_adjacency(self.graph_dropout).diag is None)

    def _bf16_train_plain(self, gcn, first) -> bool:
        """Whether this layer can be one step of a training-mode bf16 run that ``first`` starts (the run's own conditions: _bf16_train_run)."""
        fused_drop = _switch(gcn, "feature_dropout") == "fused" and 0 < self.dropout < 1
        return (type(self) is GCNIILayer and (self.activation is relu or self.activation is linear)
                and isinstance(self.a, (int, float)) and not isinstance(self.a, bool)
                and (self.dropout == 0 or fused_drop) and self.graph_dropout == first.graph_dropout
                and self.W.shape[1] == first.W.shape[1] and isinstance(getattr(self.H0, "value", None), torch.Tensor))

    def _bf16_train_run(self, gcn, stack, at):
        """The layers of the training-mode bf16 run that starts with this layer (GNN.__init__ ``gcnii_training_dtype``), or None where
        today's path applies.  Looks at the model alone -- no tensor is read, no mask stream is drawn -- so it can be asked anywhere."""
        if not (isinstance(gcn, GNN) and _switch(gcn, "gcnii_training_dtype") is torch.bfloat16 and gcn.fuse_runs
                and gcn.is_training() and torch.is_grad_enabled()):
            return None
        width = self.W.shape[1]
        # (graph_dropout != 0 is a DroppedAdjacency in training mode: its weights are made in the SpMM, and asking for it draws a stream)
        if (self.graph_dropout != 0 or width not in sparse.GCNII_BF16_TRAIN_WIDTHS or width < sparse.GCNII_BF16_TRAIN_MIN_WIDTH
                or gcn.graph.n_rows < sparse.GCNII_BF16_TRAIN_MIN_ROWS or gcn.graph.n_rows != gcn.graph.n_cols
                or not self._bf16_train_plain(gcn, self) or gcn.get_adjacency(self.graph_dropout).diag is not None):
            return None
        run = [self]
        for layer in stack[at + 1:]:
            # (a layer whose H0 is a layer INSIDE the run would need that layer's value first: it ends the run)
            if not (isinstance(layer, GCNIILayer) and layer._bf16_train_plain(gcn, self)
                    and all(layer is not seen and layer.H0 is not seen for seen in run)):
                break
            run.append(layer)
        return run if len(run) >= 2 else None

    def _run_bf16_training(self, gcn, features, run):
        adjacency = gcn.get_adjacency(self.graph_dropout)
        steps = []
        for layer in run:                                       # the mask streams in layer order: those of the f32 "fused" path
            triple = gcn._mask_triple(layer.dropout) if layer.dropout != 0 else None
            steps.append((layer.H0.value, float(layer.a), layer._transform(), layer.activation is relu, triple))
        stored = []
        out = sparse.gcnii_train_run_bf16(adjacency, features, steps, stored=stored,
                                          weight_gradient=_switch(gcn, "gcnii_weight_gradient"))
        for k, layer in enumerate(run[:-1]):
            layer.__dict__["_value"] = None
            layer.__dict__["_pending_value"] = lambda k=k: stored[k].float()
        run[-1].value = out
        return len(run), out

    def __run__(self, gcn, features, stack, at):
        if isinstance(features, torch.Tensor) and features.is_cuda and features.dtype == torch.float32:
            run = self._bf16_train_run(gcn, stack, at)
            if run is not None:
                return self._run_bf16_training(gcn, features, run)
        if _eval_storage(gcn) is not torch.bfloat16 or not isinstance(features, torch.Tensor) or not features.is_cuda \
                or not self._bf16_plain(gcn):
            return None
        run = [self]
        for layer in stack[at + 1:]:
            # (a layer whose H0 is a layer INSIDE the run would need that layer's value first: it ends the run)
            if not (isinstance(layer, GCNIILayer) and layer._bf16_plain(gcn) and layer.graph_dropout == self.graph_dropout
                    and all(layer is not seen and layer.H0 is not seen for seen in run)):
                break
            run.append(layer)
        adjacency = gcn.get_adjacency(self.graph_dropout)
        steps = [(layer.H0.value, float(layer.a), layer._transform(), layer.activation is relu) for layer in run]
        out = sparse.gcnii_chain_bf16(adjacency, features, steps)
        for k, layer in enumerate(run[:-1]):
            layer.__dict__["_value"] = None
            layer.__dict__["_pending_value"] = lambda k=k: sparse.gcnii_chain_bf16(adjacency, features, steps[:k + 1], widen_last=True)
        run[-1].value = out
        return len(run), out

    def __build__(self, architecture, H0: Layer, a: float, l: float, k: int = 0, activation=linear,
                  beta_transformer=math.log1p, dropout: float = 0.5, graph_dropout: float = 0.5, regularization=True):
        width = architecture.top_shape()[1]
        self.W = architecture.create_var((width, width), "zero", regularize=regularization)
        self.a, self.l, self.k = a, l, k
        self.activation = activation
        self.dropout = dropout
        self.graph_dropout = graph_dropout
        self.H0 = H0
        self.beta_transformer = beta_transformer
        return architecture.top_shape()

    def __forward__(self, gcn, features):
        transform = self._transform()
        adjacency = gcn.get_adjacency(self.graph_dropout)
        if features.is_cuda and adjacency.diag is None:
            fused_act = self.activation is relu or self.activation is linear
            # GNN(gcnii_weight_gradient="recomputed"): plain layers alone (the argument is passed only where it can change the path)
            wgrad = dict(weight_gradient="recomputed") if (_switch(gcn, "gcnii_weight_gradient") == "recomputed"
                                                           and type(self) is GCNIILayer and fused_act) else dict()
            # GNN(gcnii_edge_dropout="fused"): plain training layers over a DroppedAdjacency alone (passed only where it can change the path)
            if (_switch(gcn, "gcnii_edge_dropout") == "fused" and type(self) is GCNIILayer and fused_act and gcn.is_training()
                    and isinstance(adjacency, sparse.DroppedAdjacency) and features.dtype == torch.float32 and not wgrad
                    and isinstance(self.a, (int, float)) and not isinstance(self.a, bool)):
                wgrad = dict(edge_dropout="fused")
            if (_switch(gcn, "feature_dropout") == "fused" and type(self) is GCNIILayer and fused_act and gcn.is_training()
                    and 0 < self.dropout < 1):                      # (a rate of 1 or more stays with gcn.dropout and what torch makes of it)
                # GNN(feature_dropout="fused"): dropout(act(...)) leaves the layer's launch, its mask from the counter RNG
                return sparse.gcnii_step(adjacency, features, self.H0.value, self.a, transform, relu=self.activation is relu,
                                         backward=_switch(gcn, "gcnii_backward"), dropout=gcn._mask_triple(self.dropout), **wgrad)
            out = sparse.gcnii_step(adjacency, features, self.H0.value, self.a, transform, relu=self.activation is relu,
                                    backward=_switch(gcn, "gcnii_backward"), **wgrad)
            return gcn.dropout(out if fused_act else self.activation(out), self.dropout)
        tradeoff = sparse.ppr_step(adjacency, features, self.H0.value, self.a)
        return gcn.dropout(self.activation(torch.matmul(tradeoff, transform)), self.dropout)


class GCNIISpectralPreservingLayer(GCNIILayer):
    """gcn.py:30-51: GCNIILayer with a bias added before the activation and removed after it, and the dropout's survivors
    doubled: 2 * dropout(act(T.M + bias) - bias), T = (1-a) A.H + a H0, M = (1-b) I + b W.  The propagation + mix is the fused
    SpMM kernel; the transform carries the bias and the relu in the matrix-core kernel's epilogue.
    On a GNN with ``gcnii_spectral="fused"`` the whole layer is ONE launch (gnx_gcnii_step_spectral), in training mode with the
    counter RNG's dropout mask instead of torch's, and its backward keeps the mixed rows and one gate bit per element (GNN.__init__)."""

    def __build__(self, architecture, H0, a, l, k=0, **kwargs):
        shape = super().__build__(architecture, H0, a, l, k, **kwargs)
        self.bias = architecture.create_var((1, shape[1]), "zero")
        return shape

    def _fused_spectral(self, gcn, features, adjacency) -> bool:
        """Whether GNN(gcnii_spectral="fused") applies to this forward (no tensor is read, no mask stream is drawn)."""
        return (_switch(gcn, "gcnii_spectral") == "fused" and type(self) is GCNIISpectralPreservingLayer
                and (self.activation is relu or self.activation is linear)
                and isinstance(features, torch.Tensor) and features.is_cuda and features.dtype == torch.float32
                and isinstance(self.a, (int, float)) and not isinstance(self.a, bool)
                and not isinstance(adjacency, sparse.DroppedAdjacency) and adjacency.diag is None
                and (not gcn.is_training() or 0 <= self.dropout < 1))       # (a rate of 1 or more stays with torch and what it makes of it)

    def __forward__(self, gcn, features):
        adjacency = gcn.get_adjacency(self.graph_dropout)
        if self._fused_spectral(gcn, features, adjacency):
            triple = gcn._mask_triple(self.dropout) if gcn.is_training() and self.dropout != 0 else None
            return sparse.gcnii_step_spectral(adjacency, features, self.H0.value, self.a, self._transform(), self.bias,
                                              relu=self.activation is relu, dropout=triple,
                                              backward=_switch(gcn, "gcnii_backward"))
        b = self.beta_transformer(self.l / (self.k + 1))
        eye = torch.eye(self.W.shape[1], device=self.W.device, dtype=self.W.dtype)
        tradeoff = sparse.ppr_step(adjacency, features, self.H0.value, self.a)
        activated = affine(tradeoff, (1 - b) * eye + b * self.W, self.bias, self.activation)
        return 2 * gcn.dropout(activated - self.bias, self.dropout)


class GCNII(GNN):
    """gcn.py:54-74 -- http://proceedings.mlr.press/v119/chen20v/chen20v.pdf"""

    def __init__(self, graph, features, num_classes, a: float = 0.1, l: float = 0.5, latent_dims=[64], iterations=64,
                 dropout=0.6, convolution_regularization=True, layer_type=GCNIILayer, **kwargs):
        super().__init__(graph, features, **kwargs)
        self.add(Dropout(dropout))
        for latent_dim in latent_dims:
            self.add(Dense(latent_dim, dropout=0, activation=relu))
        H0 = self.top_layer()
        for iteration in range(iterations):
            self.add(layer_type(H0, a, l, iteration, activation=relu, dropout=dropout, graph_dropout=0,
                                regularization=convolution_regularization))
        self.add(Dense(num_classes, dropout=0, regularize=False))


class GCNIIReg(GNN):
    """experimental_gcn.py:9-29: GCNII whose pre-MLP Dense layers carry the feature dropout themselves, with FastReg behind H0."""

    def __init__(self, graph, features, num_classes, a: float = 0.1, l: float = 0.5, latent_dims=[64], iterations=64,
                 dropout=0.6, convolution_regularization=True, **kwargs):
        super().__init__(graph, features, **kwargs)
        self.add(Dropout(dropout))
        for latent_dim in latent_dims:
            self.add(Dense(latent_dim, dropout=dropout, activation=relu))
        H0 = self.top_layer()
        self.add(FastReg())
        for iteration in range(iterations):
            self.add(GCNIILayer(H0, a, l, iteration, activation=relu, dropout=dropout, graph_dropout=0,
                                regularization=convolution_regularization))
        self.add(Dense(num_classes, dropout=0, regularize=False))


def leaky_relu(x):
    return torch.nn.functional.leaky_relu(x, 0.2)          # tf.nn.leaky_relu's default slope


class NGCFLayer(Layer):
    """gcn.py:116-135: with A = the BIPARTITE-normalised adjacency (rows scaled by 1 / column sum, gnn.py:43-45),
    l2_normalize(dropout(act((X * (A.X)).W1 + b1) + act((A.X).W2 + b2))).  The adjacency is taken ONCE, at build time
    (gcn.py:127) -- so a ``node_dropout`` is one fixed mask, drawn while the fresh architecture is still in training mode."""

    def __build__(self, gcn, outputs: int, activation=leaky_relu, bias: bool = True, dropout: float = 0, node_dropout: float = 0,
                  regularize: float = 1):
        rows, width = gcn.top_shape()
        spread = 1. / rows ** 0.5
        self.W1 = gcn.create_var((width, outputs), regularize=regularize, normalization=spread)
        self.W2 = gcn.create_var((width, outputs), regularize=regularize, normalization=spread)
        self.b1 = gcn.create_var((1, outputs), normalization=spread) if bias else 0
        self.b2 = gcn.create_var((1, outputs), normalization=spread) if bias else 0
        self.activation, self.dropout, self.node_dropout = activation, dropout, node_dropout
        self.adjacency = gcn.get_adjacency(self.node_dropout, add_eye="none", normalized="bipartite")
        return rows, outputs

    def _fused_ngcf(self, gcn, features) -> bool:
        """Whether GNN(ngcf_layer="fused") applies to this forward (no tensor is read, no mask stream is drawn); at an input width of
        128 only together with GNN(ngcf_wide="fused")."""
        widths = sparse.NGCF_FUSED_WIDTHS + (sparse.NGCF_WIDE_WIDTHS if _switch(gcn, "ngcf_wide") == "fused" else ())
        return (_switch(gcn, "ngcf_layer") == "fused" and type(self) is NGCFLayer
                and (self.activation is leaky_relu or self.activation is relu or self.activation is linear)
                and isinstance(self.b1, torch.Tensor) == isinstance(self.b2, torch.Tensor)
                and isinstance(features, torch.Tensor) and features.is_cuda and features.dtype == torch.float32
                and features.shape[1] in widths and self.W1.shape[1] <= features.shape[1]
                and self.adjacency.diag is None)

    def __forward__(self, gcn, features):
        if self._fused_ngcf(gcn, features):
            # GNN(ngcf_layer="fused"): the whole layer in one launch; with torch's dropout in training the launch stops before the norm
            act = "leaky" if self.activation is leaky_relu else "relu" if self.activation is relu else "none"
            b1, b2 = (self.b1, self.b2) if isinstance(self.b1, torch.Tensor) else (None, None)
            # GNN(ngcf_backward=): named only where it is not the default, so the default's calls stay today's, argument for argument
            how = _switch(gcn, "ngcf_backward")
            back = dict() if how == "composed" else dict(backward=how)
            # GNN(ngcf_wide=): likewise, and only at the widths it acts on
            wide = _switch(gcn, "ngcf_wide")
            if wide != "composed" and features.shape[1] in sparse.NGCF_WIDE_WIDTHS:
                back["wide"] = wide
            # GNN(ngcf_wide_backward=): likewise
            wide_back = _switch(gcn, "ngcf_wide_backward")
            if wide_back != "composed" and features.shape[1] in sparse.NGCF_WIDE_WIDTHS:
                back["wide_backward"] = wide_back
            if not gcn.is_training() or self.dropout == 0:
                return sparse.ngcf_step(self.adjacency, features, self.W1, b1, self.W2, b2, activation=act, **back)
            if _switch(gcn, "feature_dropout") == "fused" and 0 < self.dropout < 1:
                triple = gcn._mask_triple(self.dropout)
                return sparse.ngcf_step(self.adjacency, features, self.W1, b1, self.W2, b2, activation=act, dropout=triple, **back)
            summed = sparse.ngcf_step(self.adjacency, features, self.W1, b1, self.W2, b2, activation=act, normalize=False, **back)
            return torch.nn.functional.normalize(gcn.dropout(summed, self.dropout), dim=1, eps=1e-12)
        aggregated = sparse.spmm(self.adjacency, features)                       # the propagation kernel
        interaction = self.activation(affine(features * aggregated, self.W1, self.b1))
        message = self.activation(affine(aggregated, self.W2, self.b2))
        return torch.nn.functional.normalize(gcn.dropout(interaction + message, self.dropout), dim=1, eps=1e-12)


class NGCF(GNN):
    """gcn.py:138-154 -- https://dl.acm.org/doi/pdf/10.1145/3468264.3468552.  The closing Concatenate stacks the layers'
    outputs along axis 0 exactly like the reference's (layers.py:98-101), so rows 0..N-1 of the output are the FIRST layer's
    embeddings -- which is what the link tasks index."""

    def __init__(self, graph, features, num_classes: int, latent_dims=None, dropout=0.1, **kwargs):
        super().__init__(graph, features, **kwargs)
        widths = [num_classes] * 2 if latent_dims is None else list(latent_dims)
        stack = [self.add(NGCFLayer(width, regularize=0.0, dropout=dropout, output_regularize=1)) for width in widths + [num_classes]]
        self.add(Concatenate(stack))


class MLP(Trainable):
    """The graph-free baseline (reference gnntf/core/nn/architectures/mlp.py:6-12): it falls out of the
    generic layers; no propagation kernel is involved."""

    def __init__(self, features, num_classes: int, latent_dims=[64], dropout: float = 0.5):
        super().__init__(features)
        self.add(Dropout(dropout))
        for latent_dim in latent_dims:
            self.add(Dense(latent_dim, dropout=dropout, activation=relu))
        self.add(Dense(num_classes, regularize=False))

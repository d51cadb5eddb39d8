"""gnntf on MI355X: the reference's flat namespace (reference gnntf/__init__.py:1-2) over a
HIP propagation path.  ``import gnntf`` then ``gnntf.APPNP``, ``gnntf.graph2adj``,
``gnntf.NodeClassification`` ... work as in the reference's README and demos."""
from .metrics import set_seed, acc, auc, avprec, rec, prec, f1
from .params import WrappedVariable, VariableGenerator, set_default_device, default_device
from .protocol import Layer, Layered
from .blocks import Dense, Dropout, Activation, Branch, Resume, Concatenate, Tradeoff, relu, linear
from .training import Predictor, Trainable
from .tasks import NodeClassification
from .link_tasks import LinkPrediction, MeanLinkPrediction, negative_sampling, device_negative_sampling, recommend_all, recommend, ranking_metrics
from .sparse import (SparseCOO, DeviceGraph, Adjacency, SparseRows, spmm, spmm_bias_act, ppr_step, ppr_loop, appnp_propagate, gather_rows, normalize,
                     as_coo, dense, dense_step, sparse_dense, gcn_step, gcn_step_spectral, gcn_step_back, ngcf_step, gcnii_step, gcnii_step_spectral, gcnii_step_back, gcnii_train_run_bf16, gcnii_wgrad, feature_dropout, node_ce, node_argmax, edge_scores,
                     sample_negatives, DeviceIndex, EdgePlan, rank_candidates, RankResult,
                     signal_project, signal_spmv, signal_ppr, signal_colsum, sweep, smoothness)
from .graph_io import create_nx_graph, adj2graph, graph2indices, graph2adj
from .graph_model import (MLP, GNN, Structural, NGCFLayer, NGCF, PPRIteration, PPRLoop, APPNP, GCNLayer, GCNSpectralPreservingLayer, GCN, GCNIILayer,
                          GCNIISpectralPreservingLayer, GCNII, PPRSweep, FastReg, APPNPReg, GCNIIReg)
from .datasets import load_npz, save_npz

__version__ = "0.1.0"

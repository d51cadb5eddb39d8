"""The keyword checks of GNN.__init__: every string switch and each of the three dtype keywords refuses a bad value with its message,
and a call with two bad keywords raises the one the order of the checks reaches first.  The checks run before the constructor
touches the graph or the features, so no device is needed (and none is given: both are None)."""
import pytest

from gnntf.graph_model import GNN

# (keyword, the message of a bad value), in the order GNN.__init__ checks them
MESSAGES = [
    ("dense_dropout", "GNN: dense_dropout must be one of 'torch', 'fused'"),
    ("gcn_spectral", "GNN: gcn_spectral must be one of 'composed', 'fused'"),
    ("ngcf_layer", "GNN: ngcf_layer must be one of 'composed', 'fused'"),
    ("ngcf_backward", "GNN: ngcf_backward must be one of 'composed', 'fused'"),
    ("ngcf_wide", "GNN: ngcf_wide must be one of 'composed', 'fused'"),
    ("ngcf_wide_backward", "GNN: ngcf_wide_backward must be one of 'composed', 'fused'"),
    ("gcn_backward", "GNN: gcn_backward must be one of 'composed', 'fused'"),
    ("gcn_layer", "GNN: gcn_layer must be one of 'composed', 'fused'"),
    ("gcnii_edge_dropout", "GNN: gcnii_edge_dropout must be one of 'composed', 'fused'"),
    ("gcnii_spectral", "GNN: gcnii_spectral must be one of 'composed', 'fused'"),
    ("feature_dropout", "GNN: feature_dropout must be one of 'torch', 'fused'"),
    ("gcnii_backward", "GNN: gcnii_backward must be one of 'composed', 'fused'"),
    ("train_gather_order", "GNN: train_gather_order must be one of 'caller', 'relabelled', 'auto'"),
    ("inference_dtype", "GNN: inference_dtype must be torch.float32 or torch.bfloat16"),
    ("training_dtype", "GNN: training_dtype must be torch.float32 or torch.bfloat16"),
    ("gcnii_training_dtype", "GNN: gcnii_training_dtype must be torch.float32 or torch.bfloat16"),
    ("gcnii_weight_gradient", "GNN: gcnii_weight_gradient must be one of 'stored', 'recomputed'"),
]
BAD = "neither"           # no switch takes it, and it is no dtype


def raised(**keywords) -> str:
    with pytest.raises(Exception) as caught:
        GNN(None, None, **keywords)
    return str(caught.value)


def test_the_table_names_every_keyword_once():
    names = [keyword for keyword, _ in MESSAGES]
    assert len(set(names)) == len(names) == 17


@pytest.mark.parametrize("keyword,message", MESSAGES, ids=[keyword for keyword, _ in MESSAGES])
def test_a_bad_value_raises_the_keywords_message(keyword, message):
    assert raised(**{keyword: BAD}) == message
    assert raised(**{keyword: None}) == message


@pytest.mark.parametrize("at", range(len(MESSAGES) - 1), ids=[f"{a[0]}-before-{b[0]}" for a, b in zip(MESSAGES, MESSAGES[1:])])
def test_two_bad_keywords_raise_the_one_checked_first(at):
    (first, message), (second, _) = MESSAGES[at], MESSAGES[at + 1]
    assert raised(**{second: BAD, first: BAD}) == message


def test_the_order_of_the_checks_is_not_the_order_of_the_signature():
    # dense_dropout is the signature's last keyword and the first one checked; gcnii_weight_gradient is checked after the dtypes
    assert raised(inference_dtype=BAD, dense_dropout=BAD) == "GNN: dense_dropout must be one of 'torch', 'fused'"
    assert raised(gcnii_weight_gradient=BAD, gcnii_training_dtype=BAD) == "GNN: gcnii_training_dtype must be torch.float32 or torch.bfloat16"
    assert raised(**{keyword: BAD for keyword, _ in MESSAGES}) == "GNN: dense_dropout must be one of 'torch', 'fused'"

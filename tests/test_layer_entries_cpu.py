"""What the entries of the four layer units answer to a NULL handle, without a device: gnx_gcnii.hip (13 entries), gnx_gcn.hip (4),
gnx_ngcf.hip (2) and gnx_feature_dropout.hip (3) -- the return code and the gnx_last_error() text of the first check each entry makes,
which carries the `fn` string the entry hands to its host path (gcnii_forward, gcn_backward, make_feat_drop, ...): the one thing a
move of an entry between units most easily breaks.  Pointers are fake and never dereferenced: each call fails before anything is
looked at or launched.  The texts were recorded from the library as it was before the units were split, not read off the code."""
import ctypes

import pytest

P = [ctypes.c_void_p(0x1000 * (i + 1)) for i in range(12)]      # twelve distinct fake device buffers
INVALID = -1
RELU = 1
DROP = (0.5, 7, 3)                  # dropout_p, seed, stream_id
EDGE = (P[11], 0.25, 11, 5)         # d_D, edge_p, edge_seed, edge_stream
WORK_FLOATS = 1 << 20

# entry -> (the arguments behind the handle, what gnx_last_error() says); widths 16 (C, C_in) and 8 (C_out), 100 rows
ENTRIES = {
    "gnx_gcnii_step": ((P[0], P[1], P[2], 0.1, 16, P[3], 16, RELU, P[4], P[5], None), "gnx_gcnii_step: NULL handle"),
    "gnx_gcnii_step_drop": ((P[0], P[1], P[2], 0.1, 16, P[3], 16, RELU, *DROP, P[4], P[5], None), "gnx_gcnii_step_drop: NULL handle"),
    "gnx_gcnii_step_dropped": ((*EDGE, P[1], P[2], 0.1, 16, P[3], 16, RELU, *DROP, P[4], P[5], None), "gnx_gcnii_step_dropped: NULL handle"),
    "gnx_gcnii_step_spectral": ((P[0], P[1], P[2], 0.1, 16, P[3], 16, P[6], RELU, *DROP, P[4], P[5], P[7], None),
                                "gnx_gcnii_step_spectral: NULL handle"),
    "gnx_gcnii_spectral_back": ((P[0], 16, P[7], 100, 16, RELU, *DROP, P[1], 16, P[2], P[3], WORK_FLOATS, None),
                                "gnx_gcnii_spectral_back: NULL handle"),
    "gnx_gcnii_step_bf16": ((P[0], P[1], P[2], 0.1, 16, P[3], 16, RELU, P[4], 1, P[5], None), "gnx_gcnii_step_bf16: NULL handle"),
    "gnx_gcnii_step_train_bf16": ((P[0], P[1], P[2], 0.1, 16, P[3], 16, RELU, *DROP, P[4], 1, P[5], P[6], None),
                                  "gnx_gcnii_step_train_bf16: NULL handle"),
    "gnx_gcnii_step_drop_bf16": ((P[0], P[1], P[2], 0.1, 16, P[3], 16, RELU, *DROP, P[4], 1, P[5], None),
                                 "gnx_gcnii_step_drop_bf16: NULL handle"),
    "gnx_gcnii_step_back": ((P[0], P[1], 0.1, 16, P[2], 16, P[3], P[4], 0.9, P[5], P[6], None), "gnx_gcnii_step_back: NULL handle"),
    "gnx_gcnii_step_back_dropped": ((*EDGE, P[1], 0.1, 16, P[2], 16, P[3], P[4], 0.9, P[5], P[6], None),
                                    "gnx_gcnii_step_back_dropped: NULL handle"),
    "gnx_gcnii_step_back_bf16": ((P[0], P[7], P[1], 0.1, 16, P[2], 16, P[3], P[4], 0.9, P[5], P[6], None),
                                 "gnx_gcnii_step_back_bf16: NULL handle"),
    "gnx_gcnii_wgrad": ((P[0], P[1], P[2], 0.1, 16, P[3], P[4], P[5], P[6], WORK_FLOATS, None), "gnx_gcnii_wgrad: NULL handle"),
    "gnx_gcnii_wgrad_bf16": ((P[0], P[1], P[2], 0.1, 16, P[3], P[4], P[5], P[6], WORK_FLOATS, None), "gnx_gcnii_wgrad_bf16: NULL handle"),
    "gnx_gcn_step": ((P[0], P[1], 16, 16, P[2], 8, 8, P[3], RELU, *DROP, P[4], 8, P[5], P[6], None), "gnx_gcn_step: NULL handle"),
    "gnx_gcn_step_dropped": ((*EDGE, P[1], 16, 16, P[2], 8, 8, P[3], RELU, *DROP, P[4], 8, P[5], P[6], None),
                             "gnx_gcn_step_dropped: NULL handle"),
    "gnx_gcn_step_back": ((P[0], P[1], 8, 8, P[2], 16, 16, P[3], 16, P[4], WORK_FLOATS, None), "gnx_gcn_step_back: NULL handle"),
    "gnx_gcn_step_back_dropped": ((*EDGE, P[1], 8, 8, P[2], 16, 16, P[3], 16, P[4], WORK_FLOATS, None),
                                  "gnx_gcn_step_back_dropped: NULL handle"),
    "gnx_ngcf_step": ((P[0], P[1], 16, 16, P[2], 8, P[3], 8, 8, P[4], P[5], RELU, *DROP, 1, P[6], 8, P[7], P[8], P[9], P[10], WORK_FLOATS,
                       None), "gnx_ngcf_step: NULL handle"),
    "gnx_ngcf_back_gate": ((P[0], 8, P[1], 8, P[2], P[3], 100, 8, RELU, *DROP, P[4], P[5], 8, None), "gnx_ngcf_back_gate: NULL handle"),
    "gnx_feature_dropout": ((P[0], 16, 100, 16, None, *DROP, P[1], 16, None), "gnx_feature_dropout: NULL handle"),
    "gnx_feature_dropout_back": ((P[0], 16, P[1], 16, 100, 16, *DROP, RELU, P[2], 16, None), "gnx_feature_dropout_back: NULL handle"),
    "gnx_feature_dropout_back_bf16": ((P[0], 16, P[1], 16, 100, 16, *DROP, RELU, P[2], 16, P[3], 16, None),
                                      "gnx_feature_dropout_back_bf16: NULL handle"),
}


def lib():
    from gnntf import _native
    return _native.lib()


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_null_handle_is_refused_under_the_entrys_own_name(entry):
    args, text = ENTRIES[entry]
    assert getattr(lib(), entry)(None, *args) == INVALID
    assert lib().gnx_last_error().decode() == text


def test_every_entry_of_the_layer_units_is_listed():
    from gnntf import _native
    bound = {name for name in _native.SIGNATURES if name.startswith(("gnx_gcnii_", "gnx_gcn_", "gnx_ngcf_", "gnx_feature_dropout"))}
    assert bound == set(ENTRIES)

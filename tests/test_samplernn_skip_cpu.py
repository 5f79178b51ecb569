"""Skip-connection stacks on the device-resident SampleRNN generator (PARROT_SR_SKIP_STACKS,
samplernn_generate_set_skip_stacks), as far as they can be checked without a GPU: the header and the signatures, the guard
in front of every entry with the switch set and unset, the parameter names the plan gathers against the oracle's
parameter dictionary, and the switch's row in switches.h."""
import ctypes as C
import os
import re

import pytest

from oracle import samplernn_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCH = "PARROT_SR_SKIP_STACKS"

# the descriptor as it was before the setter existed: its fields in order
DESC_FIELDS = (
    "B D T Q FS BFS feat_dim use_graph top_k temperature draw_mode seed "
    "big_Win_frames big_Win_feats big_bin big_U big_bU big_Wg big_Wc big_Wout big_bout frm_Win frm_bin frm_U frm_bU frm_Wg "
    "frm_Wc frm_Wout frm_bout emb_tbl W2 b2 W3 b3 W4 b4 features samples big_h frm_h xf_big xf_frm feat_cur gru_in P z r rh "
    "big_out frame_out o1 o2 o3 logits tbase n_rnn lstm big_L frm_L big_hs big_cs frm_hs frm_cs gate_ws layer_tmp persist_ws "
    "persist_ws_floats starts big_h0 frm_h0").split()


@pytest.fixture()
def tt():
    from parrot_amd.sampleRNN.models.conditional import three_tier
    yield three_tier
    three_tier.configure(DIM=1024, EMB_SIZE=256, RNN_TYPE='GRU', N_RNN=1, SKIP_CONN=False)


# ---- 1. the ABI ----------------------------------------------------------------------------------------------------------
def test_header_and_signatures():
    from parrot_amd import _lib
    txt = open(os.path.join(ROOT, "include", "parrot_hip.h")).read()
    assert re.search(r"int samplernn_generate_set_skip_stacks\(void\* plan, const SampleRnnSkipStacks\* skip\);", txt)
    body = re.search(r"typedef struct SampleRnnSkipStacks \{(.*?)\} SampleRnnSkipStacks;", txt, re.S).group(1)
    names = re.findall(r"\*\s*(\w+)", body)
    assert names == [n for n, _ in _lib.SampleRnnSkipStacks._fields_]
    assert names == ["big_S", "frm_S", "big_bS", "frm_bS", "big_sum", "frm_sum"]
    assert C.sizeof(_lib.SampleRnnSkipStacks) == 14 * C.sizeof(C.c_void_p)
    res, args = _lib.SIGNATURES["samplernn_generate_set_skip_stacks"]
    assert res is C.c_int and args[0] is C.c_void_p and args[1]._type_ is _lib.SampleRnnSkipStacks and len(args) == 2
    # the descriptor did not change by a byte
    assert [n for n, _ in _lib.SampleRnnGenDesc._fields_] == DESC_FIELDS
    assert C.sizeof(_lib.SampleRnnGenDesc) == 936
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "samplernn_generate_set_skip_stacks" in doc and "SampleRnnSkipStacks" in doc and SWITCH in doc


def test_c_entry_refuses_null_arguments():
    from parrot_amd import _lib
    lib = _lib.load()
    s = _lib.SampleRnnSkipStacks()
    assert lib.samplernn_generate_set_skip_stacks(None, C.byref(s)) == 10001     # PARROT_ERR_BADARG, no device call
    buf = (C.c_float * 4)()
    assert lib.samplernn_generate_set_skip_stacks(C.addressof(buf), None) == 10001   # (the plan is looked at after it)


# ---- 2. the guard ----------------------------------------------------------------------------------------------------------
def test_guard_follows_the_switch(tt, monkeypatch):
    from parrot_amd.sampleRNN.generation import device
    tt.configure(RNN_TYPE='GRU', N_RNN=2, SKIP_CONN=True)
    monkeypatch.delenv(SWITCH, raising=False)
    with pytest.raises(NotImplementedError):
        device.device_loop_guard('sequential')
    monkeypatch.setenv(SWITCH, "0")
    with pytest.raises(NotImplementedError):
        device.device_loop_guard('sequential')
    monkeypatch.setenv(SWITCH, "1")                    # read at call time, not at import
    assert device.device_loop_guard('sequential') == 0
    assert device.device_loop_guard('scan', 8, 0.5) == 1
    with pytest.raises(ValueError):                    # the other checks stay in front
        device.device_loop_guard('nope')
    monkeypatch.delenv(SWITCH)
    with pytest.raises(NotImplementedError):
        device.device_loop_guard('sequential')


def test_guard_refuses_one_layer_either_way(tt, monkeypatch):
    from parrot_amd.sampleRNN.generation import device
    tt.configure(RNN_TYPE='GRU', N_RNN=1, SKIP_CONN=True)
    for value in (None, "1"):
        if value is None:
            monkeypatch.delenv(SWITCH, raising=False)
        else:
            monkeypatch.setenv(SWITCH, value)
        with pytest.raises(NotImplementedError):
            device.device_loop_guard('sequential')
    tt.configure(SKIP_CONN=False)                      # without skip connections the switch changes nothing
    assert device.device_loop_guard('sequential') == 0


def test_literal_loop_keeps_its_refusals_without_the_switch(tt, monkeypatch):
    import numpy as np
    tt.configure(DIM=32, EMB_SIZE=8, RNN_TYPE='GRU', N_RNN=2, SKIP_CONN=True)
    monkeypatch.delenv(SWITCH, raising=False)
    feats = np.zeros((2, 1, 63), dtype=np.float32)
    for kw in (dict(top_k=8), dict(top_p=0.5), dict(draw_mode='scan'), dict(utterance_seed=3)):
        with pytest.raises(ValueError):
            tt.generate_and_save_samples("t", None, feats, None, 0., None, None, None, temperature=1.0, **kw)


# ---- 3. the names ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rnn_type,n_rnn", [("GRU", 2), ("GRU", 3), ("LSTM", 2), ("LSTM", 3)])
def test_names_are_the_oracles(rnn_type, n_rnn):
    from parrot_amd.sampleRNN.generation import inputs
    c = S.config(DIM=32, EMB_SIZE=8, RNN_TYPE=rnn_type, N_RNN=n_rnn, SKIP_CONN=True)
    keys = set(S.init_params(c, seed=1))
    named = set()
    for tier in ('BigFrameLevel', 'FrameLevel'):
        layers, outskips, bias = inputs.stack_param_names(tier, rnn_type, n_rnn, True)
        assert len(layers) == len(outskips) == n_rnn
        assert ('candidate' in layers[0]) == (rnn_type == 'GRU')
        assert '+inpskip' not in layers[0]['input'] and all('+inpskip' in l['input'] for l in layers[1:])
        linears = [v for l in layers for k, v in l.items() if k != 'bias'] + outskips
        for name in linears:
            for sfx in ('.W0', '.g0'):
                assert name + sfx in keys, name + sfx
                named.add(name + sfx)
        for name in [l['bias'] for l in layers] + [bias]:
            assert name in keys, name
            named.add(name)
    want = {k for k in keys if '+inpskip' in k or 'outskip' in k}
    assert want and want <= named, sorted(want - named)
    # among the out-skips only the first has a bias
    assert sum(1 for k in keys if 'outskip' in k and k.endswith('.b')) == 2


@pytest.mark.parametrize("rnn_type", ["GRU", "LSTM"])
def test_names_without_skip_connections_are_what_they_were(rnn_type):
    from parrot_amd.sampleRNN.generation import inputs
    c = S.config(DIM=32, EMB_SIZE=8, RNN_TYPE=rnn_type, N_RNN=2)
    keys = set(S.init_params(c, seed=1))
    layers, outskips, bias = inputs.stack_param_names('FrameLevel', rnn_type, 2, False)
    assert outskips == [] and bias is None
    assert layers[1]['input'] == 'FrameLevel.%s2.Step.Input' % rnn_type
    for l in layers:
        assert l['bias'] in keys and all(v + '.W0' in keys for k, v in l.items() if k != 'bias')
    with pytest.raises(ValueError):
        inputs.stack_param_names('FrameLevel', rnn_type, 1, True)
    with pytest.raises(ValueError):
        inputs.stack_param_names('FrameLevel', 'RNN', 2, False)


# ---- 4. the switch's row ---------------------------------------------------------------------------------------------------
def test_switch_is_in_the_table():
    txt = open(os.path.join(ROOT, "parrot_amd", "csrc", "switches.h")).read()
    table = txt[:txt.index("#pragma once")]
    row = re.search(r"^// PARROT_SR_SKIP_STACKS\s+(\S+)\s+(\S+)\s", table, re.M)
    assert row, "PARROT_SR_SKIP_STACKS has no row in the table of switches.h"
    assert row.group(1) == "0" and row.group(2) == "call"     # off by default, read at every entry
    # the library does not read it (the setter is the switch); Python reads it in one place, when called
    csrc = os.path.join(ROOT, "parrot_amd", "csrc")
    reads = [f for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h")) and f != "switches.h"
             and '"PARROT_SR_SKIP_STACKS"' in open(os.path.join(csrc, f)).read()]
    assert reads == []
    from parrot_amd.sampleRNN.generation import inputs
    assert inputs.SKIP_SWITCH == SWITCH

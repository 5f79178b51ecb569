"""The decode workspace without a device: every case of tests/decode_workspace_cases.py builds its workspace on the CPU
with the library's plan entries stubbed (which ones and why: the cases module), and its fingerprint -- descriptor scalars,
which tensor every pointer names, shape / dtype / zero-fill of every buffer, the cache key, the calls made -- equals the one
recorded in tests/golden/decode_workspace_fingerprints.json (tools/record_decode_workspace_fingerprints.py) key for key.
And the one failure path behind plan creation: whichever check fails, the plan is destroyed once and nothing is cached."""
import pytest

from parrot_amd import _lib
from tests import decode_workspace_cases as W


@pytest.fixture(scope="module")
def golden():
    return W.golden()


def test_golden_file_and_case_table_name_the_same_cases(golden):
    assert sorted(k for k in golden if k != "recorded_at_commit") == sorted(W.CASES)
    assert len(golden["recorded_at_commit"]) == 40


@pytest.mark.parametrize("name", list(W.CASES))
def test_workspace_is_the_recorded_one(name, golden, monkeypatch):
    fp, want = W.case_fingerprint(name, monkeypatch), golden[name]
    assert sorted(fp) == sorted(want)
    for part in sorted(want):
        if isinstance(want[part], dict):
            assert sorted(fp[part]) == sorted(want[part]), part
            for k in want[part]:
                assert fp[part][k] == want[part][k], (part, k)
        else:
            assert fp[part] == want[part], part
    assert "?" not in str(fp["pointers"]) and "?" not in str(fp["calls"]), "a pointer that names no tensor"


def test_the_cases_reach_their_branches(golden):
    """What each case is there for, read off the recorded fingerprints."""
    t = lambda name: golden[name]["tensors"]
    p = lambda name: golden[name]["pointers"]
    assert p("gru2_composed_feedback")["Wgx_t"][0] == "pm.tiled[x,g]" and p("gru2_composed_feedback")["Watt_t"] == "pm.Watt_t"
    for name in ("gru2_forced", "gru2_fbc0", "gru3_full_feedback", "lstm", "gru_bf16"):
        assert p(name)["Wgx_t"][0] is None and "pm.cat[x,g]" not in t(name), name
    for name in ("gru2_n17", "gru2_attfold0", "lstm", "gru_bf16"):
        assert p(name)["Watt_t"] is None and "pm.Watt_t" not in t(name), name
    assert golden["gru2_forced"]["forced_descriptor"] and p("gru2_forced")["own_x"] == "own_x"
    assert golden["gru2_forced"]["key"] == ["forced", W.S, W.N, W.U]
    assert golden["forced_stop8"]["key"] == ["forced", "stop", W.S, W.N, W.U, 8] and golden["stop8"]["key"] == ["stop", W.S, W.N, W.U, 8]
    assert golden["stop8"]["scalars"]["eou_extra"] == 8 and t("stop8")["eou_first"][2] is False
    for name in ("lstm_bf16", "gru_bf16"):
        assert golden[name]["scalars"]["bf16"] == 1 and t(name)["pm.tiled[0,g]"][1] == "torch.bfloat16"
        assert p(name)["Wg_t16"][0] == "pm.tiled[0,g]" and p(name)["Wg_t"][0] is None
    assert p("gru_bf16")["Wc_t16"][1] == "pm.tiled[1,c]" and p("lstm")["gwork"] == "gwork"
    assert "pm.ws" not in t("gmm") and p("gmm_machine")["Wrh_t"] == "pm.Wrh_t" and p("speaker_gmm")["add_co"] == "add_co"
    assert p("speaker_mse")["oadd_pad"] == "pm.oadd_pad" and t("speaker_mse")["pm.oadd_pad"][2] is True
    for name in ("layer_norm", "h72_machine_refuses", "persist_off", "gmm", "speaker_gmm"):
        assert not any(k.startswith("pm.") for k in t(name)) and golden[name]["scalars"]["persist_ws_floats"] == 0, name
    assert p("layer_norm")["ln_scratch"] == "ln_scratch" and golden["layer_norm"]["scalars"]["layer_norm"] == 1
    for name in W.CASES:
        if name not in ("layer_norm", "h72_machine_refuses", "persist_off", "gmm", "speaker_gmm"):
            assert golden[name]["scalars"]["persist_ws_floats"] == W.PERSIST_FLOATS and p(name)["persist_ws"] == "pm.ws", name
            assert t(name)["pm.ws"] == [[W.PERSIST_FLOATS], "torch.float32", True], name


def test_a_library_that_declines_the_machine_gets_no_machine_workspace(monkeypatch):
    """parrot_sample_persist_floats answers 0: the plan is made and cached without ws['pm']."""
    m, calls, build = _build("gru2_composed_feedback", monkeypatch, persist_floats=0)
    ws = build()
    assert "pm" not in ws and ws["desc"].persist_ws is None and ws["desc"].persist_ws_floats == 0
    assert [name for name, _ in calls] == ["parrot_sample_persist_floats", "parrot_sample_create", "parrot_sample_set_row_controls"]
    assert list(m._sample_ws) == [(W.S, W.N, W.U)]


# ------------------------------------------------------------------------------- one failure path behind plan creation
def _build(name, monkeypatch, **answers):
    c = W.CASES[name]
    W.set_switches(monkeypatch, c["env"])
    m = W.model(name)
    calls = W.install_stubs(monkeypatch, **answers)
    return m, calls, lambda: m._sample_workspace(W.S, c["N"], W.U, stop_extra=c["stop_extra"], forced=c["forced"])


def _destroys(calls):
    return [getattr(args[0], "value", args[0]) for name, args in calls if name == "parrot_sample_destroy"]


def test_a_plan_that_is_not_bf16_is_destroyed_once(monkeypatch):
    m, calls, build = _build("lstm_bf16", monkeypatch, is_bf16=0)
    with pytest.raises(ValueError, match="does not run bf16 operands"):
        build()
    assert len(_destroys(calls)) == 1 and _destroys(calls)[0] and not m._sample_ws


def test_a_plan_that_does_not_stop_early_is_destroyed_once(monkeypatch):
    m, calls, build = _build("forced_stop8", monkeypatch, stops_early=0)
    with pytest.raises(ValueError, match="does not stop at the end of the utterance"):
        build()
    assert len(_destroys(calls)) == 1 and _destroys(calls)[0] and not m._sample_ws


def test_a_plan_that_refuses_its_row_controls_is_destroyed_once(monkeypatch):
    m, calls, build = _build("stop8", monkeypatch, row_controls_rc=7)
    with pytest.raises(_lib.HipCallError, match="parrot_sample_set_row_controls failed with code 7"):
        build()
    assert len(_destroys(calls)) == 1 and _destroys(calls)[0] and not m._sample_ws
    assert [name for name, _ in calls][-2:] == ["parrot_sample_set_row_controls", "parrot_sample_destroy"]


def test_a_plan_that_passes_destroys_nothing(monkeypatch):
    m, calls, build = _build("forced_stop8", monkeypatch)
    ws = build()
    assert not _destroys(calls) and list(m._sample_ws) == [("forced", "stop", W.S, W.N, W.U, 8)] and build() is ws
    assert [name for name, _ in calls] == ["parrot_sample_persist_floats_forced", "parrot_sample_create_forced",
                                           "parrot_sample_stops_early", "parrot_sample_set_row_controls"]

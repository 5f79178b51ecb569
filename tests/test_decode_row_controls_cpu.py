"""The premise of tests/test_gpu_decode_row_controls.py, and everything of the per-utterance decode controls that needs no
device: the oracle with column-tensor controls IS the per-row decode, every case's seed keeps the pick and the float32
margins, a kernel that ignored the arrays could not pass; argument validation on a model that is never allocated; the list
flags of sample.py, --phrase against a character table in tmp_path, the --mix arithmetic on a hand-made table."""
import pickle

import numpy as np
import pytest
import torch

from tests import decode_row_controls_cases as RC
from tests.util import rel_err


@pytest.mark.parametrize("name", sorted(RC.CASES))
def test_case_premise(name):
    """Every case: the oracle's float32 run (controls included) within F32_MARGIN of its float64 run; GMM cases: no
    cumulative mixture weight within PICK_MARGIN of its uniform number."""
    c = RC.case(name)
    e32 = RC.f32_error(c)
    print(f"{name}: float32 error {e32:.2e}" + (f", pick margin {RC.pick_margin(c):.2e}" if c['gmm'] else ""))
    assert e32 <= RC.F32_MARGIN
    if c['gmm']:
        assert RC.pick_margin(c) >= RC.PICK_MARGIN


@pytest.mark.parametrize("name", ["gru2_mse_n5", "lstm2_k3_n5"])
def test_column_tensors_are_the_per_row_decode(name):
    """Row i of the mixed oracle run equals row i of the scalar run with row i's values exactly, and the mixed run is far
    from the all-defaults run on all six outputs."""
    c = RC.case(name)
    for i in (1, 2, 4):
        for a, b, n in zip(c['ref'], RC.row_ref(c, i), RC.NAMES):
            assert torch.equal(a[:, i], b[:, i]), f"{n}, row {i}"
    for a, b, n in zip(c['ref'], RC.plain_ref(c), RC.NAMES):
        if n == 'pi' and not c['gmm']:
            continue  # (the MSE oracle returns the frames again)
        e = rel_err(a, b)
        print(f"{name}: {n} mixed vs defaults {e:.2e}")
        assert e > 0.05, n


def test_second_control_set_of_the_replay_test():
    """The replay test holds its MSE case's second call to the oracle as well: the same float32 margin for that set."""
    e32 = RC.f32_error(RC.case('gru2_mse_n5', 'B'))
    print(f"gru2_mse_n5, second set: float32 error {e32:.2e}")
    assert e32 <= RC.F32_MARGIN


def test_the_two_control_sets_differ():
    a, b = RC.controls(5, True, 'A'), RC.controls(5, True, 'B')
    for k in ('timing', 'sharpening', 'bias'):
        assert a[k] != b[k] and sorted(a[k]) == sorted(b[k])
    assert RC.cycle(RC.TIMING, 17)[15:] == [1.0, 0.8] and len(RC.cycle(RC.BIAS, 17)) == 17


# ---------------------------------------------------------------------------------------------------- argument validation
def _never_allocated(**kw):
    from parrot_amd.model import Parrot
    return Parrot(device=torch.device('cpu'), **dict(RC.SMALL, cell_type='gru', num_layers=1, **kw))


@pytest.mark.parametrize("kw, match", [
    (dict(timing_coeffs=[1.0, 2.0]), "timing_coeffs needs 3 values"),
    (dict(sharpening_coeffs=[[1.0, 2.0, 3.0]]), "sharpening_coeffs needs 3 values"),
    (dict(timing_coeffs=[1.0, float('nan'), 1.0]), "finite"),
    (dict(sharpening_coeffs=[1.0, float('inf'), 1.0]), "finite"),
    (dict(sampling_biases=[0.0, float('-inf'), 1.0]), "finite"),
    (dict(timing_coeffs=[1.0, 0.0, 1.0]), "> 0"),
    (dict(sharpening_coeffs=[1.0, -0.5, 1.0]), "> 0"),
    (dict(sampling_biases=[0.0, 1.0]), "sampling_biases needs 3 values"),
    (dict(speaker_weights=np.eye(5)[:3]), "use_speaker"),
])
def test_bad_arguments_are_refused_before_anything_is_allocated(kw, match):
    m = _never_allocated()
    lab, lm = np.zeros((3, 4), dtype='int64'), np.ones((3, 4), dtype='float32')
    for call in (lambda: m.sample_model_device(lab, lm, None, 3, 6, **kw),
                 lambda: m.sample_model(lab, lm, None, None, 3, 6, **kw),
                 lambda: m.sample_until_end_device(lab, lm, None, 3, 6, **kw),
                 lambda: m.sample_until_end(lab, lm, None, None, 3, 6, **kw)):
        with pytest.raises(ValueError, match=match):
            call()
    assert not m._sample_ws and m.decode_path is None


def test_biases_need_a_gmm_head_and_weights_their_shape():
    m = _never_allocated(which_cost='MSE')
    with pytest.raises(ValueError, match="GMM"):
        m._check_row_controls(3, sampling_biases=[0.0, 0.5, 1.0])
    m = _never_allocated(use_speaker=True)
    with pytest.raises(ValueError, match=r"\(3, 5\)"):
        m._check_row_controls(3, speaker_weights=np.ones((3, 4)))
    with pytest.raises(ValueError, match="finite"):
        m._check_row_controls(3, speaker_weights=np.full((3, 5), np.nan))
    ctl, sw = m._check_row_controls(3, timing_coeffs=(1, 2, 0.5), sampling_biases=torch.tensor([0., -1., 2.]),
                                    speaker_weights=np.eye(5)[:3])
    assert ctl['timing'].dtype == np.float32 and ctl['timing'].tolist() == [1.0, 2.0, 0.5]
    assert ctl['sharpening'] is None and ctl['bias'].tolist() == [0.0, -1.0, 2.0]
    assert sw.dtype == np.float32 and sw.shape == (3, 5)
    assert m._check_row_controls(3) == ({'timing': None, 'sharpening': None, 'bias': None}, None)


# ---------------------------------------------------------------------------------------------------- sample.py's flags
def test_list_flags_parse_and_count():
    from parrot_amd.utils import sample_parse
    a = sample_parse(["--num_samples", "3", "--timing_coeffs", "1,0.8,1.25", "--sharpening_coeffs", " 1, 1.5 ,0.7",
                      "--sampling_biases", "0,0.5,-1"])
    assert a.timing_coeffs == [1.0, 0.8, 1.25] and a.sharpening_coeffs == [1.0, 1.5, 0.7] and a.sampling_biases == [0.0, 0.5, -1.0]
    assert (a.timing_coeff, a.sharpening_coeff, a.sampling_bias) == (1.0, 1.0, 1.0)  # (the scalar flags keep their meaning)
    d = sample_parse([])
    assert d.timing_coeffs is None and d.sharpening_coeffs is None and d.sampling_biases is None
    assert d.mix is None and d.mix_speakers == (15, 11) and d.phrase is None
    assert sample_parse(["--mix", "0.25", "--mix_speakers", "3,7"]).mix_speakers == (3, 7)
    for flag in ("--timing_coeffs", "--sharpening_coeffs", "--sampling_biases"):
        with pytest.raises(SystemExit) as e:
            sample_parse(["--num_samples", "4", flag, "1,2,3"])
        assert "3" in str(e.value) and "4" in str(e.value) and flag in str(e.value)
        with pytest.raises(SystemExit, match="not a comma-separated list"):
            sample_parse(["--num_samples", "2", flag, "1,fast"])
    with pytest.raises(SystemExit, match="mix_speakers"):
        sample_parse(["--mix_speakers", "15"])


def test_phrase_labels(tmp_path):
    from parrot_amd.utils import phrase_labels
    (tmp_path / "toyset").mkdir()
    table = {c: i + 3 for i, c in enumerate("abc d")}
    with open(tmp_path / "toyset" / "char2code.pkl", "wb") as f:
        pickle.dump(table, f)
    labels, mask = phrase_labels("a cab", "toyset", 3, data_path=str(tmp_path))
    assert labels.shape == (3, 5) and labels.tolist() == [[3, 6, 5, 3, 4]] * 3
    assert mask.shape == (3, 5) and mask.dtype == np.float32 and (mask == 1).all()
    with pytest.raises(SystemExit, match="'z'"):
        phrase_labels("a zab", "toyset", 3, data_path=str(tmp_path))
    with pytest.raises(SystemExit, match="char2code.pkl"):
        phrase_labels("abc", "otherset", 3, data_path=str(tmp_path))


def test_phrase_reads_fuel_data_path(tmp_path, monkeypatch):
    from parrot_amd.utils import phrase_labels
    monkeypatch.delenv("FUEL_DATA_PATH", raising=False)
    with pytest.raises(SystemExit, match="FUEL_DATA_PATH"):
        phrase_labels("abc", "toyset", 2)
    (tmp_path / "toyset").mkdir()
    with open(tmp_path / "toyset" / "char2code.pkl", "wb") as f:
        pickle.dump({'a': 1, 'b': 2}, f)
    monkeypatch.setenv("FUEL_DATA_PATH", str(tmp_path))
    assert phrase_labels("ab", "toyset", 2)[0].tolist() == [[1, 2], [1, 2]]


def test_mix_arithmetic_on_a_hand_made_table():
    """--mix m: every row's embedding is m * W[A] + (1 - m) * W[B] (reference sample.py:81-85), and the table is left alone."""
    from parrot_amd.utils import mix_speaker_weights
    W = np.arange(22 * 4, dtype=np.float32).reshape(22, 4) ** 2
    before = W.copy()
    w = mix_speaker_weights(0.25, (15, 11), 22, 3)
    assert w.shape == (3, 22) and w.dtype == np.float32
    assert np.count_nonzero(w[0]) == 2 and w[0, 15] == np.float32(0.25) and w[0, 11] == np.float32(0.75)
    assert np.array_equal(w @ W, np.tile(0.25 * W[15] + 0.75 * W[11], (3, 1)))
    assert np.array_equal(W, before)
    one = mix_speaker_weights(0.5, (4, 4), 5, 1)  # the same speaker twice: that speaker
    assert one[0].tolist() == [0, 0, 0, 0, 1.0]
    with pytest.raises(SystemExit, match="22 speakers"):
        mix_speaker_weights(0.5, (15, 30), 22, 2)

"""The top-p (nucleus) truncated draw of the SampleRNN generator (samplernn_generate_set_top_p,
samplernn_generate_set_utterance_top_p), as far as it can be checked without a GPU: the nucleus rule of the cases module
(ties, m >= 1, behind top-k), the premise of the GPU tests' judging rule (every listed case lies farther than 2^-14 from a
prefix mass; the float32 restatements of the device's cut find the oracle's m and keep the cap), and the interface --
validation, refusals in front of any device call, build_packed_top_p, the runner contract of StreamingGenerator, the header
and the signatures, the flag.  Cases: tests/samplernn_top_p_cases.py."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from tests import samplernn_sampling_cases as SC
from tests import samplernn_top_k_cases as KC
from tests import samplernn_top_p_cases as NC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tt():
    from parrot_amd.sampleRNN.models.conditional import three_tier
    return three_tier


# ---- 1. the rule ----------------------------------------------------------------------------------------------------------------
def test_nucleus_rule():
    # terms at T = 1: 4 e^0 and smaller ones; masses as fractions are irrational, the cuts below lie well inside
    lg = np.log(np.array([1.0, 4.0, 4.0, 0.5, 4.0, 2.0, 2.0, 0.5], dtype=np.float64)).astype(np.float32)   # tot = 18
    assert NC.order(lg).tolist() == [1, 2, 4, 5, 6, 0, 3, 7]
    for p, want in ((1e-6, [1]), (0.2, [1]), (0.23, [1, 2]), (0.44, [1, 2]), (0.45, [1, 2, 4]), (0.66, [1, 2, 4]),
                    (0.7, [1, 2, 4, 5]), (0.8, [1, 2, 4, 5, 6]), (0.93, [0, 1, 2, 4, 5, 6]), (0.96, [0, 1, 2, 3, 4, 5, 6]),
                    (0.99, list(range(8)))):
        assert np.nonzero(NC.nucleus_set(lg, 1.0, p))[0].tolist() == want, p
        assert NC.nucleus_m(lg, 1.0, p) == len(want) >= 1
    # behind top_k = 3 the nucleus is taken of the mass of K = {1, 2, 4}: thirds
    assert NC.nucleus_m(lg, 1.0, 0.3, 3) == 1 and NC.nucleus_m(lg, 1.0, 0.5, 3) == 2 and NC.nucleus_m(lg, 1.0, 0.9, 3) == 3
    assert np.nonzero(NC.nucleus_set(lg, 1.0, 0.5, 3))[0].tolist() == [1, 2]
    # off: not strictly between 0 and 1
    for p in (0.0, 1.0, 1.5):
        assert NC.nucleus_set(lg, 1.0, p).all() and NC.nucleus_m(lg, 1.0, p, 3) == 3
    # one big tie: exact masses, the cut-off's tie goes to the low indices
    b4 = np.full(SC.Q, SC.EDGE_LOGIT, dtype=np.float32)
    assert NC.equal_logits_m() == 64 == NC.nucleus_m(b4, 1.0, NC.EQUAL_P)
    assert np.nonzero(NC.nucleus_set(b4, 1.0, NC.EQUAL_P))[0].tolist() == list(range(64))
    assert NC.nucleus_m(b4, 1.0, NC.EQUAL_P, 128) == 32
    assert NC.two_maxima_m() == 2
    # a small p is the arg-max, lowest index on ties
    for name, (codes, want) in SC.TIE_MAXIMA.items():
        b4, _ = SC.tie_pattern(name)
        assert np.nonzero(NC.nucleus_set(b4, 1.0, NC.SMALL_P))[0].tolist() == [want], name


def test_combined_case_discriminates():
    b4 = SC.b4_pattern("randn")
    assert NC.nucleus_m(b4, 1.0, 0.9) == 65 and NC.nucleus_m(b4, 1.0, 0.9, 64) == 35


# ---- 2. the premise of the promise about the cut --------------------------------------------------------------------------------
def test_every_case_keeps_the_margin():
    assert len(NC.CASES) == 72 and NC.MARGIN == SC.DELTA == 2.0 ** -14
    closest = min((NC.margin(SC.b4_pattern(pattern), tau, p, k), pattern, tau, p, k) for pattern, tau, p, k in NC.CASES)
    print(f"TOPP-CPU closest prefix mass: {closest[0]:.3e} at {closest[1:]}")
    assert closest[0] > NC.MARGIN
    for pattern, tau, p, k in NC.CASES:
        assert 1 <= NC.case_m(SC.b4_pattern(pattern), tau, p, k) <= (k or SC.Q)
    # (p = 0.999 on `peaked` at temperature 2 does not keep it: such a p is no case, and case_m says so)
    assert NC.margin(SC.b4_pattern("peaked"), 2.0, 0.999) < NC.MARGIN
    with pytest.raises(AssertionError):
        NC.case_m(SC.b4_pattern("peaked"), 2.0, 0.999)


def test_wave_sum_restatement():
    v = np.arange(64, dtype=np.float32)
    assert NC.wave_sum_f32(v) == 2016.0
    assert NC.lane_layout("sequential")[5].tolist() == [5, 69, 133, 197] and NC.lane_layout("scan")[5].tolist() == [20, 21, 22, 23]
    e = np.ones(256, dtype=np.float32)
    inside = np.zeros(256, dtype=bool)
    inside[:77] = True
    for mode in NC.MODES:
        assert NC.mass_f32(e, inside, mode) == 77.0
    # monotone in the set: what makes the binary search of the device valid
    rng = np.random.RandomState(5)
    e = np.exp(rng.randn(256) * 3).astype(np.float32)
    o = np.argsort(-e, kind="stable")
    for mode in NC.MODES:
        inside = np.zeros(256, dtype=bool)
        last = np.float32(0)
        for q in o:
            inside[q] = True
            now = NC.mass_f32(e, inside, mode)
            assert now >= last
            last = now


@pytest.mark.parametrize("mode", NC.MODES)
def test_restatements_find_the_oracles_cut_and_keep_the_cap(mode):
    """Over every listed case: the device's cut restated in float32 (its lanes, its tree, its float32 bar) finds the float64
    oracle's m, and the restated draw leaves the oracle's in at most EXCUSED_CAP of the draws, only within DELTA /
    DELTA_SCAN of a boundary, never outside the nucleus."""
    worst_frac, worst_dist = 0.0, 0.0
    s = SC.BIAS_SHAPES["persist-D256-B32"]
    u = SC.u01_table(SC.SEEDS[1], s.T, s.B)
    for pattern, tau, p, k in NC.CASES:
        b4 = SC.b4_pattern(pattern)
        m = NC.case_m(b4, tau, p, k)
        assert NC.nucleus_m_f32(b4, tau, p, k, mode) == m, (pattern, tau, p, k)
        got = NC.emulate_picks_f32(b4, tau, p, k, u, mode)
        m2, draws, excused, worst = NC.judge_draws(got, b4, tau, p, k, u, mode)
        assert m2 == m
        worst_frac, worst_dist = max(worst_frac, excused / draws), max(worst_dist, worst)
    print(f"TOPP-CPU {mode}: {len(NC.CASES)} cases, worst mismatch fraction {worst_frac:.4%} (cap {SC.EXCUSED_CAP:.1%}), worst "
          f"boundary distance {worst_dist:.2e}")


def test_exact_cases_hold_in_the_restatements():
    s = SC.EDGE_SHAPES["launch-D32-B8"]
    for seed in SC.EDGE_SEEDS + tuple(KC.U1_SEEDS):
        u = SC.u01_table(seed, s.T, s.B)
        for mode in NC.MODES:
            b4 = np.full(SC.Q, SC.EDGE_LOGIT, dtype=np.float32)
            got = NC.emulate_picks_f32(b4, 1.0, NC.EQUAL_P, 0, u, mode)
            assert np.array_equal(got, KC.equal_logits_picks(64, u)) and got.max() <= 63, (seed, mode)
            assert np.array_equal(NC.emulate_picks_f32(b4, 1.0, NC.EQUAL_P, 128, u, mode), KC.equal_logits_picks(32, u))
            b4, _ = SC.tie_pattern(KC.TWO_MAXIMA)
            assert np.array_equal(NC.emulate_picks_f32(b4, 1.0, NC.TWO_MAXIMA_P, 0, u, mode), KC.two_maxima_picks(u)), (seed, mode)
            for name in SC.TIE_MAXIMA:    # a small p is the arg-max
                b4, want = SC.tie_pattern(name)
                assert np.unique(NC.emulate_picks_f32(b4, 1.0, NC.SMALL_P, 0, u, mode)).tolist() == [want]
        if seed in KC.U1_SEEDS:           # u01 == 1.0: the highest code of the nucleus, not 255
            b, t = KC.U1_SEEDS[seed]
            b4 = np.full(SC.Q, SC.EDGE_LOGIT, dtype=np.float32)
            assert u[b, t - NC.BFS] == 1.0
            assert NC.emulate_picks_f32(b4, 1.0, NC.EQUAL_P, 0, u, "sequential")[b, t - NC.BFS] == 63


# ---- 3. the interface -----------------------------------------------------------------------------------------------------------
def test_new_names_are_reexported(tt):
    from parrot_amd.sampleRNN.generation import inputs
    for name in ("build_packed_top_p", "top_p_code", "top_p_array", "top_p_active", "_per_utterance_top_p"):
        assert getattr(tt, name) is getattr(inputs, name), name


def test_top_p_values(tt):
    assert tt.top_p_code(0) == 0.0 and tt.top_p_code(0.0) == 0.0 and tt.top_p_code(1) == 1.0 and tt.top_p_code(1.5) == 1.5
    assert tt.top_p_code(0.9) == float(np.float32(0.9)) and tt.top_p_code(np.float32(0.25)) == 0.25
    assert tt.top_p_code(float("inf")) >= 1.0
    assert 0.0 < tt.top_p_code(1e-60) < 1e-30                       # a positive p stays active: it keeps the arg-max
    assert [tt.top_p_active(p) for p in (0, 0.0, 1e-60, 0.5, 1.0, 2.0)] == [False, False, True, True, False, False]
    for bad in (-0.5, -1, float("nan"), np.float32("nan"), float("-inf"), "0.9", None, True, [0.5]):
        with pytest.raises(ValueError):
            tt.top_p_code(bad)
    a = tt.top_p_array([[0, 0.5], [3.0, 1e-60]], (2, 2))
    assert a.dtype == np.float32 and a[0].tolist() == [0.0, 0.5] and a[1, 0] >= 1.0 and 0.0 < a[1, 1] < 1e-30
    for bad, shape in (([[0, -0.1]], (1, 2)), ([0, 1], (1, 2)), ([[0.5, float("nan")]], (1, 2)), ([[0, 1]], (2, 1)),
                       ([["a", "b"]], (1, 2))):
        with pytest.raises(ValueError):
            tt.top_p_array(bad, shape)
    assert tt._per_utterance_top_p(None, 3, 0.5) == [0.5] * 3 and tt._per_utterance_top_p([0.25, 0, 1], 3, 0.5) == [0.25, 0.0, 1.0]
    with pytest.raises(ValueError):
        tt._per_utterance_top_p([0.5, 0.5], 3, 0)
    with pytest.raises(ValueError):
        tt._per_utterance_top_p([0.5, -0.5, 0.5], 3, 0)


def test_build_packed_top_p(tt):
    from parrot_amd.sampleRNN.generation import inputs
    T = 4
    for s in range(T):
        got = tt.build_packed_top_p([0.5], [0], [s], T, 2)
        row = inputs.start_row(s, T)
        want = np.zeros((T, 2), dtype=np.float32)
        if row is not None:
            want[row, 0] = 0.5
        assert got.dtype == np.float32 and np.array_equal(got, want)
    assert tt.build_packed_top_k([8], [0], [0], T, 2).dtype == np.int32       # its sibling keeps its signature and result
    with pytest.raises(ValueError):
        tt.build_packed_top_p([0.5], [2], [0], T, 2)
    with pytest.raises(ValueError):
        tt.build_packed_top_p([-0.5], [0], [0], T, 2)


def test_refusals_come_before_any_device_call(tt, monkeypatch):
    from parrot_amd import _lib
    from parrot_amd.sampleRNN import lib

    def no_device(*a, **k):
        raise AssertionError("a device call in front of the top_p check")
    monkeypatch.setattr(_lib, "call", no_device)
    monkeypatch.setattr(_lib, "load", no_device)
    monkeypatch.setattr(lib, "device", no_device)
    feats = np.zeros((3, 2, 63), dtype=np.float32)
    for bad in (-0.5, float("nan"), "0.9", None):
        with pytest.raises(ValueError):
            tt.DeviceGenerator(2, 3, top_p=bad)
        with pytest.raises(ValueError):
            tt.generate_packed([feats[:, 0]], n_streams=2, top_p=bad)
        with pytest.raises(ValueError):
            next(tt.generate_stream(feats, 2, top_p=bad))
        with pytest.raises(ValueError):
            tt.StreamingGenerator(2, 2, top_p=bad)
        with pytest.raises(ValueError):
            tt.generate_and_save_samples("t", features=feats, top_p=bad)
    with pytest.raises(ValueError):                             # per-utterance values need per-utterance seeds
        tt.generate_packed([feats[:, 0]], n_streams=2, top_ps=[0.5])
    with pytest.raises(ValueError):
        tt.generate_packed([feats[:, 0]], n_streams=2, seeds=[5], top_ps=[0.5, 0.5])
    with pytest.raises(ValueError):
        tt.generate_packed([feats[:, 0]], n_streams=2, seeds=[5], top_ps=[-0.5])
    with pytest.raises(ValueError):                             # the literal three-function loop draws among all codes
        tt.generate_and_save_samples("t", features=feats, use_device_loop=False, top_p=0.9)
    tt.configure(SKIP_CONN=True)
    try:
        with pytest.raises(ValueError):
            tt.generate_and_save_samples("t", features=feats, top_p=0.9)
        with pytest.raises(NotImplementedError):                # skip-connection stacks keep being refused
            tt.DeviceGenerator(2, 3, top_p=0.9)
    finally:
        tt.configure(SKIP_CONN=False)


def _bare_plan(tt, packed, utterance_draws, B=2, T=3):
    """A DeviceGenerator without a device behind it: what generate() checks before it stages anything."""
    gen = object.__new__(tt.DeviceGenerator)
    gen.B, gen.T, gen.packed, gen.utterance_draws, gen._has_run, gen.top_k, gen.top_p = B, T, packed, utterance_draws, False, 0, 0.0
    return gen


def test_generate_refuses_top_ps_in_front_of_the_device(tt, monkeypatch):
    from parrot_amd import _lib

    def no_device(*a, **k):
        raise AssertionError("a device call in front of the top_ps check")
    monkeypatch.setattr(_lib, "call", no_device)
    feats = np.zeros((3, 2, 63), dtype=np.float32)
    starts = np.zeros((3, 2), dtype=np.int32)
    sd, tp = np.zeros((3, 2), dtype=np.uint64), np.ones((3, 2), dtype=np.float32)
    with pytest.raises(ValueError):                             # no utterance_draws: no top_ps
        _bare_plan(tt, False, False).generate(feats, top_ps=[0.5, 0.5])
    with pytest.raises(ValueError):
        _bare_plan(tt, True, False).generate(feats, starts, top_ps=np.zeros((3, 2), dtype=np.float32))
    plain, packed = _bare_plan(tt, False, True), _bare_plan(tt, True, True)
    for bad in ([0.5], [[0.5, 0.5]], [0.5, -0.1], [0.5, float("nan")], -0.5, float("nan")):
        with pytest.raises(ValueError):
            plain.generate(feats, seeds=[1, 2], temperatures=1.0, top_ps=bad)
    for bad in ([0.5, 0.5], np.zeros((2, 2), dtype=np.float32), np.full((3, 2), -0.5), np.full((3, 2), np.nan)):
        with pytest.raises(ValueError):
            packed.generate(feats, starts, seeds=sd, temperatures=tp, top_ps=bad)
    plain._has_run = True                                       # a plain plan takes them with resume=False only, like seeds
    with pytest.raises(ValueError):
        plain.generate(feats[:2], resume=True, n_frames=2, top_ps=[0.5, 0.5])


def test_submit_takes_a_top_p_with_utterance_draws_only(tt):
    runner = lambda features, starts, resume, **kw: np.zeros((2, 80 * features.shape[0]), dtype=np.int32)
    utt = np.zeros((2, 63), dtype=np.float32)
    off = tt.StreamingGenerator(2, 2, run_segment=runner)
    with pytest.raises(ValueError):
        off.submit(utt, top_p=0.5)
    on = tt.StreamingGenerator(2, 2, run_segment=runner, utterance_draws=True)
    with pytest.raises(ValueError):
        on.submit(utt, seed=1, top_p=-0.5)
    with pytest.raises(ValueError):
        on.submit(utt, seed=1, top_p=float("nan"))
    with pytest.raises(ValueError):
        on.submit(utt, top_p=0.5)                                # the seed is still required
    assert on.submit(utt, seed=1, top_p=0.5) == 0


def test_runner_contract(tt):
    """A runner of the caller's sees top_ps only when the generator uses nucleus truncation: its top_p is active, or some
    utterance was submitted with one.  Otherwise it is called as before: three arguments, five with utterance_draws, six with
    a top_k."""
    seen = []
    zeros = lambda features: np.zeros((2, 80 * features.shape[0]), dtype=np.int32)

    def three(features, starts, resume):
        seen.append(())
        return zeros(features)

    def five(features, starts, resume, seeds, temperatures):
        seen.append((seeds, temperatures))
        return zeros(features)

    def six(features, starts, resume, seeds=None, temperatures=None, top_ks=None):
        seen.append((top_ks,))
        return zeros(features)

    def seven(features, starts, resume, seeds=None, temperatures=None, top_ks=None, top_ps=None):
        seen.append((starts.copy(), seeds, temperatures, top_ks, top_ps))
        return zeros(features)

    utt = np.zeros((3, 63), dtype=np.float32)
    for off in ({}, dict(top_p=0.0), dict(top_p=1.0), dict(top_p=2.5)):    # off: the runner never sees the keyword
        sg = tt.StreamingGenerator(2, 2, run_segment=three, **off)
        sg.submit(utt)
        assert sg.drain() and seen
        sg = tt.StreamingGenerator(2, 2, run_segment=five, utterance_draws=True, **off)
        sg.submit(utt, seed=7)
        assert sg.drain()
        sg = tt.StreamingGenerator(2, 2, run_segment=six, top_k=8, **off)
        sg.submit(utt)
        assert sg.drain() and seen[-1][0] is not None
    # the generator's own top_p, without per-utterance draws: top_ps on the start rows, nothing else
    del seen[:]
    sg = tt.StreamingGenerator(2, 2, run_segment=seven, top_p=0.5)
    sg.submit(utt)
    sg.submit(utt[:2])
    assert sg.drain()
    for starts, sd, tp, tk, pp in seen:
        assert sd is None and tp is None and tk is None and pp.dtype == np.float32 and pp.shape == starts.shape
        assert np.array_equal(pp, np.where(starts != 0, np.float32(0.5), np.float32(0)))
    assert sum(int((s[0] != 0).sum()) for s in seen) == 2
    # per utterance: one submitted with a top_p switches the keyword on; the others take the generator's (here 0)
    del seen[:]
    sg = tt.StreamingGenerator(2, 2, run_segment=seven, utterance_draws=True)
    sg.submit(utt, seed=7)
    assert sg.step() and seen[-1][4] is None and seen[-1][3] is None
    sg.submit(utt, seed=8, top_p=0.25)
    sg.submit(utt, seed=9, temperature=0.5)
    assert sg.drain()
    ps = np.concatenate([pp[starts != 0] for starts, _, _, _, pp in seen[1:]])
    assert all(pp is not None and pp.dtype == np.float32 and tk is None for _, _, _, tk, pp in seen[1:])
    assert sorted(ps.tolist()) == [0.0, 0.25], ps


def test_keyword_is_everywhere_top_k_is(tt):
    from parrot_amd.model import SampleRnn
    for fn, names in ((tt.DeviceGenerator.__init__, ("top_k", "top_p")), (tt.DeviceGenerator.generate, ("top_ks", "top_ps")),
                      (tt.generate_packed, ("top_k", "top_ks", "top_p", "top_ps")), (tt.generate_stream, ("top_k", "top_p")),
                      (tt.StreamingGenerator.__init__, ("top_k", "top_p")), (tt.StreamingGenerator.submit, ("top_k", "top_p")),
                      (tt.generate_and_save_samples, ("top_k", "top_p")), (SampleRnn.sample_raw, ("top_k", "top_p"))):
        params = inspect.signature(fn).parameters
        for name in names:
            assert name in params, (fn.__qualname__, name)
    assert inspect.signature(tt.DeviceGenerator.__init__).parameters["top_p"].default == 0.0


def test_header_and_signatures():
    from parrot_amd import _lib
    txt = open(os.path.join(ROOT, "include", "parrot_hip.h")).read()
    assert re.search(r"int samplernn_generate_set_top_p\(void\* plan, float top_p\);", txt)
    assert re.search(r"int samplernn_generate_set_utterance_top_p\(void\* plan, const float\* utt_top_p\);", txt)
    for phrase in ("shortest prefix", ">= p * tot_K", "indistinguishable from a draw with top_k = m", "PARROT_ERR_UNSUPPORTED"):
        assert phrase in txt, phrase
    assert _lib.SIGNATURES["samplernn_generate_set_top_p"] == (C.c_int, [C.c_void_p, C.c_float])
    assert _lib.SIGNATURES["samplernn_generate_set_utterance_top_p"] == (C.c_int, [C.c_void_p, C.c_void_p])
    assert C.sizeof(_lib.SampleRnnGenDesc) == 936               # the descriptor did not grow: top_p arrives by the setters
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "samplernn_generate_set_top_p" in doc and "samplernn_generate_set_utterance_top_p" in doc


def test_c_entries_refuse_null_arguments():
    from parrot_amd import _lib
    lib = _lib.load()
    buf = (C.c_float * 4)()
    assert lib.samplernn_generate_set_top_p(None, C.c_float(0.5)) == 10001                 # PARROT_ERR_BADARG, no device call
    assert lib.samplernn_generate_set_utterance_top_p(None, C.addressof(buf)) == 10001
    assert lib.samplernn_generate_set_utterance_top_p(C.addressof(buf), None) == 10001    # (the plan is only looked at after the pointer)


def test_parser_has_the_flag():
    from parrot_amd.utils import sample_parse
    assert sample_parse([]).top_p == 0.0
    assert sample_parse(['--top_p', '0.9']).top_p == 0.9
    assert sample_parse(['--top_p', '0.9', '--top_k', '64']).top_k == 64
    with pytest.raises(SystemExit):
        sample_parse(['--top_p', 'most'])


def test_sample_raw_refuses_a_bad_top_p(tt):
    from parrot_amd.model import SampleRnn
    m = object.__new__(SampleRnn)      # (no parameters, no device: the check comes first)
    m.three_tier = tt
    for bad in (-0.5, float("nan")):
        with pytest.raises(ValueError):
            m.sample_raw(None, None, "t", None, top_p=bad)

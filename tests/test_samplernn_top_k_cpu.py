"""The top-k truncated draw of the SampleRNN generator (SampleRnnGenDesc::top_k, samplernn_generate_set_utterance_top_k), as
far as it can be checked without a GPU: the kept-set rule, the premises of the GPU tests' judging rule (the float32
restatements of both draw modes against the float64 oracle, the seeds whose uniform is exactly 1.0), and the interface --
refusals in front of any device call, the runner contract of StreamingGenerator, the descriptor, the flag.
Cases: tests/samplernn_top_k_cases.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import samplernn_sampling_cases as SC
from tests import samplernn_top_k_cases as KC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tt():
    from parrot_amd.sampleRNN.models.conditional import three_tier
    return three_tier


# ---- 1. the rule ----------------------------------------------------------------------------------------------------------------
def test_kept_set_rule():
    lg = np.array([1.0, 3.0, 3.0, -2.0, 3.0, 0.0, -0.0, 1.0], dtype=np.float32)
    assert np.nonzero(KC.kept_set(lg, 1))[0].tolist() == [1]                 # the arg-max's lowest-index tie rule
    assert np.nonzero(KC.kept_set(lg, 2))[0].tolist() == [1, 2]              # a tie at the cut-off goes to the lower index
    assert np.nonzero(KC.kept_set(lg, 4))[0].tolist() == [0, 1, 2, 4]
    assert np.nonzero(KC.kept_set(lg, 6))[0].tolist() == [0, 1, 2, 4, 5, 7]  # 0.0 and -0.0 tie: index 5 before 6
    assert KC.kept_set(lg, 0).all() and KC.kept_set(lg, 8).all() and KC.kept_set(lg, 9).all()
    for pattern in SC.PATTERNS:
        b4 = SC.b4_pattern(pattern)
        for k in KC.CPU_KS:
            keep = KC.kept_set(b4, k)
            assert keep.sum() == k and b4[keep].min() >= b4[~keep].max()
    for name, (codes, want) in SC.TIE_MAXIMA.items():
        b4, _ = SC.tie_pattern(name)
        assert np.nonzero(KC.kept_set(b4, 1))[0].tolist() == [want], name
    b4, _ = SC.tie_pattern(KC.TWO_MAXIMA)
    assert np.nonzero(KC.kept_set(b4, 2))[0].tolist() == [5, 69]


def test_truncated_cdf_and_fall_through():
    b4 = SC.b4_pattern("randn")
    for k in KC.CPU_KS:
        keep = KC.kept_set(b4, k)
        c = KC.cdf64(b4, 1.0, k)
        assert abs(c[-1] - 1.0) < 1e-12 and (np.diff(c, prepend=0.0)[~keep] == 0).all()
        last = int(np.nonzero(keep)[0][-1])
        picks = KC.oracle_picks(b4, 1.0, k, np.array([[1e-9, 0.5, 1.0 - 1e-12, 1.0, 1.5]]))
        assert keep[picks].all() and picks[0, -1] == last and picks[0, -2] == last
    # off is today's oracle
    u = SC.u01_table(SC.SEEDS[0], 3, 3)
    assert np.array_equal(KC.oracle_picks(b4, 1.0, 0, u), SC.oracle_picks(b4, 1.0, u))
    assert np.array_equal(KC.emulate_picks_f32(b4, 1.0, 0, u), SC.emulate_picks_f32(b4, 1.0, u))
    from tests import samplernn_draw_scan_cases as DC
    assert np.array_equal(KC.emulate_picks_scan_f32(b4, 1.0, 256, u), DC.emulate_picks_scan_f32(b4, 1.0, u))


# ---- 2. the cap check: the float32 restatements against the float64 oracle ------------------------------------------------------
@pytest.mark.parametrize("mode", KC.MODES)
def test_restatements_keep_the_cap(mode):
    """Over every shape, seed, pattern, temperature and k: the restated float32 draw leaves the float64 oracle in at most
    EXCUSED_CAP of the draws, only within DELTA / DELTA_SCAN of a boundary, and never picks outside the kept set."""
    worst_frac, worst_dist, cases = 0.0, 0.0, 0
    for shape, s in sorted(SC.BIAS_SHAPES.items()):
        for seed in SC.SEEDS:
            u = SC.u01_table(seed, s.T, s.B)
            for pattern in SC.PATTERNS:
                b4 = SC.b4_pattern(pattern)
                for temperature in SC.TEMPERATURES:
                    for k in KC.CPU_KS:
                        got = KC.EMULATE[mode](b4, temperature, k, u)
                        draws, excused, worst = KC.judge_draws(got, b4, temperature, k, u, mode)
                        worst_frac, worst_dist, cases = max(worst_frac, excused / draws), max(worst_dist, worst), cases + 1
    print(f"TOPK-CPU {mode}: {cases} cases, worst mismatch fraction {worst_frac:.4%} (cap {SC.EXCUSED_CAP:.1%}), worst "
          f"boundary distance {worst_dist:.2e} ({worst_dist / KC.DELTA[mode]:.2%} of the tolerance)")
    assert cases == len(SC.BIAS_SHAPES) * len(SC.SEEDS) * len(SC.PATTERNS) * len(SC.TEMPERATURES) * len(KC.CPU_KS)


def test_exact_cases_hold_in_the_restatements():
    s = SC.EDGE_SHAPES["launch-D32-B8"]
    for seed in SC.EDGE_SEEDS + tuple(KC.U1_SEEDS):
        u = SC.u01_table(seed, s.T, s.B)
        for mode in KC.MODES:
            for k in KC.EQUAL_KS:
                b4 = np.full(SC.Q, SC.EDGE_LOGIT, dtype=np.float32)
                assert np.array_equal(KC.EMULATE[mode](b4, 1.0, k, u), KC.equal_logits_picks(k, u)), (seed, mode, k)
            b4, _ = SC.tie_pattern(KC.TWO_MAXIMA)
            assert np.array_equal(KC.EMULATE[mode](b4, 1.0, 2, u), KC.two_maxima_picks(u)), (seed, mode)
            assert np.array_equal(KC.oracle_picks(b4, 1.0, 2, u), KC.two_maxima_picks(u))
            for name in SC.TIE_MAXIMA:    # k = 1 is the arg-max
                b4, want = SC.tie_pattern(name)
                assert np.unique(KC.EMULATE[mode](b4, 1.0, 1, u)).tolist() == [want]


# ---- 3. a uniform of exactly 1.0 ----------------------------------------------------------------------------------------------------
def test_u01_of_exactly_one():
    s = SC.EDGE_SHAPES["launch-D32-B8"]
    assert (s.B, s.T) == (8, 3) and SC.EDGE_SHAPES["persist-D256-B8"][2:4] == (8, 3)
    b4, _ = SC.tie_pattern(KC.TWO_MAXIMA)
    for seed, (b, t) in KC.U1_SEEDS.items():
        u = SC.u01_table(seed, s.T, s.B)
        assert u[b, t - KC.BFS] == 1.0, (seed, b, t, u[b, t - KC.BFS])
        assert np.argwhere(u == 1.0).tolist() == [[b, t - KC.BFS]]
        # no code satisfies u < c: the untruncated draw ends on Q - 1, the truncated one on the highest kept code
        assert SC.oracle_picks(b4, 1.0, u)[b, t - KC.BFS] == SC.Q - 1
        assert KC.oracle_picks(b4, 1.0, 2, u)[b, t - KC.BFS] == 69
        for mode in KC.MODES:
            assert KC.EMULATE[mode](b4, 1.0, 2, u)[b, t - KC.BFS] == 69, mode


# ---- 4. the interface ---------------------------------------------------------------------------------------------------------------
def test_new_names_are_reexported(tt):
    from parrot_amd.sampleRNN.generation import inputs
    for name in ("build_packed_top_k", "top_k_code", "top_k_array", "_per_utterance_top_k"):
        assert getattr(tt, name) is getattr(inputs, name), name


def test_top_k_values(tt):
    assert tt.top_k_code(0) == 0 and tt.top_k_code(64) == 64 and tt.top_k_code(np.int32(7)) == 7
    assert tt.top_k_code(2 ** 40) == 2 ** 31 - 1
    for bad in (-1, np.int64(-5), 1.5, "8", None, True):
        with pytest.raises(ValueError):
            tt.top_k_code(bad)
    a = tt.top_k_array([[0, 1], [300, 64]], (2, 2))
    assert a.dtype == np.int32 and a.tolist() == [[0, 1], [300, 64]]
    for bad, shape in (([[0, -1]], (1, 2)), ([0, 1], (1, 2)), ([[0.5, 1.0]], (1, 2)), ([[0, 1]], (2, 1))):
        with pytest.raises(ValueError):
            tt.top_k_array(bad, shape)
    assert tt._per_utterance_top_k(None, 3, 8) == [8, 8, 8] and tt._per_utterance_top_k([1, 0, 64], 3, 8) == [1, 0, 64]
    with pytest.raises(ValueError):
        tt._per_utterance_top_k([1, 2], 3, 0)
    with pytest.raises(ValueError):
        tt._per_utterance_top_k([1, -2, 3], 3, 0)


def test_build_packed_top_k(tt):
    from parrot_amd.sampleRNN.generation import inputs
    T = 4
    for s in range(T):
        got = tt.build_packed_top_k([8], [0], [s], T, 2)
        row = inputs.start_row(s, T)
        want = np.zeros((T, 2), dtype=np.int32)
        if row is not None:
            want[row, 0] = 8
        assert got.dtype == np.int32 and np.array_equal(got, want)
    seeds, temps = tt.build_packed_draws([5], [1.0], [1], [0], T, 2)           # its sibling keeps its signature and result
    assert seeds.shape == temps.shape == (T, 2)
    with pytest.raises(ValueError):
        tt.build_packed_top_k([8], [2], [0], T, 2)
    with pytest.raises(ValueError):
        tt.build_packed_top_k([-8], [0], [0], T, 2)


def test_refusals_come_before_any_device_call(tt, monkeypatch):
    from parrot_amd import _lib
    from parrot_amd.sampleRNN import lib

    def no_device(*a, **k):
        raise AssertionError("a device call in front of the top_k check")
    monkeypatch.setattr(_lib, "call", no_device)
    monkeypatch.setattr(_lib, "load", no_device)
    monkeypatch.setattr(lib, "device", no_device)
    feats = np.zeros((3, 2, 63), dtype=np.float32)
    for bad in (-1, -64, 2.0, "8"):
        with pytest.raises(ValueError):
            tt.DeviceGenerator(2, 3, top_k=bad)
        with pytest.raises(ValueError):
            tt.generate_packed([feats[:, 0]], n_streams=2, top_k=bad)
        with pytest.raises(ValueError):
            next(tt.generate_stream(feats, 2, top_k=bad))
        with pytest.raises(ValueError):
            tt.StreamingGenerator(2, 2, top_k=bad)
        with pytest.raises(ValueError):
            tt.generate_and_save_samples("t", features=feats, top_k=bad)
    with pytest.raises(ValueError):                             # per-utterance values need per-utterance seeds
        tt.generate_packed([feats[:, 0]], n_streams=2, top_ks=[8])
    with pytest.raises(ValueError):
        tt.generate_packed([feats[:, 0]], n_streams=2, seeds=[5], top_ks=[8, 8])
    with pytest.raises(ValueError):
        tt.generate_packed([feats[:, 0]], n_streams=2, seeds=[5], top_ks=[-8])
    with pytest.raises(ValueError):                             # the literal three-function loop draws among all codes
        tt.generate_and_save_samples("t", features=feats, use_device_loop=False, top_k=8)
    tt.configure(SKIP_CONN=True)
    try:
        with pytest.raises(ValueError):
            tt.generate_and_save_samples("t", features=feats, top_k=8)
    finally:
        tt.configure(SKIP_CONN=False)


def _bare_plan(tt, packed, utterance_draws, B=2, T=3):
    """A DeviceGenerator without a device behind it: what generate() checks before it stages anything."""
    gen = object.__new__(tt.DeviceGenerator)
    gen.B, gen.T, gen.packed, gen.utterance_draws, gen._has_run, gen.top_k = B, T, packed, utterance_draws, False, 0
    return gen


def test_generate_refuses_top_ks_in_front_of_the_device(tt, monkeypatch):
    from parrot_amd import _lib

    def no_device(*a, **k):
        raise AssertionError("a device call in front of the top_ks check")
    monkeypatch.setattr(_lib, "call", no_device)
    feats = np.zeros((3, 2, 63), dtype=np.float32)
    starts = np.zeros((3, 2), dtype=np.int32)
    sd, tp = np.zeros((3, 2), dtype=np.uint64), np.ones((3, 2), dtype=np.float32)
    with pytest.raises(ValueError):                             # no utterance_draws: no top_ks
        _bare_plan(tt, False, False).generate(feats, top_ks=[8, 8])
    with pytest.raises(ValueError):
        _bare_plan(tt, True, False).generate(feats, starts, top_ks=np.zeros((3, 2), dtype=np.int32))
    plain, packed = _bare_plan(tt, False, True), _bare_plan(tt, True, True)
    for bad in ([8], [[8, 8]], [8, -1], [8.0, 8.0], -1):
        with pytest.raises(ValueError):
            plain.generate(feats, seeds=[1, 2], temperatures=1.0, top_ks=bad)
    for bad in ([8, 8], np.zeros((2, 2), dtype=np.int32), np.full((3, 2), -1), np.zeros((3, 2), dtype=np.float32)):
        with pytest.raises(ValueError):
            packed.generate(feats, starts, seeds=sd, temperatures=tp, top_ks=bad)
    plain._has_run = True                                       # a plain plan takes them with resume=False only, like seeds
    with pytest.raises(ValueError):
        plain.generate(feats[:2], resume=True, n_frames=2, top_ks=[8, 8])


def test_submit_takes_a_top_k_with_utterance_draws_only(tt):
    runner = lambda features, starts, resume, **kw: np.zeros((2, 80 * features.shape[0]), dtype=np.int32)
    utt = np.zeros((2, 63), dtype=np.float32)
    off = tt.StreamingGenerator(2, 2, run_segment=runner)
    with pytest.raises(ValueError):
        off.submit(utt, top_k=8)
    on = tt.StreamingGenerator(2, 2, run_segment=runner, utterance_draws=True)
    with pytest.raises(ValueError):
        on.submit(utt, seed=1, top_k=-8)
    with pytest.raises(ValueError):
        on.submit(utt, top_k=8)                                  # the seed is still required
    assert on.submit(utt, seed=1, top_k=8) == 0


def test_runner_contract(tt):
    """A runner of the caller's sees top_ks only when the generator truncates: its top_k is non-zero, or some utterance was
    submitted with one.  Otherwise it is called as before: three arguments, or five with utterance_draws."""
    seen = []

    def three(features, starts, resume):
        seen.append(())
        return np.zeros((2, 80 * features.shape[0]), dtype=np.int32)

    def five(features, starts, resume, seeds, temperatures):
        seen.append((seeds, temperatures))
        return np.zeros((2, 80 * features.shape[0]), dtype=np.int32)

    def six(features, starts, resume, seeds=None, temperatures=None, top_ks=None):
        seen.append((starts.copy(), seeds, temperatures, top_ks))
        return np.zeros((2, 80 * features.shape[0]), dtype=np.int32)

    utt = np.zeros((3, 63), dtype=np.float32)
    sg = tt.StreamingGenerator(2, 2, run_segment=three)
    sg.submit(utt)
    assert sg.drain() and seen
    sg = tt.StreamingGenerator(2, 2, run_segment=five, utterance_draws=True)
    sg.submit(utt, seed=7)
    assert sg.drain()
    # the generator's own top_k, without per-utterance draws: top_ks on the start rows, nothing else
    del seen[:]
    sg = tt.StreamingGenerator(2, 2, run_segment=six, top_k=8)
    sg.submit(utt)
    sg.submit(utt[:2])
    assert sg.drain()
    for starts, sd, tp, tk in seen:
        assert sd is None and tp is None and tk.dtype == np.int32 and tk.shape == starts.shape
        assert np.array_equal(tk, np.where(starts != 0, 8, 0))
    assert sum(int((s[0] != 0).sum()) for s in seen) == 2
    # per utterance: one submitted with a top_k switches the keyword on; the others take the generator's (here 0)
    del seen[:]
    sg = tt.StreamingGenerator(2, 2, run_segment=six, utterance_draws=True)
    sg.submit(utt, seed=7)
    assert sg.step() and seen[-1][3] is None
    sg.submit(utt, seed=8, top_k=64)
    sg.submit(utt, seed=9, temperature=0.5)
    assert sg.drain()
    ks = np.concatenate([tk[starts != 0] for starts, _, _, tk in seen[1:]])
    assert all(tk is not None and tk.dtype == np.int32 for _, _, _, tk in seen[1:])
    assert sorted(ks.tolist()) == [0, 64], ks


def test_descriptor_and_signature():
    from parrot_amd import _lib
    D = _lib.SampleRnnGenDesc
    # the descriptor has no spare word: top_k is the upper half of the four bytes that were `int use_graph`
    assert C.sizeof(D) == 936 and (D.use_graph.offset, D.top_k.offset, D.temperature.offset) == (28, 30, 32)
    assert D.use_graph.size == 2 and D.top_k.size == 2 and D().top_k == 0
    d = D()
    d.use_graph, d.top_k = 1, 255
    assert C.cast(C.byref(d, 28), C.POINTER(C.c_int))[0] == 1 + (255 << 16)     # (little-endian: the flag stays where it was)
    txt = open(os.path.join(ROOT, "include", "parrot_hip.h")).read()
    body = txt[txt.index("typedef struct SampleRnnGenDesc {"):txt.index("} SampleRnnGenDesc;")]
    assert re.search(r"short\s+use_graph,\s*top_k;", body)
    assert re.search(r"int samplernn_generate_set_utterance_top_k\(void\* plan, const int\* utt_top_k\);", txt)
    assert _lib.SIGNATURES["samplernn_generate_set_utterance_top_k"] == (C.c_int, [C.c_void_p, C.c_void_p])
    assert _lib.SIGNATURES["samplernn_generate_set_utterance_draws"] == (C.c_int, [C.c_void_p] * 3)


def test_c_entry_refuses_null_arguments():
    from parrot_amd import _lib
    fn = _lib.load().samplernn_generate_set_utterance_top_k
    buf = (C.c_int * 4)()
    assert fn(None, C.addressof(buf)) == 10001                  # PARROT_ERR_BADARG, no device call
    assert fn(C.addressof(buf), None) == 10001                  # (the plan is only looked at after the pointer)


def test_parser_has_the_flag():
    from parrot_amd.utils import sample_parse
    assert sample_parse([]).top_k == 0
    assert sample_parse(['--top_k', '64']).top_k == 64
    with pytest.raises(SystemExit):
        sample_parse(['--top_k', 'many'])


def test_sample_raw_refuses_a_negative_top_k(tt):
    from parrot_amd.model import SampleRnn
    m = object.__new__(SampleRnn)      # (no parameters, no device: the check comes first)
    m.three_tier = tt
    with pytest.raises(ValueError):
        m.sample_raw(None, None, "t", None, top_k=-1)

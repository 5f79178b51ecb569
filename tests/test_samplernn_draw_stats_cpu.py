"""The per-step draw statistics of the SampleRNN generator (samplernn_generate_set_draw_stats), as far as they can be checked
without a GPU: the references of the cases module, the premises of the GPU tests' tolerance, and the interface -- keywords,
the order of what generate returns, the refusals in front of any device call, the header and the signature.
Cases: tests/samplernn_draw_stats_cases.py."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from tests import samplernn_draw_stats_cases as DS
from tests import samplernn_forced_cases as FC
from tests import samplernn_min_p_cases as MC
from tests import samplernn_sampling_cases as SC
from tests import samplernn_top_k_cases as KC
from tests import samplernn_top_p_cases as NC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tt():
    from parrot_amd.sampleRNN.models.conditional import three_tier
    return three_tier


def test_draw_logp_reference():
    lg = np.log(np.array([1.0, 4.0, 4.0, 0.5, 4.0, 2.0, 2.0, 0.25], dtype=np.float64)).astype(np.float32)
    s = np.arange(8)
    # untruncated at T = 1: the softmax itself (tot = 17.75)
    assert np.allclose(DS.draw_logp64(lg, 1.0, s), np.log(np.array([1, 4, 4, .5, 4, 2, 2, .25]) / 17.75), atol=1e-6)
    # top_k = 3 keeps the three maxima: a third each, -inf outside
    got = DS.draw_logp64(lg, 1.0, s, k=3)
    assert np.allclose(got[[1, 2, 4]], np.log(1 / 3), atol=1e-6) and np.isneginf(got[[0, 3, 5, 6, 7]]).all()
    # min_p = 0.4 keeps five: mass 16
    got = DS.draw_logp64(lg, 1.0, s, min_p=0.4)
    assert np.allclose(got[[1, 5]], np.log(np.array([4, 2]) / 16), atol=1e-6) and np.isneginf(got[[0, 3, 7]]).all()
    # at temperature T the terms are the T-th roots
    got = DS.draw_logp64(lg, 2.0, s)
    r = np.sqrt(np.array([1, 4, 4, .5, 4, 2, 2, .25]))
    assert np.allclose(got, np.log(r / r.sum()), atol=1e-6)
    # an argmax step: 0 for the argmax (the lowest index of the maxima), -inf for any other code
    got = DS.draw_logp64(lg, 0.0, s)
    assert got[1] == 0.0 and np.isneginf(np.delete(got, 1)).all() and DS.oracle_m(lg, 0.0) == 1
    # the probabilities of a kept set add up to one
    for kw in (dict(), dict(k=64), dict(p=0.9), dict(min_p=0.1), dict(k=64, p=0.9, min_p=0.1)):
        b4 = SC.b4_pattern("randn")
        got = DS.draw_logp64(b4, 1.0, np.arange(SC.Q), **kw)
        assert abs(np.exp(got).sum() - 1.0) < 1e-12 and int(np.isfinite(got).sum()) == DS.oracle_m(b4, 1.0, **kw)


def test_premises_of_the_tolerance():
    assert DS.TOL == SC.DELTA == 2.0 ** -14
    worst = 0.0
    for pattern in SC.PATTERNS:
        b4 = SC.b4_pattern(pattern)
        for tau in SC.TEMPERATURES:
            worst = max(worst, DS.largest_kept_argument(b4, tau))
    print(f"DRAWSTATS-CPU largest |(lg - max) / T| over the cases: {worst:.1f} (bound {DS.MAX_ARG})")
    assert worst <= DS.MAX_ARG
    # every case the kept counts are compared on keeps the margins that make the device's set the oracle's
    for pattern, tau, min_p in MC.CASES:
        assert 1 <= DS.oracle_m(SC.b4_pattern(pattern), tau, min_p=min_p) <= SC.Q
    for pattern in SC.PATTERNS:
        for tau in SC.TEMPERATURES:
            for k, p, min_p in DS.OTHER_TRUNCATIONS:
                DS.oracle_m(SC.b4_pattern(pattern), tau, k, p, min_p)
            assert (pattern, tau, 0.9, 0) in NC.CASES
    # the forced code outside the kept set, and the one inside
    b4 = SC.b4_pattern("peaked")
    keep = np.nonzero(KC.kept_set(b4, DS.OUTSIDE_K))[0].tolist()
    assert keep == list(SC.PEAKED_CODES) and DS.OUTSIDE_CODE not in keep and DS.INSIDE_CODE in keep
    assert int(np.argmax(b4)) == DS.INSIDE_CODE


def test_forced_reference_at_temperature_one_is_the_log_prob_reference():
    _, _, _, want = FC.reference('gru')
    _, _, forced, got = DS.forced_reference(1.0)
    assert got.shape == want.shape == (FC.REF_B, FC.BFS * (FC.REF_T - 1)) and np.allclose(got, want, rtol=0, atol=1e-12)
    for tau in DS.FORCED_TEMPERATURES:
        lp = DS.forced_reference(tau)[3]
        assert lp.shape == want.shape and (lp < 0).all() and not np.allclose(lp, want)


def test_keywords_and_what_is_left_out(tt):
    assert inspect.signature(tt.DeviceGenerator.__init__).parameters["draw_stats"].default is False
    assert inspect.signature(tt.generate_packed).parameters["draw_stats"].default is False
    for fn in (tt.StreamingGenerator.__init__, tt.StreamingGenerator.submit, tt.generate_stream, tt.generate_and_save_samples):
        assert "draw_stats" not in inspect.signature(fn).parameters, fn.__qualname__
    from parrot_amd.utils import sample_parse
    assert not hasattr(sample_parse([]), "draw_stats")
    assert tt.generate_packed([], draw_stats=True) == ([], [], [])
    assert tt.generate_packed([], draw_stats=True, log_probs=True) == ([], [], [], [])
    assert tt.generate_packed([], log_probs=True) == ([], []) and tt.generate_packed([]) == []


def test_unpack_keeps_the_counts_integers(tt):
    from parrot_amd.sampleRNN.generation import inputs
    kept = np.arange(2 * 240, dtype=np.int32).reshape(2, 240)
    got = inputs.unpack_log_probs(kept, [2, 1], [0, 1], [0, 1], dtype=kept.dtype)
    assert got[0].dtype == np.int32 and np.array_equal(got[0], kept[0, 80:160]) and got[1].size == 0
    assert inputs.unpack_log_probs(kept.astype(np.float64), [2], [0], [0])[0].dtype == np.float32   # (as it always did)


def test_header_and_signature():
    from parrot_amd import _lib
    txt = open(os.path.join(ROOT, "include", "parrot_hip.h")).read()
    assert re.search(r"int samplernn_generate_set_draw_stats\(void\* plan, float\* draw_logp, int\* kept\);", txt)
    assert _lib.SIGNATURES["samplernn_generate_set_draw_stats"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p])
    assert "samplernn_generate_set_draw_stats" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = _lib.load()
    buf = (C.c_float * 4)()
    assert lib.samplernn_generate_set_draw_stats(None, C.addressof(buf), C.addressof(buf)) == 10001   # PARROT_ERR_BADARG
    assert lib.samplernn_generate_set_draw_stats(C.addressof(buf), None, C.addressof(buf)) == 10001   # (pointers first)
    assert lib.samplernn_generate_set_draw_stats(C.addressof(buf), C.addressof(buf), None) == 10001

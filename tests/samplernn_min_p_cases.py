"""Cases, references and judging rules of the min-p truncated draw of the SampleRNN generator
(samplernn_generate_set_min_p, samplernn_generate_set_utterance_min_p; `srp_minp_keep` of sr_common.h as used by
`sr_pick_kernel` in samplernn.hip and by the pick of `srp_kernel` in sr_persist.hip; three_tier.DeviceGenerator(min_p=),
generate(..., min_ps=)).

The rule, for one draw with float32 logits lg[0..Q-1], temperature T > 0 and 0 < min_p <= 1:
  * e_q = expf((lg_q - max) / T) as the draw computes it; a code is kept iff e_q >= min_p (a float32 compare).  The argmax
    has e = 1.0f exactly, so the set is never empty; min_p = 1 keeps exactly the maxima;
  * the kept set of a draw is top_k's set, the nucleus of top_k's set (found without regard to min_p) and min-p's set
    intersected.  Each of the three is a prefix of the order "logit descending, index ascending" in exact arithmetic, so the
    intersection is the shortest of them;
  * every code outside gets the term 0.0f, and everything else is a top_k draw with k = m = that length.
So the judge of any such draw is tests/samplernn_top_k_cases.py's with k = m, and m comes from the float64 oracle here.

This module imports no GPU code.  tests/test_samplernn_min_p_cpu.py checks its premises; tests/test_gpu_samplernn_min_p.py
runs the cases."""
import numpy as np

from tests import samplernn_sampling_cases as SC
from tests import samplernn_top_k_cases as KC
from tests import samplernn_top_p_cases as NC

Q, BFS, LANES = KC.Q, KC.BFS, KC.LANES
MODES = KC.MODES

# How far every ratio e_q / e_max of a listed case lies from min_p, relative to min_p.  The device's term differs from the
# exact ratio by the two roundings of its argument x = (lg - max) / T -- |x| 2^-23 in all, and a code near the bar has
# |x| ~ ln(1 / min_p) <= 4 for the listed values (ln 50 = 3.9) --, which moves exp(x) by that much relatively: 4 2^-23 =
# 2^-21; plus expf's own one or two ulp, 2 2^-24 = 2^-23.  Together below 2^-20; MARGIN is four times that.
MARGIN = 2.0 ** -18
assert 4 * 2.0 ** -23 + 2 * 2.0 ** -24 < 2.0 ** -20 and MARGIN == 4 * 2.0 ** -20

MIN_PS = (0.02, 0.1, 0.5, 0.98)
assert np.log(1.0 / min(MIN_PS)) <= 4.0
CASES = [(pattern, tau, min_p) for pattern in SC.PATTERNS for tau in SC.TEMPERATURES for min_p in MIN_PS]
COMBINED_MIN_P = 0.1
COMBINED_KP = ((64, 0.0), (0, 0.9), (64, 0.9))   # (top_k, top_p) in front of min_p = 0.1


def ratios64(logits, temperature):
    """e_q / e_max in float64: exp((lg_q - max) / T) of the float32 logits."""
    lg = np.asarray(logits, dtype=np.float32).astype(np.float64)
    return np.exp((lg - lg.max()) / temperature)


def min_p_m(logits, temperature, min_p):
    """The number of codes whose ratio is >= min_p (all of them when min_p is off: outside (0, 1])."""
    r = ratios64(logits, temperature)
    if not 0.0 < min_p <= 1.0:
        return int(r.size)
    return int((r >= min_p).sum())


def margin(logits, temperature, min_p):
    """The smallest |ratio / min_p - 1| over the codes."""
    return float(np.abs(ratios64(logits, temperature) / min_p - 1.0).min())


def kept_m(logits, temperature, k=0, p=0.0, min_p=0.0):
    """m of a draw with any combination: the shortest of top_k's prefix, the nucleus of it and min-p's prefix."""
    m = int(KC.kept_set(logits, k).sum())
    m = min(m, NC.nucleus_m(logits, temperature, p, k))
    return min(m, min_p_m(logits, temperature, min_p))


def case_m(logits, temperature, min_p, k=0, p=0.0):
    """m of a case the device is judged on; asserts the premises: every ratio farther than MARGIN from min_p and, with a
    nucleus, NC.case_m's own premise."""
    if 0.0 < min_p <= 1.0:
        d = margin(logits, temperature, min_p)
        assert d > MARGIN, f"min_p = {min_p}: a ratio lies {d:.3e} from it (T = {temperature}): not a case"
    if 0.0 < p < 1.0:
        NC.case_m(logits, temperature, p, k)
    return kept_m(logits, temperature, k, p, min_p)


def kept_set(logits, temperature, k=0, p=0.0, min_p=0.0):
    """bool [Q]: the first kept_m codes of the order."""
    return KC.kept_set(logits, kept_m(logits, temperature, k, p, min_p))


def combined_cases():
    """(pattern, T, top_k, top_p) in front of min_p = COMBINED_MIN_P: every combination whose nucleus keeps NC's own margin
    (NC.case_m's premise); a combination that does not is dropped here, no margin is loosened."""
    out = []
    for pattern in SC.PATTERNS:
        b4 = SC.b4_pattern(pattern)
        for tau in SC.TEMPERATURES:
            for k, p in COMBINED_KP:
                if margin(b4, tau, COMBINED_MIN_P) <= MARGIN:
                    continue   # (none of the listed ones: test_samplernn_min_p_cpu.py checks that)
                if 0.0 < p < 1.0 and NC.margin(b4, tau, p, k) <= NC.MARGIN:
                    continue   # the nucleus' cut is not promised there
                out.append((pattern, tau, k, p))
    return out


# ---- float32 restatement --------------------------------------------------------------------------------------------------
def min_p_m_f32(logits, temperature, min_p):
    """The count as the device finds it: float32 terms against the float32 bar."""
    lg = np.asarray(logits, dtype=np.float32)
    e = np.exp((lg - lg.max()) / np.float32(temperature)).astype(np.float32)
    return int((e >= np.float32(min_p)).sum())


def emulate_picks_f32(logits, temperature, min_p, u, mode):
    """The float32 restatement of a min-p draw: the device's count, then KC's restatement of the top-k draw with k = m."""
    return KC.EMULATE[mode](logits, temperature, min_p_m_f32(logits, temperature, min_p), u)


def judge_draws(picks, logits, temperature, min_p, u, mode, k=0, p=0.0, cap=SC.EXCUSED_CAP):
    """picks [B, n] against the float64 oracle = KC.judge_draws with k = the oracle's m.  Returns (m, draws, excused
    mismatches, their largest boundary distance)."""
    m = case_m(logits, temperature, min_p, k, p)
    return (m,) + KC.judge_draws(picks, logits, temperature, m, u, mode, cap=cap)


# ---- exact cases ----------------------------------------------------------------------------------------------------------
EXACT_MIN_PS = (0.02, 0.5, 1.0)       # all-equal logits: every term is 1.0f >= any of them


def equal_logits_picks(u):
    """All logits equal, any active min_p: all 256 kept, every sum an integer: the pick is floor(256 u01) in both modes
    (u01 = 1.0: the fall-through, 255)."""
    return KC.equal_logits_picks(Q, u)


FOUR_MAXIMA = KC.TWO_MAXIMA            # SC.TIE_MAXIMA["one-lane-and-another"]: maxima at 5, 69, 133, 200
FOUR_CODES = (5, 69, 133, 200)
FOUR_MIN_PS = (1.0, 0.02)              # at T = 1 every other ratio is below 0.0183: both keep the four


def four_maxima_picks(u):
    """Four terms of exactly 1.0 at FOUR_CODES, every other 0.0f: the sums are the integers 0 .. 4 in both modes and 4 u01
    is exact, so the pick is the floor(4 u01)-th of them -- 200 where u01 is exactly 1.0 (the fall-through)."""
    j = np.minimum(np.floor(4 * np.asarray(u)), 3).astype(np.int64)
    return np.asarray(FOUR_CODES, dtype=np.int32)[j]


# ---- per utterance: one team of the persistent kernel mixes every kind of truncation ---------------------------------------
UTT_MIN_PS = (0.0, 0.1, 1.0, 0.5)      # utterance i draws with UTT_MIN_PS[i % 4] ...


def utt_min_ps(n):
    return [UTT_MIN_PS[i % len(UTT_MIN_PS)] for i in range(n)]

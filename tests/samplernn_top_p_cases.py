"""Cases, references and judging rules of the top-p (nucleus) truncated draw of the SampleRNN generator
(samplernn_generate_set_top_p, samplernn_generate_set_utterance_top_p; `srp_topp_keep` of sr_common.h as used by
`sr_pick_kernel` in samplernn.hip and by the pick of `srp_kernel` in sr_persist.hip; three_tier.DeviceGenerator(top_p=),
generate(..., top_ps=)).

The rule, for one draw with logits lg[0..Q-1], temperature T > 0, 0 < p < 1 and optionally an active top_k:
  * K = top_k's kept set (all codes without), ordered by logit descending, then by code index ascending;
  * the nucleus is the shortest prefix q_1 .. q_m of that order whose mass is >= p tot_K; m >= 1, ties to the lower index;
  * every code outside the nucleus gets the term 0.0f, and everything else is a top_k draw with k = m.
So the judge of a nucleus draw is tests/samplernn_top_k_cases.py's with k = m, and m comes from the float64 oracle here.

What is promised about the cut: m equals the oracle's whenever every prefix mass of the oracle lies farther than
SC.DELTA = 2^-14 from p, as a fraction of tot_K (any sum of at most 256 terms is off by at most (256 + 3) 2^-24 relative, a
ratio of two sums by twice that, and the bound doubles it again).  `case_m` asserts that premise for every case it serves.

This module imports no GPU code.  tests/test_samplernn_top_p_cpu.py checks its premises; tests/test_gpu_samplernn_top_p.py
runs the cases."""
import numpy as np

from tests import samplernn_sampling_cases as SC
from tests import samplernn_top_k_cases as KC

Q, BFS, LANES = KC.Q, KC.BFS, KC.LANES
MODES = KC.MODES
MARGIN = SC.DELTA                     # 2^-14: how far every prefix mass of a listed case lies from p

PS = (0.25, 0.5, 0.9, 0.95)           # draws against the oracle
WITH_K = (0, 64)                      # alone, and behind top_k = 64
CASES = [(pattern, tau, p, k) for pattern in SC.PATTERNS for tau in SC.TEMPERATURES for p in PS for k in WITH_K]
SMALL_P = 2.0 ** -10                  # m = 1 on every tie pattern: the first term alone is 1 >= p tot (tot <= 256)
EQUAL_P = 0.25                        # all-equal logits: p Q = 64 exactly
TWO_MAXIMA_P = 0.25                   # KC.TWO_MAXIMA: see two_maxima_m


def order(logits):
    """The codes by logit descending, then by code index ascending (KC.kept_set's order; -0.0 and 0.0 are one logit)."""
    lg = np.asarray(logits, dtype=np.float32)
    return np.lexsort((np.arange(lg.size), -lg.astype(np.float64)))


def prefix_masses64(logits, temperature, k=0):
    """(codes of K in the rule's order, their prefix masses as fractions of tot_K), float64."""
    lg = np.asarray(logits, dtype=np.float64)
    keep = KC.kept_set(logits, k)
    o = order(logits)
    o = o[keep[o]]
    e = np.exp((lg[o] - lg.max()) / temperature)
    c = np.cumsum(e)
    return o, c / c[-1]


def nucleus_m(logits, temperature, p, k=0):
    """m of the rule in float64: the length of the shortest prefix of K whose mass is >= p tot_K (at least 1).  p outside
    (0, 1): no nucleus, m = |K|."""
    o, c = prefix_masses64(logits, temperature, k)
    if not 0.0 < p < 1.0:
        return int(o.size)
    return int(min(np.searchsorted(c, p, side="left") + 1, o.size))


def margin(logits, temperature, p, k=0):
    """The distance of p from the nearest prefix mass of the oracle, as a fraction of tot_K."""
    _, c = prefix_masses64(logits, temperature, k)
    return float(np.abs(c - p).min())


def nucleus_set(logits, temperature, p, k=0):
    """bool [Q]: the nucleus (behind top_k = k when k is active): the first m codes of the order."""
    return KC.kept_set(logits, nucleus_m(logits, temperature, p, k))


def case_m(logits, temperature, p, k=0):
    """m of a case the device is judged on; asserts the premise of the promise about the cut."""
    d = margin(logits, temperature, p, k)
    assert d > MARGIN, f"p = {p} is {d:.3e} from a prefix mass of the oracle (T = {temperature}, k = {k}): not a case"
    return nucleus_m(logits, temperature, p, k)


# ---- float32 restatements of the device's selection ---------------------------------------------------------------------
def wave_sum_f32(v):
    """srp_wave_sum: the 64 lane values as the fixed tree of float32 adds -- lanes l and l^1, l^2, the mirror inside each
    half-row of 8 and each row of 16, then rows (0 + 1) + (2 + 3)."""
    v = np.asarray(v, dtype=np.float32)
    assert v.shape == (LANES,)
    l = np.arange(LANES)
    for src in (l ^ 1, l ^ 2, (l & ~7) | (7 - (l & 7)), (l & ~15) | (15 - (l & 15))):
        v = (v + v[src]).astype(np.float32)
    assert all(len(set(v[16 * r:16 * r + 16].tolist())) == 1 for r in range(4))   # (commutative adds: a row agrees)
    return np.float32(np.float32(v[0] + v[16]) + np.float32(v[32] + v[48]))


def lane_layout(mode, n_codes=Q):
    """[64, n] code indices: lane l's codes left to right -- l + 64 m in the sequential branches, n l + j in the scan's."""
    n = n_codes // LANES
    l = np.arange(LANES)[:, None]
    j = np.arange(n)[None, :]
    return l + LANES * j if mode == "sequential" else n * l + j


def mass_f32(e, inside, mode):
    """The device's mass of the codes `inside` (bool [Q]) with terms e (float32 [Q]): the lane's codes left to right, then
    the tree."""
    lay = lane_layout(mode, e.size)
    t = np.where(inside, e, np.float32(0)).astype(np.float32)[lay]
    s = t[:, 0]
    for j in range(1, t.shape[1]):
        s = (s + t[:, j]).astype(np.float32)
    return wave_sum_f32(s)


def nucleus_m_f32(logits, temperature, p, k, mode):
    """m as the device finds it: float32 terms (masked by top_k first), the bar p * M(K) as one float32 product, the
    shortest prefix whose float32 mass reaches it."""
    e, keep = KC._masked_terms_f32(logits, temperature, k)
    o = order(logits)
    o = o[keep[o]]
    need = np.float32(np.float32(p) * mass_f32(e, keep, mode))
    inside = np.zeros(e.size, dtype=bool)
    for m, q in enumerate(o, 1):
        inside[q] = True
        if mass_f32(e, inside, mode) >= need:
            return m
    raise AssertionError("the mass of all of K does not reach p times itself")


def emulate_picks_f32(logits, temperature, p, k, u, mode):
    """The float32 restatement of a nucleus draw: the device's cut, then KC's restatement of the top-k draw with k = m."""
    return KC.EMULATE[mode](logits, temperature, nucleus_m_f32(logits, temperature, p, k, mode), u)


def judge_draws(picks, logits, temperature, p, k, u, mode, cap=SC.EXCUSED_CAP):
    """picks [B, n] against the float64 oracle of the nucleus draw = KC.judge_draws with k = the oracle's m: no pick
    outside the nucleus; mismatches only within DELTA[mode] of a boundary of the truncated CDF, in at most `cap` of the
    draws.  Returns (m, draws, excused mismatches, their largest boundary distance)."""
    m = case_m(logits, temperature, p, k)
    return (m,) + KC.judge_draws(picks, logits, temperature, m, u, mode, cap=cap)


# ---- exact cases ----------------------------------------------------------------------------------------------------------
def equal_logits_m(p=EQUAL_P):
    """All logits equal: every term is 1.0, every mass an integer, p Q exact: m = p Q with no slack in any arithmetic."""
    m = p * Q
    assert m == int(m) and int(m) & (int(m) - 1) == 0
    return int(m)


def two_maxima_m(temperature=1.0, p=TWO_MAXIMA_P):
    """KC.TWO_MAXIMA (maxima at 5, 69, 133, 200): each maximum holds 0.155 of the mass, so the prefix masses begin 0.155,
    0.311, 0.466 and p = 0.25 cuts behind the second with a margin above 0.05: the nucleus is {5, 69}."""
    b4, _ = SC.tie_pattern(KC.TWO_MAXIMA)
    m = case_m(b4, temperature, p)
    assert m == 2 and margin(b4, temperature, p) > 0.05
    assert np.nonzero(nucleus_set(b4, temperature, p))[0].tolist() == [5, 69]
    return m


# ---- per utterance: one team of the persistent kernel mixes nuclei, truncations and temperatures -------------------------
UTT_PS = (0.0, 0.9, 2.0 ** -10, 0.5, 1.0)   # utterance i draws with UTT_PS[i % 5] ...


def utt_top_ps(n):
    return [UTT_PS[i % len(UTT_PS)] for i in range(n)]

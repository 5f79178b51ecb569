"""Cases, references and judging rules of the top-k truncated draw of the SampleRNN generator (SampleRnnGenDesc::top_k,
samplernn_generate_set_utterance_top_k; `srp_topk_keep` of sr_common.h as used by `sr_pick_kernel` in samplernn.hip and
by the pick of `srp_kernel` in sr_persist.hip; three_tier.DeviceGenerator(top_k=), generate(..., top_ks=)).

The rule, for one draw with logits lg[0..Q-1], temperature T > 0 and 1 <= k < Q:
  * kept set = the k codes that come first when the codes are ordered by logit descending, then by code index ascending
    (a tie at the cut-off goes to the lower index, like the arg-max);
  * terms e_q = expf((lg_q - max) / T) for a kept code, 0.0f for every other code;
  * the max, the key, the counter, the uniform, `u01 tot < c` and the order of the float32 additions are those of the
    untruncated draw in both modes (adding 0.0f is exact, so DELTA and DELTA_SCAN still bound the sums' error);
  * where no code satisfies u < c the pick is the highest kept code (sequential walk), or the highest kept code not above
    the code the scan falls through to without truncation (Q - 1, or the last code of the hit lane);
  * k = 0 or k >= Q: no truncation.

The constructions (bias-only logits, patterns, uniforms, shapes, seeds, tolerances) are those of
tests/samplernn_sampling_cases.py and tests/samplernn_draw_scan_cases.py.  This module imports no GPU code.
tests/test_samplernn_top_k_cpu.py checks its premises; tests/test_gpu_samplernn_top_k.py runs the cases."""
import numpy as np

from tests import samplernn_draw_scan_cases as DC
from tests import samplernn_sampling_cases as SC

Q, BFS, LANES = SC.Q, SC.BFS, DC.LANES
DELTA = {"sequential": SC.DELTA, "scan": DC.DELTA_SCAN}
MODES = ("sequential", "scan")

CPU_KS = (1, 2, 3, 64, 255)          # the cap check of the restatements
GPU_KS = (2, 64, 255)                # draws against the oracle on the device
EQUAL_KS = (2, 64, 128)              # all-equal logits: the pick is floor(k u01)
TWO_MAXIMA = "one-lane-and-another"  # SC.TIE_MAXIMA: maxima at 5, 69, 133, 200 -- with k = 2 the kept set is {5, 69}

# Plan seeds with a draw whose u01 is exactly 1.0 at B = 8, T = 3 (SC.EDGE_SHAPES), found by search: seed -> (stream,
# sample index).  With u01 = 1.0 no code satisfies u < c, and the untruncated fall-through Q - 1 lies outside the kept set.
U1_SEEDS = {1612: (5, 218), 13571: (0, 133)}


def kept_set(logits, k):
    """bool [Q]: the kept set of the rule; k <= 0 or k >= Q keeps every code.  (-0.0 and 0.0 are one logit.)"""
    lg = np.asarray(logits, dtype=np.float32)
    if k <= 0 or k >= lg.size:
        return np.ones(lg.size, dtype=bool)
    order = np.lexsort((np.arange(lg.size), -lg.astype(np.float64)))   # last key first: logit descending, then index
    keep = np.zeros(lg.size, dtype=bool)
    keep[order[:k]] = True
    return keep


def cdf64(logits, temperature, k):
    """The truncated CDF in float64: softmax(logits / temperature) over the kept codes, 0 for the others, summed."""
    lg = np.asarray(logits, dtype=np.float64)
    keep = kept_set(logits, k)
    z = (lg - lg[keep].max()) / temperature
    p = np.where(keep, np.exp(z), 0.0)
    return np.cumsum(p / p.sum())


def oracle_picks(logits, temperature, k, u):
    """First q with u < c_q of the truncated CDF; where there is none, the highest kept code."""
    c = cdf64(logits, temperature, k)
    last = int(np.nonzero(kept_set(logits, k))[0][-1])
    q = np.searchsorted(c, u, side="right")
    return np.where(q >= c.size, last, q).astype(np.int32)


def _masked_terms_f32(logits, temperature, k):
    lg = np.asarray(logits, dtype=np.float32)
    e = np.exp((lg - lg.max()) / np.float32(temperature)).astype(np.float32)   # (the max of all codes is a kept code)
    keep = kept_set(logits, k)
    return np.where(keep, e, np.float32(0)).astype(np.float32), keep


def emulate_picks_f32(logits, temperature, k, u):
    """SC.emulate_picks_f32 with masked terms: the sequential walk over all Q codes in float32; fall-through = the highest
    kept code."""
    e, keep = _masked_terms_f32(logits, temperature, k)
    c = np.cumsum(e, dtype=np.float32)
    uu = np.asarray(u).astype(np.float32) * c[-1]
    assert uu.dtype == np.float32
    q = np.searchsorted(c, uu, side="right")
    return np.where(q >= c.size, int(np.nonzero(keep)[0][-1]), q).astype(np.int32)


def emulate_picks_scan_f32(logits, temperature, k, u):
    """DC.emulate_picks_scan_f32 with masked terms; both fall-through picks are the highest kept code not above the code
    the untruncated scan falls through to."""
    e, keep = _masked_terms_f32(logits, temperature, k)
    n = e.size // LANES
    s = DC.scan_sums_f32(e)
    kept = np.nonzero(keep)[0]

    def kept_up_to(code):
        below = kept[kept <= code]
        return int(below[-1]) if below.size else int(kept[0])

    uu = (np.asarray(u).astype(np.float32) * s[-1]).astype(np.float32)
    x = uu.reshape(-1)
    hit = x[:, None] < s[None, :]                         # [draws, 64]
    ls = hit.argmax(axis=1)                               # the lowest lane with u < s_l (0 where there is none)
    c = np.where(ls == 0, np.float32(0), s[np.maximum(ls - 1, 0)]).astype(np.float32)
    pick = np.array([kept_up_to(n * l + n - 1) for l in range(LANES)])[ls]
    found = np.zeros(x.shape, dtype=bool)
    for j in range(n):                                    # inside the lane: one term at a time, the first code with u < c
        c = (c + e[n * ls + j]).astype(np.float32)
        new = ~found & (x < c)
        pick = np.where(new, n * ls + j, pick)
        found |= new
    pick = np.where(hit.any(axis=1), pick, kept_up_to(e.size - 1))
    return pick.reshape(uu.shape).astype(np.int32)


EMULATE = {"sequential": emulate_picks_f32, "scan": emulate_picks_scan_f32}


def judge_draws(picks, logits, temperature, k, u, mode, cap=SC.EXCUSED_CAP):
    """picks [B, n] against the float64 oracle of the truncated draw.  Without any excuse every pick lies in the kept set;
    a pick may differ from the oracle's only where u01 is within DELTA[mode] of the truncated CDF's boundaries between the
    two, and in at most `cap` of the draws.  Returns (draws, excused mismatches, their largest boundary distance)."""
    picks = np.asarray(picks)
    assert picks.shape == u.shape, (picks.shape, u.shape)
    keep = kept_set(logits, k)
    assert picks.min() >= 0 and picks.max() < keep.size, "a pick out of range"
    outside = np.argwhere(~keep[picks])
    assert outside.size == 0, (f"{len(outside)} picks outside the kept set of k = {k}, first: stream {outside[0][0]}, "
                               f"sample {BFS + outside[0][1]}, pick {picks[tuple(outside[0])]}")
    want = oracle_picks(logits, temperature, k, u)
    c = cdf64(logits, temperature, k)
    worst, delta = 0.0, DELTA[mode]
    bad = np.argwhere(picks != want)
    for b, j in bad:
        d = SC.boundary_distance(c, u[b, j], picks[b, j], want[b, j])
        assert d <= delta, (f"k = {k}, stream {b}, sample {BFS + j}: pick {picks[b, j]}, oracle {want[b, j]}, u01 {u[b, j]!r} "
                            f"is {d:.3e} from the boundary (allowed {delta:.3e}); {len(bad)} of {picks.size} differ")
        worst = max(worst, d)
    assert len(bad) <= cap * picks.size, f"{len(bad)} excused mismatches in {picks.size} draws (cap {cap * picks.size:.1f})"
    return picks.size, len(bad), worst


def equal_logits_picks(k, u):
    """All logits equal: the kept set is codes 0 .. k-1, every kept term is 1.0 and every sum an exact integer in both
    modes, so for k a power of two the pick is floor(k u01) with no slack (u01 = 1.0: the fall-through, k - 1)."""
    assert k & (k - 1) == 0
    return np.minimum(np.floor(k * np.asarray(u)), k - 1).astype(np.int32)


def two_maxima_picks(u):
    """TWO_MAXIMA with k = 2: two terms of exactly 1.0 at codes 5 and 69, tot = 2.0: the pick is 5 where u01 < 0.5, else
    69 -- also at u01 = 1.0, where nothing satisfies u < c and the untruncated draw would fall through to 255."""
    return np.where(np.asarray(u) < 0.5, 5, 69).astype(np.int32)


# ---- per utterance: one team of the persistent kernel mixes truncations and temperatures ------------------------------------
UTT_KS = (0, 1, 8, 64)             # utterance i draws with UTT_KS[i % 4] ...
UTT_TEMPERATURES = (0.5, 1.0, 2.0)  # ... at UTT_TEMPERATURES[i % 3]: every pair occurs among twelve utterances


def utt_top_ks(n):
    return [UTT_KS[i % len(UTT_KS)] for i in range(n)]


def utt_temperatures(n):
    return [UTT_TEMPERATURES[i % len(UTT_TEMPERATURES)] for i in range(n)]

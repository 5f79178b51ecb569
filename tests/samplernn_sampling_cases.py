"""Cases, references and judging rules of the SampleRNN sampler tests (`sr_pick_kernel` of samplernn.hip and the pick of
`srp_kernel` in sr_persist.hip): seeded draws from known logits, draws along a real trajectory, exact arg-max ties, the
eight-period chunk graph and the shape just past the persistent kernel's batch limit.

The sharp construction: with the output layer's effective weight exactly zero (weight norm: g = 0), every step of every
stream has logits == b4 bit for bit on both device paths (0 . x + b is exact), so each pick is an independent check
against `oracle.samplernn_ref.draw_pick(b4, temperature, draw_u01(seed, t, b))`.

This module imports no GPU code.  tests/test_samplernn_sampling_cases_cpu.py checks its premises;
tests/test_gpu_samplernn_sampling.py runs the cases."""
import functools
from collections import namedtuple

import numpy as np
import torch

from oracle import samplernn_ref as S

Q, BFS = 256, 80

# A pick may differ from the float64 oracle only where u01 lies within DELTA of the CDF boundary between the two picks.
# Both kernels add the Q = 256 expf terms one after the other in float32: after q additions the running sum carries a
# relative error of at most about (q + 1) 2^-24 on top of the two roundings of each term's argument and expf's own
# error (~1 ulp each), so c_q and tot are each off by at most about (256 + 3) 2^-24 relative, and their ratio -- what
# `u01 tot < c_q` compares u01 with -- by twice that: 2 (256 + 3) 2^-24 = 3.1e-5 (the CDF is <= 1, so this is absolute as
# well).  DELTA is twice that figure, as the nearest power of two: 2^-14 = 6.1e-5.
DELTA = 2.0 ** -14
assert abs(DELTA / (2 * 2 * (256 + 3) * 2.0 ** -24) - 1) < 0.02
EXCUSED_CAP = 0.005        # excused mismatches per case, as a fraction of its draws (a condition, not a measurement)
CHI2_LEVEL = 1e-6

Shape = namedtuple("Shape", "DIM EMB B T persistent")
BIAS_SHAPES = {
    "launch-D32-B3": Shape(32, 8, 3, 3, False),
    "persist-D256-B5": Shape(256, 32, 5, 3, True),     # a partial team (streams 4 | 1)
    "persist-D256-B32": Shape(256, 32, 32, 3, True),   # every team
}
TEMPERATURES = (0.5, 1.0, 2.0)
SEEDS = (234, 2 ** 40 + 3)   # the second one guards the 64-bit field
PATTERNS = ("randn", "peaked", "flat")
PEAKED_CODES = (0, 130, 255)  # the first and the last bin of the CDF among them
PARAM_SEED, FEAT_SEED = 21, 22


def b4_pattern(name):
    """The output bias (= every logit vector of the run) of a pattern, float32 [Q]."""
    r = np.random.RandomState(dict(randn=101, peaked=102, flat=103)[name])
    if name == "randn":
        b = 2.0 * r.randn(Q)
    elif name == "peaked":  # three codes carry almost all the mass (over 99 % at temperature 2, all but 1e-14 at 0.5)
        b = -14.0 + 0.3 * r.randn(Q)
        b[list(PEAKED_CODES)] = (6.0, 5.5, 5.0)
    elif name == "flat":
        b = 0.01 * r.randn(Q)
    else:
        raise KeyError(name)
    return b.astype(np.float32)


@functools.lru_cache(maxsize=None)
def u01_table(seed, T, B):
    """draw_u01(seed, t, b) of every generated sample: float64 [B, 80 (T - 1)], column j <-> sample index t = 80 + j."""
    return np.array([[S.draw_u01(seed, t, b) for t in range(BFS, BFS * T)] for b in range(B)], dtype=np.float64)


def cdf64(logits, temperature):
    return S.draw_cdf(torch.as_tensor(np.asarray(logits)), temperature).numpy()


def oracle_picks(logits, temperature, u):
    """draw_pick for a whole array of uniforms against one logit vector (first q with u < c_q, else Q - 1)."""
    c = cdf64(logits, temperature)
    return np.minimum(np.searchsorted(c, u, side="right"), c.size - 1).astype(np.int32)


def emulate_picks_f32(logits, temperature, u):
    """The kernels' arithmetic restated in numpy float32, same order: subtract the max, divide, exp, sum one by one,
    `u01 tot < c`.  (numpy's exp is not bit-equal to the device's expf; both are within an ulp or two.)"""
    lg = np.asarray(logits, dtype=np.float32)
    e = np.exp((lg - lg.max()) / np.float32(temperature)).astype(np.float32)
    c = np.cumsum(e, dtype=np.float32)  # accumulate: strictly sequential, rounded to float32 at every step
    uu = np.asarray(u).astype(np.float32) * c[-1]
    assert uu.dtype == np.float32
    return np.minimum(np.searchsorted(c, uu, side="right"), c.size - 1).astype(np.int32)


def boundary_distance(c, u, got, want):
    """Largest distance of u to the CDF boundaries that separate the picks got and want (one boundary when they are
    neighbours; all of them have to be close when bins of next to no mass lie in between)."""
    lo, hi = min(int(got), int(want)), max(int(got), int(want))
    return float(np.abs(u - c[lo:hi]).max())


def judge_draws(picks, logits, temperature, u, delta=DELTA, cap=EXCUSED_CAP):
    """picks [B, n] against the float64 oracle.  Returns (draws, excused mismatches, their largest boundary distance);
    asserts that every mismatch is within delta of the boundary between the two picks and that their number keeps the
    cap."""
    picks = np.asarray(picks)
    assert picks.shape == u.shape, (picks.shape, u.shape)
    want = oracle_picks(logits, temperature, u)
    c = cdf64(logits, temperature)
    worst = 0.0
    bad = np.argwhere(picks != want)
    for b, j in bad:
        assert 0 <= picks[b, j] < c.size, f"stream {b}, sample {BFS + j}: pick {picks[b, j]} out of range"
        d = boundary_distance(c, u[b, j], picks[b, j], want[b, j])
        assert d <= delta, (f"stream {b}, sample {BFS + j}: pick {picks[b, j]}, oracle {want[b, j]}, u01 {u[b, j]!r} is "
                            f"{d:.3e} from the boundary (allowed {delta:.3e}); {len(bad)} of {picks.size} differ")
        worst = max(worst, d)
    assert len(bad) <= cap * picks.size, f"{len(bad)} excused mismatches in {picks.size} draws (cap {cap * picks.size:.1f})"
    return picks.size, len(bad), worst


def chi_square(picks, probs, min_expect=5.0):
    """Pearson's chi-square of a histogram of picks against probs.  A bin that expects fewer than min_expect draws is
    pooled with the codes that follow it until the pool expects that many (a short pool at the end joins the bin before
    it), so a near-flat distribution over few draws still leaves bins to compare.  Returns (statistic, dof, p-value)."""
    picks = np.asarray(picks).reshape(-1)
    n = picks.size
    obs = np.bincount(picks, minlength=probs.size).astype(np.float64)
    exp = probs.astype(np.float64) * n
    o, e, po, pe = [], [], 0.0, 0.0
    for q in range(probs.size):
        po, pe = po + obs[q], pe + exp[q]
        if pe >= min_expect:
            o.append(po); e.append(pe)
            po, pe = 0.0, 0.0
    if pe > 0 or po > 0:
        if e:
            o[-1] += po; e[-1] += pe
        else:
            o.append(po); e.append(pe)
    o, e = np.array(o), np.array(e)
    assert abs(o.sum() - n) < 1e-9 and abs(e.sum() - n) < 1e-6 * n
    stat, dof = float(((o - e) ** 2 / e).sum()), len(e) - 1
    if dof == 0:
        return stat, 0, 1.0
    pval = float(torch.special.gammaincc(torch.tensor(dof / 2.0, dtype=torch.float64),
                                         torch.tensor(stat / 2.0, dtype=torch.float64)))
    return stat, dof, pval


# ---- a uniform exactly on a boundary ------------------------------------------------------------------------------------
# `u01 < c_q` is strict.  With all logits equal every term is expf(0) = 1, the running sums are the integers 1..256, and
# u01 * 256 is exact on the device (a power-of-two scaling) and in the oracle (softmax = 1/256, sums of it exact), so the
# pick is floor(256 u01) in both, with no slack -- and where 256 u01 is an integer m the draw sits exactly on c_{m-1}: the
# strict comparison picks m, `<=` would pick m - 1.  That takes a u01 that is a multiple of 2^-8: about one draw in 65 000,
# so the seeds below were searched for (streams 6 and 4 of B = 8; the CPU test checks that they still deliver).
EDGE_SHAPES = {"launch-D32-B8": Shape(32, 8, 8, 3, False), "persist-D256-B8": Shape(256, 32, 8, 3, True)}
EDGE_SEEDS = (7, 39)
EDGE_LOGIT = 0.25


def edge_hits(seed, T, B):
    """[(stream, column, m)] of the draws with 256 u01 == m, 0 < m < 256."""
    u = u01_table(seed, T, B) * Q
    return [(int(b), int(j), int(u[b, j])) for b, j in np.argwhere((u == np.floor(u)) & (u > 0) & (u < Q))]


def bias_only_params(c, b4, seed=PARAM_SEED):
    """Ordinary perturbed parameters with the output layer reduced to its bias: g = 0 under weight norm (W = 0 would
    make the fold 0 / 0), W = 0 without."""
    p = S.init_params(c, seed=seed, perturb=0.25)
    if c['WEIGHT_NORM']:
        p['SampleLevel.Output.g0'] = torch.zeros_like(p['SampleLevel.Output.g0'])
    else:
        p['SampleLevel.Output.W0'] = torch.zeros_like(p['SampleLevel.Output.W0'])
    p['SampleLevel.Output.b'] = torch.from_numpy(np.asarray(b4, dtype=np.float32)).double()
    return p


def features(T, B, seed=FEAT_SEED):
    return torch.randn(T, B, 63, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


# ---- draws along a real trajectory --------------------------------------------------------------------------------------
Traj = namedtuple("Traj", "DIM EMB B T persistent param_seed feat_seed")
TRAJ_SHAPES = {
    "launch-D32-B3": Traj(32, 8, 3, 3, False, 31, 32),
    "persist-D256-B6": Traj(256, 32, 6, 3, True, 33, 34),
}
TRAJ_TEMPERATURE, TRAJ_SEED = 1.0, 234


def traj_slack_rows(B):
    return max(1, B // 4)


@functools.lru_cache(maxsize=None)
def traj_reference(name, dtype=torch.float64):
    """(params, features, oracle samples, oracle logits) of a trajectory case; dtype float32 casts the parameters (the
    oracle then runs in float32 throughout, its CDF stays float64)."""
    s = TRAJ_SHAPES[name]
    c = S.config(DIM=s.DIM, EMB_SIZE=s.EMB)
    p = S.init_params(c, seed=s.param_seed, perturb=0.25)
    feats = features(s.T, s.B, s.feat_seed)
    pp = {k: v.to(dtype) for k, v in p.items()}
    with torch.no_grad():
        ref, logits = S.generate(pp, c, feats.to(dtype), return_logits=True, temperature=TRAJ_TEMPERATURE, seed=TRAJ_SEED)
    return p, feats, ref.numpy(), logits.double()


def draws_follow_oracle(out, ref, ref_logits, temperature, seed, B):
    """Rows equal the oracle's trajectory; a row may leave it only at a step where u01 is within
    delta_traj = e / (2 temperature) + DELTA of a boundary of the oracle's CDF, e = 2e-5 max|logit| being what
    `_greedy_follows_oracle` takes for the logit error float32 leaves: a logit error of e moves a CDF value c by at most
    c (1 - c) (exp(2 e / T) - 1) <= e / (2 T).  Returns (identical rows, [(row, sample, pick, oracle, distance, allowed)])
    and asserts the rule and the row cap B - max(1, B // 4)."""
    exact, left = [], []
    for b in range(B):
        diff = np.nonzero(out[b] != ref[b])[0]
        if diff.size == 0:
            exact.append(b)
            continue
        t = int(diff[0])
        lg = ref_logits[b, t - BFS]
        allowed = 2e-5 * float(lg.abs().max()) / (2 * temperature) + DELTA
        assert 0 <= out[b, t] < Q, f"row {b}, sample {t}: pick {out[b, t]} out of range"
        d = boundary_distance(cdf64(lg, temperature), S.draw_u01(seed, t, b), out[b, t], ref[b, t])
        left.append((b, t, int(out[b, t]), int(ref[b, t]), d, allowed))
        assert d <= allowed, (f"row {b} leaves the oracle at sample {t} (pick {out[b, t]}, oracle {ref[b, t]}): u01 is "
                              f"{d:.3e} from the boundary, allowed {allowed:.3e}")
    assert len(exact) >= B - traj_slack_rows(B), f"only {len(exact)} of {B} rows follow the oracle"
    return exact, left


# ---- exact ties at temperature 0 ----------------------------------------------------------------------------------------
# In srp_argmax_row code q is looked at by lane q % 64 in pass q // 64 (first maximum per lane, then the lowest index
# among the lanes that hold the maximum); sr_pick_kernel gives thread q code q and reduces over an LDS tree.
TIE_SHAPES = {"launch-D32-B3": Shape(32, 8, 3, 2, False), "persist-D256-B5": Shape(256, 32, 5, 2, True)}
TIE_MAXIMA = {
    "all-equal": (tuple(range(Q)), 0),
    "one-lane-and-another": ((5, 69, 133, 200), 5),   # 5, 69, 133 share lane 5; 200 is lane 8
    "later-pass-of-lower-lane": ((64, 255), 64),      # lane 0 pass 1 against lane 63 pass 3
    "last-lane-first-pass": ((63, 128), 63),          # lane 63 pass 0 against lane 0 pass 2
    "last-code": ((255,), 255),
}
ONE_HOT_CODE, ONE_HOT_LIFT = 77, 60.0


def tie_pattern(name):
    """(b4 float32 [Q], expected pick): the named codes hold the maximum 3.0 exactly, every other logit is below 0."""
    codes, want = TIE_MAXIMA[name]
    b = (-1.0 - np.abs(np.random.RandomState(104).randn(Q))).astype(np.float32)
    b[list(codes)] = 3.0
    return b, want


def one_hot_pattern():
    """One code ONE_HOT_LIFT above the largest of the rest: at temperature 1 the others hold less than 255 e^-60 = 2e-24
    of the mass, below the smallest u01 (2^-25), so every draw with u01 < 1 picks it."""
    b = (0.5 * np.random.RandomState(105).randn(Q)).astype(np.float32)
    b[ONE_HOT_CODE] = np.float32(np.delete(b, ONE_HOT_CODE).max() + ONE_HOT_LIFT)
    return b


# ---- chunked graph replay, plan reuse, the batch limit ------------------------------------------------------------------
SR_CHUNK = 8   # SrPlan::SR_CHUNK: periods per replay of the chunk graph; a run has T - 1 periods
Replay = namedtuple("Replay", "DIM EMB B T persistent chunks singles")
REPLAY_SHAPES = {
    "launch-D32-B2-T9": Replay(32, 8, 2, 9, False, 1, 0),
    "launch-D32-B2-T11": Replay(32, 8, 2, 11, False, 1, 2),
    "persist-D256-B5-T10": Replay(256, 32, 5, 10, True, 1, 1),
}
REPLAY_PARAM_SEED, REPLAY_FEAT_SEED, REPLAY_FEAT_SEED_2 = 41, 42, 43
LIMIT_SHAPE = Shape(256, 32, 33, 2, False)   # one stream more than 8 teams of 4
PERSIST_MAX_B = 32


@functools.lru_cache(maxsize=None)
def greedy_reference(DIM, EMB, B, T, param_seed=REPLAY_PARAM_SEED, feat_seed=REPLAY_FEAT_SEED):
    """(params, features, float64 greedy samples, logits).  Generation is causal, so a run over the first T' frames of the
    features is the first 80 T' columns of this one."""
    c = S.config(DIM=DIM, EMB_SIZE=EMB)
    p = S.init_params(c, seed=param_seed, perturb=0.25)
    feats = features(T, B, feat_seed)
    with torch.no_grad():
        ref, logits = S.generate(p, c, feats, return_logits=True)
    return p, feats, ref.numpy(), logits

"""Cases and references of the per-step draw statistics of the SampleRNN generator (samplernn_generate_set_draw_stats;
DeviceGenerator(draw_stats=True), generate_packed(..., draw_stats=True)): kept = the size of the set a step's pick was drawn
from, draw_logp = the log of the written sample's probability under the step's own temperature and kept set,

    draw_logp = (lg_s - max) / T - log(sum over the kept codes of exp((lg_q - max) / T)),   -inf for s outside the set;

on an argmax step (T <= 0) kept = 1 and draw_logp = 0 for the argmax, -inf for any other (forced) code.

With bias-only logits (tests/samplernn_sampling_cases.py) the logits are exact on the device, so under the margins of
tests/samplernn_min_p_cases.py and tests/samplernn_top_p_cases.py the kept set is the oracle's at every step.  On a real
trajectory the samples are forced onto given codes (tests/samplernn_forced_cases.py), so every step compares with the float64
teacher-forced pass.

This module imports no GPU code."""
import functools

import numpy as np
import torch

from oracle import samplernn_ref as S
from tests import samplernn_forced_cases as FC
from tests import samplernn_min_p_cases as MC
from tests import samplernn_sampling_cases as SC
from tests import samplernn_top_k_cases as KC
from tests import samplernn_top_p_cases as NC

Q, BFS = SC.Q, SC.BFS
MODES = KC.MODES

# draw_logp against float64 on exact logits, absolute: the mass of at most 256 kept terms is off by at most (256 + 3) 2^-24
# relative (SC.DELTA's own derivation), its logarithm by that much absolutely; the numerator's argument x = (lg_s - max) / T
# is off by |x| 2^-23 (two roundings) -- at most 2^-17 for |x| <= MAX_ARG = 64, and no listed pattern at no listed temperature
# has a code farther down (test_samplernn_draw_stats_cpu.py).  The sum of the two is 2.3e-5; SC.DELTA = 2^-14 = 6.1e-5 is
# more than twice that.
TOL = SC.DELTA
MAX_ARG = 64.0
assert 2 * ((256 + 3) * 2.0 ** -24 + MAX_ARG * 2.0 ** -23) <= TOL

SHAPES = ("launch-D32-B3", "persist-D256-B5")       # of SC.BIAS_SHAPES: both paths, a partial team
# (top_k, top_p, min_p) beside MC.CASES: a top-k case, a top-p case of NC.CASES, one combined case, no truncation
OTHER_TRUNCATIONS = ((64, 0.0, 0.0), (0, 0.9, 0.0), (64, 0.9, 0.1), (0, 0.0, 0.0))
FORCED_TEMPERATURES = (0.5, 2.0)

OUTSIDE_K = 3              # `peaked`: codes 0, 130, 255 carry the mass; under top_k = 3 they are the kept set
OUTSIDE_CODE, INSIDE_CODE = 1, 0


def oracle_m(logits, temperature, k=0, p=0.0, min_p=0.0):
    """The size of the kept set; asserts the premises under which the device's set is the oracle's."""
    if temperature <= 0:
        return 1
    return MC.case_m(logits, temperature, min_p, k, p)


def draw_logp64(logits, temperature, samples, k=0, p=0.0, min_p=0.0):
    """float64 draw_logp of `samples` (any shape) drawn from one logit vector with the given settings."""
    lg = np.asarray(logits, dtype=np.float32).astype(np.float64)
    s = np.asarray(samples)
    if temperature <= 0:
        return np.where(s == int(np.argmax(lg)), 0.0, -np.inf)
    keep = KC.kept_set(logits, MC.kept_m(logits, temperature, k, p, min_p))
    x = (lg - lg.max()) / temperature
    lse = np.log(np.exp(x[keep]).sum())
    return np.where(keep[s], x[s] - lse, -np.inf)


def largest_kept_argument(logits, temperature, k=0, p=0.0, min_p=0.0):
    """max |(lg_q - max) / T| over the kept codes: what the numerator's rounding scales with."""
    lg = np.asarray(logits, dtype=np.float32).astype(np.float64)
    keep = KC.kept_set(logits, MC.kept_m(logits, temperature, k, p, min_p))
    return float(np.abs((lg[keep] - lg.max()) / temperature).max())


@functools.lru_cache(maxsize=None)
def forced_reference(temperature):
    """(params, features, codes, float64 log softmax(logits / T)[code] of samples 80 ..) of FC.reference('gru')'s full
    forcing: the teacher-forced pass of FC.log_probs with the logits divided by the temperature."""
    p, feats, forced, _ = FC.reference('gru')
    c = S.config(DIM=FC.DIM, EMB_SIZE=FC.EMB)
    pp = {k: v.double() for k, v in p.items()}
    bfs, fs, D = c['BIG_FRAME_SIZE'], c['FRAME_SIZE'], c['DIM']
    seq = torch.as_tensor(forced).long()
    B = seq.shape[0]
    f = torch.as_tensor(feats).double().transpose(0, 1)[:, 1:]
    big_h0 = torch.zeros(B, c['N_RNN'], c['H0_MULT'] * c['BIG_DIM'], dtype=torch.float64)
    h0 = torch.zeros(B, c['N_RNN'], c['H0_MULT'] * D, dtype=torch.float64)
    with torch.no_grad():
        big_out, _, _ = S.big_frame_level_rnn(pp, c, seq[:, :-bfs], big_h0, True, f)
        frame_out, _ = S.frame_level_rnn(pp, c, seq[:, bfs - fs:-fs], big_out, h0, True)
        prev = seq[:, bfs - fs:-1].unfold(1, fs, 1).reshape(-1, fs)
        logits = S.sample_level_predictor(pp, c, frame_out.reshape(-1, D), prev)
        target = seq[:, bfs:]
        lp = torch.log_softmax(logits / temperature, -1).gather(1, target.reshape(-1, 1))[:, 0]
    return p, feats, forced, lp.reshape(target.shape).numpy()


def forced_case(temperature, B):
    p, feats, forced, lp = forced_reference(temperature)
    return p, feats[:, :B], forced[:B], lp[:B]

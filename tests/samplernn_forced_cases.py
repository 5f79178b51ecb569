"""Cases and references of the forced-sample / log-probability tests of the SampleRNN generator
(samplernn_generate_set_forced, samplernn_generate_set_log_probs; DeviceGenerator(forcing=, log_probs=)).

Under forcing there is no trajectory to leave: every sample step sees the history the caller names, so the log-probability
of every step compares with the float64 oracle at a plain tolerance.  log_probs() below is that oracle: the teacher-forced
pass of oracle.samplernn_ref (its three tier functions, learned h0, reset at the first frame) -- what compute_cost
averages, per sample.  tests/test_samplernn_forced_cpu.py pins it to compute_cost; tests/test_gpu_samplernn_forced.py
leans on it.

This module imports no GPU code."""
import functools
import math

import numpy as np
import torch

from oracle import samplernn_ref as S
from tests import samplernn_sampling_cases as SC

DIM, EMB = 256, 32           # the smallest width the persistent kernel takes
BFS, Q = 80, 256
LOG2E = math.log2(math.e)
PARITY_TOL = 1e-4            # the bar the project holds the last-step logits to (tests/test_gpu_samplernn_groups.py)

PARAM_SEED, FEAT_SEED, CODE_SEED = 91, 92, 93
LSTM_PARAM_SEED = 94
REF_B, REF_T = 33, 3         # one reference serves every single-GRU case: streams never meet, generation is causal
LSTM_B = 5

# self-replay: forced prefixes of a run's own output -- mid-frame, at a frame edge, across a big-frame edge, everything
REPLAY_T = 3
REPLAY_NS = (1, 7, 10, 85, BFS * (REPLAY_T - 1))
REPLAY_SETTINGS = {
    "argmax": dict(temperature=0.0),
    "sequential": dict(temperature=1.0),
    "scan": dict(temperature=1.0, draw_mode='scan'),
    "scan-topk-topp": dict(temperature=1.0, draw_mode='scan', top_k=64, top_p=0.9),
    "utterance-draws": dict(utterance_draws=True),
}
UTT_SEEDS = (2 ** 40 + 11, 12, 13, 2 ** 63 + 14, 15)
UTT_TEMPS = (1.0, 0.0, 0.5, 2.0, 1.0)   # rows of one team mix argmax and draws


def log_probs(p, c, sequences, features):
    """log softmax(logits)[sample] of samples 80 .. of `sequences` [B, 80 T] (integers; slot 0 = the prefix) under teacher
    forcing, [B, 80 (T - 1)] in the parameters' dtype.  features [T, B, 63] time-major as the generator takes them: row f
    conditions slot f, row 0 is not used."""
    bfs, fs, D = c['BIG_FRAME_SIZE'], c['FRAME_SIZE'], c['DIM']
    seq = torch.as_tensor(np.asarray(sequences)).long()
    B = seq.shape[0]
    dt = p['FrameLevel.h0'].dtype
    feats = torch.as_tensor(features).to(dt).transpose(0, 1)[:, 1:]
    big_h0 = torch.zeros(B, c['N_RNN'], c['H0_MULT'] * c['BIG_DIM'], dtype=dt)
    h0 = torch.zeros(B, c['N_RNN'], c['H0_MULT'] * D, dtype=dt)
    with torch.no_grad():
        big_out, _, _ = S.big_frame_level_rnn(p, c, seq[:, :-bfs], big_h0, True, feats)
        frame_out, _ = S.frame_level_rnn(p, c, seq[:, bfs - fs:-fs], big_out, h0, True)
        prev = seq[:, bfs - fs:-1].unfold(1, fs, 1).reshape(-1, fs)
        logits = S.sample_level_predictor(p, c, frame_out.reshape(-1, D), prev)
        target = seq[:, bfs:]
        lp = torch.log_softmax(logits, -1).gather(1, target.reshape(-1, 1))[:, 0]
    return lp.reshape(target.shape)


def cost_bits(p, c, sequences, features):
    """oracle.samplernn_ref.compute_cost of the same sequences (learned h0, reset, every sample counted), in bits."""
    seq = torch.as_tensor(np.asarray(sequences)).long()
    B = seq.shape[0]
    dt = p['FrameLevel.h0'].dtype
    feats = torch.as_tensor(features).to(dt).transpose(0, 1)[:, 1:]
    big_h0 = torch.zeros(B, c['N_RNN'], c['H0_MULT'] * c['BIG_DIM'], dtype=dt)
    h0 = torch.zeros(B, c['N_RNN'], c['H0_MULT'] * c['DIM'], dtype=dt)
    with torch.no_grad():
        cost, _, _, _ = S.compute_cost(p, c, seq, feats, h0, big_h0, True, torch.ones(seq.shape, dtype=dt))
    return float(cost)


def mean_bits(lp):
    """Minus the mean log-probability in bits, with compute_cost's own denominator (it guards the count with + 1e-5)."""
    lp = np.asarray(lp, dtype=np.float64)
    return float(-lp.sum() / (lp.size + 1e-5) * LOG2E)


def codes(B, T, seed=CODE_SEED):
    """Uniformly random codes [B, 80 T] int32 behind the Q/2 prefix slot."""
    out = np.random.RandomState(seed).randint(0, Q, size=(B, BFS * T)).astype(np.int32)
    out[:, :BFS] = Q // 2
    return out


@functools.lru_cache(maxsize=None)
def reference(kind):
    """(params, features [T, B, 63] float32 numpy, codes [B, 80 T], float64 log-probabilities [B, 80 (T - 1)]) of full
    forcing; kind 'gru' (GRU, N_RNN 1, REF_B streams) or 'lstm' (LSTM, N_RNN 2, LSTM_B streams).  Computed once."""
    cfg, seed, B = (dict(), PARAM_SEED, REF_B) if kind == 'gru' else (dict(RNN_TYPE='LSTM', N_RNN=2), LSTM_PARAM_SEED, LSTM_B)
    c = S.config(DIM=DIM, EMB_SIZE=EMB, **cfg)
    p = S.init_params(c, seed=seed, perturb=0.25)
    feats = SC.features(REF_T, B, FEAT_SEED)
    forced = codes(B, REF_T)
    lp = log_probs({k: v.double() for k, v in p.items()}, c, forced, feats.double())
    return p, feats.numpy(), forced, lp.numpy()


def model_config(kind):
    return dict() if kind == 'gru' else dict(RNN_TYPE='LSTM', N_RNN=2)


def case(kind, B):
    """The first B streams of reference(kind)."""
    p, feats, forced, lp = reference(kind)
    return p, feats[:, :B], forced[:B], lp[:B]


def prefix_forced(free_samples, ns):
    """forced [B, 80 T]: the first ns[b] generated samples of row b are the free run's own, the rest -1."""
    forced = np.full(free_samples.shape, -1, dtype=np.int32)
    for b, n in enumerate(ns):
        forced[b, BFS:BFS + n] = free_samples[b, BFS:BFS + n]
    return forced


def replay_ns(B, shift=0):
    """A forced length per row, every one of REPLAY_NS in turn: the rows of one team differ."""
    return [REPLAY_NS[(b + shift) % len(REPLAY_NS)] for b in range(B)]

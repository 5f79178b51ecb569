"""Cases of the per-utterance draw tests (samplernn_generate_set_utterance_draws; three_tier.DeviceGenerator(utterance_draws=
True), generate_packed(seeds=), StreamingGenerator(utterance_draws=True)): the seeds and temperature sets, which utterance
draws with what, a host emulator of the plan's entry semantics, and the float64 oracle trajectories of the utterances.

The entry semantics (include/parrot_hip.h): every stream b of a plan holds {seed, off, temperature}; a run that does not
resume sets every entry from row 1 of the caller's arrays with off = 0; a start flagged at (f, b) sets entry b from row f
with off = origin + (f - 1) BFS; a resumed segment adds the samples the ring has turned past to origin and leaves the
entries alone; the draw of buffer index t in stream b is keyed by (seed_b, origin + t - off_b).

This module imports no GPU code.  tests/test_samplernn_utt_draws_cpu.py checks its premises;
tests/test_gpu_samplernn_utt_draws.py runs the cases."""
import functools

import numpy as np
import torch

from oracle import samplernn_ref as S
from tests import samplernn_groups_cases as GC
from tests import samplernn_packed_cases as PC

M64 = (1 << 64) - 1
K1, K2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9
BFS, Q, FEAT = 80, 256, 63

SEEDS = (234, 2 ** 40 + 3, 2 ** 63 + 5)    # the last one guards the signed image of the device array
# four consecutive utterances (= the four rows of one team of the persistent kernel, utterances being numbered stream by
# stream) draw at 0 (arg-max), 0.5, 1.0 and 2.0
TEAM_TEMPERATURES = (0.0, 0.5, 1.0, 2.0)
TEMPERATURE_SETS = {
    "mixed": TEAM_TEMPERATURES,
    "mixed-rotated": (1.0, 2.0, 0.0, 0.5),
}


def old_key_seed(s, b):
    """The per-utterance seed with which stream b of a plain plan draws what the plan seed s draws there by default."""
    return (s ^ (K2 * (b + 1))) & M64


def utt_seeds(n, salt=0):
    """One seed per utterance: the three base seeds in turn, moved apart by the utterance's index."""
    return [(SEEDS[i % len(SEEDS)] + 1000 * (i + salt)) & M64 for i in range(n)]


def utt_temperatures(n, name="mixed"):
    t = TEMPERATURE_SETS[name]
    return [t[i % len(t)] for i in range(n)]


# ---- host emulator of the entry semantics ---------------------------------------------------------------------------------
def fake_pick(u01_fn, seed, n, temperature, feat, prev):
    """A stand-in for the model: the sample at counter n of an utterance as a function of exactly what the real one may
    depend on -- the utterance's seed, counter and temperature (through its uniform), its conditioning frame and the
    sample before it.  temperature <= 0 draws nothing."""
    code = int(abs(float(feat)) * 1000.0) % Q
    if temperature <= 0:
        return (5 * int(prev) + code + 1) % Q
    return (int(u01_fn(seed, n) * 2 ** 24) + int(prev) + code + int(round(4 * temperature))) % Q


class PlanEmulator:
    """A plan with per-utterance draws, on the host: ring of T slots, the draw origin, one entry per stream, the three
    launches that touch them (run initialisation, start, resume) and fake_pick as the sample step."""

    def __init__(self, u01_fn, B, T):
        self.u01, self.B, self.T = u01_fn, B, T
        self.samples = np.zeros((B, BFS * T), dtype=np.int64)
        self.features = np.zeros((T, B, FEAT), dtype=np.float32)
        self.starts = np.zeros((T, B), dtype=np.int32)
        self.utt_seed = np.zeros((T, B), dtype=object)
        self.utt_temp = np.zeros((T, B), dtype=np.float32)
        self.origin, self.last, self.entries = 0, 0, [(0, 0, 0.0)] * B

    def run(self, n_periods, resume):
        assert 1 <= n_periods <= self.T - 1 and (self.last or not resume)
        if resume:
            self.samples[:, :BFS] = self.samples[:, BFS * self.last:BFS * (self.last + 1)]
            self.origin += self.last * BFS
        else:
            self.samples[:] = 0
            self.samples[:, :BFS] = Q // 2
            self.origin = 0
            self.entries = [(int(self.utt_seed[1, b]), 0, float(self.utt_temp[1, b])) for b in range(self.B)]
        for f in range(1, n_periods + 1):
            for b in range(self.B):
                if self.starts[f, b]:
                    self.samples[b, BFS * (f - 1):BFS * f] = Q // 2
                    self.entries[b] = (int(self.utt_seed[f, b]), self.origin + (f - 1) * BFS, float(self.utt_temp[f, b]))
                seed, off, temp = self.entries[b]
                for t in range(BFS * f, BFS * (f + 1)):
                    self.samples[b, t] = fake_pick(self.u01, seed, self.origin + t - off, temp, self.features[f, b, 0],
                                                   self.samples[b, t - 1])
        self.last = n_periods
        return self.samples[:, BFS:BFS * (n_periods + 1)].copy()

    def run_segment(self, features, starts, resume, seeds=None, temperatures=None):
        """The runner a StreamingGenerator(run_segment=...) calls: rows 1 .. n of the ring."""
        n = features.shape[0]
        self.features[1:n + 1], self.starts[1:n + 1] = features, starts
        self.utt_seed[1:n + 1] = np.asarray(seeds, dtype=object)
        self.utt_temp[1:n + 1] = temperatures
        return self.run(n, resume)


def emulate_standalone(u01_fn, features, seed, temperature, B=1, stream=0):
    """The utterance on its own in `stream` of a plain plan of B streams: [80 n], the prefix included."""
    n = features.shape[0]
    if n == 1:
        return np.full(BFS, Q // 2, dtype=np.int64)
    e = PlanEmulator(u01_fn, B, n)
    e.features[:, stream] = features
    e.utt_seed[1, stream], e.utt_temp[1, stream] = seed, temperature
    return np.concatenate([np.full(BFS, Q // 2, dtype=np.int64), e.run(n - 1, False)[stream]])


# ---- admission schedules ----------------------------------------------------------------------------------------------------
# (lengths of the utterances, in ticket order) x segment_frames; five streams.  With segment_frames = 5 a stream's second
# utterance behind one of four frames has its prefix in a segment's last slot and its start flag on slot 1 of the next
# (tests/test_samplernn_utt_draws_cpu.py::test_a_prefix_in_a_segments_last_slot checks that there is one).
STREAM_B = 5
STREAM_LENGTHS = PC.GRU_PACKING.lengths
STREAM_SEGMENTS = (1, 2, 5)
# a second session: the same utterances (and seeds) submitted in another order -- ORDER_2[k] = the utterance submitted k-th
STREAM_ORDER_2 = (1, 0, 3, 2, 4, 6, 5, 8, 7, 10, 9)


def drain(sg, utts, seeds, temps, order=None):
    """Submits the utterances (in `order`), drains, and returns ({utterance: concatenated chunks}, {utterance: stream},
    {utterance: absolute slot of its prefix})."""
    order = list(range(len(utts))) if order is None else list(order)
    ticket_of = {}
    for i in order:
        ticket_of[sg.submit(utts[i], seed=seeds[i], temperature=temps[i])] = i
    chunks = {i: [] for i in order}
    for ticket, chunk, _ in sg.drain():
        chunks[ticket_of[ticket]].append(chunk)
    out = {i: np.concatenate(c) for i, c in chunks.items()}
    stream = {ticket_of[t]: sg.record[t][0] for t in ticket_of}
    slot = {ticket_of[t]: sg.record[t][1] for t in ticket_of}
    return out, stream, slot


# ---- the oracle's trajectories of the packed utterances ---------------------------------------------------------------------
# Utterance i of PC.GRU_PACKING = column i of GC.gru_reference()'s features cut to lengths[i] frames, with seed
# ORACLE_SEEDS[i] and temperature ORACLE_TEMPERATURES[i].  oracle/samplernn_ref.draw_u01(s ^ K2, n, 0) is the uniform of an
# utterance with seed s at counter n, so S.generate(..., B = 1, temperature, seed = s ^ K2) is its reference trajectory;
# temperature 0 is the greedy run GC.gru_reference() already holds.
ORACLE_CASE = PC.GRU_PACKING
ORACLE_SEEDS = utt_seeds(len(ORACLE_CASE.lengths))
ORACLE_TEMPERATURES = utt_temperatures(len(ORACLE_CASE.lengths))


@functools.lru_cache(maxsize=None)
def oracle_piece(i, dtype=torch.float64):
    """(samples [80 n], logits [80 (n - 1), Q] float64, oracle seed) of utterance i; dtype float32 casts parameters and
    features (the oracle then runs in float32 throughout)."""
    n, temp = ORACLE_CASE.lengths[i], ORACLE_TEMPERATURES[i]
    p, feats, ref, ref_logits = GC.gru_reference()
    oseed = ORACLE_SEEDS[i] ^ K2
    if temp <= 0 and dtype == torch.float64:
        return ref[i, :BFS * n], ref_logits[i, :BFS * (n - 1)], oseed
    c = S.config(DIM=GC.DIM, EMB_SIZE=GC.EMB)
    pp = {k: v.to(dtype) for k, v in p.items()}
    with torch.no_grad():
        out, logits = S.generate(pp, c, feats[:n, i:i + 1].to(dtype), return_logits=True, temperature=temp, seed=oseed)
    return out.numpy()[0], logits.double()[0], oseed

"""Packings of the packed-generation tests (three_tier.generate_packed, SampleRnnGenDesc::starts): which utterance runs
in which stream from which slot.  Utterance i is column i of the features of tests/samplernn_groups_cases.py
(gru_reference / stacked_reference) cut to lengths[i] frames; its oracle result is ref[i, :80 lengths[i]] -- generation is
causal and the streams never meet.

This module imports no GPU code.  tests/test_samplernn_packed_cpu.py checks the packings' premises;
tests/test_gpu_samplernn_packed.py runs them."""
from collections import namedtuple

Packing = namedtuple("Packing", "lengths stream first_slot T B min_len max_len")


def _from_chains(chains, B, min_len, max_len):
    """chains[b] = the lengths of stream b's utterances in order; utterances are numbered rank by rank (every stream's
    first one in stream order, then the second ones, ...)."""
    lengths, stream, first = [], [], []
    k = 0
    while any(len(c) > k for c in chains.values()):
        for b in sorted(chains):
            if len(chains[b]) > k:
                lengths.append(chains[b][k])
                stream.append(b)
                first.append(sum(chains[b][:k]))
        k += 1
    T = max(2, max(sum(c) for c in chains.values()))
    return Packing(tuple(lengths), tuple(stream), tuple(first), T, B, min_len, max_len)


# 11 utterances of 2..5 frames on 5 streams (one team of the persistent kernel and one stream of the next), T = 10: nine
# periods = one replay of the eight-period chunk graph and one single period.  Streams 0 and 1 begin their second
# utterance at frame 6 while stream 2 is in the middle of one; stream 2 begins its third at frame 9, the single period.
GRU_PACKING = _from_chains({0: [5, 5], 1: [5, 5], 2: [3, 5, 2], 3: [5, 4], 4: [4, 5]}, 5, 2, 5)

# 37 streams = two row groups (PARROT_SR_PERSIST_GROUPS = 2): group 1 holds streams 32 .. 36, stream 36 alone in a
# partial team.  Every stream runs one utterance of 2..4 frames; some go on with a second and a third.
_GROUP_CHAINS = {b: [2 + b % 3] for b in range(37)}
for _b, _more in {0: [3], 1: [3], 5: [4], 30: [2], 31: [5], 32: [4], 33: [3, 3], 35: [4, 2], 36: [4, 3]}.items():
    _GROUP_CHAINS[_b] = _GROUP_CHAINS[_b] + _more
GROUPS_PACKING = _from_chains(_GROUP_CHAINS, 37, 2, 5)

# stacked tiers: the reference has three frames, so utterances of 2..3 frames; 16 of them on 5 streams, T = 10
STACKED_PACKING = _from_chains({0: [3, 2, 3], 1: [2, 3, 3], 2: [3, 3], 3: [2, 2, 2, 2, 2], 4: [3, 3, 2]}, 5, 2, 3)


def rectangles(case):
    """[{stream: utterance}] -- rectangle k holds every stream's k-th utterance, each in the stream that carries it in the
    packed run: a plain plan of the same batch then runs the same kernels on the same tiles for it."""
    rank = {}
    out = []
    for i in sorted(range(len(case.lengths)), key=lambda i: (case.stream[i], case.first_slot[i])):
        k = rank.get(case.stream[i], 0)
        rank[case.stream[i]] = k + 1
        while len(out) <= k:
            out.append({})
        out[k][case.stream[i]] = i
    return out


def slack_utterances(n):
    """Utterances that may leave the float64 oracle at a near-tie on the GPU: one per started 16."""
    return (n + 15) // 16

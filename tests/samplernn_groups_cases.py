"""Cases and references of the row-group tests of the SampleRNN persistent sample kernel (`srp_kernel<D, true>`,
sr_persist.hip; switch PARROT_SR_PERSIST_GROUPS): batches above 32 streams in one launch, as ceil(B / 32) groups of 32.

The streams of a batch never meet (every product of the model is row-wise), and generation is causal, so ONE float64
oracle run at the largest batch and the longest utterance serves every single-GRU case: a case takes the first B
columns of the features, the first B rows and the first 80 T samples of the reference.

This module imports no GPU code.  tests/test_samplernn_groups_cpu.py checks its premises (the seeds below were searched
for there); tests/test_gpu_samplernn_groups.py runs the cases."""
import functools
from collections import namedtuple

import torch

from oracle import samplernn_ref as S
from tests import samplernn_sampling_cases as SC

DIM, EMB = 256, 32
ROWS_PER_GROUP = 32   # SRP_ROWS * SRP_NTEAMS: 8 teams (XCDs) of 4 streams
MAX_GROUPS = 8        # SRP_MAXGROUPS

Case = namedtuple("Case", "B T groups switch")
# B = 33: one live stream in group 1; 37: a partial team there (streams 36 | 3 dead lanes) and six teams without a live
# stream; 64: two full groups; 65: three groups.  `switch` is what PARROT_SR_PERSIST_GROUPS is set to.
GREEDY_CASES = {
    "B33": Case(33, 3, 2, 2),
    "B37": Case(37, 3, 2, 2),
    "B64": Case(64, 3, 2, 2),
    "B65": Case(65, 3, 3, 3),
}
CHUNK_CASE = Case(37, 10, 2, 2)    # nine periods: one replay of the eight-period chunk graph plus one single period
STACKED_CASE = Case(37, 3, 2, 2)   # RNN_TYPE = 'LSTM', N_RNN = 2: the general next_in tail, no composed frame input
REF_B = max(c.B for c in GREEDY_CASES.values())
REF_T = CHUNK_CASE.T

# Seeds (parameters, features) searched for by tests/test_samplernn_groups_cpu.py::test_seeds_condition_the_gpu_cases:
# the oracle's float32 run follows its float64 greedy run on all but at most one stream in 16 of every case.
GRU_SEEDS = (51, 52)
FEAT_SEED_2 = 53                   # the second utterance of the replay test
STACKED_SEEDS = (71, 72)
DRAW_SEEDS = (77, 78)
DRAW_PARAM_SEED, DRAW_FEAT_SEED = 56, 57


def slack_rows(B):
    """Streams that may leave the float64 oracle at a near-tie on the GPU: one per started 16."""
    return (B + 15) // 16


def f32_slack_rows(B):
    """What the float32 oracle may use of it on the CPU: at most one stream in 16."""
    return B // 16


def groups_for(B, max_groups):
    """The arithmetic of samplernn_persist_groups_dry, restated."""
    mg = min(max(max_groups, 1), MAX_GROUPS)
    return -(-B // ROWS_PER_GROUP) if 1 <= B <= ROWS_PER_GROUP * mg else 0


@functools.lru_cache(maxsize=None)
def gru_reference(dtype=torch.float64, seeds=GRU_SEEDS):
    """(params, features [REF_T, REF_B, 63], greedy samples [REF_B, 80 REF_T], logits) of the single-GRU model; dtype
    float32 casts parameters and features (the oracle then runs in float32 throughout)."""
    c = S.config(DIM=DIM, EMB_SIZE=EMB)
    p = S.init_params(c, seed=seeds[0], perturb=0.25)
    feats = SC.features(REF_T, REF_B, seeds[1])
    pp = {k: v.to(dtype) for k, v in p.items()}
    with torch.no_grad():
        ref, logits = S.generate(pp, c, feats.to(dtype), return_logits=True)
    return p, feats, ref.numpy(), logits.double()


def gru_case(case, dtype=torch.float64, seeds=GRU_SEEDS):
    """The slice of gru_reference a case compares with: (params, features [T, B, 63], samples [B, 80 T], logits)."""
    p, feats, ref, logits = gru_reference(dtype, seeds)
    return p, feats[:case.T, :case.B], ref[:case.B, :80 * case.T], logits[:case.B, :80 * (case.T - 1)]


@functools.lru_cache(maxsize=None)
def stacked_reference(dtype=torch.float64, seeds=STACKED_SEEDS):
    s = STACKED_CASE
    c = S.config(DIM=DIM, EMB_SIZE=EMB, RNN_TYPE='LSTM', N_RNN=2)
    p = S.init_params(c, seed=seeds[0], perturb=0.25)
    feats = SC.features(s.T, s.B, seeds[1])
    pp = {k: v.to(dtype) for k, v in p.items()}
    with torch.no_grad():
        ref, logits = S.generate(pp, c, feats.to(dtype), return_logits=True)
    return p, feats, ref.numpy(), logits.double()

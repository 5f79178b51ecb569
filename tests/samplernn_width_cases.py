"""Cases and references of the width tests of the SampleRNN persistent sample kernel: sr_persist.hip compiles its two
bodies -- `srp_kernel` (plain) and `srp_fx_kernel` (forced samples, log-probabilities, draw statistics: fx) -- at three
widths (D = 256, 512, 1024), each with and without the row-group loop (MG): twelve instantiations.  The other case
modules pin DIM, EMB = 256, 32, where DC / QC = 1, KQ = 1, T2V = 1 and every gather lane sits in the last wave: every
width-dependent loop of the body runs once or takes its smallest form.  The cases here are the smallest shapes at which
each of them has its second trip or its partial form, at 512 and at 1024 (the shipped width), in both bodies, with and
without the group loop -- and, at D = 256, the two frame sizes that leave the batched gather's common form: FS = 16
(FS - 1 > SRP_GMAX = 12: the loop gather, no carry) and FS = 2 (a single early row; the clamp FS - 2 = 0).

The streams of a batch never meet and generation is causal (tests/samplernn_groups_cases.py), so ONE reference per width
at B = 37, T = 3 serves every case of the width by slicing.

This module imports no GPU code.  tests/test_samplernn_width_cases_cpu.py checks its premises (the greedy seeds below were
searched for there); tests/test_gpu_samplernn_widths.py runs the cases."""
import functools
from collections import namedtuple

import torch

from oracle import samplernn_ref as S
from tests import samplernn_forced_cases as FC
from tests import samplernn_groups_cases as GC
from tests import samplernn_sampling_cases as SC
from tests.util import rel_err

WIDTHS = {256: 32, 512: 64, 1024: 256}   # DIM -> EMB_SIZE; 1024 / 256 is the shipped pair
BFS = 80                                 # BIG_FRAME_SIZE
REF_B, REF_T = 37, 3
MAX_GROUPS = 2                           # what PARROT_SR_PERSIST_GROUPS is set to for a case of two groups

# forced reference: (parameters, features, codes) -- the seeds of tests/samplernn_forced_cases.py, at every width and frame size
FORCED_SEEDS = (FC.PARAM_SEED, FC.FEAT_SEED, FC.CODE_SEED)
# greedy reference: (parameters, features) per width, the first pairs tried that pass
# tests/test_samplernn_width_cases_cpu.py::test_greedy_seeds_condition_the_gpu_cases
GREEDY_SEEDS = {512: (51, 52), 1024: (51, 52)}
FEAT_SEED_2 = 53                         # the second utterance of the replay test
DRAW_SEED = 78                           # the seeded trajectory on which the two bodies must agree

Case = namedtuple("Case", "DIM FS B groups body")
# B = 5: one group, a partial team (streams 4 | 1); 32: every team, one group; 33: two groups, one live stream in group 1;
# 37: two groups, a partial team in group 1 (stream 36 | 3 dead lanes) and six teams without a live stream
BATCHES = (5, 32, 33, 37)
FS_BATCHES = (5, 33)
FRAME_SIZES = (2, 16)
CASES = tuple(Case(D, 10, B, GC.groups_for(B, MAX_GROUPS), body)
              for D in (512, 1024) for B in BATCHES for body in ("plain", "fx"))
CASES += tuple(Case(256, FS, B, GC.groups_for(B, MAX_GROUPS), "fx") for FS in FRAME_SIZES for B in FS_BATCHES)

# The D = 256, FS = 10 instantiations are the ones every other SampleRNN case module runs; they are credited here by name
# (module, what it pins) so that the coverage table is the whole table.
CREDITED = {
    ("plain", 256, False): ("tests/samplernn_sampling_cases.py", "BIAS_SHAPES persist-D256-B5, persist-D256-B32"),
    ("plain", 256, True): ("tests/samplernn_groups_cases.py", "GREEDY_CASES B33 .. B65"),
    ("fx", 256, False): ("tests/samplernn_forced_cases.py", "reference('gru') at B = 5, 32"),
    ("fx", 256, True): ("tests/samplernn_forced_cases.py", "reference('gru') at B = 33 (test_row_groups)"),
}


def instantiation(case):
    """(body, D, MG) of the kernel a case must land on: srp_launch_width takes the fx body whenever forced codes,
    log-probabilities or draw statistics are asked for, and the group loop whenever the batch takes more than one group."""
    return (case.body, case.DIM, case.groups > 1)


def case_id(case):
    return f"D{case.DIM}-FS{case.FS}-B{case.B}-g{case.groups}-{case.body}"


def eligible(DIM, FS):
    """srp_eligible's conditions on the model, restated (2 FS <= SRP_MAXHIST = 64), and the generator's own: the frame
    size divides the big frame."""
    return DIM in WIDTHS and FS >= 1 and 2 * FS <= 64 and BFS % FS == 0


def cases(body=None, FS=None, widths=None):
    return [c for c in CASES if (body is None or c.body == body) and (FS is None or (c.FS in FS))
            and (widths is None or c.DIM in widths)]


def shapes(widths=(512, 1024)):
    """(DIM, B, groups) of the case table at FS = 10, once each."""
    return sorted({(c.DIM, c.B, c.groups) for c in CASES if c.FS == 10 and c.DIM in widths})


@functools.lru_cache(maxsize=None)
def forced_reference(DIM, FRAME_SIZE=10):
    """(params, features [T, B, 63] float32 numpy, codes [B, 80 T], float64 log-probabilities [B, 80 (T - 1)], the float32
    oracle's log-probabilities) of full forcing at REF_B streams; the float32 pass is the same pass with parameters and
    features cast (the f32 oracle's own error: what any float32 evaluation of these inputs may be expected to leave)."""
    c = S.config(DIM=DIM, EMB_SIZE=WIDTHS[DIM], FRAME_SIZE=FRAME_SIZE)
    p = S.init_params(c, seed=FORCED_SEEDS[0], perturb=0.25)
    feats = SC.features(REF_T, REF_B, FORCED_SEEDS[1])
    forced = FC.codes(REF_B, REF_T, seed=FORCED_SEEDS[2])
    lp = FC.log_probs({k: v.double() for k, v in p.items()}, c, forced, feats.double())
    lp32 = FC.log_probs({k: v.float() for k, v in p.items()}, c, forced, feats.float())
    return p, feats.numpy(), forced, lp.numpy(), lp32.numpy()


def forced_case(case):
    """The first B streams of the case's forced reference, as FC.case returns them: (params, features, codes, float64
    log-probabilities)."""
    p, feats, forced, lp, _ = forced_reference(case.DIM, case.FS)
    return p, feats[:, :case.B], forced[:case.B], lp[:case.B]


def f32_oracle_error(case):
    """Norm-wise error of the float32 oracle's log-probabilities against the float64 ones on the case's streams."""
    _, _, _, lp, lp32 = forced_reference(case.DIM, case.FS)
    return rel_err(lp32[:case.B], lp[:case.B])


@functools.lru_cache(maxsize=None)
def greedy_reference(DIM, dtype=torch.float64, seeds=None):
    """(params, features [REF_T, REF_B, 63], greedy samples [REF_B, 80 REF_T], logits) of the single-GRU model at FS = 10;
    dtype float32 casts parameters and features (the oracle then runs in float32 throughout)."""
    seeds = seeds or GREEDY_SEEDS[DIM]
    c = S.config(DIM=DIM, EMB_SIZE=WIDTHS[DIM])
    p = S.init_params(c, seed=seeds[0], perturb=0.25)
    feats = SC.features(REF_T, REF_B, seeds[1])
    pp = {k: v.to(dtype) for k, v in p.items()}
    with torch.no_grad():
        ref, logits = S.generate(pp, c, feats.to(dtype), return_logits=True)
    return p, feats, ref.numpy(), logits.double()


def greedy_case(case, dtype=torch.float64, seeds=None):
    """The slice of greedy_reference a case compares with: (params, features [T, B, 63], samples [B, 80 T], logits)."""
    p, feats, ref, logits = greedy_reference(case.DIM, dtype, seeds)
    return p, feats[:, :case.B], ref[:case.B], logits[:case.B]


# ---- draws on exact logits (tests/samplernn_sampling_cases.py's bias-only construction) inside the new instantiations ----
DrawShape = namedtuple("DrawShape", "DIM B groups")
DRAW_SHAPES = (DrawShape(512, 5, 1), DrawShape(1024, 37, 2))
DRAW_PATTERNS = ("randn", "peaked")
DRAW_TEMPERATURE = 1.0
DRAW_TRUNCATION = (64, 0.9, 0.1)         # (top_k, top_p, min_p): the combined row of samplernn_draw_stats_cases.OTHER_TRUNCATIONS

"""Cases of the decode with per-utterance controls (timing_coeffs / sharpening_coeffs / sampling_biases / speaker_weights of
Parrot.sample_model*), shared by tests/test_decode_row_controls_cpu.py (the premise) and
tests/test_gpu_decode_row_controls.py (the parity runs).  Built as tests/decode_gmm_cases.py builds its cases: SMALL, U = 9,
S = 10, init_params(seed=7, scale_by_fan_in=True), GRU2_GAIN on two-layer GRU stacks, make_batch(cfg, 2, N, U, seed=9),
randomness(N, O, seed).

The oracle needs no change for them: oracle/parrot_ref.sample_model uses cfg['timing_coeff'], cfg['sharpening_coeff'] and
cfg['sampling_bias'] in broadcasting expressions on [N, A], [N, O K] and [N, K] tensors, so a column tensor [N, 1] in each
entry IS the per-row decode (row i of such a run equals row i of a scalar run with row i's values exactly; the CPU test
asserts it).  The controls are the cycles below cut to N; N = 5 is one partial row block, N = 17 two row blocks.

A GMM case carries the seed of its randomness, chosen as in decode_gmm_cases.py: on the oracle's own run every cumulative
mixture weight stays PICK_MARGIN away from its uniform number, and the oracle's float32 run stays within F32_MARGIN of its
float64 run (searched with F32_SEARCH on one thread: search_seed).  Both are conditions on the inputs; the CPU test asserts
them for every case.  MSE cases draw nothing and need no seed.  The oracle of a case is computed once per process and never
modified."""
import functools

import torch

from tests import decode_gmm_cases as G
from tests.util import make_batch

SMALL, NAMES, U, S = G.SMALL, G.NAMES, G.U, G.S
PICK_MARGIN, F32_MARGIN, F32_SEARCH = G.PICK_MARGIN, G.F32_MARGIN, G.F32_SEARCH

TIMING = [1.0, 0.8, 1.25, 2.0, 0.5]
SHARPENING = [1.0, 1.5, 0.7, 1.0, 2.0]
BIAS = [0.0, 0.5, 1.0, 0.25, 2.0]
# the second set of the replay test: the same cycles, each shifted by another amount
TIMING_B, SHARPENING_B, BIAS_B = TIMING[2:] + TIMING[:2], SHARPENING[3:] + SHARPENING[:3], BIAS[1:] + BIAS[:1]


def cycle(vals, N):
    return (list(vals) * ((N + len(vals) - 1) // len(vals)))[:N]


def controls(N, gmm, which='A'):
    t, s, b = (TIMING, SHARPENING, BIAS) if which == 'A' else (TIMING_B, SHARPENING_B, BIAS_B)
    return dict(timing=cycle(t, N), sharpening=cycle(s, N), bias=cycle(b, N) if gmm else None)


def _stack(cell, L, cost, **kw):
    return dict(SMALL, cell_type=cell, num_layers=L, which_cost=cost, **({'weak_feedback': True} if L > 1 else {}), **kw)


# name -> (model keywords, N).  MSE heads decode on the machine by default, GMM heads (K = 3) with PARROT_PM_GMM=1.
CASES = {}
for _cell, _L in (('gru', 1), ('gru', 2), ('gru', 3), ('lstm', 1), ('lstm', 2)):
    CASES[f'{_cell}{_L}_mse_n5'] = (_stack(_cell, _L, 'MSE'), 5)
for _cell, _L in (('gru', 2), ('lstm', 2)):
    CASES[f'{_cell}{_L}_mse_n17'] = (_stack(_cell, _L, 'MSE'), 17)
CASES['lstm2_k3_n5'] = (_stack('lstm', 2, 'GMM', k_gmm=3), 5)
CASES['gru1_k3_n5'] = (_stack('gru', 1, 'GMM', k_gmm=3), 5)
CASES['lstm2_k3_n17'] = (_stack('lstm', 2, 'GMM', k_gmm=3), 17)
CASES['layer_norm'] = (_stack('gru', 2, 'MSE', layer_norm=True), 5)
CASES['speaker'] = (_stack('lstm', 2, 'MSE', use_speaker=True), 5)
# the first seed from 0 up whose oracle run, with the controls above, keeps PICK_MARGIN and F32_SEARCH (search_seed)
SEEDS = {'lstm2_k3_n5': 6, 'gru1_k3_n5': 0, 'lstm2_k3_n17': 290}
GMM = tuple(n for n, (full, _) in CASES.items() if full['which_cost'] == 'GMM')
MSE_MACHINE = tuple(n for n, (full, _) in CASES.items() if full['which_cost'] == 'MSE' and n not in ('layer_norm', 'speaker'))

# The blend of the speaker test: a one-hot row, a 50 / 50 row, a row that does not sum to 1, and two more (num_speakers = 5).
SPEAKER_WEIGHTS = [[0., 0., 1., 0., 0.],
                   [.5, 0., 0., .5, 0.],
                   [.3, .3, 0., 0., .1],
                   [0., 1., 0., 0., 0.],
                   [.25, .25, .25, .25, 0.]]


def is_gmm(name):
    return CASES[name][0]['which_cost'] == 'GMM'


def oracle_cfg(full, ctl, dtype=torch.float64):
    """The oracle's configuration of a model with the controls as column tensors [N, 1] (None: the model's scalars)."""
    from oracle import parrot_ref as R
    cfg = R.default_config(**full)
    if ctl is not None:
        col = lambda v: torch.tensor(v, dtype=dtype).unsqueeze(1)
        cfg['timing_coeff'], cfg['sharpening_coeff'] = col(ctl['timing']), col(ctl['sharpening'])
        if ctl.get('bias') is not None:
            cfg['sampling_bias'] = col(ctl['bias'])
    return cfg


def params(full):
    from oracle import parrot_ref as R
    p = R.init_params(R.default_config(**full), seed=7, scale_by_fan_in=True)
    if G.gain_of(full) != 1.0:
        p = {k: (v * G.gain_of(full) if k.endswith('.W') else v) for k, v in p.items()}
    return p


def build(name, seed, which='A'):
    """Parameters, batch, randomness, controls and the oracle's six outputs of a case with the given seed."""
    from oracle import parrot_ref as R
    full, N = CASES[name]
    gmm = full['which_cost'] == 'GMM'
    ctl = controls(N, gmm, which)
    cfg = oracle_cfg(full, ctl)
    p = params(full)
    _, _, lab, lm, spk = make_batch(cfg, 2, N, U, seed=9, speaker=cfg['use_speaker'])
    unif, noise = G.randomness(N, cfg['output_dim'], seed)
    with torch.no_grad():
        ref = R.sample_model(p, cfg, lab, lm, spk, S, unif=unif, noise=noise)
    return dict(name=name, full=full, cfg=cfg, p=p, lab=lab, lm=lm, spk=spk, N=N, U=U, S=S, unif=unif, noise=noise, ref=ref,
                ctl=ctl, gmm=gmm)


@functools.lru_cache(maxsize=None)
def case(name, which='A'):
    return build(name, SEEDS.get(name, 0), which)


def plain_ref(c):
    """The oracle's run of the case's model WITHOUT controls (the model's scalars): what a kernel that ignores the arrays
    would match."""
    from oracle import parrot_ref as R
    with torch.no_grad():
        return R.sample_model(c['p'], R.default_config(**c['full']), c['lab'], c['lm'], c['spk'], c['S'], unif=c['unif'],
                              noise=c['noise'])


def row_ref(c, i):
    """The oracle's run with row i's values as the model's scalars, for every row."""
    from oracle import parrot_ref as R
    full = dict(c['full'], timing_coeff=c['ctl']['timing'][i], sharpening_coeff=c['ctl']['sharpening'][i])
    if c['gmm']:
        full['sampling_bias'] = c['ctl']['bias'][i]
    with torch.no_grad():
        return R.sample_model(c['p'], R.default_config(**full), c['lab'], c['lm'], c['spk'], c['S'], unif=c['unif'], noise=c['noise'])


def pick_margin(c):
    return G.pick_margin(c)


def f32_error(c):
    """Worst relative error over the six outputs of the oracle run in float32 (controls included) against its float64 run."""
    from oracle import parrot_ref as R
    from tests.util import rel_err
    p32 = {k: v.float() for k, v in c['p'].items()}
    cfg32 = oracle_cfg(c['full'], c['ctl'], torch.float32)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)  # (one summation order per host; the seeds keep a factor of two to the bound for other hosts)
    try:
        with torch.no_grad():
            r32 = R.sample_model(p32, cfg32, c['lab'], c['lm'].float(), c['spk'], c['S'], unif=c['unif'], noise=c['noise'])
    finally:
        torch.set_num_threads(threads)
    return max(rel_err(a, b) for a, b in zip(r32, c['ref']))


def search_seed(name, start=0, stop=5000):
    """How SEEDS was made: the first seed whose oracle run keeps PICK_MARGIN and F32_SEARCH."""
    for seed in range(start, stop):
        c = build(name, seed)
        if pick_margin(c) >= PICK_MARGIN and f32_error(c) <= F32_SEARCH:
            return seed
    return None

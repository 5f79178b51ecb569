"""Cases of the decode with forced frames (forced_frames / n_forced of Parrot.sample_model*), shared by
tests/test_decode_forced_cpu.py (the premise) and tests/test_gpu_decode_forced.py (the parity runs).  Built as
tests/decode_row_controls_cases.py builds its cases: SMALL, U = 9, S = 10, init_params(seed=7, scale_by_fan_in=True),
GRU2_GAIN on two-layer GRU stacks, make_batch(cfg, 2, N, U, seed=9), randomness(N, O, seed).

The oracle of a forced run is forced_loop below: oracle/parrot_ref.sample_model has no hook for the fed-back frame, so the
loop is written again here from the oracle's own pieces (decoder_step, fork, linear, apply_norm, sample_gmm, initial_carry,
encoder_apply), line for line, with one line more: after step t the frame fed back is forced[t, b] where t < n[b].  With
all n = 0 it IS sample_model, bit for bit (the CPU test asserts it).  It returns seven outputs: the six of sample_model --
sample_x holding the fed-back frames -- and own_x, what the model emitted (MSE) or drew (GMM) before the select.

Prompt lengths per row are the cycle [0, 4, 1, S, S - 1] cut to N: a free row, a prompt that ends mid-run, one frame, all
forced, all but one.  The forced frames are seeded N(0, 1) scaled to the RMS of the case's free run -- NOT the oracle's own
output, so a decode that ignores them lands far from the forced oracle (CPU test: > 0.05 on sample_x behind the prompt).
Set 'B' (the replay test's second call) shifts the cycle and draws other frames.

A GMM case carries the seed of its randomness, chosen as in decode_gmm_cases.py, on every oracle run the tests compare
with -- the free run, the forced runs of set 'A' and of set 'B': no cumulative mixture weight within PICK_MARGIN of its
uniform number (every draw counts: the ones under the prompt are compared too, as own_x), and the run's float32 twin
within F32_MARGIN (searched with F32_SEARCH on one thread: search_seed).  Conditions on the inputs; the CPU test asserts
them.  The oracle of a case is computed once per process and never modified."""
import functools

import torch

from tests import decode_gmm_cases as G
from tests import decode_row_controls_cases as RC
from tests.util import make_batch, rel_err

SMALL, U, S = G.SMALL, G.U, G.S
NAMES = G.NAMES + ("own_x",)
PICK_MARGIN, F32_MARGIN, F32_SEARCH = G.PICK_MARGIN, G.F32_MARGIN, G.F32_SEARCH
PROMPTS = [0, 4, 1, S, S - 1]
PROMPTS_B = [2, 0, S, 3, 1]
FRAME_SEED = {'A': 100, 'B': 101}


def prompt_lengths(N, which='A', steps=S):
    vals = [min(v, steps) if v < S - 1 else v - S + steps for v in (PROMPTS if which == 'A' else PROMPTS_B)]
    return RC.cycle(vals, N)


def _stack(cell, L, cost, **kw):
    # (weak feedback on the one-layer stacks too: without it nothing reads the fed-back frame and forcing changes nothing)
    return dict(SMALL, cell_type=cell, num_layers=L, which_cost=cost, weak_feedback=True, **kw)


# name -> (model keywords, N).  MSE heads decode on the machine by default, GMM heads (K = 3) with PARROT_PM_GMM=1,
# layer_norm as per-step launches.  N = 5: one partial row block; N = 17: two row blocks.
CASES = {}
for _cell, _L in (('gru', 1), ('gru', 2), ('gru', 3), ('lstm', 1), ('lstm', 2)):
    CASES[f'{_cell}{_L}_mse_n5'] = (_stack(_cell, _L, 'MSE'), 5)
for _cell, _L in (('gru', 2), ('lstm', 2)):
    CASES[f'{_cell}{_L}_mse_n17'] = (_stack(_cell, _L, 'MSE'), 17)
CASES['gru1_k3_n5'] = (_stack('gru', 1, 'GMM', k_gmm=3), 5)
CASES['lstm2_k3_n5'] = (_stack('lstm', 2, 'GMM', k_gmm=3), 5)
CASES['layer_norm'] = (_stack('gru', 2, 'MSE', layer_norm=True), 5)
# the first seed from 0 up whose free run and forced runs (sets 'A' and 'B') keep PICK_MARGIN and F32_SEARCH (search_seed)
SEEDS = {'gru1_k3_n5': 930, 'lstm2_k3_n5': 1}
GMM = tuple(n for n, (full, _) in CASES.items() if full['which_cost'] == 'GMM')
MSE_MACHINE = tuple(n for n, (full, _) in CASES.items() if full['which_cost'] == 'MSE' and n != 'layer_norm')


def forced_loop(p, cfg, labels, labels_mask, speaker, num_steps, forced=None, n_forced=None, unif=None, noise=None):
    """oracle/parrot_ref.sample_model with the fed-back frame of row b replaced by forced[t, b] while t < n_forced[b].
    Returns [sample_x, k, w, pi, phi, pi_att, own_x]; an MSE head's `pi` is the model's own output frame, as sample_model's
    is.  forced None: no row is forced."""
    from oracle import parrot_ref as R
    gmm = cfg['which_cost'] == 'GMM'
    assert not gmm or (unif is not None and noise is not None), 'GMM sampling needs explicit randomness'
    L, ln = cfg['num_layers'], cfg['layer_norm']
    names = lambda l: [n for n, _ in R.layer_outs(cfg, l)]
    N = labels.shape[0]
    dt = p['/parrot.initial_w'].dtype
    n_forced = torch.zeros(N, dtype=torch.int64) if n_forced is None else torch.as_tensor(n_forced, dtype=torch.int64)
    const = [[torch.zeros(N, wd, dtype=dt) for _, wd in R.layer_outs(cfg, l)] for l in range(1, L + 1)]
    spk_readout = spk_output = None
    if cfg['use_speaker']:
        emb = p['/parrot/lookuptable.W'][speaker[:, 0]]
        spk_readout = R.linear(p, 'speaker_to_readout', emb)
        spk_output = (R.fork(p, 'speaker_to_output', emb, ['gmm_mu', 'gmm_sigma', 'gmm_coeff']) if gmm
                      else R.linear(p, 'speaker_to_output', emb))
        for l in range(1, L + 1):
            outs = R.fork(p, f'speaker_to_h{l}', emb[None], names(l))
            const[l - 1] = [c_ + R.apply_norm(o_, ln)[0] for c_, o_ in zip(const[l - 1], outs)]
    ctx = R.encoder_apply(p, cfg, labels) * labels_mask[..., None]
    init = R.initial_carry(p, cfg, N)
    h, w, k = init['h'], init['w'], init['k']
    x = torch.zeros(N, cfg['output_dim'], dtype=dt)
    xs, ks, ws, phis, pis, cos, owns = [], [], [], [], [], [], []
    for step in range(num_steps):
        seq_in = [[c_.clone() for c_ in c] for c in const]
        if cfg['weak_feedback']:
            outs = R.fork(p, 'out_to_h1', x, names(1))
            seq_in[0] = [s_ + R.apply_norm(o_, ln) for s_, o_ in zip(seq_in[0], outs)]
        if cfg['full_feedback']:
            for l in range(2, L + 1):
                outs = R.fork(p, f'out_to_h{l}', x, names(l))
                seq_in[l - 1] = [s_ + R.apply_norm(o_, ln) for s_, o_ in zip(seq_in[l - 1], outs)]
        h, hout, k, w, phi, a = R.decoder_step(p, cfg, seq_in, h, k, w, ctx, sampling=True)
        readout = 0
        for l in range(1, L + 1):
            readout = readout + R.apply_norm(R.linear(p, f'h{l}_to_readout', hout[l - 1]), ln)
        readout = readout + R.linear(p, 'att_to_readout', w)
        if cfg['use_speaker']:
            readout = readout + spk_readout
        if not gmm:
            x = R.linear(p, 'readout_to_output', readout)
            if cfg['use_speaker']:
                x = x + spk_output
            cos.append(x)
        else:
            mu, sig, co = R.fork(p, 'readout_to_output', readout, ['gmm_mu', 'gmm_sigma', 'gmm_coeff'])
            if cfg['use_speaker']:
                mu, sig, co = mu + spk_output[0], sig + spk_output[1], co + spk_output[2]
            sig = torch.exp(sig - cfg['sampling_bias']) + cfg['epsilon']
            co = torch.softmax(co * (1. + cfg['sampling_bias']), -1) + cfg['epsilon']
            x = R.sample_gmm(mu, sig, co, unif[step].to(dt), noise[step].to(dt))
            cos.append(co)
        owns.append(x)
        if forced is not None:  # the one line sample_model does not have
            x = torch.where((step < n_forced).unsqueeze(1), forced[step].to(dt), x)
        xs.append(x); ks.append(k); ws.append(w); phis.append(phi); pis.append(a)
    sx, kk, ww, ph, pa, cc, own = (torch.stack(v, 0) for v in (xs, ks, ws, phis, pis, cos, owns))
    if not gmm:
        cc = sx  # (sample_model returns the frames again in `pi`'s place: here the fed-back frames, as the model's call does)
    return [sx, kk, ww, cc, ph, pa, own]


def params(full):
    return RC.params(full)


def frames(free_x, which='A'):
    """Seeded N(0, 1) frames [S, N, O] scaled to the RMS of the free run's frames."""
    g = torch.Generator().manual_seed(FRAME_SEED[which])
    rms = float(free_x.double().pow(2).mean().sqrt())
    return torch.randn(free_x.shape, generator=g, dtype=torch.float64) * rms


def build(name, seed, which='A', ctl=None):
    """Parameters, batch, randomness, forced frames and lengths, the oracle's free run (six outputs) and forced run (seven)
    of a case with the given seed.  ctl: per-row controls (decode_row_controls_cases.controls) for both runs, or None."""
    from oracle import parrot_ref as R
    full, N = CASES[name]
    gmm = full['which_cost'] == 'GMM'
    cfg = RC.oracle_cfg(full, ctl)
    p = params(full)
    _, _, lab, lm, spk = make_batch(cfg, 2, N, U, seed=9, speaker=cfg['use_speaker'])
    unif, noise = G.randomness(N, cfg['output_dim'], seed)
    with torch.no_grad():
        free = R.sample_model(p, cfg, lab, lm, spk, S, unif=unif, noise=noise)
        forced = frames(free[0], which)
        n = prompt_lengths(N, which)
        ref = forced_loop(p, cfg, lab, lm, spk, S, forced, n, unif=unif, noise=noise)
    return dict(name=name, full=full, cfg=cfg, p=p, lab=lab, lm=lm, spk=spk, N=N, U=U, S=S, unif=unif, noise=noise, free=free,
                ref=ref, forced=forced, n=n, gmm=gmm, ctl=ctl)


@functools.lru_cache(maxsize=None)
def case(name, which='A'):
    return build(name, SEEDS.get(name, 0), which)


@functools.lru_cache(maxsize=None)
def case_with_controls(name):
    """The case with the per-row controls of decode_row_controls_cases (set 'A') on top of the forcing."""
    return build(name, SEEDS.get(name, 0), 'A', RC.controls(CASES[name][1], CASES[name][0]['which_cost'] == 'GMM'))


def free_region(c):
    """[S, N] mask: the steps of each row at or behind the end of its prompt (where sample_x is the model's own again)."""
    t = torch.arange(c['S']).unsqueeze(1)
    return t >= torch.tensor(c['n']).unsqueeze(0)


def pick_margin(c, outs):
    """min over every draw of |cumsum(pi)_k - u| on the run `outs` (inf at K = 1)."""
    pi = outs[3]
    if pi.shape[-1] < 2:
        return float('inf')
    cum = pi.cumsum(-1)[..., :-1]
    return float((cum - c['unif'].to(cum.dtype).unsqueeze(-1)).abs().min())


def f32_error(c, forced=True):
    """Worst relative error over the outputs of the oracle's run in float32 against its float64 run: the forced run (seven
    outputs, controls included) or the free run (six)."""
    from oracle import parrot_ref as R
    p32 = {k: v.float() for k, v in c['p'].items()}
    cfg32 = RC.oracle_cfg(c['full'], c['ctl'], torch.float32)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)  # (one summation order per host; the seeds keep a factor of two to the bound for other hosts)
    try:
        with torch.no_grad():
            if forced:
                r32 = forced_loop(p32, cfg32, c['lab'], c['lm'].float(), c['spk'], c['S'], c['forced'].float(), c['n'],
                                  unif=c['unif'], noise=c['noise'])
            else:
                r32 = R.sample_model(p32, cfg32, c['lab'], c['lm'].float(), c['spk'], c['S'], unif=c['unif'], noise=c['noise'])
    finally:
        torch.set_num_threads(threads)
    return max(rel_err(a, b) for a, b in zip(r32, c['ref'] if forced else c['free']))


def search_seed(name, start=0, stop=5000):
    """How SEEDS was made: the first seed whose free run and forced runs of both sets keep PICK_MARGIN and F32_SEARCH."""
    for seed in range(start, stop):
        ok = True
        for which in ('A', 'B'):
            c = build(name, seed, which)
            ok = ok and pick_margin(c, c['ref']) >= PICK_MARGIN and f32_error(c) <= F32_SEARCH
            if ok and which == 'A':
                ok = pick_margin(c, c['free']) >= PICK_MARGIN and f32_error(c, forced=False) <= F32_SEARCH
            if not ok:
                break
        if ok:
            return seed
    return None

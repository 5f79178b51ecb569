"""Cases of the resumable decode (Parrot.sample_model*(state=, return_state=), decode_segments, StreamingDecoder;
parrot_sample_save_state / _load_state), shared by tests/test_decode_segments_cpu.py (the premise) and
tests/test_gpu_decode_segments.py (the runs).  The cases, seeds, prompts and randomness are those of
tests/decode_forced_cases.py: SMALL, U = 9, S = 10, N = 5 (one partial row block) and N = 17 (two) -- the smallest shapes
at which the tiling, the row blocks and the parity of the launches' ping-pong can go wrong; the GMM seeds keep every pick
PICK_MARGIN away from a tie.

The oracle of a resumed run is carry_loop: decode_forced_cases.forced_loop written once more from the oracle's own pieces
with one thing more, the entering carry (x, kappa, w, the layers' states) in place of the learned initial states, and the
leaving carry returned.  Without an entering carry it IS forced_loop, bit for bit, and chained over any cut in float64 it
equals the one-piece loop with torch.equal (the CPU test asserts both): a step reads nothing but the carry.

Cuts over S = 10: CUTS = [1, 4, 10] -- a one-frame segment, then an odd (3) and an even (6) one, so the per-step launches
end on either ping-pong slot; SEGMENT = 4 -- segments of 4, 4 and 2, so decode_segments' last segment runs whole and is
cut."""
import functools

import torch

from tests import decode_forced_cases as FC

S, U = FC.S, FC.U
CUTS = [1, 4, 10]
SEGMENT = 4
NAMES = FC.NAMES


def carry_loop(p, cfg, labels, labels_mask, speaker, num_steps, carry=None, forced=None, n_forced=None, unif=None, noise=None):
    """forced_loop from an entering carry: dict(x [N, O], k, w, h -- per layer the state, an LSTM's (state, cells)), None:
    the learned initial states and x = 0.  forced / n_forced / unif / noise count from the call's first step.  Returns
    ([sample_x, k, w, pi, phi, pi_att, own_x], the carry after the last step)."""
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
    if carry is None:
        init = R.initial_carry(p, cfg, N)
        h, w, k = init['h'], init['w'], init['k']
        x = torch.zeros(N, cfg['output_dim'], dtype=dt)
    else:  # the one thing forced_loop does not have
        h, w, k, x = carry['h'], carry['w'], carry['k'], carry['x']
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
        if forced is not None:
            x = torch.where((step < n_forced).unsqueeze(1), forced[step].to(dt), x)
        xs.append(x); ks.append(k); ws.append(w); phis.append(phi); pis.append(a)
    sx, kk, ww, ph, pa, cc, own = (torch.stack(v, 0) for v in (xs, ks, ws, phis, pis, cos, owns))
    if not gmm:
        cc = sx
    return [sx, kk, ww, cc, ph, pa, own], dict(h=h, w=w, k=k, x=x)


def pack(carry, cfg):
    """An oracle carry as the library packs a decode state: [N, W], x (ldx = O rounded up to 4, zero padded) | kappa | w |
    h_0 .. h_{L-1} | c_0 .. c_{L-1} (LSTM)."""
    lstm = cfg.get('cell_type', 'gru') == 'lstm'
    x = carry['x']
    ldx = (x.shape[1] + 3) // 4 * 4
    parts = [torch.nn.functional.pad(x, (0, ldx - x.shape[1])), carry['k'], carry['w']]
    parts += [h[0] if lstm else h for h in carry['h']]
    if lstm:
        parts += [h[1] for h in carry['h']]
    return torch.cat(parts, dim=1)


def state_floats(cfg):
    O = cfg['output_dim']
    lstm = cfg.get('cell_type', 'gru') == 'lstm'
    return ((O + 3) // 4 * 4 + cfg['attention_size'] + cfg['encoded_input_dim']
            + cfg['num_layers'] * cfg['rnn_h_dim'] * (2 if lstm else 1))


def segment_args(c, t0, t1, forced):
    """What the segment of frames t0 .. t1 - 1 takes: the slices of unif / noise and, forced, of the frames with the
    prompt lengths counted from t0 and clamped to the segment."""
    kw = dict(unif=c['unif'][t0:t1], noise=c['noise'][t0:t1])
    if forced:
        kw.update(forced=c['forced'][t0:t1], n_forced=[min(max(n - t0, 0), t1 - t0) for n in c['n']])
    return kw


def chain(c, cuts, forced):
    """carry_loop over the segments [0, cuts[0]), [cuts[0], cuts[1]), ..: (the outputs concatenated, the last carry)."""
    carry, parts, t0 = None, [], 0
    with torch.no_grad():
        for t1 in cuts:
            outs, carry = carry_loop(c['p'], c['cfg'], c['lab'], c['lm'], c['spk'], t1 - t0, carry, **segment_args(c, t0, t1, forced))
            parts.append(outs)
            t0 = t1
    return [torch.cat(v, 0) for v in zip(*parts)], carry


@functools.lru_cache(maxsize=None)
def one_piece(name, forced=False):
    """(outputs, carry, packed state) of the oracle's one-piece run of the case: free, or with the prompts of set 'A'."""
    c = FC.case(name)
    outs, carry = chain(c, [c['S']], forced)
    return outs, carry, pack(carry, c['cfg'])

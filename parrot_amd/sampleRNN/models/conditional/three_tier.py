"""Conditional three-tier SampleRNN -- mirrors reference sampleRNN/models/conditional/three_tier.py:
the tier builders (``big_frame_level_rnn`` :291-380, ``frame_level_rnn`` :382-450,
``sample_level_predictor`` :452-515), ``compute_cost`` (:534-636), ``getting_generation_functions``
(:703-734) and ``generate_and_save_samples`` (:750-851), with the run configuration the reference
hard-codes at import time (:145-202) as module globals.

Differences by construction (no Theano graph): the functions compute eagerly on GPU tensors through
the HIP library; ``configure(...)`` can override the hard-coded hyper-parameters (tests use small
dimensions); generation has a device-resident fast path (``DeviceGenerator`` ->
samplernn_generate_*, include/parrot_hip.h) that ``generate_and_save_samples`` uses.  That path and what is
served on top of it live in the package ``parrot_amd.sampleRNN.generation``; their names are re-exported here.
"""
from __future__ import annotations

import os
from time import time

import numpy
import torch

from .... import ops as hip
from ... import lib
from ...lib import ops as lops

# --- three_tier.py:145-202: the reference calls get_args() on a hard-coded string at import time
SEQ_LEN = 4000
BIG_FRAME_SIZE = 80
FRAME_SIZE = 10
OVERLAP = BIG_FRAME_SIZE
WEIGHT_NORM = True
EMB_SIZE = 256
SKIP_CONN = False
DIM = 1024
BIG_DIM = DIM
N_RNN = 1
N_BIG_RNN = N_RNN
RNN_TYPE = 'GRU'
H0_MULT = 2 if RNN_TYPE == 'LSTM' else 1
LEARN_H0 = True
Q_LEVELS = 256
Q_TYPE = 'mu-law'
BATCH_SIZE = 8
GRAD_CLIP = 1
BITRATE = 16000
TEMPERATURE = 1.
FEAT_DIM = 63
Q_ZERO = numpy.int32(Q_LEVELS // 2)


def configure(**kw):
    """Overrides the hard-coded run configuration (extension; the reference edits the source)."""
    g = globals()
    for k, v in kw.items():
        assert k in g, k
        g[k] = v
    g['BIG_DIM'] = g['DIM']
    g['N_BIG_RNN'] = g['N_RNN']
    g['H0_MULT'] = 2 if g['RNN_TYPE'] == 'LSTM' else 1
    g['Q_ZERO'] = numpy.int32(g['Q_LEVELS'] // 2)
    g['OVERLAP'] = g['BIG_FRAME_SIZE']


def _frames_to_float(frames):
    """three_tier.py:309-310, 398-399."""
    f = (frames.to(torch.float32) / lib.floatX(Q_LEVELS // 2)) - lib.floatX(1)
    return f * lib.floatX(2)


def _stacked(name, n_rnn, in_dim, dim, inp, h0):
    if RNN_TYPE == 'GRU':
        return lops.stackedGRU(name + '.GRU', n_rnn, in_dim, dim, inp, h0, WEIGHT_NORM, SKIP_CONN)
    return lops.stackedLSTM(name + '.LSTM', n_rnn, in_dim, dim, inp, h0, WEIGHT_NORM, SKIP_CONN)


def big_frame_level_rnn(input_sequences, h0, reset, features):
    """three_tier.py:291-380: (output [B, 8n, DIM], last_hidden, independent_preds [B, 80n, Q])."""
    B = input_sequences.shape[0]
    frames = _frames_to_float(input_sequences.reshape(B, -1, BIG_FRAME_SIZE))
    rnn_inp = lops.Linear('BigFrameLevel.rnn_inp_fusion', [BIG_FRAME_SIZE, FEAT_DIM], BIG_DIM,
                          [frames, features.to(torch.float32)], initialization='he', weightnorm=WEIGHT_NORM)
    learned_h0 = lib.param('BigFrameLevel.h0', numpy.zeros((N_BIG_RNN, H0_MULT * BIG_DIM), dtype='float32'),
                           trainable=LEARN_H0)
    if reset:
        h0 = learned_h0.unsqueeze(0).expand(B, -1, -1)
    rnns_out, last_hidden = _stacked('BigFrameLevel', N_BIG_RNN, BIG_DIM, BIG_DIM, rnn_inp, h0)
    output = lops.Linear('BigFrameLevel.Output', BIG_DIM, DIM * BIG_FRAME_SIZE // FRAME_SIZE, rnns_out,
                         initialization='he', weightnorm=WEIGHT_NORM)
    output = output.reshape(B, output.shape[1] * BIG_FRAME_SIZE // FRAME_SIZE, DIM)
    independent_preds = lops.Linear('BigFrameLevel.IndependentPreds', BIG_DIM, Q_LEVELS * BIG_FRAME_SIZE, rnns_out,
                                    initialization='he', weightnorm=WEIGHT_NORM)
    independent_preds = independent_preds.reshape(B, independent_preds.shape[1] * BIG_FRAME_SIZE, Q_LEVELS)
    return output, last_hidden, independent_preds


def frame_level_rnn(input_sequences, other_input, h0, reset):
    """three_tier.py:382-450: (output [B, 10m, DIM], last_hidden)."""
    B = input_sequences.shape[0]
    frames = _frames_to_float(input_sequences.reshape(B, -1, FRAME_SIZE))
    gru_input = lops.Linear('FrameLevel.InputExpand', FRAME_SIZE, DIM, frames, initialization='he',
                            weightnorm=WEIGHT_NORM) + other_input
    learned_h0 = lib.param('FrameLevel.h0', numpy.zeros((N_RNN, H0_MULT * DIM), dtype='float32'), trainable=LEARN_H0)
    if reset:
        h0 = learned_h0.unsqueeze(0).expand(B, -1, -1)
    rnns_out, last_hidden = _stacked('FrameLevel', N_RNN, DIM, DIM, gru_input, h0)
    output = lops.Linear('FrameLevel.Output', DIM, FRAME_SIZE * DIM, rnns_out, initialization='he',
                         weightnorm=WEIGHT_NORM)
    output = output.reshape(B, output.shape[1] * FRAME_SIZE, DIM)
    return output, last_hidden


def sample_level_predictor(frame_level_outputs, prev_samples):
    """three_tier.py:452-515: logits [rows, Q_LEVELS]."""
    assert EMB_SIZE > 0, 'no support for one-hot in three_tier (three_tier.py:458)'
    # Same parameters, created in the reference's order (Embedding, L1_PrevSamples, L2, L3, Output); the arithmetic runs
    # on the fused HIP operators (round 5):
    #   * Embedding -> reshape -> L1_PrevSamples (no bias) -> + frame_level_outputs is, row by row, a sum of FRAME_SIZE rows
    #     of the folded table (Embedding . W1_j) plus the frame-tier row: hip.embed_sum (gather-sum forward, segmented-sum
    #     backward; no [rows, FRAME_SIZE * EMB_SIZE] activation and no K = FRAME_SIZE * EMB_SIZE product);
    #   * relu(L2) -> relu(L3) -> Output: hip.relu_mlp (bias + ReLU in the products' epilogues, the ReLU masks of the
    #     backward pass in the epilogues of the dx products).
    vectors = lops.Embedding('SampleLevel.Embedding', Q_LEVELS, EMB_SIZE, None)
    lops.Linear('SampleLevel.L1_PrevSamples', FRAME_SIZE * EMB_SIZE, DIM, None, biases=False, initialization='he',
                weightnorm=WEIGHT_NORM, just_params=True)
    out = hip.embed_sum(vectors, lops.effective_weight('SampleLevel.L1_PrevSamples', 0, WEIGHT_NORM),
                        prev_samples.reshape(-1, FRAME_SIZE), frame_level_outputs.reshape(-1, DIM))
    wb = []
    for name, dout, init in (('SampleLevel.L2', DIM, 'he'), ('SampleLevel.L3', DIM, 'he'), ('SampleLevel.Output', Q_LEVELS, None)):
        lops.Linear(name, DIM, dout, None, initialization=init, weightnorm=WEIGHT_NORM, just_params=True)
        wb += [lops.effective_weight(name, 0, WEIGHT_NORM), lib.param(name + '.b')]
    return hip.relu_mlp(out, *wb)


def compute_cost(sequences, features, h0, big_h0, reset, mask):
    """three_tier.py:534-636.  sequences [B, S+80] int, features [B, S/80, 63], mask [B, S+80].
    Returns (cost, ip_cost, all_params, ip_params, other_params, new_h0, new_big_h0); costs in bits."""
    big_input_sequences = sequences[:, :-BIG_FRAME_SIZE]
    input_sequences = sequences[:, BIG_FRAME_SIZE - FRAME_SIZE:-FRAME_SIZE]
    target_sequences = sequences[:, BIG_FRAME_SIZE:]
    target_mask = mask[:, BIG_FRAME_SIZE:].to(torch.float32)
    big_frame_level_outputs, new_big_h0, big_frame_independent_preds = \
        big_frame_level_rnn(big_input_sequences, big_h0, reset, features)
    frame_level_outputs, new_h0 = frame_level_rnn(input_sequences, big_frame_level_outputs, h0, reset)
    prev_samples = sequences[:, BIG_FRAME_SIZE - FRAME_SIZE:-1]
    prev_samples = prev_samples.unfold(1, FRAME_SIZE, 1).reshape(-1, FRAME_SIZE)  # images2neibs, :555-558
    sample_level_outputs = sample_level_predictor(frame_level_outputs.reshape(-1, DIM), prev_samples)
    tgt = target_sequences.reshape(-1, 1).long()
    log2e = float(numpy.log2(numpy.e))

    def ce_bits(logits):
        ce = hip.softmax_ce(logits, tgt)  # logsumexp - picked logit, one HIP pass (and one for its gradient)
        ce = ce.reshape(target_sequences.shape) * target_mask
        return ce.sum() / (target_mask.sum() + 1e-5) * log2e

    cost = ce_bits(sample_level_outputs)
    ip_cost = ce_bits(big_frame_independent_preds.reshape(-1, Q_LEVELS))
    all_named = lib.named_params()
    # three_tier.py:595-600: ip_params = the BigFrameLevel parameters the independent-prediction cost is a function of
    # (everything in that tier except its Output projection, which only feeds the frame tier); other_params = the
    # remaining parameters of `cost`; all_params = ip_params + other_params (so IndependentPreds is in, via ip_params).
    trainable = [(n, p) for n, p in all_named.items() if getattr(p, 'param', False)]
    ip_params = [p for n, p in trainable if 'BigFrameLevel' in n and not n.startswith('BigFrameLevel.Output.')]
    other_params = [p for n, p in trainable if 'BigFrameLevel' not in n or n.startswith('BigFrameLevel.Output.')]
    all_params = ip_params + other_params
    return cost, ip_cost, all_params, ip_params, other_params, new_h0, new_big_h0


# ----------------------------------------------------------------------------- generation
def getting_generation_functions(sequences=None, h0=None, big_h0=None, reset=None, features=None):
    """three_tier.py:703-734.  Returns (big_frame_level_generate_fn, frame_level_generate_fn,
    sample_level_generate_fn) taking / returning numpy arrays like the compiled Theano functions."""
    dev = lib.device()

    def _t(x, dtype=None):
        t = torch.as_tensor(numpy.asarray(x)).to(dev)
        return t.to(dtype) if dtype is not None else t

    def big_fn(seq, big_h0_, reset_, feats):
        with torch.no_grad():
            out, last, _ = big_frame_level_rnn(_t(seq), _t(big_h0_, torch.float32), bool(reset_), _t(feats, torch.float32))
        return out.cpu().numpy(), last.cpu().numpy()

    def frame_fn(seq, big_out, h0_, reset_):
        with torch.no_grad():
            out, last = frame_level_rnn(_t(seq), _t(big_out, torch.float32).unsqueeze(1), _t(h0_, torch.float32),
                                        bool(reset_))
        return out.cpu().numpy(), last.cpu().numpy()

    def sample_fn(frame_out, prev, temperature=1.0):
        with torch.no_grad():
            logits = sample_level_predictor(_t(frame_out, torch.float32), _t(prev))
            return lops.softmax_and_sample(logits, temperature=temperature).cpu().numpy().astype('int32')

    return big_fn, frame_fn, sample_fn


# the generation package's names, as they always were here (it reads the configuration above from this module when called)
from ...generation import inputs as _inputs  # noqa: E402
from ...generation.inputs import (DRAW_K1, DRAW_K2, DRAW_MODES, _M64, _per_utterance, _seed_image,  # noqa: E402,F401
                                  _per_utterance_min_p, _per_utterance_top_k, _per_utterance_top_p, _splitmix64,
                                  build_packed_draws, build_packed_inputs, build_packed_min_p, build_packed_top_k,
                                  build_packed_top_p, draw_mode_code, min_p_active, min_p_array, min_p_code,
                                  pack_utterances, schedule_segment, top_k_array, top_k_code, top_p_active, top_p_array,
                                  top_p_code, unpack_samples, utterance_draw_u01, utterance_seed)
from ...generation.inputs import (_per_utterance_prompts, build_packed_prompts, forced_array,  # noqa: E402,F401
                                  unpack_log_probs)
from ...generation.inputs import skip_stacks_enabled, stack_param_names  # noqa: E402,F401
from ...generation.device import DeviceGenerator  # noqa: E402
from ...generation.serving import (StreamingGenerator, generate_packed, generate_stream,  # noqa: E402,F401
                                   score_utterances)


def write_audio_file(name, data, path_to_save):
    """three_tier.py:739-748."""
    import scipy.io.wavfile
    data = data.astype('float32')
    data -= data.min()
    data /= data.max()
    data -= 0.5
    data *= 0.95
    scipy.io.wavfile.write(os.path.join(path_to_save, name + '.wav'), BITRATE, data)


def _write_piece(tag, i, samp, path_to_save):
    """three_tier.py:846-851 for utterance i: sample_<tag>_<i>.wav under path_to_save (None: nothing is written)."""
    if path_to_save is None:
        return
    os.makedirs(path_to_save, exist_ok=True)
    if Q_TYPE == 'mu-law':
        samp = hip.mu2linear(torch.from_numpy(samp.astype('int32')).to(lib.device())).cpu().numpy()
    write_audio_file("sample_{}_{}".format(tag, i), samp, path_to_save)


def generate_and_save_samples(tag, path_to_save=None, features=None, features_length=None, noise_level=0.,
                              big_frame_level_generate_fn=None, frame_level_generate_fn=None,
                              sample_level_generate_fn=None, npy_address=None, temperature=TEMPERATURE,
                              use_device_loop=True, pack_streams=0, stream_frames=0, utterance_seed=None,
                              draw_mode='sequential', top_k=0, top_p=0.0, min_p=0.0):
    """three_tier.py:750-851.  With use_device_loop (default) the per-sample loop runs on the GPU
    (DeviceGenerator); otherwise the reference's three-function Python loop is executed literally.  Models with
    skip-connection stacks (SKIP_CONN) take the device loop with PARROT_SR_SKIP_STACKS=1 and the literal loop, with its
    own limits (no seeds, truncation, packing or streaming), without it.

    pack_streams = N > 0 with features_length given: row i's first features_length[i] frames form utterance i, the
    utterances run through generate_packed on N streams and the wav files are written from the returned pieces (the
    return value is then that list of [80 * features_length[i]] arrays).  0: the rectangle above, as before.

    stream_frames = S > 0 with features_length given: the utterances go through a StreamingGenerator of
    pack_streams or 32 streams in segments of S frames; each wav is written as soon as its utterance has finished, and
    the return value is the list of pieces as above.

    utterance_seed = S (an integer; None: off): utterance i draws with the seed utterance_seed(S, i) of its own at
    `temperature`, in the rectangle, packed and streamed modes alike (DeviceGenerator(utterance_draws=True)): its samples
    no longer depend on where it was placed.  Device loop only.

    draw_mode = 'sequential' (default) or 'scan': how the device loop's draws at temperature > 0 find their code
    (DeviceGenerator), in the rectangle, packed and streamed modes alike.  'scan' needs the device loop.

    top_k = k > 0: those draws are taken among the k most likely codes (DeviceGenerator), in all three modes; 0
    (default): among all codes.  A non-zero top_k needs the device loop; a negative one is a ValueError.

    top_p = p strictly between 0 and 1: those draws are taken among the nucleus of the codes top_k left (DeviceGenerator),
    in all three modes; 0 (default) or >= 1: no nucleus.  An active top_p needs the device loop -- the literal
    three-function loop refuses it --; a negative one or a NaN is a ValueError.

    min_p in (0, 1]: of the codes both left, those draws keep the ones at least min_p times as likely as the most likely code
    (DeviceGenerator), in all three modes; 0 (default): off.  An active min_p needs the device loop -- the literal loop
    refuses it --; a value outside [0, 1] or a NaN is a ValueError."""
    total_time = time()
    # (the device loop takes skip-connection stacks only with PARROT_SR_SKIP_STACKS=1, read here at call time)
    device_loop = use_device_loop and (not SKIP_CONN or (_inputs.skip_stacks_enabled() and N_RNN >= 2))
    if draw_mode_code(draw_mode) != 0 and not device_loop:
        raise ValueError("draw_mode='scan' needs the device-resident generator")
    if top_k_code(top_k) != 0 and not device_loop:
        raise ValueError("top_k needs the device-resident generator")
    if top_p_active(top_p) and not device_loop:
        raise ValueError("top_p needs the device-resident generator")
    if min_p_active(min_p) and not device_loop:
        raise ValueError("min_p needs the device-resident generator")
    per_utt = utterance_seed is not None
    if per_utt and not device_loop:
        raise ValueError("utterance_seed needs the device-resident generator")
    if npy_address is not None:
        test_feats = numpy.load(npy_address).astype('float32')  # [T,B,63]
    else:
        assert features is not None
        test_feats = numpy.asarray(features, dtype='float32')
    n_seqs, n_frames = test_feats.shape[1], test_feats.shape[0]
    LENGTH = n_frames * BIG_FRAME_SIZE
    seeds = [_inputs.utterance_seed(utterance_seed, i) for i in range(n_seqs)] if per_utt else None
    placed = features_length is not None and (stream_frames > 0 or pack_streams > 0)  # (else: the rectangle)
    if placed:
        lens = [min(max(int(n), 1), n_frames) for n in features_length]
        utts = [test_feats[:lens[i], i] for i in range(n_seqs)]
        seconds = sum(lens) * BIG_FRAME_SIZE / float(BITRATE)
    if placed and stream_frames > 0:
        n_streams = int(pack_streams) if pack_streams > 0 else 32
        sg = StreamingGenerator(n_streams, int(stream_frames), temperature=temperature, utterance_draws=per_utt,
                                draw_mode=draw_mode, top_k=top_k, top_p=top_p, min_p=min_p)
        chunks = [[] for _ in range(n_seqs)]
        pieces = [None] * n_seqs
        try:
            for i in range(n_seqs):
                assert sg.submit(utts[i], **(dict(seed=seeds[i]) if per_utt else {})) == i
            while not sg.idle():
                for i, chunk, done in sg.step():
                    chunks[i].append(chunk)
                    if done:
                        pieces[i] = numpy.concatenate(chunks[i])
                        chunks[i] = None
                        _write_piece(tag, i, pieces[i], path_to_save)
        finally:
            sg.close()
        total_time = time() - total_time
        print("{} samples of {} seconds in all generated in {} seconds ({} streams, segments of {} frames).".format(
            n_seqs, seconds, total_time, n_streams, int(stream_frames)))
        return pieces
    if placed:
        pieces = generate_packed(utts, n_streams=int(pack_streams), temperature=temperature, seeds=seeds,
                                 draw_mode=draw_mode, top_k=top_k, top_p=top_p, min_p=min_p)
        total_time = time() - total_time
        print("{} samples of {} seconds in all generated in {} seconds ({} packed streams).".format(
            n_seqs, seconds, total_time, int(pack_streams)))
        for i, samp in enumerate(pieces):
            _write_piece(tag, i, samp, path_to_save)
        return pieces
    if device_loop:
        gen = DeviceGenerator(n_seqs, n_frames, temperature=temperature, utterance_draws=per_utt, draw_mode=draw_mode,
                              top_k=top_k, top_p=top_p, min_p=min_p)
        draws = dict(seeds=seeds, temperatures=float(temperature)) if per_utt else {}
        samples = gen.generate(test_feats, **draws).cpu().numpy()
        gen.close()
    else:
        feats_bt = test_feats.transpose(1, 0, 2)
        samples = numpy.zeros((n_seqs, LENGTH), dtype='int32')
        samples[:, :BIG_FRAME_SIZE] = Q_ZERO
        big_h0 = numpy.zeros((n_seqs, N_BIG_RNN, H0_MULT * BIG_DIM), dtype='float32')
        h0 = numpy.zeros((n_seqs, N_RNN, H0_MULT * DIM), dtype='float32')
        big_out = frame_out = None
        for t in range(BIG_FRAME_SIZE, LENGTH):
            if t % BIG_FRAME_SIZE == 0:
                big_out, big_h0 = big_frame_level_generate_fn(
                    samples[:, t - BIG_FRAME_SIZE:t], big_h0, numpy.int32(t == BIG_FRAME_SIZE),
                    feats_bt[:, t // BIG_FRAME_SIZE, :][:, None, :])
            if t % FRAME_SIZE == 0:
                frame_out, h0 = frame_level_generate_fn(
                    samples[:, t - FRAME_SIZE:t], big_out[:, (t // FRAME_SIZE) % (BIG_FRAME_SIZE // FRAME_SIZE)],
                    h0, numpy.int32(t == BIG_FRAME_SIZE))
            samples[:, t] = sample_level_generate_fn(frame_out[:, t % FRAME_SIZE], samples[:, t - FRAME_SIZE:t],
                                                     temperature)
    total_time = time() - total_time
    print("{} samples of {} seconds length generated in {} seconds.".format(n_seqs, LENGTH / float(BITRATE), total_time))
    for i in range(n_seqs):
        _write_piece(tag, i, samples[i, :int(features_length[i]) * 80] if features_length is not None else samples[i],
                     path_to_save)
    return samples

"""Argument parsers of the entry points -- same flags, defaults and quirks as reference utils.py
(train_parse utils.py:173-253, sample_parse utils.py:256-327), including the `type=bool` flags for
which any non-empty string is truthy.  Plotting / animation helpers (utils.py:30-170) are cosmetic
and out of scope.

Extra flags (not in the reference): --num_layers, --cell_type, --compute_dtype, --encoder_literal, --synthetic_examples, --max_steps,
--device, --use_graph; sample.py: --decode_dtype, --stop_at_end, --pack_streams, --stream_frames,
--utterance_seed, --draw_mode, --top_k, --top_p, --min_p.
"""
from __future__ import annotations

import argparse
import os
import re

SPTK_DIR = '/data/lisatmp4/kumarkun/merlin/tools/bin/SPTK-3.9/'   # utils.py:20
WORLD_DIR = '/data/lisatmp4/kumarkun/merlin/tools/bin/WORLD/'     # utils.py:21


_ATOI = re.compile(r'[ \t\n\v\f\r]*([+-]?[0-9]+)')


def env_int(name, default):
    """Integer / on-off PARROT_* switch, parsed like the HIP library's (csrc/switches.h, the table of every switch): C's
    atoi -- optional leading blanks and sign, then the leading digits, anything else 0 -- and `default` when unset."""
    v = os.environ.get(name)
    if v is None:
        return default
    m = _ATOI.match(v)
    return int(m.group(1)) if m else 0


def env_str(name, default=None):
    """String-valued PARROT_* switch (paths, flags, backend names): the value as set, `default` when unset."""
    return os.environ.get(name, default)


def _results_dir():
    return os.environ.get('RESULTS_DIR', os.path.join(os.getcwd(), 'results'))


def _common_extras(parser):
    parser.add_argument('--num_layers', type=int, default=3, help='decoder GRU layers (reference: 3)')
    parser.add_argument('--cell_type', type=str, default='gru', choices=('gru', 'lstm'),
                        help="decoder layers: 'gru' (the reference's GatedRecurrent) or 'lstm' (BASELINE configs[3])")
    parser.add_argument('--compute_dtype', type=str, default='float32', choices=('float32', 'bf16'),
                        help='bf16: bf16 MFMA operands, f32 accumulation / states / master weights (DESIGN.md 3.4)')
    parser.add_argument('--encoder_literal', type=int, default=1,
                        help='1: scan the encoder over the batch axis like the reference does')
    parser.add_argument('--device', type=str, default='cuda')
    parser.add_argument('--use_graph', type=int, default=1)
    parser.add_argument('--synthetic_examples', type=int, default=64)


def train_parse(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument('--experiment_name', type=str, default='baseline')
    parser.add_argument('--encoder_type', type=str, default='bidirectional')
    parser.add_argument('--encoder_dim', type=int, default=128)
    parser.add_argument('--input_dim', type=int, default=420)
    parser.add_argument('--output_dim', type=int, default=63)
    parser.add_argument('--rnn_h_dim', type=int, default=1024)
    parser.add_argument('--readouts_dim', type=int, default=1024)
    parser.add_argument('--weak_feedback', type=bool, default=False)
    parser.add_argument('--full_feedback', type=bool, default=False)
    parser.add_argument('--feedback_noise_level', type=float, default=None)
    parser.add_argument('--layer_norm', type=bool, default=False)
    parser.add_argument('--labels_type', type=str, default='text')  # reference default 'full_labels' cannot feed model.py:511 (imatrix)
    parser.add_argument('--which_cost', type=str, default='MSE')
    parser.add_argument('--attention_type', type=str, default='graves')
    parser.add_argument('--attention_alignment', type=float, default=1.)
    parser.add_argument('--num_characters', type=int, default=43)
    parser.add_argument('--batch_size', type=int, default=8)
    parser.add_argument('--seq_size', type=int, default=50)
    parser.add_argument('--save_every', type=int, default=500)
    parser.add_argument('--learning_rate', type=float, default=1e-4)
    parser.add_argument('--grad_clip', type=float, default=0.9)
    parser.add_argument('--lr_schedule', type=bool, default=False)
    parser.add_argument('--load_experiment', type=str, default=None)
    parser.add_argument('--raw_output', type=bool, default=False)
    parser.add_argument('--time_limit', type=float, default=None)
    parser.add_argument('--use_speaker', type=bool, default=False)
    parser.add_argument('--num_speakers', type=int, default=22)
    parser.add_argument('--speaker_dim', type=int, default=128)
    parser.add_argument('--dataset', type=str, default='vctk')
    parser.add_argument('--save_dir', type=str, default=_results_dir())
    parser.add_argument('--max_steps', type=int, default=None, help='stop after this many windows')
    _common_extras(parser)
    args = parser.parse_args(argv)
    if args.dataset not in args.save_dir:
        args.save_dir = os.path.join(args.save_dir, args.dataset)
    return args


def sample_parse(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument('--experiment_name', type=str, default='baseline')
    parser.add_argument('--sampling_bias', type=float, default=1.)
    parser.add_argument('--timing_coeff', type=float, default=1.)
    parser.add_argument('--sharpening_coeff', type=float, default=1.)
    parser.add_argument('--num_samples', type=int, default=10)
    parser.add_argument('--num_steps', type=int, default=2048)
    parser.add_argument('--samples_name', type=str, default='sample')
    parser.add_argument('--speaker_id', type=int, default=None)
    parser.add_argument('--mix', type=float, default=None)
    parser.add_argument('--dataset', type=str, default='vctk')
    parser.add_argument('--new_sentences', type=bool, default=False)
    parser.add_argument('--save_dir', type=str, default=_results_dir())
    parser.add_argument('--sptk_dir', type=str, default=SPTK_DIR)
    parser.add_argument('--world_dir', type=str, default=WORLD_DIR)
    parser.add_argument('--process_originals', type=bool, default=False)
    parser.add_argument('--do_post_filtering', type=bool, default=False)
    parser.add_argument('--animation', type=bool, default=False)
    parser.add_argument('--debug_plot', type=bool, default=False)
    parser.add_argument('--sample_one_step', type=bool, default=False)
    parser.add_argument('--use_last', type=bool, default=False)
    parser.add_argument('--phrase', type=str, default=None)
    parser.add_argument('--random_speaker', type=bool, default=False)
    parser.add_argument('--plot_raw', type=bool, default=False)
    parser.add_argument('--device', type=str, default='cuda')
    parser.add_argument('--decode_dtype', type=str, default='float32', choices=('float32', 'bf16'),
                        help='bf16: the recurrent-layer products of the decode loop round both operands to bf16 '
                             '(LSTM decoders on the persistent machine, DESIGN.md 3.6); float32: f32 operands, whatever '
                             'the experiment was trained with')
    parser.add_argument('--stop_at_end', type=int, default=0,
                        help='1: the decode kernel itself stops at the end of the utterance (the rule of sample.py:145-163) '
                             'instead of decoding --num_steps frames and cutting afterwards; same frames, same lengths')
    parser.add_argument('--pack_streams', type=int, default=0,
                        help='N > 0 (with --raw_output): the SampleRNN vocoder packs the utterances, each cut at its own '
                             'length, one after the other into N streams of one generation plan instead of running '
                             '--num_steps frames for every row (DESIGN.md 3.6); 0: the rectangle')
    parser.add_argument('--stream_frames', type=int, default=0,
                        help='S > 0 (with --raw_output): the SampleRNN vocoder runs the utterances through one plan of S + 1 '
                             'slots used as a ring, in segments of S frames on --pack_streams (or 32) streams, and writes '
                             'each wav as its utterance finishes (DESIGN.md 3.6); 0: one closed run')
    parser.add_argument('--utterance_seed', type=int, default=-1,
                        help='S >= 0 (with --raw_output): utterance i of the SampleRNN vocoder draws with a seed of its own, '
                             'derived from S and i, in the rectangle, with --pack_streams and with --stream_frames alike: its '
                             'samples do not depend on where it was placed (DESIGN.md 3.6); -1: the plan\'s seed and the '
                             'stream key the draws')
    parser.add_argument('--draw_mode', type=str, default='sequential', choices=('sequential', 'scan'),
                        help="(with --raw_output) how the SampleRNN vocoder's draws at temperature > 0 find their code: "
                             "'sequential' walks the 256 codes in one lane (the samples of every earlier version); 'scan' is "
                             "the wave-parallel draw -- same uniforms, the CDF summed as a fixed tree: faster, and a few "
                             "draws per ten thousand land on the neighbouring code (DESIGN.md 3.6)")
    parser.add_argument('--top_k', type=int, default=0,
                        help="K > 0 (with --raw_output): the SampleRNN vocoder's draws at temperature > 0 are taken among the "
                             "K most likely of the 256 codes (ties at the cut-off go to the lower code), in both draw modes; "
                             "0: among all of them (DESIGN.md 3.6)")
    parser.add_argument('--top_p', type=float, default=0.0,
                        help="P strictly between 0 and 1 (with --raw_output): the SampleRNN vocoder's draws at temperature > 0 "
                             "are taken among the nucleus -- the most likely codes (of those --top_k left) that together "
                             "hold P of the probability, ties at the cut-off to the lower code --, in both draw modes; 0 or "
                             ">= 1: no nucleus (DESIGN.md 3.6)")
    parser.add_argument('--min_p', type=float, default=0.0,
                        help="M in (0, 1] (with --raw_output): of the codes --top_k and --top_p left, the SampleRNN vocoder's "
                             "draws at temperature > 0 keep those at least M times as likely as the most likely code, in both "
                             "draw modes; 0: off (DESIGN.md 3.6)")
    parser.add_argument('--timing_coeffs', type=str, default=None,
                        help='comma-separated list of exactly --num_samples values: utterance i decodes with its own '
                             'speaking rate in place of --timing_coeff (Parrot.sample_model(timing_coeffs=..))')
    parser.add_argument('--sharpening_coeffs', type=str, default=None,
                        help='comma-separated list of exactly --num_samples values: utterance i decodes with its own window '
                             'sharpening in place of --sharpening_coeff')
    parser.add_argument('--sampling_biases', type=str, default=None,
                        help='comma-separated list of exactly --num_samples values (GMM head): utterance i samples with its '
                             'own bias in place of --sampling_bias')
    parser.add_argument('--mix_speakers', type=str, default='15,11',
                        help='A,B: the two speakers --mix blends, m * W[A] + (1 - m) * W[B] (the pair of sample.py:81-85)')
    parser.add_argument('--prime_frames', type=int, default=0,
                        help="N > 0: every test utterance is primed with its own first min(N, length) feature frames -- they "
                             "are fed back in place of the decoder's while they last, then it continues freely "
                             "(Parrot.sample_model(forced_frames=.., n_forced=..)); not with --phrase, whose text has no frames")
    parser.add_argument('--segment_frames', type=int, default=0,
                        help='F > 0: the decoder runs in segments of F frames on one resumable plan and hands each on as it '
                             'completes (Parrot.decode_segments; same feature files); --stop_at_end 1 then ends after the '
                             'segment in which the longest utterance ends; 0: one call for all --num_steps frames; not with '
                             '--sample_one_step')
    parser.add_argument('--stream_audio', type=int, default=0,
                        help='1 (a --raw_output experiment, with --segment_frames F and --stream_frames S): text to audio in '
                             'one stream -- every decoder segment is handed to the SampleRNN vocoder on the device as it '
                             'completes (Parrot.synthesize_segments), so the first audio is out after one decoder segment and '
                             'one vocoder segment; the same wav and feature files; composes with --pack_streams, '
                             '--utterance_seed, --draw_mode, --top_k, --top_p, --min_p and the per-utterance decode controls; '
                             'not with --sample_one_step; 0: decode everything, then the vocoder')
    parser.add_argument('--synthetic_examples', type=int, default=64)
    args = parser.parse_args(argv)
    if args.stream_audio not in (0, 1):
        raise SystemExit("--stream_audio %d: 0 or 1" % args.stream_audio)
    if args.stream_audio and args.sample_one_step:
        raise SystemExit("--stream_audio hands the segments of the free-running decode to the vocoder; --sample_one_step "
                         "decodes no such loop: give one of the two")
    if args.stream_audio and args.segment_frames < 1:
        raise SystemExit("--stream_audio needs --segment_frames F > 0: the decoder segments it hands to the vocoder")
    if args.stream_audio and args.stream_frames < 1:
        raise SystemExit("--stream_audio needs --stream_frames S > 0: the vocoder segments that take them")
    if args.dataset not in args.save_dir:
        args.save_dir = os.path.join(args.save_dir, args.dataset)
    if args.prime_frames < 0:
        raise SystemExit("--prime_frames %d: the number of frames cannot be negative" % args.prime_frames)
    if args.prime_frames and args.phrase is not None:
        raise SystemExit("--prime_frames primes each test utterance with its own feature frames; --phrase replaces the text, "
                         "and the frames would belong to other words: give one of the two")
    if args.prime_frames and args.sample_one_step:
        raise SystemExit("--prime_frames has no meaning with --sample_one_step, which forces every frame already")
    if args.segment_frames < 0:
        raise SystemExit("--segment_frames %d: the number of frames cannot be negative" % args.segment_frames)
    if args.segment_frames and args.sample_one_step:
        raise SystemExit("--segment_frames cuts the free-running decode into segments; --sample_one_step decodes no such loop: "
                         "give one of the two")
    for flag in ('timing_coeffs', 'sharpening_coeffs', 'sampling_biases'):
        if getattr(args, flag) is not None:
            setattr(args, flag, parse_float_list(getattr(args, flag), args.num_samples, '--' + flag))
    args.mix_speakers = parse_speaker_pair(args.mix_speakers)
    return args


def prime_frames(features, features_mask, count, num_steps):
    """--prime_frames: (forced_frames [P, N, O], n_forced [N]) from a batch's own time-major features [T, N, O] and mask
    [T, N]: utterance b is primed with its first min(count, its length) frames, P = min(count, T, num_steps)."""
    import numpy
    features, features_mask = numpy.asarray(features), numpy.asarray(features_mask)
    P = int(min(count, features.shape[0], num_steps))
    lengths = features_mask.sum(axis=0).astype('int64')
    return features[:P].astype('float32'), numpy.minimum(lengths, P).astype('int32')


def parse_float_list(text, count, flag):
    """'0.8,1,1.25' -> [0.8, 1.0, 1.25]; SystemExit naming both numbers unless there are exactly `count` values."""
    items = [x.strip() for x in str(text).split(',') if x.strip()]
    try:
        vals = [float(x) for x in items]
    except ValueError:
        raise SystemExit("%s: %r is not a comma-separated list of numbers" % (flag, text))
    if len(vals) != count:
        raise SystemExit("%s has %d values, --num_samples is %d: one value per utterance" % (flag, len(vals), count))
    return vals


def parse_speaker_pair(text):
    try:
        a, b = (int(x) for x in str(text).split(','))
    except ValueError:
        raise SystemExit("--mix_speakers: %r is not a pair of speaker indices A,B" % (text,))
    return a, b


def mix_speaker_weights(mix, pair, num_speakers, num_samples):
    """The blend of sample.py:81-85 as Parrot.sample_model's speaker_weights: every row mix * W[pair[0]] +
    (1 - mix) * W[pair[1]], float32 [num_samples, num_speakers].  The checkpoint's table stays as it is."""
    import numpy
    a, b = pair
    if not (0 <= a < num_speakers and 0 <= b < num_speakers):
        raise SystemExit("--mix_speakers %d,%d: the model has %d speakers" % (a, b, num_speakers))
    w = numpy.zeros((num_samples, num_speakers), dtype=numpy.float32)
    w[:, a] += numpy.float32(mix)
    w[:, b] += numpy.float32(1. - mix)
    return w


def phrase_labels(phrase, dataset, num_samples, data_path=None):
    """sample.py:68-76: the phrase's characters through $FUEL_DATA_PATH/<dataset>/char2code.pkl, tiled to num_samples rows,
    with a mask of ones.  SystemExit naming a missing file or an unknown character."""
    import pickle

    import numpy
    if data_path is None:
        data_path = os.environ.get('FUEL_DATA_PATH')
        if not data_path:
            raise SystemExit("--phrase needs FUEL_DATA_PATH: char2code.pkl is read from $FUEL_DATA_PATH/%s/" % dataset)
    path = os.path.join(data_path, dataset, 'char2code.pkl')
    if not os.path.isfile(path):
        raise SystemExit("--phrase: %s not found (the dataset's own character table)" % path)
    with open(path, 'rb') as f:
        char2code = pickle.load(f)
    for ch in phrase:
        if ch not in char2code:
            raise SystemExit("--phrase: character %r is not in %s" % (ch, path))
    labels = numpy.array([char2code[ch] for ch in phrase], dtype='int32')
    labels = numpy.tile(labels, (num_samples, 1))
    return labels, numpy.ones(labels.shape, dtype='float32')


def end_of_utterance(phi, labels_length, num_steps, extra=40):
    """sample.py:145-163: first step whose window weight on the position just past the text exceeds the
    weight on every real character, plus `extra` frames; num_steps if never."""
    import numpy
    try:
        t = numpy.where((phi[:, labels_length, numpy.newaxis] > phi[:, :labels_length - 1]).all(axis=1))[0][0]
        return int(numpy.minimum(num_steps, t + extra))
    except Exception:
        return int(num_steps)


def end_of_utterance_args(labels_mask, U):
    """The two indices per row that the decode kernel's end-of-utterance rule takes (Parrot.sample_until_end_device), built
    from labels_mask exactly as sample.py and end_of_utterance do, Python slicing included: the rule compares
    phi[:, pos] with phi[:, :pos - 1], and for pos = 0 the slice [:-1] is all but the LAST position.  Returns (pos, ncmp),
    int32 arrays [N]: the row fires at the first step with phi[pos] > phi[j] for every j < ncmp."""
    import numpy
    mask = numpy.asarray(labels_mask)
    pos = numpy.zeros(mask.shape[0], dtype=numpy.int32)
    ncmp = numpy.zeros(mask.shape[0], dtype=numpy.int32)
    for i in range(mask.shape[0]):
        ll = int(mask[i].sum())
        pos[i] = min(ll, U - 1)
        ncmp[i] = pos[i] - 1 if pos[i] >= 1 else U - 1
    return pos, ncmp

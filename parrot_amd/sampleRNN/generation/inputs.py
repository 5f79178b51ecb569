"""What a generation plan is fed, computed on the host with numpy alone (no torch, no device): the seeded draw in Python
integers -- the hash sr_pick_kernel and srp_kernel key their uniforms with, a seed per utterance, the draw modes' names,
the checks of a top_k, a top_p and a min_p --
and where utterances go: into the streams of one packed plan (pack_utterances and the arrays of such a packing) and into
the segments of a plan that never ends (schedule_segment)."""
import numpy


def config():
    """The three_tier module, whose globals are the run configuration.  Looked up when called: configure() rebinds those
    globals between plans, and three_tier imports this package, so no module of it imports three_tier while loading."""
    from ..models.conditional import three_tier
    return three_tier


SKIP_SWITCH = "PARROT_SR_SKIP_STACKS"


def skip_stacks_enabled():
    """PARROT_SR_SKIP_STACKS (csrc/switches.h), read when called: 1 = the device-resident loop takes skip-connection
    stacks."""
    from ...utils import env_int
    return env_int(SKIP_SWITCH, 0) != 0


def stack_param_names(tier, rnn_type, n_rnn, skip_conn):
    """The reference's names of a tier's RNN stack ('BigFrameLevel' / 'FrameLevel'; ops.py:612-777, 823-989), no device:
    (layers, outskips, outskip_bias).  layers[k-1] = the Linear names (each has '.W0' and, under weight norm, '.g0') and the
    bias parameter of layer k: dict(input=, gates=, candidate= (GRU only), bias=) -- GRU: '<Input>.b', LSTM: '<Step>.b'.
    With skip_conn the layers above the first are '<tier>.GRU<k>+inpskip' / '<tier>.LSTM<k>+inpskip' (their Input is
    [2 DIM, N]: h_{k-1} rows first, then the stack's input), outskips[k-1] = '<tier>.GRU.outskip<k>y' /
    '<tier>.LSTM<k>.outskip<k>y' and outskip_bias = the first one's '.b', the only one there is; without it outskips is
    empty and outskip_bias None."""
    if rnn_type not in ('GRU', 'LSTM'):
        raise ValueError("rnn_type must be 'GRU' or 'LSTM', got %r" % (rnn_type,))
    if skip_conn and n_rnn < 2:
        raise ValueError("a single-layer stack has no skip connections")
    lstm = rnn_type == 'LSTM'
    layers, outskips = [], []
    for k in range(1, int(n_rnn) + 1):
        step = '%s.%s%d%s.Step' % (tier, rnn_type, k, '+inpskip' if skip_conn and k > 1 else '')
        names = dict(input=step + '.Input', gates=step + '.Recurrent_Gates', bias=step + ('.b' if lstm else '.Input.b'))
        if not lstm:
            names['candidate'] = step + '.Recurrent_Candidate'
        layers.append(names)
        if skip_conn:
            outskips.append('%s.LSTM%d.outskip%dy' % (tier, k, k) if lstm else '%s.GRU.outskip%dy' % (tier, k))
    return layers, outskips, (outskips[0] + '.b' if skip_conn else None)


_M64 = (1 << 64) - 1
DRAW_K1, DRAW_K2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9
DRAW_MODES = {'sequential': 0, 'scan': 1}


def u64(seed):
    """A seed as the unsigned 64-bit integer the kernels see."""
    return int(seed) & _M64


def _splitmix64(x):
    """The splitmix64 finaliser, in Python integers masked to 64 bits."""
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & _M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def utterance_draw_u01(seed, n):
    """The uniform an utterance with seed `seed` draws at counter n = the sample's index in the utterance's own buffer,
    prefix included (the first generated sample has n = BIG_FRAME_SIZE): seed ^ K1 (n + 1) through the splitmix64
    finaliser; the top 24 bits plus one half, rounded to float32, times 2^-24.  What sr_pick_kernel and the pick of
    srp_kernel compute with per-utterance draws (samplernn_generate_set_utterance_draws); no stream term."""
    x = _splitmix64(u64(seed) ^ u64(DRAW_K1 * (int(n) + 1)))
    return float(numpy.float32(float(x >> 40) + 0.5)) / 2.0 ** 24


def utterance_seed(seed, index):
    """One 64-bit seed per utterance from a base seed: seed + K1 (index + 1) through the splitmix64 finaliser."""
    return _splitmix64(u64(u64(seed) + DRAW_K1 * (int(index) + 1)))


def _seed_image(seeds):
    """Unsigned 64-bit seeds (Python integers or any integer array) as their two's-complement int64 image."""
    flat = [u64(s) for s in numpy.asarray(seeds, dtype=object).reshape(-1)]
    return numpy.array(flat, dtype=numpy.uint64).reshape(numpy.shape(seeds)).view(numpy.int64)


def draw_mode_code(draw_mode):
    """SampleRnnGenDesc::draw_mode of a mode's name; ValueError on any other name (no device call)."""
    if draw_mode not in DRAW_MODES:
        raise ValueError("draw_mode must be one of %s, got %r" % (sorted(DRAW_MODES), draw_mode))
    return DRAW_MODES[draw_mode]


def top_k_code(top_k):
    """SampleRnnGenDesc::top_k of a plan's or an utterance's top_k: the int itself, 0 = no truncation; ValueError on a
    negative value or on anything that is not an integer (no device call)."""
    if isinstance(top_k, bool) or not isinstance(top_k, (int, numpy.integer)):
        raise ValueError("top_k must be an integer >= 0 (0: no truncation), got %r" % (top_k,))
    if top_k < 0:
        raise ValueError("top_k must be >= 0 (0: no truncation), got %d" % top_k)
    return min(int(top_k), 2 ** 31 - 1)


def top_k_array(top_ks, shape):
    """Per-utterance top_k values as the int32 array of `shape` a plan is fed: ValueError on another shape, a negative
    value or a non-integer array (no device call).  Values >= Q_LEVELS mean no truncation, like 0."""
    a = numpy.asarray(top_ks)
    if a.dtype.kind not in 'iu' or a.shape != tuple(shape):
        raise ValueError("top_ks must be integers of shape %s, got %s of %s" % (list(shape), a.dtype, list(a.shape)))
    if a.size and a.min() < 0:
        raise ValueError("top_ks must be >= 0 (0: no truncation)")
    return numpy.minimum(a, 2 ** 31 - 1).astype(numpy.int32)


def _per_utterance_top_k(top_ks, n, default_top_k):
    """top_ks: one per utterance or a scalar; None = default_top_k for all."""
    if top_ks is None:
        top_ks = default_top_k
    top_ks = [top_ks] * n if numpy.ndim(top_ks) == 0 else list(top_ks)
    if len(top_ks) != n:
        raise ValueError("%d utterances, but %d top_ks" % (n, len(top_ks)))
    return [top_k_code(k) for k in top_ks]


_TINY32 = float(numpy.finfo(numpy.float32).tiny)


def top_p_code(top_p):
    """The float a plan or an utterance is handed as its top_p (samplernn_generate_set_top_p): 0.0 or >= 1.0 = no nucleus,
    strictly between = active; ValueError on a negative value, a NaN or anything that is not a real number (no device
    call)."""
    if isinstance(top_p, bool) or not isinstance(top_p, (int, float, numpy.integer, numpy.floating)):
        raise ValueError("top_p must be a number in [0, 1] (0 or 1: no nucleus), got %r" % (top_p,))
    if not top_p >= 0:
        raise ValueError("top_p must be >= 0 and not NaN (0 or >= 1: no nucleus), got %r" % (top_p,))
    # (as the float32 the device sees; a positive value below float32's normal range stays active: it keeps the argmax)
    p = float(numpy.float32(min(float(top_p), 2.0)))
    return max(p, _TINY32) if top_p > 0 else 0.0


def top_p_active(top_p):
    """Whether a checked top_p truncates: strictly between 0 and 1 as the float32 the device sees."""
    return 0.0 < top_p_code(top_p) < 1.0


def top_p_array(top_ps, shape):
    """Per-utterance top_p values as the float32 array of `shape` a plan is fed: ValueError on another shape, a negative
    value, a NaN or a non-numeric array (no device call).  Values >= 1 mean no nucleus, like 0."""
    a = numpy.asarray(top_ps)
    if a.dtype.kind not in 'iuf' or a.shape != tuple(shape):
        raise ValueError("top_ps must be numbers of shape %s, got %s of %s" % (list(shape), a.dtype, list(a.shape)))
    if a.size and not bool(numpy.all(a >= 0)):
        raise ValueError("top_ps must be >= 0 and not NaN (0 or >= 1: no nucleus)")
    a = a.astype(numpy.float64)
    return numpy.where(a > 0, numpy.clip(a, _TINY32, 2.0), 0.0).astype(numpy.float32)


def _per_utterance_top_p(top_ps, n, default_top_p):
    """top_ps: one per utterance or a scalar; None = default_top_p for all."""
    if top_ps is None:
        top_ps = default_top_p
    top_ps = [top_ps] * n if numpy.ndim(top_ps) == 0 else list(top_ps)
    if len(top_ps) != n:
        raise ValueError("%d utterances, but %d top_ps" % (n, len(top_ps)))
    return [top_p_code(p) for p in top_ps]


def min_p_code(min_p):
    """The float a plan or an utterance is handed as its min_p (samplernn_generate_set_min_p): 0.0 = off, in (0, 1] = active
    (1.0 keeps the most likely codes only); ValueError on a negative value, a value above 1, a NaN or anything that is not a
    real number (no device call)."""
    if isinstance(min_p, bool) or not isinstance(min_p, (int, float, numpy.integer, numpy.floating)):
        raise ValueError("min_p must be a number in [0, 1] (0: off), got %r" % (min_p,))
    if not 0 <= min_p <= 1:
        raise ValueError("min_p must be in [0, 1] and not NaN (0: off), got %r" % (min_p,))
    # (as the float32 the device sees; a positive value below float32's normal range stays active: it keeps every code
    # whose term does not underflow)
    p = float(numpy.float32(float(min_p)))
    return max(p, _TINY32) if min_p > 0 else 0.0


def min_p_active(min_p):
    """Whether a checked min_p truncates: in (0, 1] as the float32 the device sees."""
    return 0.0 < min_p_code(min_p) <= 1.0


def min_p_array(min_ps, shape):
    """Per-utterance min_p values as the float32 array of `shape` a plan is fed: ValueError on another shape, a negative
    value, a value above 1, a NaN or a non-numeric array (no device call)."""
    a = numpy.asarray(min_ps)
    if a.dtype.kind not in 'iuf' or a.shape != tuple(shape):
        raise ValueError("min_ps must be numbers of shape %s, got %s of %s" % (list(shape), a.dtype, list(a.shape)))
    if a.size and not bool(numpy.all((a >= 0) & (a <= 1))):
        raise ValueError("min_ps must be in [0, 1] and not NaN (0: off)")
    a = a.astype(numpy.float64)
    return numpy.where(a > 0, numpy.clip(a, _TINY32, 1.0), 0.0).astype(numpy.float32)


def _per_utterance_min_p(min_ps, n, default_min_p):
    """min_ps: one per utterance or a scalar; None = default_min_p for all."""
    if min_ps is None:
        min_ps = default_min_p
    min_ps = [min_ps] * n if numpy.ndim(min_ps) == 0 else list(min_ps)
    if len(min_ps) != n:
        raise ValueError("%d utterances, but %d min_ps" % (n, len(min_ps)))
    return [min_p_code(p) for p in min_ps]


def _per_utterance(seeds, temperatures, n, default_temperature):
    """seeds: one per utterance; temperatures: one per utterance, a scalar, or None = default_temperature."""
    seeds = [u64(s) for s in seeds]
    if temperatures is None:
        temperatures = default_temperature
    temperatures = [float(temperatures)] * n if numpy.ndim(temperatures) == 0 else [float(t) for t in temperatures]
    if len(seeds) != n or len(temperatures) != n:
        raise ValueError("%d utterances, but %d seeds and %d temperatures" % (n, len(seeds), len(temperatures)))
    return seeds, temperatures



def pack_utterances(lengths, n_streams):
    """Places utterances of `lengths[i]` big frames one after the other into `n_streams` streams: longest first onto the
    least-loaded stream (ties: the lower utterance index first, the lower stream index).  Returns (stream, first_slot, T):
    utterance i occupies slots first_slot[i] .. first_slot[i] + lengths[i] - 1 of stream[i]; T = max(2, the longest
    stream) is the frame count of the plan that runs them.  Pure Python and deterministic."""
    lengths = [int(n) for n in lengths]
    n_streams = int(n_streams)
    if n_streams < 1:
        raise ValueError("n_streams must be at least 1")
    if any(n < 1 for n in lengths):
        raise ValueError("every utterance needs at least one frame (its prefix slot)")
    load = [0] * n_streams
    stream, first_slot = [0] * len(lengths), [0] * len(lengths)
    for i in sorted(range(len(lengths)), key=lambda i: (-lengths[i], i)):
        b = min(range(n_streams), key=lambda b: (load[b], b))
        stream[i], first_slot[i] = b, load[b]
        load[b] += lengths[i]
    return stream, first_slot, max(2, max(load))


def start_row(first_slot, T):
    """The row of a plan of T slots that holds the start flag, the seed and the temperature of the utterance whose Q/2
    prefix is slot first_slot: the slot of its frame 1, where the generator overwrites the slot before with the prefix and
    restarts the stream's state.  None when that row is not below T: the prefix alone in the last slot draws nothing."""
    return first_slot + 1 if first_slot + 1 < T else None


def build_packed_inputs(utterances, stream, first_slot, T, n_streams):
    """(features [T, n_streams, 63] float32, starts [T, n_streams] int32) of a packing: utterance i's frame j at slot
    first_slot[i] + j of stream[i], zeros elsewhere; starts = 1 on every utterance's start_row."""
    feat_dim = numpy.asarray(utterances[0]).shape[1] if len(utterances) else config().FEAT_DIM
    features = numpy.zeros((T, n_streams, feat_dim), dtype='float32')
    starts = numpy.zeros((T, n_streams), dtype='int32')
    for u, b, s in zip(utterances, stream, first_slot):
        u = numpy.asarray(u, dtype='float32')
        if not (0 <= b < n_streams and 0 <= s and s + u.shape[0] <= T):
            raise ValueError("utterance of %d frames does not fit at slot %d of stream %d" % (u.shape[0], s, b))
        features[s:s + u.shape[0], b] = u
        row = start_row(s, T)
        if row is not None:
            starts[row, b] = 1
    return features, starts


def build_packed_draws(seeds, temperatures, stream, first_slot, T, n_streams):
    """(utt_seed [T, n_streams] uint64, utt_temp [T, n_streams] float32) of a packing, the sibling of build_packed_inputs:
    utterance i's seed and temperature on its start_row; zeros elsewhere."""
    utt_seed = numpy.zeros((T, n_streams), dtype=numpy.uint64)
    utt_temp = numpy.zeros((T, n_streams), dtype='float32')
    for sd, tp, b, s in zip(seeds, temperatures, stream, first_slot):
        if not (0 <= b < n_streams and 0 <= s < T):
            raise ValueError("no slot %d in stream %d" % (s, b))
        row = start_row(s, T)
        if row is not None:
            utt_seed[row, b], utt_temp[row, b] = u64(sd), tp
    return utt_seed, utt_temp


def build_packed_top_k(top_ks, stream, first_slot, T, n_streams):
    """utt_top_k [T, n_streams] int32 of a packing, the sibling of build_packed_draws: utterance i's top_k on its
    start_row; zeros (no truncation) elsewhere."""
    utt_top_k = numpy.zeros((T, n_streams), dtype=numpy.int32)
    for k, b, s in zip(top_ks, stream, first_slot):
        if not (0 <= b < n_streams and 0 <= s < T):
            raise ValueError("no slot %d in stream %d" % (s, b))
        row = start_row(s, T)
        if row is not None:
            utt_top_k[row, b] = top_k_code(k)
    return utt_top_k


def build_packed_top_p(top_ps, stream, first_slot, T, n_streams):
    """utt_top_p [T, n_streams] float32 of a packing, the sibling of build_packed_top_k: utterance i's top_p on its
    start_row; zeros (no nucleus) elsewhere."""
    utt_top_p = numpy.zeros((T, n_streams), dtype=numpy.float32)
    for p_, b, s in zip(top_ps, stream, first_slot):
        if not (0 <= b < n_streams and 0 <= s < T):
            raise ValueError("no slot %d in stream %d" % (s, b))
        row = start_row(s, T)
        if row is not None:
            utt_top_p[row, b] = top_p_code(p_)
    return utt_top_p


FREE = -1  # in a forced array: the step picks freely


def forced_array(forced, shape):
    """Forced samples as the int32 array of `shape` a plan is fed (samplernn_generate_set_forced): ValueError on another
    shape, a non-integer array or a value that is neither -1 (free) nor a code in 0 .. Q_LEVELS-1 (no device call)."""
    a = numpy.asarray(forced)
    if a.dtype.kind not in 'iu' or a.shape != tuple(shape):
        raise ValueError("forced must be integers of shape %s, got %s of %s" % (list(shape), a.dtype, list(a.shape)))
    Q = config().Q_LEVELS
    if a.size and (a.min() < FREE or a.max() >= Q):
        raise ValueError("forced values must be -1 (free) or codes in 0 .. %d" % (Q - 1))
    return a.astype(numpy.int32)


def _per_utterance_prompts(prompts, lengths):
    """prompts: per utterance None or an integer array of at most 80 * (n_i - 1) codes in 0 .. Q_LEVELS-1; None = no prompt
    for anybody.  Returns one int32 array per utterance (empty: no prompt).  ValueError otherwise (no device call)."""
    tt = config()
    n = len(lengths)
    prompts = [None] * n if prompts is None else list(prompts)
    if len(prompts) != n:
        raise ValueError("%d utterances, but %d prompts" % (n, len(prompts)))
    out = []
    for p, frames in zip(prompts, lengths):
        a = numpy.zeros(0, dtype=numpy.int32) if p is None else numpy.asarray(p)
        if a.ndim != 1 or (a.size and a.dtype.kind not in 'iu'):
            raise ValueError("a prompt is a one-dimensional integer array, got %s of %s" % (a.dtype, list(a.shape)))
        if a.size > tt.BIG_FRAME_SIZE * (int(frames) - 1):
            raise ValueError("a prompt of %d codes is longer than the %d samples its utterance of %d frames generates"
                             % (a.size, tt.BIG_FRAME_SIZE * (int(frames) - 1), frames))
        if a.size and (a.min() < 0 or a.max() >= tt.Q_LEVELS):
            raise ValueError("prompt codes must lie in 0 .. %d" % (tt.Q_LEVELS - 1))
        out.append(a.astype(numpy.int32))
    return out


def build_packed_prompts(prompts, lengths, stream, first_slot, T, n_streams):
    """forced [n_streams, 80 T] int32 of a packing, the counterpart of build_packed_inputs on the sample grid: code j of
    utterance i's prompt at sample 80 + j of its own buffer, i.e. column 80 (first_slot[i] + 1) + j of stream[i]; -1 (free)
    everywhere else -- prefix slots and idle slots included.  unpack_samples cuts it back into the utterances' pieces."""
    BFS = config().BIG_FRAME_SIZE
    forced = numpy.full((n_streams, BFS * T), FREE, dtype=numpy.int32)
    for p, n, b, s in zip(_per_utterance_prompts(prompts, lengths), lengths, stream, first_slot):
        if not (0 <= b < n_streams and 0 <= s and s + n <= T):
            raise ValueError("utterance of %d frames does not fit at slot %d of stream %d" % (n, s, b))
        forced[b, BFS * (s + 1):BFS * (s + 1) + p.size] = p
    return forced


def unpack_log_probs(logp, lengths, stream, first_slot, dtype='float32'):
    """The utterances' pieces of a packed run's log-probabilities [B, 80 T]: per utterance the float32 values of its samples
    80 .. 80 n_i - 1 (the prefix slot has none).  (Any per-step array is cut this way: dtype='int32' for the kept counts.)"""
    BFS = config().BIG_FRAME_SIZE
    return [numpy.array(logp[b, BFS * (s + 1):BFS * (s + n)], dtype=dtype) for n, b, s in zip(lengths, stream, first_slot)]


def build_packed_min_p(min_ps, stream, first_slot, T, n_streams):
    """utt_min_p [T, n_streams] float32 of a packing, the sibling of build_packed_top_p: utterance i's min_p on its
    start_row; zeros (off) elsewhere."""
    utt_min_p = numpy.zeros((T, n_streams), dtype=numpy.float32)
    for p_, b, s in zip(min_ps, stream, first_slot):
        if not (0 <= b < n_streams and 0 <= s < T):
            raise ValueError("no slot %d in stream %d" % (s, b))
        row = start_row(s, T)
        if row is not None:
            utt_min_p[row, b] = min_p_code(p_)
    return utt_min_p


def unpack_samples(samples, lengths, stream, first_slot):
    """The utterances' pieces of a packed run's samples [B, 80 T].  (The prefix of a one-frame utterance in the last slot
    of the plan has no period behind it that would write it: it is Q/2 by definition.)"""
    tt = config()
    BFS = tt.BIG_FRAME_SIZE
    T = samples.shape[1] // BFS
    out = []
    for n, b, s in zip(lengths, stream, first_slot):
        piece = numpy.array(samples[b, BFS * s:BFS * (s + n)], dtype='int32')
        if start_row(s, T) is None:
            piece[:BFS] = tt.Q_ZERO
        out.append(piece)
    return out


def schedule_segment(running, queue, n_streams, segment_frames):
    """One segment of continuous admission (StreamingGenerator): which utterance takes which slots 1 .. segment_frames of
    which stream.  Pure Python and deterministic; the arguments are not changed.

    running[b] = None or (ticket, placed, length): stream b's utterance and how many of its `length` frames earlier
    segments have placed (>= 1; its last one is the ring's slot 0).  queue = [(ticket, length), ...], oldest first.
    The rules: a stream goes on with its utterance from slot 1; when that ends at slot k < segment_frames (k = 0: the
    stream was idle) a queued utterance may begin at slot k + 1 of the same stream -- that slot is its Q/2 prefix, its
    start flag is on the slot of its frame 1, in this segment or at slot 1 of the next.  The queue is FIFO: its oldest
    utterance takes the earliest free slot of any stream (the lower stream index among equals), until no stream has a
    free slot or the queue is empty.

    Returns (placements, starts, n_slots, running', queue'): placements = [(ticket, stream, slot, frame, count)] --
    frames frame .. frame + count - 1 of the utterance at slots slot .. slot + count - 1 --, starts = [(slot, stream)],
    n_slots = the busiest stream's last slot (the periods the segment runs: no period with every stream idle; 0 = nothing to
    run).  Whenever an utterance is left unfinished it has reached slot segment_frames = n_slots, so its next frame is
    slot 1 of the next segment."""
    B, S = int(n_streams), int(segment_frames)
    if B < 1:
        raise ValueError("n_streams must be at least 1")
    if S < 1:
        raise ValueError("segment_frames must be at least 1")
    running = list(running)
    if len(running) != B:
        raise ValueError("running must hold one entry per stream")
    queue = [(t, int(n)) for t, n in queue]
    placements = []
    free = [1] * B  # the stream's first slot nobody has taken yet

    def place(b, ticket, placed, length):
        count = min(length - placed, S - free[b] + 1)
        placements.append((ticket, b, free[b], placed, count))
        free[b] += count
        running[b] = (ticket, placed + count, length) if placed + count < length else None

    for b in range(B):
        if running[b] is not None:
            place(b, *running[b])
    while queue:
        b = min(range(B), key=lambda b: (free[b], b))
        if free[b] > S or running[b] is not None:  # (a stream whose utterance goes on is full: free = S + 1)
            break
        ticket, length = queue.pop(0)
        if length < 1:
            raise ValueError("every utterance needs at least one frame (its prefix slot)")
        place(b, ticket, 0, length)
    placements.sort(key=lambda x: (x[1], x[2]))
    starts = [(slot + 1 - frame, b) for _, b, slot, frame, count in placements if frame <= 1 < frame + count]
    n_slots = max(free) - 1
    return placements, starts, n_slots, running, queue

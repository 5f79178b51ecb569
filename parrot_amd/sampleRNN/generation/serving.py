"""Entry points on top of the device plan: a list of utterances packed into one run (generate_packed), a rectangle in
segments on a ring (generate_stream) and continuous admission on a plan that never ends (StreamingGenerator)."""
import numpy
import torch

from .device import DeviceGenerator, device_loop_guard
from .inputs import (FREE, _per_utterance, _per_utterance_min_p, _per_utterance_prompts, _per_utterance_top_k,
                     _per_utterance_top_p, build_packed_draws, build_packed_inputs, build_packed_min_p, build_packed_prompts,
                     build_packed_top_k, build_packed_top_p, config, min_p_code, pack_utterances, schedule_segment, start_row,
                     top_k_code, top_p_code, u64, unpack_log_probs, unpack_samples)


def generate_packed(utterances, n_streams=32, temperature=1.0, seed=234, use_graph=True, seeds=None,
                    temperatures=None, draw_mode='sequential', top_k=0, top_ks=None, top_p=0.0, top_ps=None, prompts=None,
                    log_probs=False, min_p=0.0, min_ps=None, draw_stats=False):
    """Generates a list of utterances ([n_i, 63] conditioning frames each) on `n_streams` streams of ONE plan, several
    utterances one after the other per stream (pack_utterances), instead of one rectangle of max(n_i) frames per
    n_streams utterances.  Returns a list of int32 arrays [80 * n_i], the Q/2 prefix included.

    At temperature = 0 element i equals what DeviceGenerator returns for that utterance generated on its own.  At
    temperature > 0 without `seeds` the draws are seeded and repeatable, but they are keyed by the packed (sample index,
    stream) of the run, so they are NOT the draws of the utterance's standalone run.

    seeds = one unsigned 64-bit seed per utterance (temperatures = one temperature per utterance or a scalar; default:
    `temperature` for all): the plan runs with per-utterance draws (DeviceGenerator(utterance_draws=True)).  Element i is
    then a function of the model, the plan's shape (n_streams), the carrying stream, and the utterance's features, seed
    and temperature: it equals, bit for bit, what a plain plan of n_streams streams in that mode returns for the utterance
    carried alone in the same stream with the same seed and temperature, and does not depend on its slot, the order of
    the list or its neighbours.  (The carrying stream is pack_utterances' choice, which does depend on the list.)

    draw_mode: 'sequential' or 'scan', see DeviceGenerator.  (temperature's default: three_tier.TEMPERATURE as imported.)

    top_k: the draws at temperature > 0 are taken among the k most likely codes (0: among all; see DeviceGenerator).
    top_ks = one top_k per utterance (needs `seeds`; default: `top_k` for all).

    top_p: those draws are taken among the nucleus of the codes top_k left (0 or >= 1: no nucleus; see DeviceGenerator).
    top_ps = one top_p per utterance (needs `seeds`; default: `top_p` for all).

    min_p: of the codes both left, those draws keep the ones at least min_p times as likely as the most likely code (0: off;
    in (0, 1]; see DeviceGenerator).  min_ps = one min_p per utterance (needs `seeds`; default: `min_p` for all).

    prompts = per utterance None or an integer array of at most 80 * (n_i - 1) codes in 0 .. Q_LEVELS-1: code j is sample
    80 + j of that utterance's own buffer, whatever the model would have picked there (DeviceGenerator(forcing=True)); the
    utterance goes on freely behind its prompt, drawing with the uniforms of its own sample indices.  A longer prompt, a
    non-integer array or another value: ValueError, before a plan is created.

    log_probs=True: returns (samples_list, logp_list), logp_list[i] = float32 [80 * (n_i - 1)], the natural logarithm of the
    model's probability (temperature 1, no truncation) of samples 80 .. of utterance i (DeviceGenerator(log_probs=True)).

    draw_stats=True: two more lists behind (samples_list[, logp_list]), draw_logp_list[i] float32 and kept_list[i] int32, both
    [80 * (n_i - 1)] and cut like logp_list: what each of utterance i's steps drew from (DeviceGenerator(draw_stats=True))."""
    device_loop_guard(draw_mode, top_k, top_p, min_p)
    utterances = [numpy.asarray(u, dtype='float32') for u in utterances]
    lengths = [u.shape[0] for u in utterances]
    if prompts is not None:  # (before a plan is created)
        prompts = _per_utterance_prompts(prompts, lengths)
    if seeds is None and temperatures is not None:
        raise ValueError("temperatures per utterance need seeds per utterance")
    if seeds is None and top_ks is not None:
        raise ValueError("top_ks per utterance need seeds per utterance")
    if seeds is None and top_ps is not None:
        raise ValueError("top_ps per utterance need seeds per utterance")
    if seeds is None and min_ps is not None:
        raise ValueError("min_ps per utterance need seeds per utterance")
    if seeds is not None:  # (before a plan is created)
        seeds, temperatures = _per_utterance(seeds, temperatures, len(utterances), temperature)
        top_ks = _per_utterance_top_k(top_ks, len(utterances), top_k)
        top_ps = _per_utterance_top_p(top_ps, len(utterances), top_p)
        min_ps = _per_utterance_min_p(min_ps, len(utterances), min_p)
    if not utterances:
        return ([],) * (1 + bool(log_probs) + 2 * bool(draw_stats)) if log_probs or draw_stats else []
    stream, first_slot, T = pack_utterances(lengths, n_streams)
    features, starts = build_packed_inputs(utterances, stream, first_slot, T, n_streams)
    gen = DeviceGenerator(n_streams, T, temperature=temperature, seed=seed, use_graph=use_graph, packed=True,
                          utterance_draws=seeds is not None, draw_mode=draw_mode, top_k=top_k, top_p=top_p,
                          forcing=prompts is not None, log_probs=log_probs, min_p=min_p, draw_stats=draw_stats)
    try:
        draws = {}
        if seeds is not None:
            draws['seeds'], draws['temperatures'] = build_packed_draws(seeds, temperatures, stream, first_slot, T, n_streams)
            draws['top_ks'] = build_packed_top_k(top_ks, stream, first_slot, T, n_streams)
            draws['top_ps'] = build_packed_top_p(top_ps, stream, first_slot, T, n_streams)
            draws['min_ps'] = build_packed_min_p(min_ps, stream, first_slot, T, n_streams)
        if prompts is not None:
            draws['forced'] = build_packed_prompts(prompts, lengths, stream, first_slot, T, n_streams)
        out = gen.generate(features, starts, **draws)
        out = [o.cpu().numpy() for o in (out if isinstance(out, tuple) else (out,))]
    finally:
        gen.close()
    # (the per-step arrays behind the samples are all cut as the log-probabilities are)
    res = (unpack_samples(out[0], lengths, stream, first_slot),) + \
        tuple(unpack_log_probs(o, lengths, stream, first_slot, dtype=o.dtype) for o in out[1:])
    return res if len(res) > 1 else res[0]


def score_utterances(utterances, samples, n_streams=32):
    """Log-probabilities of given audio under the model, at generation speed: generate_packed with every sample forced and
    log_probs=True.  utterances = [n_i, 63] conditioning frames each, samples = per utterance the integer codes [80 * n_i] of
    its buffer, prefix slot included (its 80 values are not looked at), or the [80 * (n_i - 1)] codes behind it.  Returns,
    per utterance, the float32 array of the natural log-probabilities of samples 80 ..; minus their mean times log2(e) is
    the bits per sample compute_cost reports."""
    BFS = config().BIG_FRAME_SIZE
    utterances = [numpy.asarray(u, dtype='float32') for u in utterances]
    samples = list(samples)
    if len(samples) != len(utterances):
        raise ValueError("%d utterances, but %d sample arrays" % (len(utterances), len(samples)))
    prompts = []
    for u, s in zip(utterances, samples):
        s = numpy.asarray(s)
        gen_len = BFS * (u.shape[0] - 1)
        if s.ndim != 1 or s.shape[0] not in (gen_len, gen_len + BFS):
            raise ValueError("an utterance of %d frames is scored on %d samples (or %d with its prefix slot), got %s"
                             % (u.shape[0], gen_len, gen_len + BFS, list(s.shape)))
        prompts.append(s[s.shape[0] - gen_len:])
    return generate_packed(utterances, n_streams=n_streams, temperature=0.0, prompts=prompts, log_probs=True)[1]


def generate_stream(features, segment_frames, temperature=1.0, seed=234, use_graph=True, gen=None, draw_mode='sequential',
                    top_k=0, top_p=0.0, min_p=0.0):
    """Generator over a rectangle features [N, B, 63] on a plan of segment_frames + 1 slots used as a ring: yields int32
    arrays [B, 80 n] -- the first one holds the Q/2 prefix and up to segment_frames frames, every later one up to
    segment_frames frames -- whose concatenation is the [B, 80 N] result of DeviceGenerator(B, N).generate(features), bit
    for bit, seeded draws included.  The plan does not grow with N, and the first samples are out after segment_frames
    periods.  gen: a plain DeviceGenerator(B, segment_frames + 1) of the caller's to run on (it is left open; temperature,
    seed, use_graph, draw_mode, top_k, top_p and min_p are then the plan's); default: a plan of its own for this call, with
    draw_mode 'sequential' or 'scan', top_k, top_p and min_p (see DeviceGenerator) and temperature's default as in
    generate_packed."""
    device_loop_guard(draw_mode, top_k, top_p, min_p)
    features = numpy.asarray(features, dtype='float32')
    S = int(segment_frames)
    if S < 1:
        raise ValueError("segment_frames must be at least 1")
    if features.ndim != 3 or features.shape[0] < 2:
        raise ValueError("features must be [N, B, %d] with N >= 2 (the prefix slot and one frame)" % config().FEAT_DIM)
    N, B = features.shape[0], features.shape[1]
    own = gen is None
    if own:
        gen = DeviceGenerator(B, S + 1, temperature=temperature, seed=seed, use_graph=use_graph, draw_mode=draw_mode,
                              top_k=top_k, top_p=top_p, min_p=min_p)
    elif gen.packed or (gen.B, gen.T) != (B, S + 1):
        raise ValueError("gen must be a plain plan of %d streams and %d slots" % (B, S + 1))
    try:
        k = min(S, N - 1)
        yield gen.generate(features[:k + 1], n_frames=k).cpu().numpy()
        done = k + 1
        while done < N:
            k = min(S, N - done)
            yield gen.generate(features[done:done + k], resume=True, n_frames=k).cpu().numpy()
            done += k
    finally:
        if own:
            gen.close()


class StreamingGenerator:
    """Continuous admission on ONE packed plan of segment_frames + 1 slots that never ends: utterances are submitted at any
    time, every step() runs one segment of the ring (schedule_segment decides who takes which slots) and hands out the
    samples of every utterance that had slots in it.

    The first 80 samples of an utterance's first chunk are its Q/2 prefix.  At temperature = 0 the concatenated chunks of
    an utterance equal what a plain plan of n_streams returns for it carried in the same stream (record[ticket] =
    (stream, absolute slot of its prefix)); at temperature > 0 without utterance_draws the draws are repeatable for the
    same sequence of submit / step calls, but they are not the draws of the utterance's standalone run.

    utterance_draws=True: submit takes the utterance's seed (required) and temperature (default: the generator's).  The
    concatenated chunks of an utterance are then a function of the model, the plan's shape (n_streams; segment_frames does
    not enter), the carrying stream, and the utterance's features, seed and temperature: they equal, bit for bit, what a
    plain plan of n_streams streams in that mode returns for the utterance carried alone in stream record[ticket][0] with
    the same seed and temperature, and do not depend on its slot, the segment boundaries, the submission order or its
    neighbours.  (Which stream carries it is schedule_segment's choice, and that does depend on the traffic.)

    run_segment(features [n, B, 63], starts [n, B], resume) -> samples [B, 80 n] of slots 1 .. n is the callable that
    runs a segment; the default runs it on the device.  With utterance_draws it is called with two more keyword arguments,
    seeds [n, B] uint64 and temperatures [n, B] float32: what the utterance whose start flag is on that row draws with.

    draw_mode: 'sequential' or 'scan', the plan's (see DeviceGenerator); a run_segment of the caller's does not see it.

    top_k: the plan's truncation (see DeviceGenerator), what every utterance draws with unless submit(..., top_k=) names
    its own (utterance_draws=True only).  A generator that truncates -- its top_k is non-zero, or some utterance was
    submitted with one -- calls run_segment with one more keyword argument, top_ks [n, B] int32: the top_k of the utterance
    whose start flag is on that row, zeros elsewhere.  A generator that does not calls it exactly as before.

    top_p: the plan's nucleus (see DeviceGenerator), what every utterance draws with unless submit(..., top_p=) names its
    own (utterance_draws=True only).  Likewise, a generator that uses nucleus truncation -- its top_p is active, or some
    utterance was submitted with one -- calls run_segment with one more keyword argument, top_ps [n, B] float32; a
    generator that does not never passes it.

    min_p: the plan's min-p bar (see DeviceGenerator), what every utterance draws with unless submit(..., min_p=) names its
    own (utterance_draws=True only).  Likewise, a generator that uses it -- its min_p is active, or some utterance was
    submitted with one -- calls run_segment with one more keyword argument, min_ps [n, B] float32; a generator that does
    not never passes it.

    Prompts: submit(..., prompt=) primes an utterance with up to 80 * (n - 1) codes, the samples 80 .. of its own buffer;
    the prompt is cut across segment boundaries as the features are and may end mid-frame.  From the first utterance
    submitted with a prompt on, run_segment is called with one more keyword argument, forced [B, 80 n] int32, aligned with
    the samples it returns: the code of each forced sample, -1 where the step picks freely (prefix slots and idle slots
    included).  log_probs=True: run_segment must return (samples, logp), logp [B, 80 n] float32, and step() hands out
    (ticket, chunk, logp_chunk, done) -- logp_chunk aligned with chunk, zeros on the prefix slot.  A generator in which no
    utterance has a prompt and log_probs is off calls run_segment exactly as before.  forcing=True builds the generator's own
    device plan so that it takes prompts (DeviceGenerator(forcing=True)), which a plan cannot learn once it has run: on the
    device, submit refuses a prompt without it; a plan built without it runs the kernels it always ran.

    open_utterances=True: utterances whose frames arrive while they run.  open(...) -> ticket opens one, feed(ticket,
    frames [k, 63], last=False) appends frames (a numpy array is uploaded once, at feed time; a float32 tensor on the plan's
    device, row stride 63 or 64, stays there), last=True or close(ticket) ends it; submit(features, ...) is open, one feed
    and the close.  The frames live in a store of the generator's, on the plan's device: store_utterances rows (default:
    2 n_streams) of max_frames frames of 64 floats; an utterance holds a row from open() until it is reported done, open()
    raises RuntimeError while none is free (free_rows) and feed ValueError when the row would overflow.  step() hands the
    plan an index table into the store (DeviceGenerator.generate(gather=)), so no frame visits the host; a run_segment of
    the caller's gets the gathered host array, as before.  Prompts and log_probs are for submit only.  The schedule:
      1. no slot runs a frame that has not been fed;
      2. a stream never idles inside an utterance: a segment is cut to the frames every unfinished open utterance placed
         in it can supply, and while some running open utterance has nothing new no segment runs -- step() returns [] (or
         only the reports of rule 5) and `starved` says why (None after a step that was not starved);
      3. an utterance is placed only once its frame 0, the prefix slot, has been fed (a later one that has it goes first);
      4. when every utterance is closed before its first placement the placements are schedule_segment's;
      5. an utterance closed after all its frames were placed is reported done by the next step() with an empty chunk;
      6. once every open utterance is closed drain() terminates (while one starves it raises RuntimeError).
    It is schedule_segment on a shortened segment, with the length of an utterance whose end is unknown one past what has
    been fed.  At temperature 0, or with utterance_draws=True, the concatenated chunks of an utterance are bit for bit those
    of submit() of its whole features, whatever the feeds were and whenever they came."""

    def __init__(self, n_streams, segment_frames, temperature=0.0, seed=234, use_graph=True, run_segment=None,
                 utterance_draws=False, draw_mode='sequential', top_k=0, top_p=0.0, log_probs=False, forcing=False,
                 min_p=0.0, open_utterances=False, max_frames=1024, store_utterances=None):
        device_loop_guard(draw_mode, top_k, top_p, min_p)
        self.open_utterances = bool(open_utterances)
        if self.open_utterances:
            self.max_frames = int(max_frames)
            n_rows = 2 * int(n_streams) if store_utterances is None else int(store_utterances)
            if self.max_frames < 1 or n_rows < 1:
                raise ValueError("max_frames and store_utterances must be at least 1")
        self.log_probs = bool(log_probs)
        self.forcing = bool(forcing)   # the generator's own device plan takes prompts (a runner of the caller's always may)
        self._forcing = False          # some utterance was submitted with a prompt
        self.top_k = top_k_code(top_k)
        self._truncates = self.top_k != 0
        self.top_p = top_p_code(top_p)
        self._nucleus = 0.0 < self.top_p < 1.0
        self.min_p = min_p_code(min_p)
        self._min_p = self.min_p > 0.0
        self.B, self.S = int(n_streams), int(segment_frames)
        if self.B < 1:
            raise ValueError("n_streams must be at least 1")
        if self.S < 1:
            raise ValueError("segment_frames must be at least 1")
        self.gen = None
        self.utterance_draws = bool(utterance_draws)
        self.temperature = float(temperature)
        if run_segment is None:
            self.gen = DeviceGenerator(self.B, self.S + 1, temperature=temperature, seed=seed, use_graph=use_graph,
                                       packed=True, utterance_draws=self.utterance_draws, draw_mode=draw_mode,
                                       top_k=self.top_k, top_p=self.top_p, forcing=self.forcing, log_probs=self.log_probs,
                                       min_p=self.min_p)
            run_segment = self._run_on_device
        self._run = run_segment
        self._resume = False
        self._next_ticket = 0
        self._slots_run = 0            # periods run so far: slot s of this segment is absolute slot _slots_run + s
        self.running = [None] * self.B
        self.queue = []
        self._features = {}
        self._draws = {}               # ticket -> (seed, temperature), until the utterance's start flag has been placed
        self._top_ks = {}              # ticket -> top_k, likewise (utterance_draws only)
        self._top_ps = {}              # ticket -> top_p, likewise
        self._min_ps = {}              # ticket -> min_p, likewise
        self._prompts = {}             # ticket -> its prompt, until the utterance is done
        self.record = {}
        self._starved = None
        if self.open_utterances:
            # the frame store, [store row * max_frames + frame][64]: on the plan's device, or on the host for a runner of
            # the caller's; ticket -> {row, fed, closed} from open() until the utterance is reported done
            if self.gen is not None:
                self._store = torch.zeros(n_rows * self.max_frames, 64, device=self.gen.ws['features'].device)
            else:
                self._store = numpy.zeros((n_rows * self.max_frames, 64), dtype='float32')
            self._free_rows = list(range(n_rows))
            self._open = {}

    @property
    def starved(self):
        """Why the last step() ran no segment although utterances are waiting (a string), or None."""
        return self._starved

    @property
    def free_rows(self):
        """Store rows no utterance holds: how many more open() will take (open_utterances=True)."""
        return len(self._free_rows) if self.open_utterances else 0

    def _run_on_device(self, features, starts, resume, seeds=None, temperatures=None, top_ks=None, top_ps=None, forced=None,
                       min_ps=None, index=None):
        # (without utterance_draws the plan has no entries: every utterance draws with the plan's top_k)
        draws = {} if seeds is None else dict(seeds=seeds, temperatures=temperatures)
        if seeds is not None and top_ks is not None:
            draws['top_ks'] = top_ks
        if seeds is not None and top_ps is not None:
            draws['top_ps'] = top_ps
        if seeds is not None and min_ps is not None:
            draws['min_ps'] = min_ps
        n, BFS = starts.shape[0], config().BIG_FRAME_SIZE
        # (a plan built to take forced samples is handed them in every call: all free until some utterance has a prompt)
        if self.forcing and forced is None:
            forced = numpy.full((self.B, BFS * n), FREE, dtype=numpy.int32)
        more = {} if forced is None else dict(forced=forced)
        host = lambda out, cut: tuple(o.cpu().numpy()[:, cut:] for o in out) if self.log_probs else out.cpu().numpy()[:, cut:]
        if index is not None:  # (open utterances: the frames are gathered from the store on the device; -1 = an idle slot)
            if not resume:
                index = numpy.concatenate([numpy.full_like(index[:1], -1), index])
            more['gather'] = (self._store, index)
        if resume:
            return host(self.gen.generate(features, starts, resume=True, n_frames=n, **more, **draws), 0)
        # the first segment: slot 0 is the run's prefix slot, no stream uses it
        if features is not None:
            features = numpy.concatenate([numpy.zeros_like(features[:1]), features])
        starts = numpy.concatenate([numpy.zeros_like(starts[:1]), starts])
        draws = {k: numpy.concatenate([numpy.zeros_like(v[:1]), v]) for k, v in draws.items()}
        if forced is not None:
            more['forced'] = numpy.concatenate([numpy.full((self.B, BFS), FREE, dtype=numpy.int32), forced], axis=1)
        return host(self.gen.generate(features, starts, n_frames=n, **more, **draws), BFS)

    def _check_draws(self, seed, temperature, top_k, top_p, min_p):
        """What submit and open refuse about an utterance's draw arguments; returns the codes of (top_k, top_p, min_p)."""
        if (seed is not None) != self.utterance_draws or (temperature is not None and not self.utterance_draws):
            raise ValueError("a seed (and a temperature) per utterance is given exactly when the generator was built with "
                             "utterance_draws=True")
        if top_k is not None and not self.utterance_draws:
            raise ValueError("a top_k per utterance needs a generator built with utterance_draws=True")
        if top_k is not None:
            top_k = top_k_code(top_k)
        if top_p is not None and not self.utterance_draws:
            raise ValueError("a top_p per utterance needs a generator built with utterance_draws=True")
        if top_p is not None:
            top_p = top_p_code(top_p)
        if min_p is not None and not self.utterance_draws:
            raise ValueError("a min_p per utterance needs a generator built with utterance_draws=True")
        if min_p is not None:
            min_p = min_p_code(min_p)
        return top_k, top_p, min_p

    def _ticket(self, seed, temperature, top_k, top_p, min_p, prompt=None):
        """The next ticket, with the (checked) draw arguments and prompt of its utterance on record."""
        ticket = self._next_ticket
        self._next_ticket += 1
        if prompt is not None:
            self._prompts[ticket] = prompt
            self._forcing = True
        if self.utterance_draws:
            self._draws[ticket] = (u64(seed), self.temperature if temperature is None else float(temperature))
            self._top_ks[ticket] = self.top_k if top_k is None else top_k
            self._truncates = self._truncates or top_k is not None
            self._top_ps[ticket] = self.top_p if top_p is None else top_p
            self._nucleus = self._nucleus or top_p is not None
            self._min_ps[ticket] = self.min_p if min_p is None else min_p
            self._min_p = self._min_p or min_p is not None
        return ticket

    def submit(self, features, seed=None, temperature=None, top_k=None, top_p=None, prompt=None, min_p=None):
        """features [n, 63], n >= 1 (frame 0 is the prefix slot) -> the utterance's ticket, numbered in submission order.
        seed (an unsigned 64-bit integer), temperature, top_k, top_p and min_p (defaults: the generator's): with
        utterance_draws=True only, where the seed is required.  prompt: up to 80 * (n - 1) integer codes in
        0 .. Q_LEVELS-1, the utterance's samples 80 ..: it goes on freely behind them."""
        top_k, top_p, min_p = self._check_draws(seed, temperature, top_k, top_p, min_p)
        features = numpy.asarray(features, dtype='float32')
        if features.ndim != 2 or features.shape[0] < 1 or features.shape[1] != config().FEAT_DIM:
            raise ValueError("an utterance is [n, %d] conditioning frames with n >= 1, got %s" % (config().FEAT_DIM, features.shape))
        if prompt is not None:
            if self.gen is not None and not self.forcing:
                raise ValueError("a prompt needs a generator built with forcing=True: its device plan is built to take them")
            prompt = _per_utterance_prompts([prompt], [features.shape[0]])[0]
        if self.open_utterances:  # open, one feed, close -- refused as a whole where either would be
            if features.shape[0] > self.max_frames:
                raise ValueError("an utterance of %d frames overflows a store row of max_frames = %d"
                                 % (features.shape[0], self.max_frames))
            ticket = self._open_ticket(seed, temperature, top_k, top_p, min_p, prompt)
            self.feed(ticket, features, last=True)
            return ticket
        ticket = self._ticket(seed, temperature, top_k, top_p, min_p, prompt)
        self._features[ticket] = features
        self.queue.append((ticket, features.shape[0]))
        return ticket

    def _need_open(self):
        if not self.open_utterances:
            raise ValueError("open, feed and close need a generator built with open_utterances=True")

    def _open_ticket(self, seed, temperature, top_k, top_p, min_p, prompt=None):
        if not self._free_rows:
            raise RuntimeError("every row of the frame store holds an utterance (store_utterances = %d): wait for one to be "
                               "reported done" % (self._store.shape[0] // self.max_frames))
        ticket = self._ticket(seed, temperature, top_k, top_p, min_p, prompt)
        self._open[ticket] = dict(row=self._free_rows.pop(0), fed=0, closed=False)
        self.queue.append((ticket, None))  # (its length is read from the record above at every step)
        return ticket

    def open(self, seed=None, temperature=None, top_k=None, top_p=None, min_p=None):
        """Opens an utterance whose frames arrive through feed() -> its ticket.  The draw arguments follow submit's rules."""
        self._need_open()
        if self.log_probs:
            raise ValueError("log_probs are handed out for submitted utterances only, not for open ones")
        return self._open_ticket(seed, temperature, *self._check_draws(seed, temperature, top_k, top_p, min_p))

    def feed(self, ticket, frames, last=False):
        """Appends frames [k, 63], k >= 0, to an open utterance: a numpy array (uploaded now), or a float32 tensor on the
        plan's device with row stride 63 or 64 (copied on the device).  last=True closes the utterance: its length is then
        known, and it needs at least its frame 0.  ValueError on another shape, an unknown or closed ticket, and when the
        utterance's store row (max_frames) would overflow; nothing is stored then."""
        self._need_open()
        u = self._open.get(ticket)
        if u is None or u['closed']:
            raise ValueError("ticket %r is not an open utterance" % (ticket,))
        F = config().FEAT_DIM
        if torch.is_tensor(frames):
            if frames.dtype != torch.float32:
                raise ValueError("frames on the device must be float32, got %s" % frames.dtype)
            if isinstance(self._store, numpy.ndarray) or frames.device.type == 'cpu':  # (taken like an array)
                frames = frames.detach().cpu().numpy()
            elif frames.device != self._store.device:
                raise ValueError("frames live on %s, the plan on %s" % (frames.device, self._store.device))
        if not torch.is_tensor(frames):
            frames = numpy.asarray(frames, dtype='float32')
        if frames.ndim != 2 or frames.shape[1] != F:
            raise ValueError("frames are [k, %d], got %s" % (F, tuple(frames.shape)))
        k = int(frames.shape[0])
        if u['fed'] + k > self.max_frames:
            raise ValueError("%d more frames overflow the utterance's store row: %d fed, max_frames = %d"
                             % (k, u['fed'], self.max_frames))
        if last and u['fed'] + k < 1:
            raise ValueError("every utterance needs at least one frame (its prefix slot)")
        if k:
            lo = u['row'] * self.max_frames + u['fed']
            if isinstance(self._store, numpy.ndarray):
                self._store[lo:lo + k, :F] = frames
            else:
                if not torch.is_tensor(frames):
                    frames = torch.from_numpy(numpy.ascontiguousarray(frames))
                self._store[lo:lo + k, :F].copy_(frames)
            u['fed'] += k
        u['closed'] = bool(last)

    def close(self, ticket=None):
        """close(ticket): feed with no frames and last=True.  close(): releases the generator's device plan."""
        if ticket is not None:
            return self.feed(ticket, numpy.zeros((0, config().FEAT_DIM), dtype='float32'), last=True)
        if self.gen is not None:
            self.gen.close()
            self.gen = None

    def idle(self):
        return not self.queue and all(r is None for r in self.running)

    def short_of_segment(self):
        """Whether some open utterance that is running, or that the next step could place (the oldest queued ones, one per
        idle stream), has not been closed and holds fewer unplaced frames than a full segment: feeding it first lets the
        next step run longer, or at all."""
        self._need_open()
        short = lambda t, placed: not self._open[t]['closed'] and self._open[t]['fed'] - placed < self.S
        if any(r is not None and short(r[0], r[1]) for r in self.running):
            return True
        n_idle = sum(r is None for r in self.running)
        return any(short(t, 0) for t, _ in self.queue[:n_idle])

    def step(self):
        """Runs one segment; returns [(ticket, chunk int32 [80 k], done)] for every utterance that had slots in it --
        (ticket, chunk, logp_chunk float32 [80 k], done) with log_probs=True."""
        if self.open_utterances:
            return self._step_open()
        placements, starts, n, self.running, self.queue = schedule_segment(self.running, self.queue, self.B, self.S)
        if n == 0:
            return []
        feats = numpy.zeros((n, self.B, config().FEAT_DIM), dtype='float32')
        for ticket, b, slot, frame, count in placements:
            feats[slot - 1:slot - 1 + count, b] = self._features[ticket][frame:frame + count]
        return self._run_placements(placements, starts, n, feats, None,
                                    lambda ticket, placed: placed == self._features[ticket].shape[0])

    def _step_open(self):
        """step() with open utterances: the rules of the class's docstring."""
        self._starved = None
        out, S = [], self.S
        length = lambda t: self._open[t]['fed'] + (not self._open[t]['closed'])  # (end unknown: one past what has been fed)
        running = []
        for b, r in enumerate(self.running):
            if r is not None and self._open[r[0]]['closed'] and r[1] == self._open[r[0]]['fed']:  # rule 5
                empty = numpy.zeros(0, dtype='int32')
                out.append((r[0], empty, numpy.zeros(0, dtype='float32'), True) if self.log_probs else (r[0], empty, True))
                self._forget(r[0])
                r = self.running[b] = None
            running.append(None if r is None else (r[0], r[1], length(r[0])))
        for r in running:
            if r is not None and r[1] == self._open[r[0]]['fed']:  # rule 2: (not closed, or rule 5 had taken it)
                self._starved = "utterance %d has run all %d frames it was fed and is not closed" % (r[0], r[1])
                return out
        queue = [(t, length(t)) for t, _ in self.queue if self._open[t]['fed'] >= 1]  # rule 3
        while True:  # rules 1 and 2: no open utterance may reach the length it was lent, so it ends at the segment's last slot
            placements, starts, n, running_after, _ = schedule_segment(running, queue, self.B, S)
            cut = S
            for ticket, b, slot, frame, count in placements:
                u = self._open[ticket]
                if not u['closed'] and frame + count > u['fed']:
                    cut = min(cut, slot + (u['fed'] - frame) - 1)
            if cut == S:
                break
            S = cut
        if n == 0:
            if self.queue:
                self._starved = "no queued utterance has been fed its frame 0"
            return out
        placed = set(p[0] for p in placements)
        self.running = running_after
        self.queue = [q for q in self.queue if q[0] not in placed]
        index = numpy.full((n, self.B), -1, dtype=numpy.int32)
        for ticket, b, slot, frame, count in placements:
            lo = self._open[ticket]['row'] * self.max_frames + frame
            index[slot - 1:slot - 1 + count, b] = numpy.arange(lo, lo + count)
        feats = None
        if self.gen is None:  # a runner of the caller's: the gathered host array
            feats = numpy.where((index >= 0)[:, :, None], self._store[numpy.maximum(index, 0), :config().FEAT_DIM], 0.)
            feats = feats.astype('float32')
        return out + self._run_placements(placements, starts, n, feats, index if self.gen is not None else None,
                                          lambda t, n_placed: self._open[t]['closed'] and n_placed == self._open[t]['fed'])

    def _forget(self, ticket):
        """Drops what the generator holds for an utterance that is done; its store row is free again."""
        self._features.pop(ticket, None)
        self._draws.pop(ticket, None)
        self._top_ks.pop(ticket, None)
        self._top_ps.pop(ticket, None)
        self._min_ps.pop(ticket, None)
        self._prompts.pop(ticket, None)
        if self.open_utterances:
            self._free_rows.append(self._open.pop(ticket)['row'])
            self._free_rows.sort()

    def _run_placements(self, placements, starts, n, feats, index, finished):
        """Runs the segment schedule_segment laid out -- feats [n, B, 63], or on the device index [n, B] into the frame
        store -- and cuts its samples into the utterances' chunks; finished(ticket, frames placed) says who is done."""
        tt = config()
        BFS = tt.BIG_FRAME_SIZE
        flags = numpy.zeros((n, self.B), dtype='int32')
        for ticket, b, slot, frame, count in placements:
            if frame == 0:
                self.record[ticket] = (b, self._slots_run + slot)
        for slot, b in starts:
            flags[slot - 1, b] = 1
        draws = {}
        if self.utterance_draws:
            draws = dict(seeds=numpy.zeros((n, self.B), dtype=numpy.uint64),
                         temperatures=numpy.zeros((n, self.B), dtype='float32'))
            for ticket, b, slot, frame, count in placements:
                if frame <= 1 < frame + count:
                    # the utterance's start_row in the ring of this segment, whose slot 0 is the last slot of the segment
                    # before (where its prefix may lie); the arrays hold the ring's rows 1 .. n
                    row = start_row(slot - frame, n + 1) - 1
                    assert flags[row, b] == 1
                    draws['seeds'][row, b], draws['temperatures'][row, b] = self._draws[ticket]
        if self._truncates:  # (like the seeds: on the row of the utterance's start flag)
            draws['top_ks'] = numpy.zeros((n, self.B), dtype=numpy.int32)
            for ticket, b, slot, frame, count in placements:
                if frame <= 1 < frame + count:
                    draws['top_ks'][start_row(slot - frame, n + 1) - 1, b] = self._top_ks.get(ticket, self.top_k)
        if self._nucleus:
            draws['top_ps'] = numpy.zeros((n, self.B), dtype=numpy.float32)
            for ticket, b, slot, frame, count in placements:
                if frame <= 1 < frame + count:
                    draws['top_ps'][start_row(slot - frame, n + 1) - 1, b] = self._top_ps.get(ticket, self.top_p)
        if self._min_p:
            draws['min_ps'] = numpy.zeros((n, self.B), dtype=numpy.float32)
            for ticket, b, slot, frame, count in placements:
                if frame <= 1 < frame + count:
                    draws['min_ps'][start_row(slot - frame, n + 1) - 1, b] = self._min_ps.get(ticket, self.min_p)
        if self._forcing:  # sample j of an utterance's buffer is column 80 (slot - 1) + (j - 80 frame) of this segment
            draws['forced'] = numpy.full((self.B, BFS * n), FREE, dtype=numpy.int32)
            for ticket, b, slot, frame, count in placements:
                p = self._prompts.get(ticket)
                if p is None:
                    continue
                lo, hi = max(BFS * frame, BFS), min(BFS * (frame + count), BFS + p.size)  # the prompt's share, buffer indices
                if lo < hi:
                    col = BFS * (slot - 1) - BFS * frame
                    draws['forced'][b, col + lo:col + hi] = p[lo - BFS:hi - BFS]
        if index is not None:
            draws['index'] = index
        got = self._run(feats, flags, self._resume, **draws)
        logp = None
        if self.log_probs:
            if not isinstance(got, (tuple, list)) or len(got) != 2:
                raise ValueError("with log_probs=True the segment runner returns (samples, logp)")
            got, logp = got[0], numpy.asarray(got[1], dtype='float32')
            if logp.shape != (self.B, BFS * n):
                raise ValueError("the segment runner returned log-probabilities %s, not %s" % (logp.shape, (self.B, BFS * n)))
        samples = numpy.asarray(got)
        if samples.shape != (self.B, BFS * n):
            raise ValueError("the segment runner returned %s, not %s" % (samples.shape, (self.B, BFS * n)))
        self._resume = True
        self._slots_run += n
        out = []
        for ticket, b, slot, frame, count in placements:
            chunk = numpy.array(samples[b, BFS * (slot - 1):BFS * (slot - 1 + count)], dtype='int32')
            if frame == 0:
                chunk[:BFS] = tt.Q_ZERO  # (the period that would write it may lie in the next segment)
            done = finished(ticket, frame + count)
            if done:
                self._forget(ticket)
            if logp is None:
                out.append((ticket, chunk, done))
                continue
            lchunk = numpy.array(logp[b, BFS * (slot - 1):BFS * (slot - 1 + count)], dtype='float32')
            if frame == 0:
                lchunk[:BFS] = 0.0  # (the prefix slot: nothing was asked of the model there)
            out.append((ticket, chunk, lchunk, done))
        return out

    def drain(self):
        """Steps until nothing is queued or running; returns the chunks of all those steps in order.  (Open utterances:
        RuntimeError when a step starves -- an utterance that is not closed waits for frames nobody can feed here.)"""
        out = []
        while not self.idle():
            out += self.step()
            if self._starved is not None:
                raise RuntimeError("drain() cannot go on: " + self._starved)
        return out

"""The plan of the device-resident generation loop: folded weights, workspace, runs in one piece or in resumable segments."""
import ctypes as C

import numpy
import torch

from ... import _lib
from ... import ops as hip
from .. import lib
from ..lib import ops as lops
from .inputs import (FREE, _seed_image, config, draw_mode_code, forced_array, min_p_array, min_p_code, skip_stacks_enabled,
                     stack_param_names, top_k_array, top_k_code, top_p_array, top_p_code)


def device_loop_guard(draw_mode, top_k=0, top_p=0.0, min_p=0.0):
    """What every entry to the device-resident loop checks before any device call: draw_mode's code (ValueError on an
    unknown name), top_k (ValueError on a negative one), top_p (ValueError on a negative one or a NaN), min_p (ValueError outside [0, 1] or a NaN), and the model's
    stacks: skip-connection stacks (SKIP_CONN) are taken only with PARROT_SR_SKIP_STACKS=1, read here at call time, and only
    with N_RNN >= 2 (the reference asserts that no one-layer stack has skip connections); NotImplementedError otherwise."""
    mode = draw_mode_code(draw_mode)
    top_k_code(top_k)
    top_p_code(top_p)
    min_p_code(min_p)
    if config().SKIP_CONN:
        if not skip_stacks_enabled():
            raise NotImplementedError("the device-resident generator takes skip-connection stacks only with "
                                      "PARROT_SR_SKIP_STACKS=1")
        if config().N_RNN < 2:
            raise NotImplementedError("a single-layer stack cannot have skip connections")
    return mode


class DeviceGenerator:
    """Device-resident generation loop (samplernn_generate_*, include/parrot_hip.h)."""

    forcing = False    # (a plan takes forced samples / returns log-probabilities only when it was built that way)
    log_probs = False
    draw_stats = False

    def __init__(self, batch, n_frames, temperature=0.0, seed=234, use_graph=True, packed=False, utterance_draws=False,
                 draw_mode='sequential', top_k=0, top_p=0.0, forcing=False, log_probs=False, min_p=0.0,
                 draw_stats=False):
        """GRU or LSTM tiers, 1..5 stacked layers (three_tier.py:147-169).  Stacks with skip connections (SKIP_CONN, 2..5
        layers) are taken with PARROT_SR_SKIP_STACKS=1 (samplernn_generate_set_skip_stacks: one more K segment in the step
        jobs of the layers above the first, one more job per tier step for the summed out-skips; everything below is the
        same for them); without the switch they are refused (NotImplementedError) and generate_and_save_samples runs them
        on the literal three-function loop.

        packed=True: the plan takes per-stream utterance starts (SampleRnnGenDesc::starts): generate(features, starts)
        then begins a new utterance in stream b at big frame f wherever starts[f][b] != 0 (see generate_packed).

        utterance_draws=True: every utterance draws with a seed and a temperature of its own
        (samplernn_generate_set_utterance_draws): generate(..., seeds=, temperatures=) takes them, aligned with starts on a
        packed plan, one per stream on a plain one; the plan's temperature and seed are then not used.  An utterance's
        samples are then a function of the model, the plan's shape, the carrying stream, and the utterance's features,
        seed and temperature (utterance_draw_u01 is the uniform of its n-th sample): they do not depend on its slot, the
        segment boundaries or its neighbours.

        draw_mode: how a draw at temperature > 0 finds its code.  'sequential' (default): one lane walks the 256 codes, the
        samples every earlier version drew.  'scan': the wave-parallel draw (SampleRnnGenDesc::draw_mode = 1) -- the same
        terms and uniforms, the CDF as a fixed tree of float32 sums; faster, and a different (equally valid) rounding of the
        CDF, so a few draws per ten thousand land on the neighbouring code.  Argmax (temperature <= 0) is the same in both.

        top_k = k > 0: a draw at temperature > 0 is taken among the k most likely codes (SampleRnnGenDesc::top_k) -- the k
        first codes by logit descending, then by index ascending; every other code's term is 0 in the same sums, with the
        same uniforms, in both draw modes.  0 (default) or k >= Q_LEVELS: among all codes, the samples of every earlier
        version.  k = 1 picks the argmax.  With utterance_draws=True it is what an utterance draws with unless
        generate(..., top_ks=) names its own.  Negative: ValueError.

        top_p = p strictly between 0 and 1: a draw at temperature > 0 is taken among the nucleus (samplernn_generate_set_top_p)
        -- of the codes top_k left (all of them without), ordered the same way, the shortest prefix whose mass reaches p of
        their mass; never empty, ties at the cut-off to the lower index, every other code's term 0 in the same sums: a draw
        with top_p = p is a draw with top_k = the length of that prefix.  0 (default) or >= 1: no nucleus, the samples of
        every earlier version.  A very small p picks the argmax.  With utterance_draws=True it is what an utterance draws
        with unless generate(..., top_ps=) names its own.  Negative or NaN: ValueError.

        min_p in (0, 1]: a draw at temperature > 0 is taken among the codes whose probability is at least min_p times the
        most likely code's (samplernn_generate_set_min_p) -- those whose float32 term expf((logit - max) / temperature) is
        >= min_p; never empty.  Applied last: the kept set is top_k's set, its nucleus and this set intersected, every
        other code's term 0 in the same sums, so such a draw is again a draw with top_k = the size of what is left.
        min_p = 1 keeps the maxima only.  0 (default): off, the samples of every earlier version.  With
        utterance_draws=True it is what an utterance draws with unless generate(..., min_ps=) names its own.  Negative,
        above 1 or NaN: ValueError.

        forcing=True: the plan takes forced samples (samplernn_generate_set_forced): generate(..., forced=) names, per
        stream and sample, a code the sample step takes instead of its pick, or -1 where it picks freely.  The step computes
        its logits either way, and the forced code is what every later step, both tiers above and a resumed segment see.
        The draw counter stays the sample's index (a forced step consumes no uniform), so forcing a run's own earlier
        output reproduces that run bit for bit, in every draw setting.  Priming, teacher forcing.

        log_probs=True: generate returns (samples, logp), logp [B, 80 T] float32 (samplernn_generate_set_log_probs): the
        natural logarithm of the MODEL's probability of each sample it wrote, forced or picked -- temperature 1, no
        truncation, whatever the step draws with; the quantity compute_cost averages.  The prefix slot holds zeros.

        draw_stats=True: generate returns two more arrays of the samples' shape behind (samples[, logp]), draw_logp float32
        and kept int32 (samplernn_generate_set_draw_stats): what each step drew from.  kept = the size of the set the step's
        pick was drawn from -- 1 on an argmax step (temperature <= 0), Q_LEVELS on an untruncated draw, else what top_k,
        top_p and min_p left, forced step or not.  draw_logp = the natural logarithm of the probability of the sample that
        was written under the step's own temperature and kept set, (logit - max) / temperature - log(sum of the kept
        terms): -inf for a (forced) sample outside the kept set or off the argmax of an argmax step, 0 for the argmax of an
        argmax step.  The prefix slot holds zeros in both.

        All three are independent of each other and of every other setting; a plan built with none runs the kernels it ran
        before they existed."""
        self.draw_mode = draw_mode
        mode = device_loop_guard(draw_mode, top_k, top_p, min_p)
        self.top_k = top_k_code(top_k)
        self.top_p = top_p_code(top_p)
        self.min_p = min_p_code(min_p)
        self.B, self.T = batch, n_frames
        self.packed = bool(packed)
        self.utterance_draws = bool(utterance_draws)
        self.forcing, self.log_probs = bool(forcing), bool(log_probs)
        self.draw_stats = bool(draw_stats)
        dev = lib.device()
        f = dict(device=dev, dtype=torch.float32)
        tt = config()
        D, FS, BFS, Q, N_RNN, RNN_TYPE = tt.DIM, tt.FRAME_SIZE, tt.BIG_FRAME_SIZE, tt.Q_LEVELS, tt.N_RNN, tt.RNN_TYPE
        nfr = BFS // FS
        ew = lambda n, i=0: lops.effective_weight(n, i, tt.WEIGHT_NORM).detach().contiguous()
        pb = lambda n: lib.param(n + '.b').detach().contiguous()
        with torch.no_grad():
            single = RNN_TYPE == 'GRU' and N_RNN == 1
            w = dict(
                big_Win_frames=ew('BigFrameLevel.rnn_inp_fusion', 0), big_Win_feats=ew('BigFrameLevel.rnn_inp_fusion', 1),
                big_bin=pb('BigFrameLevel.rnn_inp_fusion'),
                big_Wout=ew('BigFrameLevel.Output'), big_bout=pb('BigFrameLevel.Output'),
                frm_Win=ew('FrameLevel.InputExpand'), frm_bin=pb('FrameLevel.InputExpand'),
                frm_Wout=ew('FrameLevel.Output'), frm_bout=pb('FrameLevel.Output'),
                W2=ew('SampleLevel.L2'), b2=pb('SampleLevel.L2'), W3=ew('SampleLevel.L3'), b3=pb('SampleLevel.L3'),
                W4=ew('SampleLevel.Output'), b4=pb('SampleLevel.Output'))
            # fold Embedding . L1_PrevSamples into a [FS, Q, D] table (one GEMM per previous-sample position)
            emb = lib.param('SampleLevel.Embedding').detach().contiguous()
            W1 = ew('SampleLevel.L1_PrevSamples')
            tbl = torch.empty(FS, Q, D, **f)
            for pos in range(FS):
                hip.gemm(emb, W1[pos * tt.EMB_SIZE:(pos + 1) * tt.EMB_SIZE], out=tbl[pos])
            w['emb_tbl'] = tbl
            # the RNN stacks of the two tiers: per layer (Input.W, Input.b | b, Recurrent_Gates, Recurrent_Candidate | -)
            # (skip stacks: the Input of a layer above the first is [2 D, N], folded as ONE matrix -- weight norm scales a
            # column over all its rows --, and every layer has an out-skip matrix, the first one a bias)
            self.layers = {}
            self.skip = bool(tt.SKIP_CONN)
            self.outskips = {}
            for tier, tag in (('BigFrameLevel', 'big'), ('FrameLevel', 'frm')):
                names, outskips, outskip_bias = stack_param_names(tier, RNN_TYPE, N_RNN, self.skip)
                for k, nm in enumerate(names):
                    layer = [ew(nm['input']), lib.param(nm['bias']).detach().contiguous(), ew(nm['gates'])]
                    if RNN_TYPE == 'GRU':
                        layer.append(ew(nm['candidate']))
                    self.layers[(tag, k)] = layer
                if self.skip:
                    self.outskips[tag] = ([ew(n) for n in outskips], lib.param(outskip_bias).detach().contiguous())
            if single:
                for tag in ('big', 'frm'):
                    U_, bU_, Wg_, Wc_ = self.layers[(tag, 0)]
                    w.update({f'{tag}_U': U_, f'{tag}_bU': bU_, f'{tag}_Wg': Wg_, f'{tag}_Wc': Wc_})
        self.w = w
        self.single = single
        self.ws = dict(
            samples=torch.zeros(batch, BFS * n_frames, device=dev, dtype=torch.int32),
            features=torch.zeros(n_frames, batch, tt.FEAT_DIM, **f),
            big_h=torch.zeros(batch, D, **f), frm_h=torch.zeros(batch, D, **f),
            xf_big=torch.zeros(batch, BFS, **f), xf_frm=torch.zeros(batch, FS, **f),
            feat_cur=torch.zeros(batch, tt.FEAT_DIM, **f), gru_in=torch.zeros(batch, D, **f),
            P=torch.zeros(batch, 4 * D, **f), z=torch.zeros(batch, D, **f), r=torch.zeros(batch, D, **f),
            rh=torch.zeros(batch, D, **f), big_out=torch.zeros(batch, nfr * D, **f),
            frame_out=torch.zeros(batch, FS * D, **f), o1=torch.zeros(batch, D, **f), o2=torch.zeros(batch, D, **f),
            o3=torch.zeros(batch, D, **f), logits=torch.zeros(batch, Q, **f),
            tbase=torch.zeros(1, device=dev, dtype=torch.int32))
        if self.packed:
            self.ws['starts'] = torch.zeros(n_frames, batch, device=dev, dtype=torch.int32)
            # the learned initial states, [N_RNN, H0_MULT * D]: what a stream restarts from inside the loop
            w['big_h0'] = lib.param('BigFrameLevel.h0').detach().to(**f).contiguous()
            w['frm_h0'] = lib.param('FrameLevel.h0').detach().to(**f).contiguous()
        d = _lib.SampleRnnGenDesc()
        d.B, d.D, d.T, d.Q, d.FS, d.BFS, d.feat_dim, d.use_graph = batch, D, n_frames, Q, FS, BFS, tt.FEAT_DIM, int(use_graph)
        d.temperature, d.seed, d.draw_mode = float(temperature), int(seed), mode
        d.top_k = self.top_k if self.top_k < Q else 0  # (k >= Q: no truncation)
        for k, v in list(w.items()) + list(self.ws.items()):
            setattr(d, k, v.data_ptr())
        if not self.single:
            lstm = RNN_TYPE == 'LSTM'
            d.n_rnn, d.lstm = N_RNN, int(lstm)
            self.states = {}
            for tag in ('big', 'frm'):
                for k in range(N_RNN):
                    for q, t in enumerate(self.layers[(tag, k)]):
                        getattr(d, tag + '_L')[k][q] = t.data_ptr()
                    self.states[(tag, 'h', k)] = torch.zeros(batch, D, **f)
                    getattr(d, tag + '_hs')[k] = self.states[(tag, 'h', k)].data_ptr()
                    if lstm:
                        self.states[(tag, 'c', k)] = torch.zeros(batch, D, **f)
                        getattr(d, tag + '_cs')[k] = self.states[(tag, 'c', k)].data_ptr()
            self.ws['gate_ws'] = torch.zeros(batch, 4 * D, **f)
            self.ws['layer_tmp'] = torch.zeros(batch, D, **f)
            d.gate_ws, d.layer_tmp = self.ws['gate_ws'].data_ptr(), self.ws['layer_tmp'].data_ptr()
        # persistent-thread sample kernel (sr_persist.hip): zero-filled exchange / barrier workspace when the shape qualifies
        n = int(_lib.load().samplernn_persist_floats(C.byref(d)))
        if n > 0:
            self.ws['persist_ws'] = torch.zeros(n, **f)
            d.persist_ws, d.persist_ws_floats = self.ws['persist_ws'].data_ptr(), n
        self.desc = d
        self.plan = C.c_void_p()
        _lib.call('samplernn_generate_create', C.byref(d), C.byref(self.plan))
        if 0.0 < self.top_p < 1.0:  # (the descriptor has no word for it; off is a new plan's state)
            _lib.call('samplernn_generate_set_top_p', self.plan, C.c_float(self.top_p))
        if self.min_p > 0.0:
            _lib.call('samplernn_generate_set_min_p', self.plan, C.c_float(self.min_p))
        if self.skip:
            self.set_skip_stacks()
        self.persistent = bool(_lib.load().samplernn_generate_is_persistent(self.plan))
        # row groups of 32 streams per launch of that kernel (PARROT_SR_PERSIST_GROUPS lifts the limit of one); 0: launches
        self.persist_groups = int(_lib.load().samplernn_generate_persist_groups(self.plan))
        self._has_run = False
        if self.forcing:  # [B, 80 T] like samples; -1 = free
            self.ws['forced'] = torch.full((batch, BFS * n_frames), FREE, device=dev, dtype=torch.int32)
            _lib.call('samplernn_generate_set_forced', self.plan, self.ws['forced'].data_ptr())
        if self.log_probs:
            self.ws['logp'] = torch.zeros(batch, BFS * n_frames, **f)
            _lib.call('samplernn_generate_set_log_probs', self.plan, self.ws['logp'].data_ptr())
        if self.draw_stats:
            self.ws['draw_logp'] = torch.zeros(batch, BFS * n_frames, **f)
            self.ws['kept'] = torch.zeros(batch, BFS * n_frames, device=dev, dtype=torch.int32)
            _lib.call('samplernn_generate_set_draw_stats', self.plan, self.ws['draw_logp'].data_ptr(),
                      self.ws['kept'].data_ptr())
        if self.utterance_draws:
            # [T, B] like starts (ring rows): row f = what an utterance that begins at big frame f draws with; utt_seed is the
            # two's-complement image of the unsigned 64-bit seed
            self.ws['utt_seed'] = torch.zeros(n_frames, batch, device=dev, dtype=torch.int64)
            self.ws['utt_temp'] = torch.zeros(n_frames, batch, **f)
            self.ws['utt_top_k'] = torch.zeros(n_frames, batch, device=dev, dtype=torch.int32)
            self.ws['utt_top_p'] = torch.zeros(n_frames, batch, **f)
            self.ws['utt_min_p'] = torch.zeros(n_frames, batch, **f)
            self.set_utterance_draws()

    def set_skip_stacks(self):
        """Hands the plan the out-skip matrices, their bias and the [B, DIM] scratch of the summed output per tier
        (samplernn_generate_set_skip_stacks); refused (HipCallError) once the plan has run."""
        _lib.call('samplernn_generate_set_skip_stacks', self.plan, C.byref(self.skip_struct()))

    def skip_struct(self):
        """The SampleRnnSkipStacks of this plan's model; the scratch buffers live in the workspace."""
        s = _lib.SampleRnnSkipStacks()
        for tag in ('big', 'frm'):
            mats, bias = self.outskips[tag]
            for k, m in enumerate(mats):
                getattr(s, tag + '_S')[k] = m.data_ptr()
            setattr(s, tag + '_bS', bias.data_ptr())
            key = tag + '_skip_sum'
            if key not in self.ws:
                self.ws[key] = torch.zeros(self.B, config().DIM, device=bias.device, dtype=torch.float32)
            setattr(s, tag + '_sum', self.ws[key].data_ptr())
        return s

    def set_utterance_draws(self):
        """Hands the plan its per-utterance seed, temperature, top_k, top_p and min_p arrays; refused (HipCallError) once the plan
        has run."""
        _lib.call('samplernn_generate_set_utterance_draws', self.plan, self.ws['utt_seed'].data_ptr(),
                  self.ws['utt_temp'].data_ptr())
        _lib.call('samplernn_generate_set_utterance_top_k', self.plan, self.ws['utt_top_k'].data_ptr())
        _lib.call('samplernn_generate_set_utterance_top_p', self.plan, self.ws['utt_top_p'].data_ptr())
        _lib.call('samplernn_generate_set_utterance_min_p', self.plan, self.ws['utt_min_p'].data_ptr())

    def generate(self, features=None, starts=None, resume=False, n_frames=None, seeds=None, temperatures=None, top_ks=None,
                 top_ps=None, forced=None, min_ps=None, gather=None):
        """features [T, B, 63] time-major (what generate_and_save_samples receives) -> samples [B, 80*T] int32.
        starts [T, B] (packed plans only, and required there): non-zero where stream b begins a new utterance at big
        frame f, whose Q/2 prefix is slot f - 1.

        A run in segments (samplernn_generate_run_segment): n_frames = k in 1 .. T-1 generates k frames in this call.
        resume=False starts a run: features (and starts) hold k + 1 rows, slot 0 = the prefix, and the [B, 80 (k + 1)]
        samples come back, prefix included.  resume=True continues the run of the last call from the states where they
        stand: features (and starts) hold k rows, for slots 1 .. k of the ring -- slot 0 is the last slot of the call
        before --, nothing is re-initialised and the [B, 80 k] samples of this segment come back (a copy: the next
        segment overwrites the ring).  The segments of a run equal the run in one piece, seeded draws included.

        seeds / temperatures (plans built with utterance_draws=True only, and both required there): on a packed plan
        [rows, B] aligned with starts -- row f, stream b holds what the utterance that starts[f][b] flags draws with, and the
        row of slot 1 of a run that does not resume what every stream's first utterance draws with --; on a plain plan [B],
        one utterance per stream, with resume=False only (the segments that resume go on with them).  Seeds are unsigned
        64-bit integers (Python integers or an integer array).

        top_ks (optional, accepted exactly where seeds is): integers of the same shape as seeds, or one integer for all --
        the top_k each utterance draws with (0 or >= Q_LEVELS: no truncation); omitted, every utterance takes the plan's
        top_k.  A negative value or another shape: ValueError.

        top_ps (optional, likewise): numbers of the same shape as seeds, or one number for all -- the top_p each utterance
        draws with (0 or >= 1: no nucleus); omitted, every utterance takes the plan's top_p.  A negative value, a NaN or
        another shape: ValueError.

        min_ps (optional, likewise): numbers of the same shape as seeds, or one number for all -- the min_p each utterance
        draws with (0: off); omitted, every utterance takes the plan's min_p.  A value outside [0, 1], a NaN or another
        shape: ValueError.

        forced (plans built with forcing=True only, and required there): integers [B, 80 rows], aligned with the rows of
        `features` of this call -- [B, 80 T] for a run in one piece (its first 80 columns, the prefix slot, are ignored),
        [B, 80 k] for a segment that resumes.  A code in 0 .. Q_LEVELS-1 is the sample of that step; -1: the step picks.
        Another shape, a non-integer dtype or any other value: ValueError, before anything is staged.

        gather=(src, index), in place of `features` (exactly one of the two): the rows `features` would have held are
        gathered on the device (samplernn_generate_stage_features) from src, a float32 tensor [R, ld] on the plan's device
        with ld >= 63 and unit column stride (its first 63 columns are the frame), through index, an int32 array [rows, B]
        with the `rows` of this call (T, k + 1 or k): row index[r][b] of src, or zeros where the entry is negative (an idle
        slot) or >= R.  No frame visits the host; everything else about the call is what it is with `features`.  Another
        shape or dtype, a src on another device or narrower than 63, both or neither of features and gather: ValueError,
        before anything is staged.

        A plan built with log_probs=True returns (samples, logp): logp float32, sliced like samples and, like them, a
        copy when the run is in segments.  A plan built with draw_stats=True returns (samples[, logp], draw_logp, kept),
        sliced and copied the same way."""
        segment, resume, k, rows, first = self._resolve(starts, resume, n_frames, seeds, temperatures, top_ks, top_ps, min_ps)
        if (forced is not None) != self.forcing:
            raise ValueError("forced must be given exactly when the plan was built with forcing=True")
        if forced is not None:  # (its values and shape before anything is staged on the device)
            forced = forced_array(forced, (self.B, config().BIG_FRAME_SIZE * rows))
        if gather is not None or features is None:
            gather = self._check_gather(features, gather, rows)
        self._stage(features, starts, seeds, temperatures, segment, rows, first, top_ks, top_ps, min_ps, gather)
        BFS = config().BIG_FRAME_SIZE
        if forced is not None:
            fo = self.ws['forced']
            fo[:, BFS * first:BFS * (first + rows)].copy_(torch.from_numpy(forced).to(fo.device))
        self._launch(segment, resume, k)
        cut = (lambda x: x) if not segment else (lambda x: x[:, BFS * first:BFS * (k + 1)].clone())
        out = (cut(self.ws['samples']),)
        if self.log_probs:
            out += (cut(self.ws['logp']),)
        if self.draw_stats:
            out += (cut(self.ws['draw_logp']), cut(self.ws['kept']))
        return out if len(out) > 1 else out[0]

    def _resolve(self, starts, resume, n_frames, seeds, temperatures, top_ks=None, top_ps=None, min_ps=None):
        """Which arguments this plan takes in which kind of run -> (segment, resume, k, rows, first): a run in segments or
        in one piece, k frames to generate, `rows` rows of input for the ring's slots from `first` on."""
        if (starts is not None) != self.packed:
            raise ValueError("starts must be given exactly when the plan was built with packed=True")
        resume = bool(resume)
        takes_draws = self.utterance_draws and (self.packed or not resume)
        if (seeds is not None) != takes_draws or (temperatures is not None) != takes_draws:
            raise ValueError("seeds and temperatures must both be given exactly when the plan was built with "
                             "utterance_draws=True (a plain plan takes them with resume=False only)")
        if top_ks is not None and not takes_draws:
            raise ValueError("top_ks is accepted only where seeds is: on a plan built with utterance_draws=True (a plain "
                             "plan takes them with resume=False only)")
        if top_ps is not None and not takes_draws:
            raise ValueError("top_ps is accepted only where seeds is: on a plan built with utterance_draws=True (a plain "
                             "plan takes them with resume=False only)")
        if min_ps is not None and not takes_draws:
            raise ValueError("min_ps is accepted only where seeds is: on a plan built with utterance_draws=True (a plain "
                             "plan takes them with resume=False only)")
        if resume and not self._has_run:
            raise ValueError("resume=True needs a run to continue: call generate(..., resume=False) first")
        k = self.T - 1 if n_frames is None else int(n_frames)
        if not 1 <= k <= self.T - 1:
            raise ValueError("n_frames must be in 1 .. T-1 = %d, got %d" % (self.T - 1, k))
        rows = k if resume else (k + 1 if n_frames is not None else self.T)
        if top_ks is not None:  # (its values and shape before anything is staged on the device)
            top_k_code(top_ks) if numpy.ndim(top_ks) == 0 else top_k_array(top_ks, (rows, self.B) if self.packed else (self.B,))
        if top_ps is not None:
            top_p_code(top_ps) if numpy.ndim(top_ps) == 0 else top_p_array(top_ps, (rows, self.B) if self.packed else (self.B,))
        if min_ps is not None:
            min_p_code(min_ps) if numpy.ndim(min_ps) == 0 else min_p_array(min_ps, (rows, self.B) if self.packed else (self.B,))
        return resume or n_frames is not None, resume, k, rows, 1 if resume else 0

    def _check_gather(self, features, gather, rows):
        """gather=(src, index) of generate as (src, index int32 [rows, B]); ValueError on anything the staging entry cannot
        take, and on both or neither of features and gather."""
        if (features is None) == (gather is None):
            raise ValueError("exactly one of features and gather=(src, index) must be given")
        F = config().FEAT_DIM
        try:
            src, index = gather
        except (TypeError, ValueError):
            raise ValueError("gather must be (src, index)") from None
        dev = self.ws['features'].device
        if not torch.is_tensor(src) or src.dtype != torch.float32 or src.dim() != 2 or src.shape[0] < 1:
            raise ValueError("gather's src must be a float32 tensor [R, ld] with R >= 1")
        if src.shape[1] < F or src.stride(1) != 1 or src.stride(0) < src.shape[1]:
            raise ValueError("gather's src needs rows of ld >= %d floats with unit column stride, got shape %s, strides %s"
                             % (F, tuple(src.shape), tuple(src.stride())))
        if src.device != dev:
            raise ValueError("gather's src lives on %s, the plan on %s" % (src.device, dev))
        index = numpy.asarray(index)
        if index.dtype != numpy.int32 or index.shape != (rows, self.B):
            raise ValueError("gather's index must be int32 [%d, %d], got %s %s" % (rows, self.B, index.dtype, index.shape))
        return src, numpy.ascontiguousarray(index)

    def _stage(self, features, starts, seeds, temperatures, segment, rows, first, top_ks=None, top_ps=None, min_ps=None,
               gather=None):
        """Checks the arrays' shapes and copies them into rows first .. first + rows - 1 of the workspace (gather: the
        features by samplernn_generate_stage_features, from device memory)."""
        ws = self.ws
        feats = None if gather is not None else torch.as_tensor(features)
        if feats is not None and segment and (feats.dim() != 3 or tuple(feats.shape[:2]) != (rows, self.B)):
            raise ValueError("features must be [%d, %d, %d], got %s" % (rows, self.B, config().FEAT_DIM, tuple(feats.shape)))
        if self.packed:
            st = torch.as_tensor(numpy.asarray(starts))
            if tuple(st.shape) != (rows, self.B):
                raise ValueError("starts must be [%s, B] = [%d, %d], got %s" % ("T" if not segment else "rows", rows, self.B,
                                                                                 tuple(st.shape)))
            ws['starts'][first:first + rows].copy_((st != 0).to(ws['starts'].device, torch.int32))
        if seeds is not None:
            want = (rows, self.B) if self.packed else (self.B,)
            sd = _seed_image(seeds)
            tp = numpy.broadcast_to(numpy.asarray(temperatures, dtype='float32'), want) if numpy.ndim(temperatures) == 0 \
                else numpy.asarray(temperatures, dtype='float32')
            if sd.shape != want or tp.shape != want:
                raise ValueError("seeds and temperatures must be %s, got %s and %s" % (list(want), sd.shape, tp.shape))
            if top_ks is None or numpy.ndim(top_ks) == 0:
                tk = numpy.full(want, top_k_code(self.top_k if top_ks is None else top_ks), dtype=numpy.int32)
            else:
                tk = top_k_array(top_ks, want)
            if top_ps is None or numpy.ndim(top_ps) == 0:
                pp = numpy.full(want, top_p_code(self.top_p if top_ps is None else top_ps), dtype=numpy.float32)
            else:
                pp = top_p_array(top_ps, want)
            if min_ps is None or numpy.ndim(min_ps) == 0:
                mp = numpy.full(want, min_p_code(self.min_p if min_ps is None else min_ps), dtype=numpy.float32)
            else:
                mp = min_p_array(min_ps, want)
            # (a plain plan: one utterance per stream, prefix in slot 0 -- the row of slot 1, like a start flagged there)
            lo, hi = (first, first + rows) if self.packed else (1, 2)
            ws['utt_min_p'][lo:hi].copy_(torch.from_numpy(numpy.ascontiguousarray(mp).reshape(hi - lo, self.B)).to(ws['utt_min_p'].device))
            ws['utt_top_p'][lo:hi].copy_(torch.from_numpy(numpy.ascontiguousarray(pp).reshape(hi - lo, self.B)).to(ws['utt_top_p'].device))
            ws['utt_top_k'][lo:hi].copy_(torch.from_numpy(numpy.ascontiguousarray(tk).reshape(hi - lo, self.B)).to(ws['utt_top_k'].device))
            ws['utt_seed'][lo:hi].copy_(torch.from_numpy(sd.reshape(hi - lo, self.B)).to(ws['utt_seed'].device))
            ws['utt_temp'][lo:hi].copy_(torch.from_numpy(numpy.ascontiguousarray(tp).reshape(hi - lo, self.B)).to(ws['utt_temp'].device))
        if gather is not None:
            src, index = gather
            index = torch.from_numpy(index).to(ws['features'].device)
            _lib.call('samplernn_generate_stage_features', self.plan, src.data_ptr(), src.shape[0], src.stride(0),
                      index.data_ptr(), first, rows, hip._stream())
            return
        ws['features'][first:first + rows].copy_(feats.to(ws['features'].device, torch.float32))

    def _launch(self, segment, resume, k):
        """Initialises a run that does not resume, launches it and asks for its status."""
        if not resume:
            self._init_run()
        if not segment:
            _lib.call('samplernn_generate_run', self.plan, hip._stream())
        else:
            _lib.call('samplernn_generate_run_segment', self.plan, k, int(resume), hip._stream())
        self._has_run = True
        if self.persistent or segment:  # a team of the persistent kernel that gave up leaves invalid samples: fail loudly
            _lib.call('samplernn_generate_status', self.plan)

    def _init_run(self):
        """The prefix slot and the learned initial states: what a run that does not resume starts from."""
        tt = config()
        ws = self.ws
        ws['samples'].zero_()
        ws['samples'][:, :tt.BIG_FRAME_SIZE] = int(tt.Q_ZERO)  # three_tier.py:795
        # reset = (t == BIG_FRAME_SIZE): the first step of both tiers starts from the learned h0 (:334-342, 411-419)
        if self.single:
            ws['big_h'].copy_(lib.param('BigFrameLevel.h0').detach()[0].unsqueeze(0).expand(self.B, -1))
            ws['frm_h'].copy_(lib.param('FrameLevel.h0').detach()[0].unsqueeze(0).expand(self.B, -1))
        else:  # h0 [N_RNN, H0_MULT * D]: LSTM layers carry [s | c] (ops.py:552)
            for tier, tag in (('BigFrameLevel', 'big'), ('FrameLevel', 'frm')):
                h0 = lib.param(tier + '.h0').detach()
                for k in range(tt.N_RNN):
                    self.states[(tag, 'h', k)].copy_(h0[k, :tt.DIM].unsqueeze(0).expand(self.B, -1))
                    if tt.RNN_TYPE == 'LSTM':
                        self.states[(tag, 'c', k)].copy_(h0[k, tt.DIM:].unsqueeze(0).expand(self.B, -1))

    def close(self):
        if self.plan:
            _lib.load().samplernn_generate_destroy(self.plan)
            self.plan = None

"""Conditional three-tier SampleRNN -- mirrors reference sampleRNN/models/conditional/three_tier.py:
the tier builders (``big_frame_level_rnn`` :291-380, ``frame_level_rnn`` :382-450,
``sample_level_predictor`` :452-515), ``compute_cost`` (:534-636), ``getting_generation_functions``
(:703-734) and ``generate_and_save_samples`` (:750-851), with the run configuration the reference
hard-codes at import time (:145-202) as module globals.

Differences by construction (no Theano graph): the functions compute eagerly on GPU tensors through
the HIP library; ``configure(...)`` can override the hard-coded hyper-parameters (tests use small
dimensions); generation has a device-resident fast path (``DeviceGenerator`` ->
samplernn_generate_*, include/parrot_hip.h) that ``generate_and_save_samples`` uses.
"""
from __future__ import annotations

import ctypes as C
import os
from time import time

import numpy
import torch

from .... import _lib
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


_M64 = (1 << 64) - 1
DRAW_K1, DRAW_K2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9


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
    x = _splitmix64((int(seed) & _M64) ^ ((DRAW_K1 * (int(n) + 1)) & _M64))
    return float(numpy.float32(float(x >> 40) + 0.5)) / 2.0 ** 24


def utterance_seed(seed, index):
    """One 64-bit seed per utterance from a base seed: seed + K1 (index + 1) through the splitmix64 finaliser."""
    return _splitmix64(((int(seed) & _M64) + DRAW_K1 * (int(index) + 1)) & _M64)


_derive_seed = utterance_seed  # (generate_and_save_samples has an argument of that name)


def _seed_image(seeds):
    """Unsigned 64-bit seeds (Python integers or any integer array) as their two's-complement int64 image."""
    flat = [int(s) & _M64 for s in numpy.asarray(seeds, dtype=object).reshape(-1)]
    return numpy.array(flat, dtype=numpy.uint64).reshape(numpy.shape(seeds)).view(numpy.int64)


DRAW_MODES = {'sequential': 0, 'scan': 1}


def draw_mode_code(draw_mode):
    """SampleRnnGenDesc::draw_mode of a mode's name; ValueError on any other name (no device call)."""
    if draw_mode not in DRAW_MODES:
        raise ValueError("draw_mode must be one of %s, got %r" % (sorted(DRAW_MODES), draw_mode))
    return DRAW_MODES[draw_mode]


class DeviceGenerator:
    """Device-resident generation loop (samplernn_generate_*, include/parrot_hip.h)."""

    def __init__(self, batch, n_frames, temperature=0.0, seed=234, use_graph=True, packed=False, utterance_draws=False,
                 draw_mode='sequential'):
        """GRU or LSTM tiers, 1..5 stacked layers (three_tier.py:147-169).  Stacks with skip connections run on the literal
        three-function loop (generate_and_save_samples(..., use_device_loop=False) is chosen automatically).

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
        CDF, so a few draws per ten thousand land on the neighbouring code.  Argmax (temperature <= 0) is the same in both."""
        self.draw_mode = draw_mode
        mode = draw_mode_code(draw_mode)
        if SKIP_CONN:
            raise NotImplementedError("the device-resident generator does not take skip-connection stacks")
        self.B, self.T = batch, n_frames
        self.packed = bool(packed)
        self.utterance_draws = bool(utterance_draws)
        dev = lib.device()
        f = dict(device=dev, dtype=torch.float32)
        D, FS, BFS, Q = DIM, FRAME_SIZE, BIG_FRAME_SIZE, Q_LEVELS
        nfr = BFS // FS
        ew = lambda n, i=0: lops.effective_weight(n, i, WEIGHT_NORM).detach().contiguous()
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
                hip.gemm(emb, W1[pos * EMB_SIZE:(pos + 1) * EMB_SIZE], out=tbl[pos])
            w['emb_tbl'] = tbl
            # the RNN stacks of the two tiers: per layer (Input.W, Input.b | b, Recurrent_Gates, Recurrent_Candidate | -)
            self.layers = {}
            for tier, tag in (('BigFrameLevel', 'big'), ('FrameLevel', 'frm')):
                for k in range(1, N_RNN + 1):
                    if RNN_TYPE == 'GRU':
                        pre = f'{tier}.GRU{k}.Step'
                        self.layers[(tag, k - 1)] = [ew(pre + '.Input'), pb(pre + '.Input'), ew(pre + '.Recurrent_Gates'),
                                                     ew(pre + '.Recurrent_Candidate')]
                    else:
                        pre = f'{tier}.LSTM{k}.Step'
                        self.layers[(tag, k - 1)] = [ew(pre + '.Input'), lib.param(pre + '.b').detach().contiguous(),
                                                     ew(pre + '.Recurrent_Gates')]
            if single:
                for tag in ('big', 'frm'):
                    U_, bU_, Wg_, Wc_ = self.layers[(tag, 0)]
                    w.update({f'{tag}_U': U_, f'{tag}_bU': bU_, f'{tag}_Wg': Wg_, f'{tag}_Wc': Wc_})
        self.w = w
        self.single = single
        self.ws = dict(
            samples=torch.zeros(batch, BFS * n_frames, device=dev, dtype=torch.int32),
            features=torch.zeros(n_frames, batch, FEAT_DIM, **f),
            big_h=torch.zeros(batch, D, **f), frm_h=torch.zeros(batch, D, **f),
            xf_big=torch.zeros(batch, BFS, **f), xf_frm=torch.zeros(batch, FS, **f),
            feat_cur=torch.zeros(batch, FEAT_DIM, **f), gru_in=torch.zeros(batch, D, **f),
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
        d.B, d.D, d.T, d.Q, d.FS, d.BFS, d.feat_dim, d.use_graph = batch, D, n_frames, Q, FS, BFS, FEAT_DIM, int(use_graph)
        d.temperature, d.seed, d.draw_mode = float(temperature), int(seed), mode
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
        self.persistent = bool(_lib.load().samplernn_generate_is_persistent(self.plan))
        # row groups of 32 streams per launch of that kernel (PARROT_SR_PERSIST_GROUPS lifts the limit of one); 0: launches
        self.persist_groups = int(_lib.load().samplernn_generate_persist_groups(self.plan))
        self._has_run = False
        if self.utterance_draws:
            # [T, B] like starts (ring rows): row f = what an utterance that begins at big frame f draws with; utt_seed is the
            # two's-complement image of the unsigned 64-bit seed
            self.ws['utt_seed'] = torch.zeros(n_frames, batch, device=dev, dtype=torch.int64)
            self.ws['utt_temp'] = torch.zeros(n_frames, batch, **f)
            self.set_utterance_draws()

    def set_utterance_draws(self):
        """Hands the plan its per-utterance seed and temperature arrays; refused (HipCallError) once the plan has run."""
        _lib.call('samplernn_generate_set_utterance_draws', self.plan, self.ws['utt_seed'].data_ptr(),
                  self.ws['utt_temp'].data_ptr())

    def generate(self, features, starts=None, resume=False, n_frames=None, seeds=None, temperatures=None):
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
        64-bit integers (Python integers or an integer array)."""
        if (starts is not None) != self.packed:
            raise ValueError("starts must be given exactly when the plan was built with packed=True")
        resume = bool(resume)
        takes_draws = self.utterance_draws and (self.packed or not resume)
        if (seeds is not None) != takes_draws or (temperatures is not None) != takes_draws:
            raise ValueError("seeds and temperatures must both be given exactly when the plan was built with "
                             "utterance_draws=True (a plain plan takes them with resume=False only)")
        if resume and not self._has_run:
            raise ValueError("resume=True needs a run to continue: call generate(..., resume=False) first")
        segment = resume or n_frames is not None
        k = self.T - 1 if n_frames is None else int(n_frames)
        if not 1 <= k <= self.T - 1:
            raise ValueError("n_frames must be in 1 .. T-1 = %d, got %d" % (self.T - 1, k))
        rows = k if resume else (k + 1 if n_frames is not None else self.T)
        first = 1 if resume else 0
        ws = self.ws
        feats = torch.as_tensor(features)
        if segment and (feats.dim() != 3 or tuple(feats.shape[:2]) != (rows, self.B)):
            raise ValueError("features must be [%d, %d, %d], got %s" % (rows, self.B, FEAT_DIM, tuple(feats.shape)))
        if self.packed:
            st = torch.as_tensor(numpy.asarray(starts))
            if tuple(st.shape) != (rows, self.B):
                raise ValueError("starts must be [%s, B] = [%d, %d], got %s" % ("T" if not segment else "rows", rows, self.B,
                                                                                 tuple(st.shape)))
            ws['starts'][first:first + rows].copy_((st != 0).to(ws['starts'].device, torch.int32))
        if takes_draws:
            want = (rows, self.B) if self.packed else (self.B,)
            sd = _seed_image(seeds)
            tp = numpy.broadcast_to(numpy.asarray(temperatures, dtype='float32'), want) if numpy.ndim(temperatures) == 0 \
                else numpy.asarray(temperatures, dtype='float32')
            if sd.shape != want or tp.shape != want:
                raise ValueError("seeds and temperatures must be %s, got %s and %s" % (list(want), sd.shape, tp.shape))
            # (a plain plan: one utterance per stream, prefix in slot 0 -- the row of slot 1, like a start flagged there)
            lo, hi = (first, first + rows) if self.packed else (1, 2)
            ws['utt_seed'][lo:hi].copy_(torch.from_numpy(sd.reshape(hi - lo, self.B)).to(ws['utt_seed'].device))
            ws['utt_temp'][lo:hi].copy_(torch.from_numpy(numpy.ascontiguousarray(tp).reshape(hi - lo, self.B)).to(ws['utt_temp'].device))
        if not segment:
            ws['features'].copy_(feats.to(ws['features'].device, torch.float32))
        else:
            ws['features'][first:first + rows].copy_(feats.to(ws['features'].device, torch.float32))
        if not resume:
            self._init_run()
        if not segment:
            _lib.call('samplernn_generate_run', self.plan, hip._stream())
        else:
            _lib.call('samplernn_generate_run_segment', self.plan, k, int(resume), hip._stream())
        self._has_run = True
        if self.persistent or segment:  # a team of the persistent kernel that gave up leaves invalid samples: fail loudly
            _lib.call('samplernn_generate_status', self.plan)
        if not segment:
            return ws['samples']
        return ws['samples'][:, BIG_FRAME_SIZE * first:BIG_FRAME_SIZE * (k + 1)].clone()

    def _init_run(self):
        """The prefix slot and the learned initial states: what a run that does not resume starts from."""
        ws = self.ws
        ws['samples'].zero_()
        ws['samples'][:, :BIG_FRAME_SIZE] = int(Q_ZERO)  # three_tier.py:795
        # reset = (t == BIG_FRAME_SIZE): the first step of both tiers starts from the learned h0 (:334-342, 411-419)
        if self.single:
            ws['big_h'].copy_(lib.param('BigFrameLevel.h0').detach()[0].unsqueeze(0).expand(self.B, -1))
            ws['frm_h'].copy_(lib.param('FrameLevel.h0').detach()[0].unsqueeze(0).expand(self.B, -1))
        else:  # h0 [N_RNN, H0_MULT * D]: LSTM layers carry [s | c] (ops.py:552)
            for tier, tag in (('BigFrameLevel', 'big'), ('FrameLevel', 'frm')):
                h0 = lib.param(tier + '.h0').detach()
                for k in range(N_RNN):
                    self.states[(tag, 'h', k)].copy_(h0[k, :DIM].unsqueeze(0).expand(self.B, -1))
                    if RNN_TYPE == 'LSTM':
                        self.states[(tag, 'c', k)].copy_(h0[k, DIM:].unsqueeze(0).expand(self.B, -1))

    def close(self):
        if self.plan:
            _lib.load().samplernn_generate_destroy(self.plan)
            self.plan = None


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


def build_packed_inputs(utterances, stream, first_slot, T, n_streams):
    """(features [T, n_streams, 63] float32, starts [T, n_streams] int32) of a packing: utterance i's frame j at slot
    first_slot[i] + j of stream[i], zeros elsewhere; starts[first_slot[i] + 1][stream[i]] = 1 wherever that slot is
    below T (the generator overwrites slot first_slot[i] with the Q/2 prefix there and restarts the stream's state)."""
    feat_dim = numpy.asarray(utterances[0]).shape[1] if len(utterances) else FEAT_DIM
    features = numpy.zeros((T, n_streams, feat_dim), dtype='float32')
    starts = numpy.zeros((T, n_streams), dtype='int32')
    for u, b, s in zip(utterances, stream, first_slot):
        u = numpy.asarray(u, dtype='float32')
        if not (0 <= b < n_streams and 0 <= s and s + u.shape[0] <= T):
            raise ValueError("utterance of %d frames does not fit at slot %d of stream %d" % (u.shape[0], s, b))
        features[s:s + u.shape[0], b] = u
        if s + 1 < T:
            starts[s + 1, b] = 1
    return features, starts


def build_packed_draws(seeds, temperatures, stream, first_slot, T, n_streams):
    """(utt_seed [T, n_streams] uint64, utt_temp [T, n_streams] float32) of a packing, the sibling of build_packed_inputs:
    utterance i's seed and temperature on the row of its start flag, first_slot[i] + 1 of stream[i], wherever that row is
    below T (an utterance that is its prefix alone in the last slot draws nothing); zeros elsewhere."""
    utt_seed = numpy.zeros((T, n_streams), dtype=numpy.uint64)
    utt_temp = numpy.zeros((T, n_streams), dtype='float32')
    for sd, tp, b, s in zip(seeds, temperatures, stream, first_slot):
        if not (0 <= b < n_streams and 0 <= s < T):
            raise ValueError("no slot %d in stream %d" % (s, b))
        if s + 1 < T:
            utt_seed[s + 1, b] = int(sd) & _M64
            utt_temp[s + 1, b] = tp
    return utt_seed, utt_temp


def _per_utterance(seeds, temperatures, n, default_temperature):
    """seeds: one per utterance; temperatures: one per utterance, a scalar, or None = default_temperature."""
    seeds = [int(s) & _M64 for s in seeds]
    if temperatures is None:
        temperatures = default_temperature
    temperatures = [float(temperatures)] * n if numpy.ndim(temperatures) == 0 else [float(t) for t in temperatures]
    if len(seeds) != n or len(temperatures) != n:
        raise ValueError("%d utterances, but %d seeds and %d temperatures" % (n, len(seeds), len(temperatures)))
    return seeds, temperatures


def generate_packed(utterances, n_streams=32, temperature=TEMPERATURE, seed=234, use_graph=True, seeds=None,
                    temperatures=None, draw_mode='sequential'):
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

    draw_mode: 'sequential' or 'scan', see DeviceGenerator."""
    draw_mode_code(draw_mode)
    if SKIP_CONN:
        raise NotImplementedError("the device-resident generator does not take skip-connection stacks")
    utterances = [numpy.asarray(u, dtype='float32') for u in utterances]
    if seeds is None and temperatures is not None:
        raise ValueError("temperatures per utterance need seeds per utterance")
    if seeds is not None:  # (before a plan is created)
        seeds, temperatures = _per_utterance(seeds, temperatures, len(utterances), temperature)
    if not utterances:
        return []
    stream, first_slot, T = pack_utterances([u.shape[0] for u in utterances], n_streams)
    features, starts = build_packed_inputs(utterances, stream, first_slot, T, n_streams)
    gen = DeviceGenerator(n_streams, T, temperature=temperature, seed=seed, use_graph=use_graph, packed=True,
                          utterance_draws=seeds is not None, draw_mode=draw_mode)
    try:
        if seeds is not None:
            utt_seed, utt_temp = build_packed_draws(seeds, temperatures, stream, first_slot, T, n_streams)
            samples = gen.generate(features, starts, seeds=utt_seed, temperatures=utt_temp).cpu().numpy()
        else:
            samples = gen.generate(features, starts).cpu().numpy()
    finally:
        gen.close()
    return unpack_samples(samples, [u.shape[0] for u in utterances], stream, first_slot)


def unpack_samples(samples, lengths, stream, first_slot):
    """The utterances' pieces of a packed run's samples [B, 80 T].  (The prefix of a one-frame utterance in the last slot
    of the plan has no period behind it that would write it: it is Q/2 by definition.)"""
    T = samples.shape[1] // BIG_FRAME_SIZE
    out = []
    for n, b, s in zip(lengths, stream, first_slot):
        piece = numpy.array(samples[b, BIG_FRAME_SIZE * s:BIG_FRAME_SIZE * (s + n)], dtype='int32')
        if s + 1 >= T:
            piece[:BIG_FRAME_SIZE] = Q_ZERO
        out.append(piece)
    return out


def generate_stream(features, segment_frames, temperature=TEMPERATURE, seed=234, use_graph=True, gen=None,
                    draw_mode='sequential'):
    """Generator over a rectangle features [N, B, 63] on a plan of segment_frames + 1 slots used as a ring: yields int32
    arrays [B, 80 n] -- the first one holds the Q/2 prefix and up to segment_frames frames, every later one up to
    segment_frames frames -- whose concatenation is the [B, 80 N] result of DeviceGenerator(B, N).generate(features), bit
    for bit, seeded draws included.  The plan does not grow with N, and the first samples are out after segment_frames
    periods.  gen: a plain DeviceGenerator(B, segment_frames + 1) of the caller's to run on (it is left open; temperature,
    seed, use_graph and draw_mode are then the plan's); default: a plan of its own for this call, with draw_mode
    'sequential' or 'scan' (see DeviceGenerator)."""
    draw_mode_code(draw_mode)
    if SKIP_CONN:
        raise NotImplementedError("the device-resident generator does not take skip-connection stacks")
    features = numpy.asarray(features, dtype='float32')
    S = int(segment_frames)
    if S < 1:
        raise ValueError("segment_frames must be at least 1")
    if features.ndim != 3 or features.shape[0] < 2:
        raise ValueError("features must be [N, B, %d] with N >= 2 (the prefix slot and one frame)" % FEAT_DIM)
    N, B = features.shape[0], features.shape[1]
    own = gen is None
    if own:
        gen = DeviceGenerator(B, S + 1, temperature=temperature, seed=seed, use_graph=use_graph, draw_mode=draw_mode)
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

    draw_mode: 'sequential' or 'scan', the plan's (see DeviceGenerator); a run_segment of the caller's does not see it."""

    def __init__(self, n_streams, segment_frames, temperature=0.0, seed=234, use_graph=True, run_segment=None,
                 utterance_draws=False, draw_mode='sequential'):
        draw_mode_code(draw_mode)
        if SKIP_CONN:
            raise NotImplementedError("the device-resident generator does not take skip-connection stacks")
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
                                       packed=True, utterance_draws=self.utterance_draws, draw_mode=draw_mode)
            run_segment = self._run_on_device
        self._run = run_segment
        self._resume = False
        self._next_ticket = 0
        self._slots_run = 0            # periods run so far: slot s of this segment is absolute slot _slots_run + s
        self.running = [None] * self.B
        self.queue = []
        self._features = {}
        self._draws = {}               # ticket -> (seed, temperature), until the utterance's start flag has been placed
        self.record = {}

    def _run_on_device(self, features, starts, resume, seeds=None, temperatures=None):
        draws = {} if seeds is None else dict(seeds=seeds, temperatures=temperatures)
        if resume:
            return self.gen.generate(features, starts, resume=True, n_frames=features.shape[0], **draws).cpu().numpy()
        n = features.shape[0]  # the first segment: slot 0 is the run's prefix slot, no stream uses it
        features = numpy.concatenate([numpy.zeros_like(features[:1]), features])
        starts = numpy.concatenate([numpy.zeros_like(starts[:1]), starts])
        draws = {k: numpy.concatenate([numpy.zeros_like(v[:1]), v]) for k, v in draws.items()}
        return self.gen.generate(features, starts, n_frames=n, **draws).cpu().numpy()[:, BIG_FRAME_SIZE:]

    def submit(self, features, seed=None, temperature=None):
        """features [n, 63], n >= 1 (frame 0 is the prefix slot) -> the utterance's ticket, numbered in submission order.
        seed (an unsigned 64-bit integer) and temperature (default: the generator's): with utterance_draws=True only, where
        the seed is required."""
        if (seed is not None) != self.utterance_draws or (temperature is not None and not self.utterance_draws):
            raise ValueError("a seed (and a temperature) per utterance is given exactly when the generator was built with "
                             "utterance_draws=True")
        features = numpy.asarray(features, dtype='float32')
        if features.ndim != 2 or features.shape[0] < 1 or features.shape[1] != FEAT_DIM:
            raise ValueError("an utterance is [n, %d] conditioning frames with n >= 1, got %s" % (FEAT_DIM, features.shape))
        ticket = self._next_ticket
        self._next_ticket += 1
        if self.utterance_draws:
            self._draws[ticket] = (int(seed) & _M64, self.temperature if temperature is None else float(temperature))
        self._features[ticket] = features
        self.queue.append((ticket, features.shape[0]))
        return ticket

    def idle(self):
        return not self.queue and all(r is None for r in self.running)

    def step(self):
        """Runs one segment; returns [(ticket, chunk int32 [80 k], done)] for every utterance that had slots in it."""
        placements, starts, n, self.running, self.queue = schedule_segment(self.running, self.queue, self.B, self.S)
        if n == 0:
            return []
        feats = numpy.zeros((n, self.B, FEAT_DIM), dtype='float32')
        flags = numpy.zeros((n, self.B), dtype='int32')
        for ticket, b, slot, frame, count in placements:
            feats[slot - 1:slot - 1 + count, b] = self._features[ticket][frame:frame + count]
            if frame == 0:
                self.record[ticket] = (b, self._slots_run + slot)
        for slot, b in starts:
            flags[slot - 1, b] = 1
        draws = {}
        if self.utterance_draws:
            # on the row of the utterance's start flag: the slot of its frame 1, in the segment that holds that frame even
            # when its prefix was the last slot of the segment before
            draws = dict(seeds=numpy.zeros((n, self.B), dtype=numpy.uint64),
                         temperatures=numpy.zeros((n, self.B), dtype='float32'))
            for ticket, b, slot, frame, count in placements:
                if frame <= 1 < frame + count:
                    row = slot - frame  # = (slot + 1 - frame) - 1
                    assert flags[row, b] == 1
                    draws['seeds'][row, b], draws['temperatures'][row, b] = self._draws[ticket]
        samples = numpy.asarray(self._run(feats, flags, self._resume, **draws))
        if samples.shape != (self.B, BIG_FRAME_SIZE * n):
            raise ValueError("the segment runner returned %s, not %s" % (samples.shape, (self.B, BIG_FRAME_SIZE * n)))
        self._resume = True
        self._slots_run += n
        out = []
        for ticket, b, slot, frame, count in placements:
            chunk = numpy.array(samples[b, BIG_FRAME_SIZE * (slot - 1):BIG_FRAME_SIZE * (slot - 1 + count)], dtype='int32')
            if frame == 0:
                chunk[:BIG_FRAME_SIZE] = Q_ZERO  # (the period that would write it may lie in the next segment)
            done = frame + count == self._features[ticket].shape[0]
            if done:
                del self._features[ticket]
                self._draws.pop(ticket, None)
            out.append((ticket, chunk, done))
        return out

    def drain(self):
        """Steps until nothing is queued or running; returns the chunks of all those steps in order."""
        out = []
        while not self.idle():
            out += self.step()
        return out

    def close(self):
        if self.gen is not None:
            self.gen.close()
            self.gen = None


def write_audio_file(name, data, path_to_save):
    """three_tier.py:739-748."""
    import scipy.io.wavfile
    data = data.astype('float32')
    data -= data.min()
    data /= data.max()
    data -= 0.5
    data *= 0.95
    scipy.io.wavfile.write(os.path.join(path_to_save, name + '.wav'), BITRATE, data)


def generate_and_save_samples(tag, path_to_save=None, features=None, features_length=None, noise_level=0.,
                              big_frame_level_generate_fn=None, frame_level_generate_fn=None,
                              sample_level_generate_fn=None, npy_address=None, temperature=TEMPERATURE,
                              use_device_loop=True, pack_streams=0, stream_frames=0, utterance_seed=None,
                              draw_mode='sequential'):
    """three_tier.py:750-851.  With use_device_loop (default) the per-sample loop runs on the GPU
    (DeviceGenerator); otherwise the reference's three-function Python loop is executed literally.

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
    (DeviceGenerator), in the rectangle, packed and streamed modes alike.  'scan' needs the device loop."""
    total_time = time()
    if draw_mode_code(draw_mode) != 0 and not (use_device_loop and not SKIP_CONN):
        raise ValueError("draw_mode='scan' needs the device-resident generator")
    per_utt = utterance_seed is not None
    if per_utt and not (use_device_loop and not SKIP_CONN):
        raise ValueError("utterance_seed needs the device-resident generator")
    if npy_address is not None:
        test_feats = numpy.load(npy_address).astype('float32')  # [T,B,63]
    else:
        assert features is not None
        test_feats = numpy.asarray(features, dtype='float32')
    n_seqs, n_frames = test_feats.shape[1], test_feats.shape[0]
    LENGTH = n_frames * BIG_FRAME_SIZE
    if stream_frames > 0 and features_length is not None:
        lens = [min(max(int(n), 1), n_frames) for n in features_length]
        n_streams = int(pack_streams) if pack_streams > 0 else 32
        if path_to_save is not None:
            os.makedirs(path_to_save, exist_ok=True)
        sg = StreamingGenerator(n_streams, int(stream_frames), temperature=temperature, utterance_draws=per_utt,
                                draw_mode=draw_mode)
        chunks = [[] for _ in range(n_seqs)]
        pieces = [None] * n_seqs
        try:
            for i in range(n_seqs):
                draws = dict(seed=_derive_seed(utterance_seed, i)) if per_utt else {}
                assert sg.submit(test_feats[:lens[i], i], **draws) == i
            while not sg.idle():
                for i, chunk, done in sg.step():
                    chunks[i].append(chunk)
                    if not done:
                        continue
                    pieces[i] = samp = numpy.concatenate(chunks[i])
                    chunks[i] = None
                    if path_to_save is not None:
                        if Q_TYPE == 'mu-law':
                            samp = hip.mu2linear(torch.from_numpy(samp.astype('int32')).to(lib.device())).cpu().numpy()
                        write_audio_file("sample_{}_{}".format(tag, i), samp, path_to_save)
        finally:
            sg.close()
        total_time = time() - total_time
        print("{} samples of {} seconds in all generated in {} seconds ({} streams, segments of {} frames).".format(
            n_seqs, sum(lens) * BIG_FRAME_SIZE / float(BITRATE), total_time, n_streams, int(stream_frames)))
        return pieces
    if pack_streams > 0 and features_length is not None:
        lens = [min(max(int(n), 1), n_frames) for n in features_length]
        seeds = [_derive_seed(utterance_seed, i) for i in range(n_seqs)] if per_utt else None
        pieces = generate_packed([test_feats[:lens[i], i] for i in range(n_seqs)], n_streams=int(pack_streams),
                                 temperature=temperature, seeds=seeds, draw_mode=draw_mode)
        total_time = time() - total_time
        print("{} samples of {} seconds in all generated in {} seconds ({} packed streams).".format(
            n_seqs, sum(lens) * BIG_FRAME_SIZE / float(BITRATE), total_time, int(pack_streams)))
        if path_to_save is not None:
            os.makedirs(path_to_save, exist_ok=True)
            for i, samp in enumerate(pieces):
                if Q_TYPE == 'mu-law':
                    samp = hip.mu2linear(torch.from_numpy(samp.astype('int32')).to(lib.device())).cpu().numpy()
                write_audio_file("sample_{}_{}".format(tag, i), samp, path_to_save)
        return pieces
    if use_device_loop and not SKIP_CONN:  # (the device loop does not take the skip-connection stacks: literal loop)
        gen = DeviceGenerator(n_seqs, n_frames, temperature=temperature, utterance_draws=per_utt, draw_mode=draw_mode)
        draws = dict(seeds=[_derive_seed(utterance_seed, i) for i in range(n_seqs)],
                     temperatures=float(temperature)) if per_utt else {}
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
    if path_to_save is not None:
        os.makedirs(path_to_save, exist_ok=True)
        for i in range(n_seqs):
            samp = samples[i, :int(features_length[i]) * 80] if features_length is not None else samples[i]
            if Q_TYPE == 'mu-law':
                samp = hip.mu2linear(torch.from_numpy(samp.astype('int32')).to(lib.device())).cpu().numpy()
            write_audio_file("sample_{}_{}".format(tag, i), samp, path_to_save)
    return samples

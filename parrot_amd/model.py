"""Parrot: the attention-GRU encoder-decoder that emits vocoder feature frames.

Host-side mirror of reference model.py (``Parrot``, ``Encoder``, ``RecurrentWithFork``) with the
same constructor keywords, method names and return conventions (model.py:250-277, 508-554,
1061-1083).  Where the reference builds a Theano graph and lets Blocks/Theano run it, this class
drives the HIP library directly:

  * ``compute_cost``    -> encoder GRU scan plan + batched MFMA GEMMs + decoder scan plan
                           (parrot_decoder_seq_fwd/bwd, include/parrot_hip.h) + masked cost;
                           the returned cost is a torch scalar whose ``backward()`` runs the
                           hand-written reverse pass and fills the flat gradient buffer;
  * ``sample_model``    -> parrot_sample_run (whole autoregressive loop in one hipGraph); the decode half
                           lives in decode.py (``_DecodeMixin``: workspace, plan, the sample_* calls);
  * parameters          -> one flat float32 buffer, exposed under the Blocks brick paths
                           (``/parrot/rnn1.state_to_state`` ...) as views.

Generalisations beyond the reference (flagged in SURVEY.md 8a): ``num_layers`` in {1,2,3} (the
reference hard-wires 3) and ``encoder_literal`` (True reproduces the reference's encoder scan over
the batch axis), ``cell_type='lstm'`` (BASELINE configs[3]).  ``layer_norm=True`` runs on the chunk-skewed scan
schedule (in-scan normalised projections); ``raw_output=True`` trains the SampleRNN head on the predicted frames
inside compute_cost (model.py:793-820).
"""
from __future__ import annotations

import collections
import ctypes as C
from collections import OrderedDict

import numpy
import torch

from . import _lib, ops
from .bricks import Brick, Constant, IsotropicGaussian
from .decode import _DecodeMixin, compose_readout_output  # noqa: F401  (compose_readout_output: also imported from here)
from .params import ParamStore
from .utils import env_int

floatX = "float32"


def _simple_norm(x, eps=1e-5):
    """model.py:24-27."""
    return (x - x.mean(-1, keepdim=True)) / (eps + x.std(-1, unbiased=False, keepdim=True))


def logsumexp(x, axis=None):
    """model.py:37-41."""
    x_max = x.max(axis, keepdim=True)[0]
    z = torch.log(torch.exp(x - x_max).sum(axis, keepdim=True)) + x_max
    return z.sum(axis)


def cost_gmm(y, mu, sig, weight):
    """model.py:65-91 (Gaussian-mixture negative log-likelihood)."""
    shape_y = y.shape
    k = weight.shape[-1]
    y2 = y.reshape(-1, shape_y[-1])[..., None]
    mu = mu.reshape(-1, shape_y[-1], k)
    sig = sig.reshape(-1, shape_y[-1], k)
    weight = weight.reshape(-1, k)
    inner = -0.5 * ((y2 - mu) ** 2 / sig ** 2 + 2 * torch.log(sig) + float(numpy.log(2 * numpy.pi))).sum(-2)
    nll = -logsumexp(torch.log(weight) + inner, -1)
    return nll.reshape(shape_y[:-1])


class _CostFn(torch.autograd.Function):
    """Ties the hand-written backward pass of one compute_cost call to ``cost.backward()``."""

    @staticmethod
    def forward(ctx, anchor, engine, token, cost_value):
        ctx.engine, ctx.token = engine, token
        return cost_value.clone()

    @staticmethod
    def backward(ctx, g):
        ctx.engine._backward(ctx.token, g)
        return None, None, None, None


class _LRU(collections.OrderedDict):
    """Bounded cache: `get` refreshes an entry, inserting beyond `cap` entries evicts the least recently used one
    through `on_evict` (which frees the plan / graph the entry owns)."""

    def __init__(self, cap, on_evict):
        super().__init__()
        self.cap, self.on_evict = max(1, cap), on_evict

    def get(self, key, default=None):
        if key in self:
            self.move_to_end(key)
            return super().__getitem__(key)
        return default

    def __setitem__(self, key, value):
        super().__setitem__(key, value)
        self.move_to_end(key)
        while len(self) > self.cap:
            _, old = self.popitem(last=False)
            self.on_evict(old)

    def clear(self):
        while len(self):
            _, old = self.popitem(last=False)
            self.on_evict(old)


class Parrot(_DecodeMixin, Brick):
    def __init__(
            self,
            input_dim=420, output_dim=63, rnn_h_dim=1024, readouts_dim=1024,
            weak_feedback=False, full_feedback=False, feedback_noise_level=None,
            layer_norm=False, use_speaker=False, num_speakers=21, speaker_dim=128,
            which_cost='MSE', k_gmm=20, sampling_bias=0, epsilon=1e-5, num_characters=43,
            attention_type='graves', attention_size=10, attention_alignment=1.,
            sharpening_coeff=1., timing_coeff=1., encoder_type=None, encoder_dim=128,
            raw_output=False,
            # --- extensions (not in the reference) ---
            num_layers=3, encoder_literal=True, use_graph=True, seed=1234,
            cell_type='gru', lstm_forget_bias=3.0, compute_dtype='float32', decode_dtype='float32',
            **kwargs):
        kwargs.setdefault('name', 'parrot')
        kwargs.setdefault('weights_init', IsotropicGaussian(0.01))  # train.py:30
        kwargs.setdefault('biases_init', Constant(0.))              # train.py:31
        super().__init__(seed=seed, **kwargs)
        assert which_cost in ('MSE', 'GMM')
        assert attention_type in ('graves', 'softmax')
        assert encoder_type in (None, 'bidirectional')  # model.py:209
        assert 1 <= num_layers <= _lib.MAX_LAYERS
        assert cell_type in ('gru', 'lstm')
        assert compute_dtype in ('float32', 'bf16', 'bfloat16')
        # bf16 (BASELINE configs[3]): bf16 MFMA operands (weights AND activations rounded where they enter a GEMM of
        # the decoder: scan steps, batched projections, readouts, deferred weight gradients), f32 accumulation, f32
        # master weights / states / gradients / optimiser.  Encoder, attention window and cost stay f32.
        self.compute_bf16 = compute_dtype != 'float32'
        # decode_dtype='bf16': the recurrent-layer products of the decode loop (sample_model) round both operands to bf16
        # and accumulate in f32 -- the arithmetic compute_dtype='bf16' trains in.  A switch of its own: the default decodes
        # with f32 operands whatever compute_dtype says.  LSTM decoders on the persistent machine only; anything else is
        # refused when the decode workspace is made (_sample_workspace), never decoded in f32 instead.
        assert decode_dtype in ('float32', 'bf16', 'bfloat16')
        self.decode_bf16 = decode_dtype != 'float32'
        self.input_dim, self.output_dim = input_dim, output_dim
        self.rnn_h_dim, self.readouts_dim = rnn_h_dim, readouts_dim
        self.layer_norm, self.which_cost, self.use_speaker = layer_norm, which_cost, use_speaker
        self.full_feedback = full_feedback
        self.weak_feedback = bool(weak_feedback or full_feedback)  # model.py:485
        self.feedback_noise_level = feedback_noise_level
        self.epsilon = epsilon
        self.num_characters, self.attention_type = num_characters, attention_type
        self.attention_alignment, self.attention_size = attention_alignment, attention_size
        self.sharpening_coeff, self.timing_coeff = sharpening_coeff, timing_coeff
        self.encoder_type, self.encoder_dim = encoder_type, encoder_dim
        self.encoded_input_dim = 2 * encoder_dim if encoder_type == 'bidirectional' else input_dim
        self.raw_output = raw_output
        self.num_speakers, self.speaker_dim = num_speakers, speaker_dim
        self.k_gmm, self.sampling_bias = k_gmm, sampling_bias
        self.num_layers, self.encoder_literal, self.use_graph = num_layers, encoder_literal, use_graph
        # Pre-activation groups of a decoder layer: (key, width, Fork output suffix, packed matrix, name of the
        # recurrent block).  GRU (Blocks GatedRecurrent): gates 2H + candidate H.  LSTM (cell_type='lstm', the
        # BASELINE configs[3] generalisation; cell algebra of sampleRNN/lib/ops.py:505-553): one 4H group.
        self.cell_type, self.lstm_forget_bias = cell_type, float(lstm_forget_bias)
        H_ = rnn_h_dim
        if cell_type == 'lstm':
            self._groups = [('g', 4 * H_, 'inputs', 'dec.Wg', 'W_state')]
        else:
            self._groups = [('g', 2 * H_, 'gates', 'dec.Wg', 'state_to_gates'),
                            ('c', H_, 'inputs', 'dec.Wc', 'state_to_state')]

        self.store = ParamStore()
        self._declare_parameters()
        self._allocated = False
        # Workspaces + instantiated hipGraph plans are cached per shape (T, B, U) -- with real data U changes every
        # batch and the last TBPTT window of a batch has its own T, so the caches are LRU-bounded (PARROT_WS_CACHE
        # entries each, default 6) and an evicted entry destroys its plan: HBM use stays bounded however many
        # distinct shapes a run sees.  Only the most recent compute_cost can have a backward pending (self._saved is
        # a single slot) and its encoder + decoder workspaces are the two most recently used entries, so an
        # eviction never touches a workspace that is still needed (cap >= 4).
        cap = max(4, env_int('PARROT_WS_CACHE', 6))
        self._train_ws = _LRU(cap, self._evict_train_ws)
        self._sample_ws = _LRU(max(2, cap // 2), self._evict_sample_ws)
        self._carry = {}
        self._token = 0
        self._saved = None
        if raw_output:
            from .sampleRNN.models.conditional import three_tier  # noqa: F401  (import check only)
            self.sampleRnn = SampleRnn(name='samplernn', device=self.device)

    # ------------------------------------------------------------------ parameters
    def _declare_parameters(self):
        s = self.store
        H, R, O, E = self.rnn_h_dim, self.readouts_dim, self.output_dim, self.encoded_input_dim
        A, L = self.attention_size, self.num_layers
        P = '/' + self.name

        def fork_separate(name, din, outs):
            for on, od in outs:
                s.add(f'{P}/{name}/fork_{on}.W', (din, od), 'weight')
                s.add(f'{P}/{name}/fork_{on}.b', (od,), 'bias')

        if self.encoder_type == 'bidirectional':
            D, ED = self.input_dim, self.encoder_dim
            s.add(f'{P}/encoder/embed_label.W', (self.num_characters, D), 'weight')
            for d in ('forward', 'backward'):
                q = f'{P}/encoder/encoder/{d}'
                s.add(f'{q}/fork/fork_inputs.W', (D, ED), 'weight')
                s.add(f'{q}/fork/fork_inputs.b', (ED,), 'bias')
                s.add(f'{q}/fork/fork_gate_inputs.W', (D, 2 * ED), 'weight')
                s.add(f'{q}/fork/fork_gate_inputs.b', (2 * ED,), 'bias')
                s.add(f'{q}/gatedrecurrent.state_to_state', (ED, ED), 'weight')
                s.add(f'{q}/gatedrecurrent.state_to_gates', (ED, 2 * ED), 'weight')
                s.add(f'{q}/gatedrecurrent.initial_state', (ED,), 'initial_state')
        # decoder layers: packed [h_l ; w ; h_1..h_{l-1}] weight matrices (include/parrot_hip.h)
        for l in range(1, L + 1):
            K = H + E + (l - 1) * H
            for key, wd, suf, mat, rec in self._groups:
                s.add(f'{mat}{l}', (K, wd), 'weight', alias=False)
            for key, wd, suf, mat, rec in reversed(self._groups):
                s.alias(f'{P}/rnn{l}.{rec}', f'{mat}{l}', rows=(0, H))
            s.add(f'{P}/rnn{l}.initial_state', (H,), 'initial_state')
            if self.cell_type == 'lstm':
                s.add(f'{P}/rnn{l}.initial_cells', (H,), 'initial_state')
            for key, wd, suf, mat, rec in reversed(self._groups):
                s.alias(f'{P}/inp_to_h{l}/fork_rnn{l}_{suf}.W', f'{mat}{l}', rows=(H, H + E))
                s.add(f'{P}/inp_to_h{l}/fork_rnn{l}_{suf}.b', (wd,), 'bias')
            for j in range(1, l):
                r0 = H + E + (j - 1) * H
                for key, wd, suf, mat, rec in reversed(self._groups):
                    s.alias(f'{P}/h{j}_to_h{l}/fork_rnn{l}_{suf}.W', f'{mat}{l}', rows=(r0, r0 + H))
                    s.add(f'{P}/h{j}_to_h{l}/fork_rnn{l}_{suf}.b', (wd,), 'bias')
        s.add('dec.WattT', (3 * A, H), 'weight', alias=False)  # h1_to_att weights, stored transposed
        s.add('dec.batt', (3 * A,), 'bias', alias=False)
        for i, n in enumerate(('alpha', 'beta', 'kappa')):
            s.alias(f'{P}/h1_to_att/fork_{n}.W', 'dec.WattT', rows=(i * A, (i + 1) * A), transpose=True)
            s.alias(f'{P}/h1_to_att/fork_{n}.b', 'dec.batt', rows=(i * A, (i + 1) * A), role='bias')
        s.add('dec.Wr', (L * H + E, R), 'weight', alias=False)
        for l in range(1, L + 1):
            s.alias(f'{P}/h{l}_to_readout.W', 'dec.Wr', rows=((l - 1) * H, l * H))
            s.add(f'{P}/h{l}_to_readout.b', (R,), 'bias')
        s.alias(f'{P}/att_to_readout.W', 'dec.Wr', rows=(L * H, L * H + E))
        s.add(f'{P}/att_to_readout.b', (R,), 'bias')
        if self.which_cost == 'MSE':
            s.add(f'{P}/readout_to_output.W', (R, O), 'weight')
            s.add(f'{P}/readout_to_output.b', (O,), 'bias')
            self._out_names = [(f'{P}/readout_to_output.W', f'{P}/readout_to_output.b', O)]
        else:
            K = self.k_gmm
            fork_separate('readout_to_output', R, [('gmm_mu', O * K), ('gmm_sigma', O * K), ('gmm_coeff', K)])
            self._out_names = [(f'{P}/readout_to_output/fork_{n}.W', f'{P}/readout_to_output/fork_{n}.b', d)
                               for n, d in (('gmm_mu', O * K), ('gmm_sigma', O * K), ('gmm_coeff', K))]
        if self.use_speaker:
            SD = self.speaker_dim
            s.add(f'{P}/lookuptable.W', (self.num_speakers, SD), 'weight')  # sample.py:83
            for l in range(1, L + 1):
                fork_separate(f'speaker_to_h{l}', SD, self._fork_outs(l))
            s.add(f'{P}/speaker_to_readout.W', (SD, R), 'weight')
            s.add(f'{P}/speaker_to_readout.b', (R,), 'bias')
            if self.which_cost == 'MSE':
                s.add(f'{P}/speaker_to_output.W', (SD, O), 'weight')
                s.add(f'{P}/speaker_to_output.b', (O,), 'bias')
                self._spk_out_names = [(f'{P}/speaker_to_output.W', f'{P}/speaker_to_output.b', O)]
            else:
                K = self.k_gmm
                fork_separate('speaker_to_output', SD,
                              [('gmm_mu', O * K), ('gmm_sigma', O * K), ('gmm_coeff', K)])
                self._spk_out_names = [
                    (f'{P}/speaker_to_output/fork_{n}.W', f'{P}/speaker_to_output/fork_{n}.b', d)
                    for n, d in (('gmm_mu', O * K), ('gmm_sigma', O * K), ('gmm_coeff', K))]
        self._fb_layers = []
        if self.weak_feedback:
            self._fb_layers = [1]
        if self.full_feedback:
            self._fb_layers = list(range(1, L + 1))
        for l in self._fb_layers:
            fork_separate(f'out_to_h{l}', O, self._fork_outs(l))
        s.add(f'{P}.initial_w', (E,), 'initial_state')

    def _fork_outs(self, l):
        """Fork output (name, width) list feeding layer l, reference order (inputs before gates,
        model.py:331-349)."""
        return [(f'rnn{l}_{suf}', wd) for key, wd, suf, mat, rec in reversed(self._groups)]

    def allocate(self):
        if not self._allocated:
            self.store.allocate(self._dev())
            self._allocated = True
        return self

    def initialize(self, gen=None):
        """Initializable.initialize (train.py:79-80): weights ~ weights_init, biases ~ biases_init,
        initial states zero (model.py:502-506)."""
        self.allocate()
        if gen is None:
            gen = torch.Generator().manual_seed(int(self.seed))
        with torch.no_grad():
            for name in self.store.names():
                t = self.store.param(name)
                role = self.store.role(name)
                if role == 'weight':
                    t.copy_(self.weights_init.generate(gen, tuple(t.shape)).to(t.device))
                elif role == 'bias':
                    t.copy_(self.biases_init.generate(gen, tuple(t.shape)).to(t.device))
                else:
                    t.zero_()
            if self.cell_type == 'lstm':  # forget-gate bias (sampleRNN/lib/ops.py:526) lives in the learnable bias
                H = self.rnn_h_dim
                for l in range(1, self.num_layers + 1):
                    self._p(f'/inp_to_h{l}/fork_rnn{l}_inputs.b')[H:2 * H].add_(self.lstm_forget_bias)
        self.initialized = True
        return self

    # Blocks Model-like accessors -------------------------------------------------
    def get_parameter_dict(self, prefix=""):
        self.allocate()
        return self.store.named_parameters()

    def get_parameter_values(self):
        return OrderedDict((k, v.detach().cpu().numpy().copy()) for k, v in self.get_parameter_dict().items())

    def set_parameter_values(self, values):
        """Model.set_parameter_values (sample.py:127): name -> ndarray / tensor."""
        self.allocate()
        with torch.no_grad():
            for k, v in values.items():
                if k not in self.store._aliases:
                    raise KeyError(f'unknown parameter {k}')
                t = self.store.param(k)
                v = torch.as_tensor(numpy.asarray(v) if not isinstance(v, torch.Tensor) else v)
                if tuple(v.shape) != tuple(t.shape):
                    raise ValueError(f'{k}: shape {tuple(v.shape)} != {tuple(t.shape)}')
                t.copy_(v.to(t.device, torch.float32))

    def get_gradient_dict(self):
        return self.store.named_gradients()

    def early_gradient_range(self):
        """[lo, hi) of the flat gradient buffer that is complete BEFORE the backward scan starts: the readout stack
        (`dec.Wr`, the `*_to_readout` biases) and the output layer (model.py:739-755) -- one contiguous run of the
        declaration order, 2.4 of the 13.9 M parameters at configs[1].  None when the raw-audio head routes the output
        gradient through torch autograd first (its order is not ours to promise)."""
        self.allocate()
        if self.raw_output:
            return None
        names = list(self.store._entries)
        i0 = names.index('dec.Wr')
        early = {'dec.Wr', f'/{self.name}/att_to_readout.b'}
        early |= {f'/{self.name}/h{l}_to_readout.b' for l in range(1, self.num_layers + 1)}
        for wn, bn, _ in self._out_names:
            early |= {wn, bn}
        i1 = i0
        while i1 < len(names) and names[i1] in early:
            i1 += 1
        lo = self.store.offsets[names[i0]][0]
        o, n = self.store.offsets[names[i1 - 1]]
        return lo, o + (n + 3) // 4 * 4

    @property
    def flat_parameters(self):
        return self.allocate().store.flat

    @property
    def flat_gradients(self):
        return self.allocate().store.flat_grad

    def zero_grad(self):
        self.store.zero_grad()

    def _p(self, short):
        return self.store.param(f'/{self.name}{short}')

    def _g(self, short):
        return self.store.grad(f'/{self.name}{short}')

    # ------------------------------------------------------------------ reference surface
    def symbolic_input_variables(self):
        """model.py:508-527.  There is no symbolic graph here; the names are returned in the
        reference order so callers can bind batch sources by name (Blocks does, model.py:509-522)."""
        speaker = 'speaker_index' if self.use_speaker else None
        raw = 'raw_audio' if self.raw_output else None
        return 'features', 'features_mask', 'labels', 'labels_mask', speaker, 'start_flag', raw

    def initial_states(self, batch_size):
        """model.py:529-549: (initial_h1, last_h1, ..., initial_w, last_w, initial_k, last_k).
        For num_layers < 3 the missing layers are returned as None."""
        dev = self._dev()
        f = dict(device=dev, dtype=torch.float32)
        out = []
        carry = self._get_carry(batch_size)
        for l in range(1, 4):
            if l <= self.num_layers:
                out += [self._p(f'/rnn{l}.initial_state').unsqueeze(0).expand(batch_size, -1), carry['h'][l - 1]]
            else:
                out += [None, None]
        out += [self._p('.initial_w').unsqueeze(0).expand(batch_size, -1), carry['w'],
                torch.zeros(batch_size, self.attention_size, **f), carry['k']]
        return tuple(out)

    def _get_carry(self, B):
        c = self._carry.get(B)
        if c is None:
            f = dict(device=self._dev(), dtype=torch.float32)
            c = dict(h=[torch.zeros(B, self.rnn_h_dim, **f) for _ in range(self.num_layers)],
                     c=[torch.zeros(B, self.rnn_h_dim, **f) for _ in range(self.num_layers)],
                     w=torch.zeros(B, self.encoded_input_dim, **f),
                     k=torch.zeros(B, self.attention_size, **f))
            self._carry[B] = c
        return c

    def _samplernn_carry(self, B):
        c = self._carry.get(('srn', B))
        if c is None:
            c = self.sampleRnn.initial_states(B)
            self._carry[('srn', B)] = c
        return c

    def apply_updates(self, updates):
        """Applies the (shared variable, new value) pairs compute_cost returns -- what Blocks'
        GradientDescent.add_updates(extra_updates) did implicitly (train.py:108, model.py:786-791)."""
        with torch.no_grad():
            for dst, src in updates:
                dst.copy_(src)

    # ------------------------------------------------------------------ encoder
    def _encoder_dims(self, B, U):
        return (B, U) if self.encoder_literal else (U, B)

    def _enc_runner(self, B, U):
        key = ('enc', B, U)
        ws = self._train_ws.get(key)
        if ws is None:
            Te, Be = self._encoder_dims(B, U)
            run = ops.GruSeqRunner(Te, Be, self.encoder_dim, 2, [0, 1], self._dev(), use_graph=self.use_graph)
            ws = dict(run=run)
            self._train_ws[key] = ws
        return ws

    def _encoder_forward(self, labels, labels_mask, save):
        """Encoder.apply (model.py:233-247) * labels_mask (model.py:645-646)."""
        if self.encoder_type is None:
            ctx = labels.to(torch.float32) * labels_mask[..., None]
            return ctx.contiguous()
        B, U = labels.shape
        # (sampling passes save=None and keeps the products: one pass per utterance, and decoded frames follow ctx to the bit)
        tables = save is not None and self._encoder_tables(B, U)
        self._encoder_path = 'tables' if tables else 'products'
        if tables:
            return self._encoder_forward_tables(labels, labels_mask, save)
        P = '/encoder/encoder'
        emb = self._p('/encoder/embed_label.W')[labels.long()]  # LookupTable gather [B,U,D]
        x = emb if self.encoder_literal else emb.transpose(0, 1)
        x = x.contiguous()
        Te, Be, D = x.shape
        ws = self._enc_runner(B, U)
        run = ws['run']
        x2 = x.reshape(Te * Be, D)
        Wg, Wc = [], []
        for i, d in enumerate(('forward', 'backward')):
            ops.gemm(x2, self._p(f'{P}/{d}/fork/fork_inputs.W'), bias=self._p(f'{P}/{d}/fork/fork_inputs.b'),
                     out=run.inputs[i].view(Te * Be, -1))
            ops.gemm(x2, self._p(f'{P}/{d}/fork/fork_gate_inputs.W'),
                     bias=self._p(f'{P}/{d}/fork/fork_gate_inputs.b'), out=run.gate_inputs[i].view(Te * Be, -1))
            run.h[i][0].copy_(self._p(f'{P}/{d}/gatedrecurrent.initial_state').unsqueeze(0).expand(Be, -1))
            Wg.append(self._p(f'{P}/{d}/gatedrecurrent.state_to_gates'))
            Wc.append(self._p(f'{P}/{d}/gatedrecurrent.state_to_state'))
        run.bind(Wg, Wc)
        run.forward()
        out = torch.cat([run.h[0][1:], run.h[1][1:].flip(0)], dim=-1)  # [Te,Be,2*enc]
        if not self.encoder_literal:
            out = out.transpose(0, 1)
        ctx = (out * labels_mask[..., None]).contiguous()
        if save is not None:
            save.update(enc_x2=x2, enc_labels=labels, enc_mask=labels_mask)
        return ctx

    def _encoder_backward(self, dctx, save):
        if self.encoder_type is None:
            return
        if 'enc_lab32' in save:
            return self._encoder_backward_tables(dctx, save)
        labels, mask, x2 = save['enc_labels'], save['enc_mask'], save['enc_x2']
        B, U = labels.shape
        P = '/encoder/encoder'
        ED = self.encoder_dim
        run = self._enc_runner(B, U)['run']
        Te, Be = run.T, run.B
        d_out = dctx * mask[..., None]
        if not self.encoder_literal:
            d_out = d_out.transpose(0, 1)
        for i in range(2):
            run.dh[i].zero_()
        run.dh[0][1:].copy_(d_out[..., :ED])
        run.dh[1][1:].copy_(d_out[..., ED:].flip(0))
        run.backward()
        dx = torch.zeros_like(x2)
        for i, d in enumerate(('forward', 'backward')):
            dC = run.dC[i].view(Te * Be, ED)
            dG = run.dG[i].view(Te * Be, 2 * ED)
            hprev = run.h[i][:Te] if i == 0 else run.h[i][:Te].flip(0)
            hprev = hprev.reshape(Te * Be, ED)
            ops.gemm(x2.t(), dC, out=self._g(f'{P}/{d}/fork/fork_inputs.W'), accumulate=True)
            ops.gemm(x2.t(), dG, out=self._g(f'{P}/{d}/fork/fork_gate_inputs.W'), accumulate=True)
            ops.colsum(dC, out=self._g(f'{P}/{d}/fork/fork_inputs.b'), accumulate=True)
            ops.colsum(dG, out=self._g(f'{P}/{d}/fork/fork_gate_inputs.b'), accumulate=True)
            ops.gemm(run.rh[i].view(Te * Be, ED).t(), dC,
                     out=self._g(f'{P}/{d}/gatedrecurrent.state_to_state'), accumulate=True)
            ops.gemm(hprev.t(), dG, out=self._g(f'{P}/{d}/gatedrecurrent.state_to_gates'), accumulate=True)
            ops.colsum(run.dh[i][0], out=self._g(f'{P}/{d}/gatedrecurrent.initial_state'), accumulate=True)
            ops.gemm(dC, self._p(f'{P}/{d}/fork/fork_inputs.W').t(), out=dx, accumulate=True)
            ops.gemm(dG, self._p(f'{P}/{d}/fork/fork_gate_inputs.W').t(), out=dx, accumulate=True)
        demb = dx.view(Te, Be, -1)
        if not self.encoder_literal:
            demb = demb.transpose(0, 1)
        self._scatter_rows_add(self._g('/encoder/embed_label.W'), labels.long().reshape(-1),
                               demb.reshape(-1, demb.shape[-1]))

    # ------------------------------------------------------------------ encoder through label tables
    @property
    def encoder_path(self):
        """'tables' or 'products': how the last encoder pass formed the products with the embedded text (None before the
        first call and for models without an encoder)."""
        return getattr(self, '_encoder_path', None)

    def _encoder_tables(self, B, U):
        """True when the Fork products of the encoder run as lookups in projected label tables (csrc/labeltables.hip):
        every row of the embedded text is one of num_characters table rows, so x . W = (embed_label.W . W)[labels] and
        x^T . dY = embed_label.W^T . S with S the per-label sums of dY.  A bidirectional encoder whose table fits the
        segmented-sum kernel.  PARROT_ENCODER_TABLES=0 (read per step) keeps the products with the embedded text."""
        return (self.encoder_type == 'bidirectional' and self.encoder_dim % 4 == 0
                and ops.label_tables_supported(B * U, self._p('/encoder/embed_label.W').shape[0])
                and env_int('PARROT_ENCODER_TABLES', 1) != 0)

    def _enc_tables_ws(self, ws):
        if 'P' not in ws:
            Q, ED = self._p('/encoder/embed_label.W').shape[0], self.encoder_dim
            f = dict(device=self._dev(), dtype=torch.float32)
            ws['P'] = [torch.empty(Q, ED * (1 + k % 2), **f) for k in range(4)]  # per direction: inputs | gate inputs
            ws['S'] = [torch.empty(Q, ED * (1 + k % 2), **f) for k in range(4)]
            ws['seg_ws'] = None
        return ws

    def _encoder_forward_tables(self, labels, labels_mask, save):
        B, U = labels.shape
        P = '/encoder/encoder'
        Te, Be = self._encoder_dims(B, U)
        ws = self._enc_tables_ws(self._enc_runner(B, U))
        run = ws['run']
        emb_W = self._p('/encoder/embed_label.W')
        lab = (labels if self.encoder_literal else labels.t()).to(torch.int32).contiguous().view(-1)  # scan order
        Wg, Wc = [], []
        with ops.gemm_precision(ops.PRECISION_F32):  # (tables of a few thousand entries: nothing to gain from bf16 operands)
            for i, d in enumerate(('forward', 'backward')):
                ops.gemm(emb_W, self._p(f'{P}/{d}/fork/fork_inputs.W'), bias=self._p(f'{P}/{d}/fork/fork_inputs.b'),
                         out=ws['P'][2 * i])
                ops.gemm(emb_W, self._p(f'{P}/{d}/fork/fork_gate_inputs.W'),
                         bias=self._p(f'{P}/{d}/fork/fork_gate_inputs.b'), out=ws['P'][2 * i + 1])
        ops.label_gather(lab, ws['P'], [b[i].view(Te * Be, -1) for i in range(2) for b in (run.inputs, run.gate_inputs)])
        for i, d in enumerate(('forward', 'backward')):
            run.h[i][0].copy_(self._p(f'{P}/{d}/gatedrecurrent.initial_state').unsqueeze(0).expand(Be, -1))
            Wg.append(self._p(f'{P}/{d}/gatedrecurrent.state_to_gates'))
            Wc.append(self._p(f'{P}/{d}/gatedrecurrent.state_to_state'))
        run.bind(Wg, Wc)
        run.forward()
        out = torch.cat([run.h[0][1:], run.h[1][1:].flip(0)], dim=-1)  # [Te,Be,2*enc]
        if not self.encoder_literal:
            out = out.transpose(0, 1)
        ctx = (out * labels_mask[..., None]).contiguous()
        if save is not None:
            save.update(enc_lab32=lab, enc_labels=labels, enc_mask=labels_mask)
        return ctx

    def _encoder_backward_tables(self, dctx, save):
        labels, mask, lab = save['enc_labels'], save['enc_mask'], save['enc_lab32']
        B, U = labels.shape
        P = '/encoder/encoder'
        ED = self.encoder_dim
        ws = self._enc_tables_ws(self._enc_runner(B, U))
        run = ws['run']
        Te, Be = run.T, run.B
        d_out = dctx * mask[..., None]
        if not self.encoder_literal:
            d_out = d_out.transpose(0, 1)
        for i in range(2):
            run.dh[i].zero_()
        run.dh[0][1:].copy_(d_out[..., :ED])
        run.dh[1][1:].copy_(d_out[..., ED:].flip(0))
        run.backward()
        # per-label sums of the gradients of the candidate / gate inputs: all the Fork and the LookupTable need
        ws['seg_ws'] = ops.label_segsum(lab, [b[i].view(Te * Be, -1) for i in range(2) for b in (run.dC, run.dG)],
                                        ws['S'], ws['seg_ws'])
        emb_W, demb = self._p('/encoder/embed_label.W'), self._g('/encoder/embed_label.W')
        with ops.gemm_precision(ops.PRECISION_F32):
            for i, d in enumerate(('forward', 'backward')):
                for S, name in ((ws['S'][2 * i], 'fork_inputs'), (ws['S'][2 * i + 1], 'fork_gate_inputs')):
                    ops.gemm(emb_W.t(), S, out=self._g(f'{P}/{d}/fork/{name}.W'), accumulate=True)
                    ops.colsum(S, out=self._g(f'{P}/{d}/fork/{name}.b'), accumulate=True)
                    ops.gemm(S, self._p(f'{P}/{d}/fork/{name}.W').t(), out=demb, accumulate=True)
        for i, d in enumerate(('forward', 'backward')):
            dC = run.dC[i].view(Te * Be, ED)
            dG = run.dG[i].view(Te * Be, 2 * ED)
            hprev = run.h[i][:Te] if i == 0 else run.h[i][:Te].flip(0)
            hprev = hprev.reshape(Te * Be, ED)
            ops.gemm(run.rh[i].view(Te * Be, ED).t(), dC,
                     out=self._g(f'{P}/{d}/gatedrecurrent.state_to_state'), accumulate=True)
            ops.gemm(hprev.t(), dG, out=self._g(f'{P}/{d}/gatedrecurrent.state_to_gates'), accumulate=True)
            ops.colsum(run.dh[i][0], out=self._g(f'{P}/{d}/gatedrecurrent.initial_state'), accumulate=True)

    # ------------------------------------------------------------------ training workspace
    def _train_workspace(self, T, B, U):
        ws_key = ('dec', T, B, U)
        ws = self._train_ws.get(ws_key)
        if ws is not None:
            return ws
        H, E, A, L, R = self.rnn_h_dim, self.encoded_input_dim, self.attention_size, self.num_layers, self.readouts_dim
        f = dict(device=self._dev(), dtype=torch.float32)
        ws = dict(
            h=[torch.zeros(T + 1, B, H, **f) for _ in range(L)],
            w=torch.zeros(T + 1, B, E, **f), kappa=torch.zeros(T + 1, B, A, **f),
            a=torch.empty(T, B, A, **f), b=torch.empty(T, B, A, **f), phi=torch.empty(T, B, U, **f),
            dh=[torch.zeros(T + 1, B, H, **f) for _ in range(L)], dw=torch.zeros(T + 1, B, E, **f),
            dw0=torch.zeros(T + 1, B, E, **f),
            dhup=[torch.zeros(T + 1, B, H, **f) if l < L - 1 else None for l in range(L)],
            dkappa=torch.zeros(B, A, **f),
            dp=torch.empty(T, B, 3 * A, **f),
            ctx=torch.zeros(B, U, E, **f),
        )  # (`readouts` [T*B, R] comes from _readouts_buffer: the composed readout path never allocates it)
        lstm = self.cell_type == 'lstm'
        if lstm:
            ws.update(cst=[torch.zeros(T + 1, B, H, **f) for _ in range(L)],
                      gate4=[torch.empty(T, B, 4 * H, **f) for _ in range(L)],
                      dcell=[torch.zeros(B, H, **f) for _ in range(L)])
            if self.compute_bf16 and B <= 64 and H % 32 == 0:
                # second accumulators of the backward scan (ParrotDecoderDesc::dh_b ...): the transposed products of a
                # tick run as two K halves; zero-filled once (the scan stores into every slot it later reads).  (Only
                # where the C plan can take them -- B <= 64, the wide kernel's widths: ADVICE r04 -- so that nothing is
                # allocated, zeroed per window and added back for a plan that declines the split.)
                ws.update(dh_b=[torch.zeros(T + 1, B, H, **f) for _ in range(L)],
                          dhup_b=[torch.zeros(T + 1, B, H, **f) if l < L - 1 else None for l in range(L)],
                          dw_b=torch.zeros(T + 1, B, E, **f), dw0_b=torch.zeros(T + 1, B, E, **f))
        else:
            for n in ('z', 'r', 'rh', 'c'):
                ws[n] = [torch.empty(T, B, H, **f) for _ in range(L)]
        for key, wd, suf, mat, rec in self._groups:
            ws['d' + key.upper()] = [torch.empty(T, B, wd, **f) for _ in range(L)]
            ws['b' + key] = [torch.zeros(wd, **f) for _ in range(L)]
            # layers >= 2 always get the buffer: the plan batches the lower layers' projections into it
            ws['seq_' + key] = [torch.zeros(T, B, wd, **f) if (l in self._fb_layers or self.use_speaker or l >= 2)
                                else None for l in range(1, L + 1)]
        if (not lstm and L in (2, 3) and not self.compute_bf16 and not self.layer_norm and B <= 64 and H % 16 == 0 and E % 16 == 0
                and env_int('PARROT_BWD_HETERO', 1) != 0):
            # second / third accumulators of the K-balanced backward tick (ParrotDecoderDesc::dh_b ... dw0_c, plans.hip bwd8)
            ws.update(dh_b=[torch.zeros(T + 1, B, H, **f) for _ in range(L)],
                      dhup_b=[torch.zeros(T + 1, B, H, **f) if l < L - 1 else None for l in range(L)],
                      dhup_c=[torch.zeros(T + 1, B, H, **f) if l < L - 1 else None for l in range(L)],
                      dw_b=torch.zeros(T + 1, B, E, **f), dw0_b=torch.zeros(T + 1, B, E, **f),
                      dw_c=torch.zeros(T + 1, B, E, **f), dw0_c=torch.zeros(T + 1, B, E, **f))
        ln = self.layer_norm and L >= 2
        if ln:
            # (l, j) pairs, 0-based, j < l: normalised projections of h_j into layer l and their row std
            for key, wd, suf, mat, rec in self._groups:
                ws['ln_y' + key] = {(l, j): torch.empty(T, B, wd, **f) for l in range(1, L) for j in range(l)}
                ws['ln_s' + key] = {(l, j): torch.empty(T, B, **f) for l in range(1, L) for j in range(l)}
        d = _lib.DecoderDesc()
        d.cell = 1 if lstm else 0
        d.layer_norm = 1 if ln else 0
        d.bf16 = 1 if self.compute_bf16 else 0
        if ln:
            for key, wd, suf, mat, rec in self._groups:
                for (l, j), t_ in ws['ln_y' + key].items():
                    pj = l * _lib.MAX_LAYERS + j
                    getattr(d, 'ln_y' + key)[pj] = t_.data_ptr()
                    getattr(d, 'ln_s' + key)[pj] = ws['ln_s' + key][(l, j)].data_ptr()
                    getattr(d, 'ln_b' + key)[pj] = self._p(f'/h{j + 1}_to_h{l + 1}/fork_rnn{l + 1}_{suf}.b').data_ptr()
        d.seq_init = sum(1 << (l - 1) for l in range(1, L + 1) if (l in self._fb_layers or self.use_speaker))
        d.T, d.B, d.H, d.E, d.A, d.U, d.L = T, B, H, E, A, U, L
        d.att_type = 1 if self.attention_type == 'softmax' else 0
        d.use_graph = int(self.use_graph)
        d.reserved = 0
        d.eps, d.alignment, d.sharpening, d.timing = self.epsilon, self.attention_alignment, 1.0, 1.0
        st = self.store.storage
        for l in range(L):
            for key, wd, suf, mat, rec in self._groups:
                getattr(d, 'W' + key)[l] = st[f'{mat}{l + 1}'].data_ptr()
                getattr(d, 'b' + key)[l] = ws['b' + key][l].data_ptr()
                sq = ws['seq_' + key][l]
                getattr(d, 'seq_' + key)[l] = sq.data_ptr() if sq is not None else None
                getattr(d, 'd' + key.upper())[l] = ws['d' + key.upper()][l].data_ptr()
            for n in (('h', 'dh', 'cst', 'gate4', 'dcell') if lstm else ('h', 'dh', 'z', 'r', 'rh', 'c')):
                getattr(d, n)[l] = ws[n][l].data_ptr()
            d.dhup[l] = ws['dhup'][l].data_ptr() if ws['dhup'][l] is not None else None
            if 'dh_b' in ws:
                d.dh_b[l] = ws['dh_b'][l].data_ptr()
                d.dhup_b[l] = ws['dhup_b'][l].data_ptr() if ws['dhup_b'][l] is not None else None
                if 'dhup_c' in ws:
                    d.dhup_c[l] = ws['dhup_c'][l].data_ptr() if ws['dhup_c'][l] is not None else None
        tl = self._tiled_weights()
        if tl is not None:
            for l in range(L):
                for key, wd, suf, mat, rec in self._groups:
                    getattr(d, f'W{key}_f')[l] = tl[(l, key, 'f')].data_ptr()
                    getattr(d, f'W{key}_r')[l] = tl[(l, key, 'r')].data_ptr()
        ws['att_sup'] = torch.zeros(T, B, 2, device=self._dev(), dtype=torch.int32)
        d.att_sup = ws['att_sup'].data_ptr()
        if env_int('PARROT_SCHEDULE', -1) == 4 and tl is not None:
            # persistent forward scan: zero-filled workspace for the machine's slabs / unit table / barrier words
            n = int(_lib.load().parrot_decoder_persist_floats(C.byref(d)))
            if n > 0:
                ws['persist_ws'] = torch.zeros(n, **f)
                d.persist_ws, d.persist_ws_floats = ws['persist_ws'].data_ptr(), n
        d.WattT, d.batt, d.ctx = st['dec.WattT'].data_ptr(), st['dec.batt'].data_ptr(), ws['ctx'].data_ptr()
        for n in ('w', 'kappa', 'a', 'b', 'phi', 'dw', 'dw0', 'dkappa', 'dp'):
            setattr(d, n, ws[n].data_ptr())
        if 'dw_b' in ws:
            d.dw_b, d.dw0_b = ws['dw_b'].data_ptr(), ws['dw0_b'].data_ptr()
        if 'dw_c' in ws:
            d.dw_c, d.dw0_c = ws['dw_c'].data_ptr(), ws['dw0_c'].data_ptr()
        if lstm and self._bf16_weight_grads(0, T, T) and env_int('PARROT_BF16_DG16', 1) != 0:
            # the backward scan leaves the pre-activation gradients in bf16 too (ParrotDecoderDesc::dG16): no conversion
            # pass over 3 x [T,B,4H] floats before the weight-gradient products
            cp = self._bf16_copies(ws, T, B)
            for l in range(L):
                d.dG16[l] = cp['d']['g'][l].data_ptr()
        plan = C.c_void_p()
        _lib.call('parrot_decoder_create', C.byref(d), C.byref(plan))
        ws['plan'], ws['desc'] = plan, d
        ws['plan_writes_d16'] = bool(_lib.load().parrot_decoder_writes_bf16_grads(plan))
        self._train_ws[ws_key] = ws  # (`key` is the group key of the loops above)
        return ws

    @staticmethod
    def _scatter_rows_add(grad, idx, src):
        """grad[idx[i]] += src[i] (LookupTable gradient) as onehot^T . src on the HIP GEMM: same result as
        index_add_, but summed in a fixed order (no float atomics), so gradients are reproducible bit for bit."""
        onehot = torch.zeros(idx.numel(), grad.shape[0], device=grad.device, dtype=torch.float32)
        onehot.scatter_(1, idx.reshape(-1, 1), 1.0)
        with ops.gemm_precision(ops.PRECISION_F32):  # a gather-sum, not a product: keep the addends exact
            ops.gemm(onehot.t(), src.contiguous(), out=grad, accumulate=True)

    def _tiled_weights(self, refresh=False):
        """Fragment-major copies of the packed layer matrices for the scan kernels (parrot_tile_weights);
        None when the widths are not multiples of 16.  refresh=True re-derives them from the current weights."""
        H, E = self.rnn_h_dim, self.encoded_input_dim
        bf = self.compute_bf16
        if bf and (H % 32 or E % 32 or self.layer_norm):
            raise ValueError("compute_dtype='bf16' needs rnn_h_dim and the encoder width to be multiples of 32 "
                             "and layer_norm=False")
        if H % 16 or E % 16:
            return None
        if getattr(self, '_tiled', None) is None:
            st = self.store.storage
            self._tiled = {}
            for l in range(self.num_layers):
                for key, wd, suf, mat, rec in self._groups:
                    for which in ('f', 'r'):
                        self._tiled[(l, key, which)] = torch.empty_like(
                            st[f'{mat}{l + 1}'], dtype=torch.bfloat16 if bf else torch.float32)
            refresh = True
        if refresh:
            st = self.store.storage
            for l in range(self.num_layers):
                for key, wd, suf, mat, rec in self._groups:
                    W = st[f'{mat}{l + 1}']
                    lstm_h = H if self.cell_type == 'lstm' else 0
                    fn = 'parrot_tile_weights_bf16' if bf else 'parrot_tile_weights'
                    _lib.call(fn, W.data_ptr(), W.shape[0], W.shape[1], W.shape[1],
                              self._tiled[(l, key, 'f')].data_ptr(), 0, lstm_h, ops._stream())
                    _lib.call(fn, W.data_ptr(), W.shape[0], W.shape[1], W.shape[1],
                              self._tiled[(l, key, 'r')].data_ptr(), 1, 0, ops._stream())
        return self._tiled

    def _layer_bias_names(self, l, suf):
        """Names of the bias parameters that add into layer l's pre-activation group `suf`
        ('inputs' / 'gates'): the Forks from the attention context and from the layers below."""
        names = [f'/inp_to_h{l}/fork_rnn{l}_{suf}.b']
        if not self.layer_norm:  # with layer_norm those biases sit inside the normalised projection
            names += [f'/h{j}_to_h{l}/fork_rnn{l}_{suf}.b' for j in range(1, l)]
        return names

    def _sum_layer_biases(self, ws, extra_fb=False):
        for l in range(1, self.num_layers + 1):
            for key, wd, suf, mat, rec in self._groups:
                b = ws['b' + key][l - 1]
                b.zero_()
                for n in self._layer_bias_names(l, suf):
                    b.add_(self._p(n))
                if extra_fb and l in self._fb_layers:
                    b.add_(self._p(f'/out_to_h{l}/fork_rnn{l}_{suf}.b'))

    # ------------------------------------------------------------------ compute_cost
    def compute_cost(self, *args, **kwargs):
        """Parrot.compute_cost (model.py:551-824); see _compute_cost.  Runs under the model's operand precision."""
        with ops.gemm_precision(ops.PRECISION_BF16 if self.compute_bf16 else ops.full_precision()):
            return self._compute_cost(*args, **kwargs)

    def _backward(self, token, gscale):
        with ops.gemm_precision(ops.PRECISION_BF16 if self.compute_bf16 else ops.full_precision()):
            return self._backward_f(token, gscale)

    def _compute_cost(self, features, features_mask, labels, labels_mask, speaker, start_flag,
                      batch_size, raw_audio=None, feedback_noise=None):
        """Parrot.compute_cost (model.py:551-824).

        features [T+1,B,O], features_mask [T+1,B] (time-major), labels [B,U] int, labels_mask [B,U],
        speaker [B,1] int or None, start_flag 0/1.  Returns (cost, updates, attention_vars, cost_raw)
        like the reference; ``cost.backward()`` fills ``flat_gradients`` (accumulating), and
        ``apply_updates(updates)`` carries the final scan state into the next TBPTT window."""
        self.allocate()
        if speaker is None:
            assert not self.use_speaker  # model.py:556-557
        if self.raw_output and raw_audio is None:
            raise ValueError("raw_output=True needs the raw_audio source (datasets.py:194-203)")
        dev = self._dev()
        features = features.to(dev, torch.float32)
        features_mask = features_mask.to(dev, torch.float32)
        labels_mask = labels_mask.to(dev, torch.float32)
        labels = labels.to(dev)
        target = features[1:]
        mask = features_mask[1:].contiguous()
        T, B = mask.shape
        assert B == batch_size
        U = labels.shape[1]
        H, E, L, R, O = self.rnn_h_dim, self.encoded_input_dim, self.num_layers, self.readouts_dim, self.output_dim
        ws = self._train_workspace(T, B, U)
        save = dict(T=T, B=B, U=U, ws=ws, start_flag=int(bool(start_flag)))

        # --- per-step additive inputs: feedback (model.py:571-603) and speaker (model.py:605-627)
        inp = None
        if self.weak_feedback:
            inp = features[:-1]
            if self.feedback_noise_level:
                if feedback_noise is None:
                    feedback_noise = self.feedback_noise_level * torch.randn_like(inp)
                inp = inp + feedback_noise
            inp = inp.reshape(T * B, O).contiguous()
            save['fb_inp'] = inp
        emb_spk = None
        if self.use_speaker:
            emb_spk = self._p('/lookuptable.W')[speaker[:, 0].long()].contiguous()  # [B,SD]
            save['spk_idx'], save['emb_spk'] = speaker[:, 0].long(), emb_spk
        for l in range(1, L + 1):
            for key, wd, suf, mat, rec in self._groups:
                sq = ws['seq_' + key][l - 1]
                if sq is None or not (l in self._fb_layers or self.use_speaker):
                    continue
                have = False
                if l in self._fb_layers:
                    if self.layer_norm:  # model.py:580-603: the Fork output is normalised row-wise
                        y, sig = ops.simple_norm_fwd(
                            ops.gemm(inp, self._p(f'/out_to_h{l}/fork_rnn{l}_{suf}.W'),
                                     bias=self._p(f'/out_to_h{l}/fork_rnn{l}_{suf}.b')))
                        save[('ln_fb', l, key)] = (y, sig)
                        sq.view(T * B, wd).copy_(y)
                    else:
                        ops.gemm(inp, self._p(f'/out_to_h{l}/fork_rnn{l}_{suf}.W'),
                                 bias=self._p(f'/out_to_h{l}/fork_rnn{l}_{suf}.b'), out=sq.view(T * B, wd))
                    have = True
                if self.use_speaker:
                    sp = ops.gemm(emb_spk, self._p(f'/speaker_to_h{l}/fork_rnn{l}_{suf}.W'),
                                  bias=self._p(f'/speaker_to_h{l}/fork_rnn{l}_{suf}.b'))
                    if self.layer_norm:  # model.py:612-627
                        sp, sig = ops.simple_norm_fwd(sp)
                        save[('ln_spk', l, key)] = (sp, sig)
                    if have:
                        sq.add_(sp.unsqueeze(0))
                    else:
                        sq.copy_(sp.unsqueeze(0).expand(T, -1, -1))

        # --- initial state of the window (model.py:629-643)
        carry = self._get_carry(B)
        for l in range(L):
            if start_flag:
                ws['h'][l][0].copy_(self._p(f'/rnn{l + 1}.initial_state').unsqueeze(0).expand(B, -1))
            else:
                ws['h'][l][0].copy_(carry['h'][l])
            if self.cell_type == 'lstm':
                if start_flag:
                    ws['cst'][l][0].copy_(self._p(f'/rnn{l + 1}.initial_cells').unsqueeze(0).expand(B, -1))
                else:
                    ws['cst'][l][0].copy_(carry['c'][l])
        if start_flag:
            ws['w'][0].copy_(self._p('.initial_w').unsqueeze(0).expand(B, -1))
            ws['kappa'][0].zero_()
        else:
            ws['w'][0].copy_(carry['w'])
            ws['kappa'][0].copy_(carry['k'])

        # --- encoder (model.py:645-646) and summed layer biases
        with ops.gemm_precision(ops.PRECISION_F32):  # the encoder stays f32 in every operand mode
            ws['ctx'].copy_(self._encoder_forward(labels, labels_mask, save))
        self._sum_layer_biases(ws)
        self._tiled_weights(refresh=True)

        # --- the scan (model.py:651-737)
        _lib.call('parrot_decoder_seq_fwd', ws['plan'], ops._stream())
        if 'persist_ws' in ws:  # opt-in persistent forward scan: fail before the cost or any gradient of a launch
            _lib.call('parrot_decoder_status', ws['plan'])  # that gave up is consumed (synchronises)

        # --- readouts and output (model.py:739-755)
        composed = save['readout_composed'] = self._readout_composed()
        self._readout_path = 'composed' if composed else 'factored'
        if composed:
            # nothing non-linear between the readout stack and the output layer: pred = [h_0 .. h_{L-1} | w] . (Wr . Wo) + b'
            # in one launch of width 64 (csrc/readout.hip); no [T*B, R] readouts buffer
            rd = self._readout_desc(ws, T, B)
            pr = torch.empty(T * B, O, device=dev, dtype=torch.float32)
            rd.pred = pr.data_ptr()
            _lib.call('parrot_readout_composed_fwd', C.byref(rd), ws['ro_ws'].data_ptr(), ops._stream())
            preds = [pr.view(T, B, O)]
        else:
            preds = self._readouts_factored(ws, save, T, B, emb_spk)

        # --- masked cost (model.py:757-784); small [T,B,O] elementwise math with local autograd
        gmm_fused = self._gmm_cost_fused()
        self._gmm_cost_path = None if self.which_cost != 'GMM' else ('fused' if gmm_fused else 'torch')
        leafs = [] if gmm_fused else [p.detach().requires_grad_(True) for p in preds]
        with torch.enable_grad():
            if gmm_fused:
                # the mixture-density head in one HIP pass over the pre-activations (csrc/gmmcost.hip): no [T*B, O, K]
                # temporaries; logr (the log responsibilities) is what the backward pass needs
                M = T * B
                tgt, heads = target.reshape(M, O), [p.view(M, -1) for p in preds]
                nll, pi, logr = ops.gmm_cost_fwd(tgt, *heads, self.epsilon)
                mrow, msum = mask.view(M), mask.sum() + 1e-5
                cost_val = (nll * mrow).sum() / msum
                save['gmm'] = (tgt, heads, logr, mrow / msum)
                next_x, coeff = preds[0], pi.view(T, B, self.k_gmm)
            elif self.which_cost == 'MSE':
                cost_tb = ((leafs[0] - target) ** 2).sum(-1)
                next_x, coeff = preds[0], preds[0]
            else:
                sigma = torch.exp(leafs[1]) + self.epsilon
                coeff_ = torch.softmax(leafs[2], -1) + self.epsilon
                cost_tb = cost_gmm(target, leafs[0], sigma, coeff_)
                next_x, coeff = preds[0], coeff_.detach()  # sampled next_x is stochastic in the reference
            if not gmm_fused:
                cost_val = (cost_tb * mask).sum() / (mask.sum() + 1e-5)
        cost_raw = None
        if self.raw_output:
            # model.py:793-820: the SampleRNN head is trained on the predicted frames; the reference sets
            # cost = 0 * cost + 1 * cost_raw, so only the raw-audio cost drives the gradient.
            tt = self.sampleRnn.three_tier
            raw = torch.as_tensor(raw_audio).to(dev)
            raw_mask = features_mask.repeat_interleave(80, dim=0).t().contiguous()          # model.py:795-796
            raw_seq = raw.permute(1, 0, 2).reshape(B, -1).long()                              # model.py:805-806
            last_h0, last_big_h0 = self._samplernn_carry(B)
            with torch.enable_grad():
                cost_raw, ip_cost, _, _, _, new_h0, new_big_h0 = tt.compute_cost(
                    raw_seq, leafs[0].transpose(0, 1), last_h0, last_big_h0, bool(start_flag), raw_mask)
                total = 0.0 * cost_val + 1.0 * cost_raw                                       # model.py:818-820
            save['torch_cost'] = total
            save['leafs'] = leafs
            cost_val = total.detach()
        elif not gmm_fused:  # (the fused head's gradients are computed in the backward pass, already scaled)
            dpreds = torch.autograd.grad(cost_val, leafs)
            save['dpreds'] = [d.reshape(T * B, -1).contiguous() for d in dpreds]

        # --- carried state (model.py:786-791)
        updates = [(carry['h'][l], ws['h'][l][T].clone()) for l in range(L)]
        updates += [(carry['k'], ws['kappa'][T].clone()), (carry['w'], ws['w'][T].clone())]
        if self.cell_type == 'lstm':
            updates += [(carry['c'][l], ws['cst'][l][T].clone()) for l in range(L)]

        if self.raw_output:
            updates += [(last_h0, new_h0.detach()), (last_big_h0, new_big_h0.detach())]    # model.py:815-816
        attention_vars = [next_x, ws['kappa'][1:], ws['w'][1:], coeff, ws['phi'], ws['a']]
        self._token += 1
        self._saved = (self._token, save)
        anchor = torch.zeros((), device=dev, requires_grad=True)
        cost = _CostFn.apply(anchor, self, self._token, cost_val.detach())
        return cost, updates, attention_vars, (cost_raw.detach() if cost_raw is not None else None)

    def _readouts_factored(self, ws, save, T, B, emb_spk):
        """The readout stack and the output layer as the reference writes them (model.py:739-755): readouts [T*B, R] =
        sum of the `*_to_readout` bricks, then one product per output head.  Returns the heads' predictions."""
        H, E, L, R, O = self.rnn_h_dim, self.encoded_input_dim, self.num_layers, self.readouts_dim, self.output_dim
        readouts = self._readouts_buffer(ws, T, B)
        Wr = self.store.storage['dec.Wr']
        rb = self._p('/att_to_readout.b').clone()
        for l in range(1, L + 1):
            rb.add_(self._p(f'/h{l}_to_readout.b'))
        if self.layer_norm:
            # model.py:739-753: each h{l}_to_readout output is normalised on its own, then summed
            ops.gemm(ws['w'][1:].view(T * B, E), Wr[L * H:], bias=self._p('/att_to_readout.b'), out=readouts)
            for l in range(L):
                y, sig = ops.simple_norm_fwd(
                    ops.gemm(ws['h'][l][1:].view(T * B, H), Wr[l * H:(l + 1) * H],
                             bias=self._p(f'/h{l + 1}_to_readout.b')), add_into=readouts)
                save[('ln_ro', l)] = (y, sig)
        elif self._bf16_readouts(T, R):
            # bf16-operand decoders (round 5): the readout products on bf16 COPIES of the state / context histories and of
            # Wr (parrot_gemm_bf16in_ex, 256 x 256 tiles) instead of f32 operands rounded inside the product -- the same
            # values rounded the same way (nearest even).  The copies are reused by the backward pass (dread . Wr^T, the
            # readout and scan weight gradients).
            cp = self._bf16_copies(ws, T, B, convert=('h', 'w'))
            save['bf16_hw_done'] = True
            Wr16 = save['Wr16'] = ops.to_bf16(Wr)
            ops.gemm16(cp['h'][0][1:T + 1].view(T * B, H), Wr16[0:H], out=readouts, bias=rb)
            for l in range(1, L):
                ops.gemm16(cp['h'][l][1:T + 1].view(T * B, H), Wr16[l * H:(l + 1) * H], out=readouts, accumulate=True)
            ops.gemm16(cp['w'][1:T + 1].view(T * B, E), Wr16[L * H:], out=readouts, accumulate=True)
        else:
            ops.gemm(ws['h'][0][1:].view(T * B, H), Wr[0:H], bias=rb, out=readouts)
            for l in range(1, L):
                ops.gemm(ws['h'][l][1:].view(T * B, H), Wr[l * H:(l + 1) * H], out=readouts, accumulate=True)
            ops.gemm(ws['w'][1:].view(T * B, E), Wr[L * H:], out=readouts, accumulate=True)
        if self.use_speaker:
            spr = ops.gemm(emb_spk, self._p('/speaker_to_readout.W'), bias=self._p('/speaker_to_readout.b'))
            readouts.view(T, B, R).add_(spr.unsqueeze(0))
        preds = []
        for i, (wn, bn, dim) in enumerate(self._out_names):
            pr = ops.gemm(readouts, self.store.param(wn), bias=self.store.param(bn)).view(T, B, dim)
            if self.use_speaker:
                swn, sbn, _ = self._spk_out_names[i]
                pr.add_(ops.gemm(emb_spk, self.store.param(swn), bias=self.store.param(sbn)).unsqueeze(0))
            preds.append(pr)
        return preds

    # ------------------------------------------------------------------ composed readout -> output path
    @property
    def readout_path(self):
        """'composed' or 'factored': how the last compute_cost() ran the readout stack and the output layer (None before
        the first call)."""
        return getattr(self, '_readout_path', None)

    def _readout_composed(self):
        """True when readouts -> output runs as one composed affine map (csrc/readout.hip): MSE head (one head, at most
        64 wide), no layer norm between the bricks, no speaker terms, f32 operands, a readout wide enough for the
        composition to pay.  PARROT_READOUT_COMPOSED=0 (read per step) keeps the factored products."""
        H, E = self.rnn_h_dim, self.encoded_input_dim
        return (not self.layer_norm and not self.use_speaker and not self.compute_bf16
                and len(self._out_names) == 1 and sum(d for _, _, d in self._out_names) <= 64
                and self.readouts_dim >= 256 and H % 16 == 0 and E % 16 == 0
                and env_int('PARROT_READOUT_COMPOSED', 1) != 0)

    # ------------------------------------------------------------------ mixture-density head
    @property
    def gmm_cost_path(self):
        """'fused' or 'torch': how the last compute_cost() ran the GMM head's cost and gradient (None before the first
        call and for MSE models)."""
        return getattr(self, '_gmm_cost_path', None)

    def _gmm_cost_fused(self):
        """True when the GMM head's cost and gradient run as the two HIP kernels of csrc/gmmcost.hip: a GMM model that
        does not train a SampleRNN head on the predicted frames (raw_output keeps its torch graph through the leafs) with
        at most 64 components.  PARROT_GMM_COST_FUSED=0 (read per step) keeps the torch element-wise path."""
        return (self.which_cost == 'GMM' and not self.raw_output and self.k_gmm <= 64
                and env_int('PARROT_GMM_COST_FUSED', 1) != 0)

    def _gmm_grad_buffers(self, ws, T, B):
        """(dmu, dsig_hat, dco_hat) of the fused head, made once per training workspace."""
        if 'gmm_grads' not in ws:
            ws['gmm_grads'] = tuple(torch.empty(T * B, d, device=self._dev(), dtype=torch.float32)
                                    for _, _, d in self._out_names)
        return ws['gmm_grads']

    def _readouts_buffer(self, ws, T, B):
        if 'readouts' not in ws:
            ws['readouts'] = torch.empty(T * B, self.readouts_dim, device=self._dev(), dtype=torch.float32)
        return ws['readouts']

    def _readout_desc(self, ws, T, B):
        """ParrotReadoutComposedDesc over the window's histories and its workspace (made once per training workspace).
        It holds raw pointers into the flat parameter / gradient buffers and into the workspace's histories: both are
        allocated once (ParamStore.allocate, one workspace per (T, B, U)) and never reallocated; only `pred` and `dp`
        change per step."""
        if 'ro_desc' in ws:
            return ws['ro_desc']
        H, E, L, R, O = self.rnn_h_dim, self.encoded_input_dim, self.num_layers, self.readouts_dim, self.output_dim
        d = _lib.ReadoutComposedDesc()
        d.M, d.nseg, d.R, d.O, d.zero_rows, d.slice_rows = T * B, L + 1, R, O, B, 0
        for l in range(L):
            d.K[l], d.ldx[l], d.lddx[l] = H, H, H
            d.x[l], d.dx[l] = ws['h'][l][1:].data_ptr(), ws['dh'][l].data_ptr()
        d.K[L], d.ldx[L], d.lddx[L] = E, E, E
        d.x[L], d.dx[L] = ws['w'][1:].data_ptr(), ws['dw'].data_ptr()
        Wr, gWr = self.store.storage['dec.Wr'], self.store.storage_grad['dec.Wr']
        wn, bn, _ = self._out_names[0]
        Wo, gWo = self.store.param(wn), self.store.grad(wn)
        d.Wr, d.ldwr, d.gWr, d.ldgwr = Wr.data_ptr(), Wr.stride(0), gWr.data_ptr(), gWr.stride(0)
        d.Wo, d.ldwo, d.gWo, d.ldgwo = Wo.data_ptr(), Wo.stride(0), gWo.data_ptr(), gWo.stride(0)
        d.bo, d.gbo = self.store.param(bn).data_ptr(), self.store.grad(bn).data_ptr()
        names = [f'/h{l}_to_readout.b' for l in range(1, L + 1)] + ['/att_to_readout.b']
        d.nbias = len(names)
        for i, n in enumerate(names):
            d.rb[i], d.grb[i] = self._p(n).data_ptr(), self._g(n).data_ptr()
        d.ldp, d.lddp = O, O
        n = int(_lib.load().parrot_readout_composed_ws_floats(C.byref(d)))
        if n <= 0:
            raise _lib.HipCallError(f"parrot_readout_composed_ws_floats failed with code {-n}")
        ws['ro_ws'] = torch.empty(n, device=self._dev(), dtype=torch.float32)
        d.ws_floats = n
        ws['ro_desc'] = d
        return d

    # ------------------------------------------------------------------ backward
    def _backward_f(self, token, gscale):
        if self._saved is None or self._saved[0] != token:
            raise RuntimeError("backward() must follow the compute_cost() call that produced this cost "
                               "(workspaces are reused between calls)")
        save = self._saved[1]
        ws, T, B, U = save['ws'], save['T'], save['B'], save['U']
        H, E, L, R, O, A = (self.rnn_h_dim, self.encoded_input_dim, self.num_layers, self.readouts_dim,
                            self.output_dim, self.attention_size)
        emb_spk = save.get('emb_spk')
        demb_spk = torch.zeros_like(emb_spk) if emb_spk is not None else None

        if 'torch_cost' in save:
            # SampleRNN head: torch autograd through the HIP ops gives d(cost)/d(predicted frames) and
            # accumulates the SampleRNN parameter gradients into their registry tensors.
            leafs = save['leafs']
            srn = [p_ for p_ in self.sampleRnn.parameters if p_.requires_grad]
            torch.autograd.backward(save['torch_cost'], grad_tensors=gscale.to(save['torch_cost'].dtype),
                                    inputs=list(leafs) + srn)
            save['dpreds'] = [(l.grad if l.grad is not None else torch.zeros_like(l)).reshape(T * B, -1).contiguous()
                              for l in leafs]
            gscale = torch.ones((), device=gscale.device)
        if 'gmm' in save:
            # fused mixture-density head: mask / (sum mask + 1e-5) and the upstream gradient enter the kernel as one factor
            # per row (a device array: gscale is never read on the host), so the three gradients arrive scaled
            tgt, heads, logr, mrow = save['gmm']
            save['dpreds'] = ops.gmm_cost_bwd(tgt, *heads, logr, (mrow * gscale.to(torch.float32)).contiguous(),
                                              self.epsilon, out=self._gmm_grad_buffers(ws, T, B))
            gscale = None  # (nothing left to scale in _readouts_factored_bwd)
        if save['readout_composed']:
            # dh_l / dw (slot 0 zero-filled in the same launch) and every gradient of the readout stack and the output layer
            # through the composed map, final before the backward scan starts (csrc/readout.hip)
            # (the call reads the W' that this step's forward call left in ws['ro_ws']: _backward_f only accepts the token
            # of the LAST compute_cost, so no other forward call on this workspace and no optimiser step lies in between)
            rd = self._readout_desc(ws, T, B)
            dp = (save['dpreds'][0] * gscale).contiguous()
            rd.dp = dp.data_ptr()
            _lib.call('parrot_readout_composed_bwd', C.byref(rd), ws['ro_ws'].data_ptr(), ops._stream())
            readout_weight_grads = None
        else:
            readout_weight_grads = self._readouts_factored_bwd(ws, save, T, B, gscale, emb_spk, demb_spk)
        ws['dkappa'].zero_()
        ws['dw0'].zero_()
        for t_ in (ws['dhup'] + ws.get('dcell', []) + ws.get('dhup_b', []) + ws.get('dhup_c', []) +
                   [ws[n] for n in ('dw_b', 'dw_c') if n in ws]):
            if t_ is not None:
                t_.zero_()

        self._scan_bwd_and_weight_grads(ws, save, T, B, before=readout_weight_grads)
        if 'dh_b' in ws:  # slot 0 (the gradient wrt what entered the window): add the second accumulators' share
            for l in range(L):
                ws['dh'][l][0].add_(ws['dh_b'][l][0])
            ws['dw'][0].add_(ws['dw_b'][0])
            ws['dw0'][0].add_(ws['dw0_b'][0])
            if 'dw_c' in ws:
                ws['dw'][0].add_(ws['dw_c'][0])
            if 'dw0_c' in ws:
                ws['dw0'][0].add_(ws['dw0_c'][0])

        # the rest of the deferred gradients of the scan (biases, per-step additive inputs)
        sg_, sc_ = self.store.storage_grad, self.store.storage
        for l in range(L):
            ll = l + 1
            for key, wd, suf, mat, rec in self._groups:
                dP = ws['d' + key.upper()][l].view(T * B, wd)
                if self.layer_norm:  # the normalised lower-layer Forks keep their own biases (model.py:703-722)
                    for j in range(l):
                        self._g(f'/h{j + 1}_to_h{ll}/fork_rnn{ll}_{suf}.b').add_(
                            ops.colsum(ws['ln_y' + key][(l, j)].view(T * B, wd)))
                db = ops.colsum(dP)
                for n in self._layer_bias_names(ll, suf):
                    self._g(n).add_(db)
                # per-step additive inputs
                if ll in self._fb_layers:
                    dPf, dbf = dP, db
                    if self.layer_norm:
                        dPf = ops.simple_norm_bwd(dP, *save[('ln_fb', ll, key)])
                        dbf = ops.colsum(dPf)
                    ops.gemm(save['fb_inp'].t(), dPf, out=self._g(f'/out_to_h{ll}/fork_rnn{ll}_{suf}.W'),
                             accumulate=True)
                    self._g(f'/out_to_h{ll}/fork_rnn{ll}_{suf}.b').add_(dbf)
                if self.use_speaker:
                    dPs = dP.view(T, B, wd).sum(0)
                    if self.layer_norm:
                        dPs = ops.simple_norm_bwd(dPs, *save[('ln_spk', ll, key)])
                        db = ops.colsum(dPs)
                    ops.gemm(emb_spk.t(), dPs, out=self._g(f'/speaker_to_h{ll}/fork_rnn{ll}_{suf}.W'),
                             accumulate=True)
                    self._g(f'/speaker_to_h{ll}/fork_rnn{ll}_{suf}.b').add_(db)
                    ops.gemm(dPs, self._p(f'/speaker_to_h{ll}/fork_rnn{ll}_{suf}.W').t(), out=demb_spk,
                             accumulate=True)
            if save['start_flag']:
                ops.colsum(ws['dh'][l][0], out=self._g(f'/rnn{ll}.initial_state'), accumulate=True)
                if self.cell_type == 'lstm':
                    ops.colsum(ws['dcell'][l], out=self._g(f'/rnn{ll}.initial_cells'), accumulate=True)
        if save['start_flag']:
            ops.colsum(ws['dw'][0], out=self._g('.initial_w'), accumulate=True)
            ops.colsum(ws['dw0'][0], out=self._g('.initial_w'), accumulate=True)
        # attention projection bias (the weight gradient is part of _weight_grad_rows)
        ops.colsum(ws['dp'].view(T * B, 3 * A), out=sg_['dec.batt'], accumulate=True)
        # encoder output: dctx[b] = phi[:, b, :]^T . dw_total[1:, b, :]   (batched over b).  (Round 4 ran this share -- the
        # d ctx product and the encoder's backward scan, two latency chains of 0.5 ms -- on a side stream BESIDE the weight-
        # gradient GEMMs: 76.5 vs 72.3 ms per cfg2 step, the chains and the MFMA-bound products slow each other down; removed.)
        dctx = torch.empty(B, U, E, device=ws['ctx'].device, dtype=torch.float32)
        with ops.gemm_precision(ops.PRECISION_F32):  # attention + encoder: f32 operands in every operand mode
            _lib.call('parrot_gemm', ws['phi'].data_ptr(), B * U, 1, ws['dw'][1:].data_ptr(), B * E, 0,
                      dctx.data_ptr(), E, U, E, T, None, 1.0, 0, 0, B, U, E, U * E, 1, ops._stream())
            if self.use_speaker:
                self._scatter_rows_add(self._g('/lookuptable.W'), save['spk_idx'], demb_spk)
            self._encoder_backward(dctx, save)
        self._saved = None

    def _readouts_factored_bwd(self, ws, save, T, B, gscale, emb_spk, demb_spk):
        """Backward of _readouts_factored: output layer, readout biases, the gradients entering the scan (dh_l, dw).
        Returns the closure that adds the readout weight gradients (run by _scan_bwd_and_weight_grads)."""
        H, E, L, R = self.rnn_h_dim, self.encoded_input_dim, self.num_layers, self.readouts_dim
        readouts = ws['readouts']
        # output layer
        dread = torch.empty(T * B, R, device=readouts.device, dtype=torch.float32)  # (the first head's product stores: no fill)
        for i, (wn, bn, dim) in enumerate(self._out_names):
            dp = save['dpreds'][i] if gscale is None else save['dpreds'][i] * gscale
            ops.gemm(readouts.t(), dp, out=self.store.grad(wn), accumulate=True)
            ops.colsum(dp, out=self.store.grad(bn), accumulate=True)
            ops.gemm(dp, self.store.param(wn).t(), out=dread, accumulate=i > 0)
            if self.use_speaker:
                swn, sbn, _ = self._spk_out_names[i]
                dsum = dp.view(T, B, dim).sum(0)
                ops.gemm(emb_spk.t(), dsum, out=self.store.grad(swn), accumulate=True)
                ops.colsum(dsum, out=self.store.grad(sbn), accumulate=True)
                ops.gemm(dsum, self.store.param(swn).t(), out=demb_spk, accumulate=True)
        # readouts
        gWr = self.store.storage_grad['dec.Wr']
        Wr = self.store.storage['dec.Wr']
        db = ops.colsum(dread)
        dro = [dread] * L  # gradient wrt each h{l}_to_readout output
        if self.layer_norm:
            dro = [ops.simple_norm_bwd(dread, *save[('ln_ro', l)]) for l in range(L)]
        # weight gradients of the readout stack: nothing in the backward scan needs them, so they are handed to
        # _scan_bwd_and_weight_grads, which may run them beside the scan
        def readout_weight_grads():
            if self._bf16_weight_grads(0, T, T) and R % 8 == 0 and not self.layer_norm:
                # bf16-operand decoders: from the bf16 copies of the state / context histories (made here, reused by the
                # scan's weight gradients below) and a bf16 copy of the readout gradient
                cp = self._bf16_copies(ws, T, B, convert=() if save.get('bf16_hw_done') else ('h', 'w'))
                ws['bf16_hw_fresh'] = True
                d16 = save['d16'] if 'd16' in save else ops.to_bf16(dread)
                for l in range(L):
                    ops.gemm_bf16in(cp['h'][l][1:T + 1].view(T * B, H), d16, gWr[l * H:(l + 1) * H], accumulate=True)
                ops.gemm_bf16in(cp['w'][1:T + 1].view(T * B, E), d16, gWr[L * H:], accumulate=True)
                return
            for l in range(L):
                ops.gemm(ws['h'][l][1:].view(T * B, H).t(), dro[l], out=gWr[l * H:(l + 1) * H], accumulate=True)
            ops.gemm(ws['w'][1:].view(T * B, E).t(), dread, out=gWr[L * H:], accumulate=True)
        for l in range(L):
            self._g(f'/h{l + 1}_to_readout.b').add_(ops.colsum(dro[l]) if self.layer_norm else db)
        self._g('/att_to_readout.b').add_(db)
        if self.use_speaker:
            dsum = dread.view(T, B, R).sum(0)
            ops.gemm(emb_spk.t(), dsum, out=self._g('/speaker_to_readout.W'), accumulate=True)
            ops.colsum(dsum, out=self._g('/speaker_to_readout.b'), accumulate=True)
            ops.gemm(dsum, self._p('/speaker_to_readout.W').t(), out=demb_spk, accumulate=True)
        # gradients entering the scan through the readouts
        if 'Wr16' in save:  # bf16-operand decoders: dread . Wr^T on the bf16 copies (one copy of dread, shared with gWr)
            Wr16 = save['Wr16']
            d16 = save['d16'] = ops.to_bf16(dread)
            for l in range(L):
                ws['dh'][l][0].zero_()
                ops.gemm16(d16, Wr16[l * H:(l + 1) * H].t(), out=ws['dh'][l][1:].view(T * B, H))
            ws['dw'][0].zero_()
            ops.gemm16(d16, Wr16[L * H:].t(), out=ws['dw'][1:].view(T * B, E))
        else:
            for l in range(L):
                ws['dh'][l][0].zero_()
                ops.gemm(dro[l], Wr[l * H:(l + 1) * H].t(), out=ws['dh'][l][1:].view(T * B, H))
            ws['dw'][0].zero_()
            ops.gemm(dread, Wr[L * H:].t(), out=ws['dw'][1:].view(T * B, E))
        return readout_weight_grads

    def _weight_grad_rows(self, ws, save, T, B, t0, t1):
        """Deferred weight gradients of the scan for the steps [t0, t1): dW += X[t0:t1]^T . dPre[t0:t1] over the
        (t, b) rows (the Theano gradient of the Fork / GatedRecurrent weights inside model.py:651-724, summed over the
        scan's steps).  Called once for the whole window, or part by part beside the backward scan."""
        if t1 <= t0:
            return
        H, E, L = self.rnn_h_dim, self.encoded_input_dim, self.num_layers
        sg_ = self.store.storage_grad
        R = (t1 - t0) * B
        if self._bf16_weight_grads(t0, t1, T):
            return self._weight_grad_rows_bf16(ws, T, B)
        for l in range(L):
            ll = l + 1
            hprev = ws['h'][l][t0:t1].view(R, H)
            wsrc = (ws['w'][t0:t1] if l == 0 else ws['w'][t0 + 1:t1 + 1]).view(R, E)
            for key, wd, suf, mat, rec in self._groups:
                dP = ws['d' + key.upper()][l][t0:t1].view(R, wd)
                gW = sg_[f'{mat}{ll}']
                # the candidate block of the GRU multiplies r*h_prev, every other block h_prev
                rec_in = ws['rh'][l][t0:t1].view(R, H) if key == 'c' else hprev
                ops.gemm(rec_in.t(), dP, out=gW[0:H], accumulate=True)
                ops.gemm(wsrc.t(), dP, out=gW[H:H + E], accumulate=True)
                for j in range(l):
                    r0 = H + E + j * H
                    dPj = dP
                    if self.layer_norm:  # seq_bwd left the gradient wrt the pre-norm projection in ln_y
                        dPj = ws['ln_y' + key][(l, j)][t0:t1].view(R, wd)
                    ops.gemm(ws['h'][j][t0 + 1:t1 + 1].view(R, H).t(), dPj, out=gW[r0:r0 + H], accumulate=True)
                if t0 == 0 and t1 == T:
                    self._gradient_ready(f'{mat}{ll}')  # data-parallel: this matrix's all-reduce starts beside the next products
        # (Measured in round 4: all of these as ONE grouped grid -- 74.47 vs 74.43 ms per cfg2 step, no gain: the
        # products are long enough that the chip's drain between them does not show; the grouped launch was removed.)
        # attention projection (h1_to_att Fork)
        A = self.attention_size
        with ops.gemm_precision(ops.PRECISION_F32):  # the attention window stays f32 in every operand mode
            ops.gemm(ws['dp'][t0:t1].view(R, 3 * A).t(), ws['h'][0][t0 + 1:t1 + 1].view(R, H),
                     out=sg_['dec.WattT'], accumulate=True)

    def _gradient_ready(self, storage_name):
        """Reports a storage entry whose gradient is final for this step to `on_gradient_ready(lo, hi)` (flat-buffer range;
        set by the trainer in data-parallel runs: dist.GradientExchange.mark_ready)."""
        hook = getattr(self, 'on_gradient_ready', None)
        if hook is not None:
            o, n = self.store.offsets[storage_name]
            hook(o, o + (n + 3) // 4 * 4)

    def _bf16_weight_grads(self, t0, t1, T):
        """bf16-operand decoders take the whole window's weight gradients from bf16 COPIES of the saved activations and
        pre-activation gradients (one conversion pass, then parrot_gemm_bf16in: half the operand bytes, 256 x 256 tiles)
        instead of rounding f32 operands inside the product.  Same rounding (nearest even) of the same values."""
        H, E = self.rnn_h_dim, self.encoded_input_dim
        return (self.compute_bf16 and not self.layer_norm and t0 == 0 and t1 == T and H % 8 == 0 and E % 8 == 0
                and env_int('PARROT_BF16_DW', 1) != 0)

    def _bf16_readouts(self, T, R):
        """bf16-operand decoders whose readout stack (model.py:739-755) runs on bf16 copies (parrot_gemm_bf16in_ex)."""
        return (self._bf16_weight_grads(0, T, T) and R % 8 == 0 and not self.use_speaker
                and env_int('PARROT_BF16_READOUT', 1) != 0)

    def _bf16_copies(self, ws, T, B, convert=()):
        """bf16 copies of the scan's histories (allocated once per workspace).  convert: 'h' / 'w' (state and context
        histories: final once the forward scan is done), 'd' (r * h and the pre-activation gradients: after the backward
        scan)."""
        H, E, L = self.rnn_h_dim, self.encoded_input_dim, self.num_layers
        cp = ws.get('bf16_copies')
        if cp is None:
            bf = dict(device=self._dev(), dtype=torch.bfloat16)
            cp = ws['bf16_copies'] = dict(
                h=[torch.empty(T + 1, B, H, **bf) for _ in range(L)], w=torch.empty(T + 1, B, E, **bf),
                rh=[torch.empty(T, B, H, **bf) for _ in range(L)] if self.cell_type != 'lstm' else None,
                d={key: [torch.empty(T, B, wd, **bf) for _ in range(L)] for key, wd, _, _, _ in self._groups})
        if 'w' in convert:
            ops.to_bf16(ws['w'], out=cp['w'])
        for l in range(L):
            if 'h' in convert:
                ops.to_bf16(ws['h'][l], out=cp['h'][l])
            if 'd' in convert:
                if cp['rh'] is not None:
                    ops.to_bf16(ws['rh'][l], out=cp['rh'][l])
                for key, wd, _, _, _ in self._groups:
                    ops.to_bf16(ws['d' + key.upper()][l], out=cp['d'][key][l])
        return cp

    def _weight_grad_rows_bf16(self, ws, T, B):
        H, E, L = self.rnn_h_dim, self.encoded_input_dim, self.num_layers
        sg_ = self.store.storage_grad
        R = T * B
        # (the state / context copies were made by the readout weight gradients when those ran on them)
        fresh = ('d',) if ws.pop('bf16_hw_fresh', False) else ('h', 'w', 'd')
        if ws.get('plan_writes_d16'):  # the backward scan wrote the bf16 gradient rows itself
            fresh = tuple(x for x in fresh if x != 'd')
        cp = self._bf16_copies(ws, T, B, convert=fresh)
        for l in range(L):
            ll = l + 1
            hprev = cp['h'][l][0:T].view(R, H)
            wsrc = (cp['w'][0:T] if l == 0 else cp['w'][1:T + 1]).view(R, E)
            for key, wd, suf, mat, rec in self._groups:
                dP = cp['d'][key][l].view(R, wd)
                gW = sg_[f'{mat}{ll}']
                rec_in = cp['rh'][l].view(R, H) if key == 'c' else hprev  # (the GRU candidate multiplies r * h_prev)
                ops.gemm_bf16in(rec_in, dP, gW[0:H], accumulate=True)
                ops.gemm_bf16in(wsrc, dP, gW[H:H + E], accumulate=True)
                for j in range(l):
                    r0 = H + E + j * H
                    ops.gemm_bf16in(cp['h'][j][1:T + 1].view(R, H), dP, gW[r0:r0 + H], accumulate=True)
        A = self.attention_size
        with ops.gemm_precision(ops.PRECISION_F32):  # the attention window stays f32 in every operand mode
            ops.gemm(ws['dp'].view(R, 3 * A).t(), ws['h'][0][1:T + 1].view(R, H), out=sg_['dec.WattT'], accumulate=True)

    def _scan_bwd_and_weight_grads(self, ws, save, T, B, before=None):
        """`before()` (the readout weight gradients: operands ready before the scan starts), the backward scan, then the
        deferred weight-gradient GEMMs that only read what the scan leaves behind.  (Rounds 2-4 could also run those GEMMs
        part by part BESIDE the scan on a second stream: measured slower every time -- docs/DESIGN_rounds_1_5.md 3.2 -- and removed.)"""
        if before is not None:
            before()
        hook = getattr(self, 'on_early_gradients', None)
        if hook is not None:  # data-parallel runs: the readout / output gradients are final -> their all-reduce starts
            hook()            # now and travels beside the backward scan (dist.GradientExchange)
        _lib.call('parrot_decoder_seq_bwd', ws['plan'], ops._stream())
        self._weight_grad_rows(ws, save, T, B, 0, T)

    # ------------------------------------------------------------------ sampling (sample_model and its kin: decode.py)
    def sample_using_input(self, data_tr, num_samples):
        """model.py:1085-1111: teacher-forced pass on a batch dict; returns
        [sample_x, k, w, pi, phi, pi_att] as numpy arrays."""
        dev = self._dev()
        t = lambda k: torch.as_tensor(data_tr[k]).to(dev) if data_tr.get(k) is not None else None
        with torch.no_grad():
            _, _, av, _ = self.compute_cost(t('features'), t('features_mask'), t('labels'), t('labels_mask'),
                                            t('speaker_index'), data_tr.get('start_flag', 1), num_samples)
        return [a.detach().cpu().numpy().copy() for a in av]

    @staticmethod
    def _evict_train_ws(ws):
        if 'plan' in ws:
            _lib.load().parrot_decoder_destroy(ws.pop('plan'))
        if 'run' in ws:
            ws.pop('run').close()

    def close(self):
        self._train_ws.clear()
        self._sample_ws.clear()


class SampleRnn(Brick):
    """model.py:121-169: adapter brick around the conditional three-tier SampleRNN."""

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        from .sampleRNN import lib as srn_lib
        from .sampleRNN.models.conditional import three_tier
        self.three_tier = three_tier
        self.N_RNN = three_tier.N_RNN
        dev = self._dev()
        if dev.type == 'cuda':
            # model.py:124: the parameters are registered by building the cost graph once on dummy inputs
            srn_lib.set_device(dev)
            tt = three_tier
            with torch.no_grad():
                seq = torch.full((1, 2 * tt.BIG_FRAME_SIZE), int(tt.Q_ZERO), device=dev, dtype=torch.long)
                tt.compute_cost(seq, torch.zeros(1, 1, tt.FEAT_DIM, device=dev),
                                torch.zeros(1, tt.N_RNN, tt.H0_MULT * tt.DIM, device=dev),
                                torch.zeros(1, tt.N_RNN, tt.H0_MULT * tt.BIG_DIM, device=dev), True,
                                torch.ones(1, 2 * tt.BIG_FRAME_SIZE, device=dev))
        self.parameters = srn_lib.get_params(lambda n, p_: getattr(p_, 'param', False))

    def initial_states(self, batch_size):
        tt = self.three_tier
        dev = self._dev()
        last_big_h0 = torch.zeros(batch_size, tt.N_RNN, tt.H0_MULT * tt.BIG_DIM, device=dev)
        last_h0 = torch.zeros(batch_size, tt.N_RNN, tt.H0_MULT * tt.DIM, device=dev)
        return last_h0, last_big_h0

    def apply(self, sequences, features, h0, big_h0, reset, mask):
        return self.three_tier.compute_cost(sequences, features, h0, big_h0, reset, mask)

    def sample_raw(self, test_feats, features_length, tag, path_to_save, pack_streams=0, stream_frames=0, utterance_seed=None,
                   draw_mode='sequential', top_k=0, top_p=0.0, min_p=0.0):
        """pack_streams = N > 0: the utterances (row i cut at features_length[i]) are packed one after the other into N
        streams of one generation plan (three_tier.generate_packed) instead of one rectangle of num_steps frames.
        stream_frames = S > 0: they run through a three_tier.StreamingGenerator (pack_streams or 32 streams) in segments of
        S frames, and each wav is written as its utterance finishes.
        utterance_seed = S (None: off): utterance i draws with three_tier.utterance_seed(S, i), whichever of the three ways
        it runs: its samples do not depend on where it was placed.
        draw_mode = 'sequential' or 'scan' (three_tier.DeviceGenerator): ValueError on any other name, before any device call.
        top_k = k > 0: the draws at temperature > 0 are taken among the k most likely codes (three_tier.DeviceGenerator); 0:
        among all; ValueError on a negative one, before any device call.
        top_p = p strictly between 0 and 1: those draws are taken among the nucleus of the codes top_k left
        (three_tier.DeviceGenerator); 0 or >= 1: no nucleus; ValueError on a negative one or a NaN, before any device call.
        min_p in (0, 1]: of the codes both left, those draws keep the ones at least min_p times as likely as the most likely
        code (three_tier.DeviceGenerator); 0: off; ValueError outside [0, 1] or on a NaN, before any device call."""
        tt = self.three_tier
        tt.draw_mode_code(draw_mode)
        tt.top_k_code(top_k)
        tt.top_p_code(top_p)
        tt.min_p_code(min_p)
        fns = tt.getting_generation_functions(None, None, None, None, None)
        return tt.generate_and_save_samples(
            tag, path_to_save=path_to_save, features=test_feats, features_length=features_length,
            noise_level=0., big_frame_level_generate_fn=fns[0], frame_level_generate_fn=fns[1],
            sample_level_generate_fn=fns[2], npy_address=None, pack_streams=pack_streams, stream_frames=stream_frames,
            utterance_seed=utterance_seed, draw_mode=draw_mode, top_k=top_k, top_p=top_p, min_p=min_p)

"""Parrot's decode half (``sample_model`` and its kin -> parrot_sample_run: the whole autoregressive loop as one resident
kernel, csrc/persist.h, or as per-step launches in one hipGraph), as a mixin of ``parrot_amd.model.Parrot``.  It uses what
Parrot provides -- ``_p``, ``store``, ``_groups``, ``_fb_layers``, ``_encoder_forward``, ``_sum_layer_biases``,
``_sample_ws``, ``_dev()``, ``allocate()`` -- and holds no state of its own.  ``model.py:NNN`` is the reference's model.py."""
import ctypes as C

import numpy
import torch

from . import _lib, ops
from .utils import env_int

_GMM_HEADS = (('mu', 'gmm_mu'), ('sig', 'gmm_sigma'), ('co', 'gmm_coeff'))  # (descriptor / workspace suffix, fork name)
_PER_UTTERANCE = ('timing_coeffs', 'sharpening_coeffs', 'sampling_biases', 'speaker_weights', 'forced_frames', 'n_forced')


def _as_numpy(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else x


class _DecodeMixin:
    def _sample_workspace(self, S, N, U, stop_extra=0, forced=False):
        ws_key = self._sample_ws_key(S, N, U, stop_extra, forced)
        ws = self._sample_ws.get(ws_key)
        if ws is not None:
            return ws
        why = self._decode_bf16_refusal(N) if self.decode_bf16 else ''
        if why:  # (before anything is allocated)
            raise ValueError("decode_dtype='bf16' " + why)
        ws = self._sample_buffers(S, N, U, stop_extra, forced)
        fd, d = self._sample_descriptor(ws, S, N, U, stop_extra, forced)
        self._sample_machine_operands(ws, d, fd, N, forced)
        self._sample_create_plan(ws, d, fd, S, N, U, stop_extra)
        self._sample_ws[ws_key] = ws
        return ws

    @staticmethod
    def _sample_ws_key(S, N, U, stop_extra, forced):
        """A plan that stops at the end of the utterance is another plan: a workspace key of its own; so is a plan with
        forced frames -- a call without them keeps the key, and the plan, it had."""
        key = ('stop', S, N, U, stop_extra) if stop_extra else (S, N, U)
        return ('forced',) + key if forced else key

    def _sample_buffers(self, S, N, U, stop_extra, forced):
        """Every tensor of the workspace but the machine's operand copies (ws['pm'])."""
        H, E, A, L, R, O = (self.rnn_h_dim, self.encoded_input_dim, self.attention_size, self.num_layers,
                            self.readouts_dim, self.output_dim)
        ldx = (O + 3) // 4 * 4
        f = dict(device=self._dev(), dtype=torch.float32)
        i32 = dict(device=self._dev(), dtype=torch.int32)
        gmm = self.which_cost == 'GMM'
        ws = dict(
            x=torch.zeros(S + 1, N, ldx, **f), h=[torch.zeros(2, N, H, **f) for _ in range(L)],
            w=torch.zeros(S + 1, N, E, **f), kappa=torch.zeros(S + 1, N, A, **f),
            a=torch.empty(S, N, A, **f), bwork=torch.empty(N, A, **f), phi=torch.empty(S, N, U, **f),
            zwork=torch.empty(N, H, **f), rwork=torch.empty(N, H, **f), rhwork=torch.empty(N, H, **f),
            readout=torch.empty(N, R, **f), ctx=torch.zeros(N, U, E, **f),
            br=torch.zeros(R, **f), ldx=ldx,
            radd=torch.zeros(N, R, **f) if self.use_speaker else None,
            oadd=torch.zeros(N, O, **f) if (self.use_speaker and not gmm) else None,
        )
        for key, wd, suf, mat, rec in self._groups:
            ws['b' + key] = [torch.zeros(wd, **f) for _ in range(L)]
            ws['seq_' + key] = [torch.zeros(N, wd, **f) if self.use_speaker else None for _ in range(L)]
        if self.cell_type == 'lstm':
            ws.update(cwork=[torch.zeros(2, N, H, **f) for _ in range(L)], gwork=torch.empty(N, 4 * H, **f))
        if gmm:
            K = self.k_gmm
            ws.update(unif=torch.zeros(S, N, **f), noise=torch.zeros(S, N, O, **f),
                      gmm_mu=torch.empty(N, O * K, **f), gmm_sig=torch.empty(N, O * K, **f),
                      gmm_co=torch.empty(N, K, **f), pi_out=torch.empty(S, N, K, **f),
                      add_mu=torch.zeros(N, O * K, **f) if self.use_speaker else None,
                      add_sig=torch.zeros(N, O * K, **f) if self.use_speaker else None,
                      add_co=torch.zeros(N, K, **f) if self.use_speaker else None)
        if self.layer_norm:  # scratch of the per-step normalised projections (see _sample_descriptor)
            widths = sum(wd for key, wd, suf, mat, rec in self._groups)
            ws['ln_scratch'] = torch.empty(N * (5 * widths + (L + 1) * R), **f)
        if stop_extra:  # ParrotSampleDesc::eou_*: the rule's two indices per row, filled per call; first firing step per row
            ws.update(eou_pos=torch.zeros(N, **i32), eou_ncmp=torch.zeros(N, **i32), eou_first=torch.full((N,), -1, **i32))
        if forced:  # ParrotSampleForcedDesc::forced / n_forced / own_x: filled per call (_sample_device)
            ws.update(forced=torch.zeros(S, N, ldx, **f), n_forced=torch.zeros(N, **i32), own_x=torch.zeros(S, N, ldx, **f))
        # per-row controls (parrot_sample_set_row_controls): the arrays live here and the plan is given them before its
        # first run; every call writes all of them -- the caller's values, or else the model's scalars (_write_row_controls)
        ws['row_timing'], ws['row_sharpening'] = torch.empty(N, **f), torch.empty(N, **f)
        ws['row_bias'] = torch.empty(N, **f) if gmm else None
        return ws

    def _sample_descriptor(self, ws, S, N, U, stop_extra, forced):
        """(fd, d): the decode descriptor d of the workspace; forced: inside fd, ParrotSampleForcedDesc (else fd is None)."""
        H, E, A, L, R, O = (self.rnn_h_dim, self.encoded_input_dim, self.attention_size, self.num_layers,
                            self.readouts_dim, self.output_dim)
        fd = _lib.SampleForcedDesc() if forced else None
        d = fd.base if forced else _lib.SampleDesc()
        d.S, d.B, d.H, d.E, d.A, d.U, d.L, d.O, d.R, d.ldx = S, N, H, E, A, U, L, O, R, ws['ldx']
        d.att_type = 1 if self.attention_type == 'softmax' else 0
        d.use_graph = int(self.use_graph)
        d.eps, d.alignment = self.epsilon, self.attention_alignment
        d.sharpening, d.timing = self.sharpening_coeff, self.timing_coeff
        st = self.store.storage
        lstm = self.cell_type == 'lstm'
        d.cell = 1 if lstm else 0
        d.bf16 = 1 if self.decode_bf16 else 0  # (the library refuses what the bf16 machine does not take)
        for l in range(L):
            for key, wd, suf, mat, rec in self._groups:
                getattr(d, 'W' + key)[l] = st[f'{mat}{l + 1}'].data_ptr()
                getattr(d, 'b' + key)[l] = ws['b' + key][l].data_ptr()
                if (l + 1) in self._fb_layers:
                    getattr(d, 'Wf' + key)[l] = self._p(f'/out_to_h{l + 1}/fork_rnn{l + 1}_{suf}.W').data_ptr()
                if self.use_speaker:
                    getattr(d, 'seq_' + key)[l] = ws['seq_' + key][l].data_ptr()
            d.h[l] = ws['h'][l].data_ptr()
            if lstm:
                d.cwork[l] = ws['cwork'][l].data_ptr()
        if lstm:
            d.gwork = ws['gwork'].data_ptr()
        if self.layer_norm:
            # model.py:899-1006 with _apply_norm active: the plan normalises the feedback / lower-layer / readout
            # projections per step, so their biases are passed separately instead of being summed into bg/bc/br
            d.layer_norm = 1
            d.ln_scratch, d.ln_scratch_floats = ws['ln_scratch'].data_ptr(), ws['ln_scratch'].numel()
            for l in range(L):
                d.br_l[l] = self._p(f'/h{l + 1}_to_readout.b').data_ptr()
                for key, wd, suf, mat, rec in self._groups:
                    if (l + 1) in self._fb_layers:
                        getattr(d, 'bf' + key)[l] = self._p(f'/out_to_h{l + 1}/fork_rnn{l + 1}_{suf}.b').data_ptr()
                    for j in range(l):
                        getattr(d, 'ln_b' + key)[l * _lib.MAX_LAYERS + j] = \
                            self._p(f'/h{j + 1}_to_h{l + 1}/fork_rnn{l + 1}_{suf}.b').data_ptr()
        d.WattT, d.batt = st['dec.WattT'].data_ptr(), st['dec.batt'].data_ptr()
        d.Wr, d.br = st['dec.Wr'].data_ptr(), ws['br'].data_ptr()
        d.radd = ws['radd'].data_ptr() if ws['radd'] is not None else None
        if self.which_cost != 'GMM':
            d.Wo, d.bo = self._p('/readout_to_output.W').data_ptr(), self._p('/readout_to_output.b').data_ptr()
            d.oadd = ws['oadd'].data_ptr() if ws['oadd'] is not None else None
        else:
            d.gmm_K, d.sampling_bias = self.k_gmm, float(self.sampling_bias)
            for nm, key in _GMM_HEADS:
                setattr(d, 'W' + nm, self._p(f'/readout_to_output/fork_{key}.W').data_ptr())
                setattr(d, 'b' + nm, self._p(f'/readout_to_output/fork_{key}.b').data_ptr())
                if self.use_speaker:
                    setattr(d, 'add_' + nm, ws['add_' + nm].data_ptr())
            for n in ('unif', 'noise', 'gmm_mu', 'gmm_sig', 'gmm_co', 'pi_out'):
                setattr(d, n, ws[n].data_ptr())
        for n in ('ctx', 'x', 'w', 'kappa', 'a', 'bwork', 'phi', 'zwork', 'rwork', 'rhwork', 'readout'):
            setattr(d, n, ws[n].data_ptr())
        if stop_extra:
            d.eou_pos, d.eou_ncmp, d.eou_first = (ws[k].data_ptr() for k in ('eou_pos', 'eou_ncmp', 'eou_first'))
            d.eou_extra = int(stop_extra)
        if forced:  # (held by the plan by value)
            fd.forced, fd.n_forced, fd.own_x = (ws[k].data_ptr() for k in ('forced', 'n_forced', 'own_x'))
        return fd, d

    def _sample_machine_operands(self, ws, d, fd, N, forced):
        """Persistent phase machine (csrc/persist.h): the decode loop as one resident kernel.  It wants fragment-major
        copies of the packed layer matrices with the fed-back-output rows appended (padded to 64 rows), of the readout
        stack and of the output projection (63 -> 64 columns); sample_model_device refreshes them per call.  LSTM decoders:
        the one 4H-wide group, tiled in the gate-interleaved column order of the machine's LSTM units.  Allocates them as
        ws['pm'], sets their descriptor fields and the machine's own workspace -- or nothing, where the machine refuses."""
        if self._decode_machine_refusal(N):
            return
        H, E, A, L, R, O = (self.rnn_h_dim, self.encoded_input_dim, self.attention_size, self.num_layers,
                            self.readouts_dim, self.output_dim)
        f = dict(device=self._dev(), dtype=torch.float32)
        f32_gru = self.cell_type != 'lstm' and not self.decode_bf16
        pm = dict(cat={}, tiled={})
        for l in range(L):
            fb = 64 if (l + 1) in self._fb_layers else 0
            for key, wd, suf, mat, rec in self._groups:
                rows = H + E + l * H + fb
                pm['cat'][(l, key)] = torch.zeros(rows, wd, **f)
                if self.decode_bf16:  # the bf16 copy in the machine's K order takes the place of the f32 one
                    pm['tiled'][(l, key)] = torch.empty(rows, wd, device=self._dev(), dtype=torch.bfloat16)
                    getattr(d, f'W{key}_t16')[l] = pm['tiled'][(l, key)].data_ptr()  # (GRU: 'g' and 'c', a copy each)
                    continue
                pm['tiled'][(l, key)] = torch.empty(rows, wd, **f)
                getattr(d, f'W{key}_t')[l] = pm['tiled'][(l, key)].data_ptr()
        if self.which_cost == 'GMM':  # (the refusal is '' for a GMM head only under PARROT_PM_GMM=1)
            # readout stack -> three head projections is linear without layer norm (the reasoning of
            # compose_readout_output): the machine takes Wr . [W_mu | W_sig | W_co], columns zero-padded to a multiple
            # of 16, and the constant rows with the speaker terms (ParrotSampleDesc::Wrh_t / rh_const / rh_cols)
            NH16 = (2 * O * self.k_gmm + self.k_gmm + 15) // 16 * 16
            pm['Wh_pad'], pm['ch_pad'] = torch.zeros(R, NH16, **f), torch.zeros(N, NH16, **f)
            pm['Wrh'], pm['Wrh_t'] = torch.empty(L * H + E, NH16, **f), torch.empty(L * H + E, NH16, **f)
            pm['rh_const'] = torch.zeros(N, NH16, **f)
            d.Wrh_t, d.rh_const, d.rh_cols = pm['Wrh_t'].data_ptr(), pm['rh_const'].data_ptr(), NH16
        else:
            pm['Wr_t'] = torch.empty(L * H + E, R, **f)
            pm['Wo_pad'], pm['Wo_t'] = torch.zeros(R, 64, **f), torch.empty(R, 64, **f)
            pm['bo_pad'] = torch.zeros(64, **f)
            d.Wr_t, d.Wo_t, d.bo_pad = pm['Wr_t'].data_ptr(), pm['Wo_t'].data_ptr(), pm['bo_pad'].data_ptr()
            if ws['oadd'] is not None:
                pm['oadd_pad'] = torch.zeros(N, 64, **f)
                d.oadd_pad = pm['oadd_pad'].data_ptr()
            # readout -> output is linear here (model.py:992-1013, MSE head, no layer norm): the machine takes the
            # composed matrix Wr . Wo and the constant rows (br + radd) . Wo + bo + oadd, and x[t+1] costs ONE phase
            pm['Wro'], pm['Wro_t'] = torch.empty(L * H + E, 64, **f), torch.empty(L * H + E, 64, **f)
            pm['ro_const'] = torch.zeros(N, 64, **f)
            d.Wro_t, d.ro_const = pm['Wro_t'].data_ptr(), pm['ro_const'].data_ptr()
            # (bf16 operands: neither the fold nor the composed feedback rows below -- both would round at other points
            # than the products they replace, and the bf16 plan does not take them)
            if f32_gru and N <= 16 and 3 * A <= 32 and env_int('PARROT_PM_ATTFOLD', 1) != 0:
                # round 5: the attention projection as an [H, 32] matrix (fragment-major): layer 0's candidate units fold
                # their tile's share of h_1 . Watt into their epilogue (ParrotSampleDesc::Watt_t)
                pm['Watt_pad'], pm['Watt_t'] = torch.zeros(H, 32, **f), torch.empty(H, 32, **f)
                d.Watt_t = pm['Watt_t'].data_ptr()
            # round 5: the fed-back frame out of the step's chain (weak feedback, L >= 2): layer 0's matrices with the rows
            # A . Wf appended, A = the last layer's rows of Wr . Wo (ParrotSampleDesc::Wgx_t / Wcx_t)
            # (a forced plan keeps the frame on the chain and does not take them)
            if f32_gru and not forced and L >= 2 and self._fb_layers == [1] and env_int('PARROT_PM_FBC', 1) != 0:
                for key, wd, suf, mat, rec in self._groups:
                    rows = H + E + 64 + H
                    pm['cat'][('x', key)] = torch.zeros(rows, wd, **f)
                    pm['tiled'][('x', key)] = torch.empty(rows, wd, **f)
                    getattr(d, f'W{key}x_t')[0] = pm['tiled'][('x', key)].data_ptr()
        n = int(_lib.load().parrot_sample_persist_floats_forced(C.byref(fd)) if forced
                else _lib.load().parrot_sample_persist_floats(C.byref(d)))
        if n > 0:
            pm['ws'] = torch.zeros(n, **f)
            d.persist_ws, d.persist_ws_floats = pm['ws'].data_ptr(), n
            ws['pm'] = pm

    def _sample_create_plan(self, ws, d, fd, S, N, U, stop_extra):
        """ws['plan'] / ws['desc']: the plan, verified to be what was asked for and given its row controls (else destroyed)."""
        lib, plan = _lib.load(), C.c_void_p()
        try:
            if fd is not None:
                _lib.call('parrot_sample_create_forced', C.byref(fd), C.byref(plan))
            else:
                _lib.call('parrot_sample_create', C.byref(d), C.byref(plan))
        except _lib.HipCallError as e:
            if stop_extra:
                raise ValueError(f"sample_until_end: the library did not build a decode machine that stops early for S={S}, "
                                 f"N={N}, U={U} ({e}); the per-step launches cannot stop") from e
            if not self.decode_bf16:
                raise
            raise ValueError(f"decode_dtype='bf16': the library did not build the bf16 decode machine for S={S}, "
                             f"N={N}, U={U} ({e}); there is no f32 decode behind this switch") from e
        try:
            if self.decode_bf16 and lib.parrot_sample_is_bf16(plan) != 1:
                raise ValueError("decode_dtype='bf16': the plan the library built does not run bf16 operands")
            if stop_extra and lib.parrot_sample_stops_early(plan) != 1:
                raise ValueError("sample_until_end: the plan the library built does not stop at the end of the utterance")
            _lib.call('parrot_sample_set_row_controls', plan, ws['row_timing'].data_ptr(), ws['row_sharpening'].data_ptr(),
                      ws['row_bias'].data_ptr() if ws['row_bias'] is not None else None)
        except Exception:
            lib.parrot_sample_destroy(plan)
            raise
        ws['plan'], ws['desc'] = plan, (fd if fd is not None else d)

    @staticmethod
    def _evict_sample_ws(ws):
        if 'plan' in ws:
            _lib.load().parrot_sample_destroy(ws.pop('plan'))

    def _check_row_controls(self, N, timing_coeffs=None, sharpening_coeffs=None, sampling_biases=None, speaker_weights=None):
        """Validates the per-utterance arguments of the decode calls without touching the device (a model that was never
        allocated can be asked): returns (controls, speaker_weights) -- controls maps 'timing' / 'sharpening' / 'bias' to a
        float32 numpy array of N values, or to None where the model's scalar holds for every row; speaker_weights is a float32
        [N, num_speakers] numpy array or None.  ValueError on a wrong length, a non-finite value, a timing or sharpening
        coefficient <= 0, biases on a model without a GMM head, weights on a model without speakers."""
        ctl = {}
        for name, key, vals in (('timing_coeffs', 'timing', timing_coeffs), ('sharpening_coeffs', 'sharpening', sharpening_coeffs),
                                ('sampling_biases', 'bias', sampling_biases)):
            if vals is None:
                ctl[key] = None
                continue
            if key == 'bias' and self.which_cost != 'GMM':
                raise ValueError(f"sampling_biases needs which_cost='GMM': the {self.which_cost} head has no sampling bias")
            a = numpy.asarray(_as_numpy(vals), dtype=numpy.float64)
            if a.shape != (N,):
                raise ValueError(f"{name} needs {N} values (one per utterance), got shape {tuple(a.shape)}")
            a32 = a.astype(numpy.float32)
            if not numpy.all(numpy.isfinite(a32)):
                raise ValueError(f"{name} must be finite, got {a.tolist()}")
            if key != 'bias' and not numpy.all(a32 > 0):
                raise ValueError(f"{name} must be > 0, got {a.tolist()}")
            ctl[key] = a32
        sw = None
        if speaker_weights is not None:
            if not self.use_speaker:
                raise ValueError("speaker_weights needs use_speaker=True: this model has no speaker table to blend")
            sw = numpy.asarray(_as_numpy(speaker_weights), dtype=numpy.float32)
            if sw.shape != (N, self.num_speakers):
                raise ValueError(f"speaker_weights needs shape ({N}, {self.num_speakers}) = (utterances, num_speakers), "
                                 f"got {tuple(sw.shape)}")
            if not numpy.all(numpy.isfinite(sw)):
                raise ValueError("speaker_weights must be finite")
        return ctl, sw

    def _check_forced(self, N, S, forced_frames=None, n_forced=None):
        """Validates the forced frames of a decode call without touching the device: returns None (no forcing), or
        (frames, n) -- frames a float32 numpy array [P, N, O] (time-major, P <= S), n an int32 numpy array of N prompt
        lengths, 0 <= n[b] <= P.  ValueError when only one of the two is given, on a wrong shape, P > S, a non-finite frame,
        a length that is no integer or lies outside 0 .. P, and on a model that decodes with bf16 operands."""
        if forced_frames is None and n_forced is None:
            return None
        if forced_frames is None or n_forced is None:
            raise ValueError("forced_frames and n_forced go together: got only "
                             + ("n_forced" if forced_frames is None else "forced_frames"))
        why = self._decode_forced_refusal()
        if why:
            raise ValueError("forced_frames " + why)
        O = self.output_dim
        fr = numpy.asarray(_as_numpy(forced_frames), dtype=numpy.float64)
        if fr.ndim != 3 or fr.shape[1:] != (N, O):
            raise ValueError(f"forced_frames needs shape (P, {N}, {O}) = (frames, utterances, output_dim), time-major, "
                             f"got {tuple(fr.shape)}")
        P = fr.shape[0]
        if P > S:
            raise ValueError(f"forced_frames holds {P} frames, the call decodes {S} steps: needs P <= {S}")
        fr32 = fr.astype(numpy.float32)
        if not numpy.all(numpy.isfinite(fr32)):
            raise ValueError("forced_frames must be finite")
        n = numpy.asarray(_as_numpy(n_forced))
        if n.shape != (N,):
            raise ValueError(f"n_forced needs {N} values (one per utterance), got shape {tuple(n.shape)}")
        if not numpy.all(numpy.isfinite(n.astype(numpy.float64))) or not numpy.all(n == numpy.floor(n)):
            raise ValueError(f"n_forced must be whole numbers, got {n.tolist()}")
        if not numpy.all((n >= 0) & (n <= P)):
            raise ValueError(f"n_forced must lie in 0 .. {P} (the frames given), got {n.tolist()}")
        return fr32, n.astype(numpy.int32)

    def _write_row_controls(self, ws, ctl):
        """Every decode call writes all of the workspace's control arrays: a call without controls after one with them
        decodes with the model's scalars again."""
        ctl = ctl or {}
        for key, scalar in (('timing', self.timing_coeff), ('sharpening', self.sharpening_coeff), ('bias', self.sampling_bias)):
            t = ws['row_' + key]
            if t is None:
                continue
            vals = ctl.get(key)
            if vals is None:
                t.fill_(float(scalar))
            else:
                t.copy_(torch.from_numpy(numpy.ascontiguousarray(vals)))

    def _decode_machine_refusal(self, N):
        """Why this model / batch does not decode on the persistent machine ('' when it does).  The one statement of the
        machine's conditions on the Python side: _sample_workspace prepares the machine's operands when it is '', and the
        switches that exist on the machine only (decode_dtype='bf16', sample_until_end) refuse with it."""
        H, E, R, O = self.rnn_h_dim, self.encoded_input_dim, self.readouts_dim, self.output_dim
        if self.which_cost != 'MSE':
            # the one read of the switch on this side (csrc/switches.h): the GMM head on the machine is opt-in
            if self.which_cost != 'GMM' or env_int('PARROT_PM_GMM', 0) == 0:
                return "needs which_cost='MSE': the GMM head does not decode on the persistent machine"
            if self.k_gmm > 64:
                return f"covers at most 64 mixture components (one lane of the sampling wave each), got {self.k_gmm}"
        if self.layer_norm:
            return "does not cover layer_norm=True (that decode runs as per-step launches)"
        if N > 64:
            return f"covers at most 64 sequences per call, got {N}"
        if H % 16 or E % 16 or R % 16 or not 61 <= O <= 64:
            return (f"needs rnn_h_dim, the encoder width and readouts_dim to be multiples of 16 and an output frame of 61 .. 64 "
                    f"values (the persistent machine's tiles), got {H}, {E}, {R} and {O}")
        if env_int('PARROT_SAMPLE_PERSIST', 1) == 0:
            return "runs on the persistent machine only, and PARROT_SAMPLE_PERSIST=0 turns that off"
        return ''

    def _decode_bf16_refusal(self, N):
        """Why this model / batch cannot decode with bf16 operands ('' when it can): what the bf16 machine does not take."""
        H, E = self.rnn_h_dim, self.encoded_input_dim
        # the one read of the switch on this side (csrc/switches.h): bf16 operands for GRU decoders are opt-in
        if self.cell_type != 'lstm' and env_int('PARROT_PM_GRU_BF16', 0) == 0:
            return ("needs cell_type='lstm': GRU decoders have no bf16 decode path "
                    "(unless PARROT_PM_GRU_BF16=1 opts in to the bf16 GRU programs)")
        why = self._decode_machine_refusal(N)
        if not why and self.which_cost != 'MSE':  # (PARROT_PM_GMM=1: the machine takes the head, with f32 operands only)
            return "needs which_cost='MSE': the GMM head decodes on the persistent machine with f32 operands only"
        if not why and (H % 32 or E % 32):
            return (f"needs rnn_h_dim and the encoder width to be multiples of 32 (v_mfma_f32_16x16x32_bf16 walks K in "
                    f"steps of 32), got {H} and {E}")
        return why

    def _decode_forced_refusal(self):
        """Why this model cannot decode with forced frames ('' when it can): the machine's kernels with forcing have f32
        operands only."""
        if self.decode_bf16:
            return ("does not cover decode_dtype='bf16': forced frames decode with f32 operands only "
                    "(the bf16 programs have no kernels with forcing)")
        return ''

    def _decode_stop_refusal(self, N, extra):
        """Why this model / batch cannot stop at the end of the utterance ('' when it can): the stop lives inside the
        persistent machine, so whatever decodes as per-step launches cannot have it."""
        if int(extra) < 8:
            return (f"needs extra >= 8, got {extra}: the workgroups agree on the last tick from a word published when the "
                    f"last row fires, and without grid barriers some are a few ticks ahead of it")
        return self._decode_machine_refusal(N)

    def sample_until_end_device(self, labels, labels_mask, speaker, num_samples, max_steps, extra=40, unif=None, noise=None,
                                seed=None, timing_coeffs=None, sharpening_coeffs=None, sampling_biases=None,
                                speaker_weights=None, forced_frames=None, n_forced=None):
        """sample_model_device that stops at the end of the utterance INSIDE the decode kernel instead of decoding
        max_steps frames and cutting afterwards.  The rule is end_of_utterance's (reference sample.py:145-163): a row ends
        `extra` frames after the first step whose window weight on the position just past its text beats the weight on every
        real character.  Returns (outs, lengths): the six tensors of sample_model_device cut to steps_run = max(lengths)
        along time -- bit-identical to the first steps_run steps of sample_model_device(.., max_steps) -- and lengths [N]
        (int64, on the device) = what end_of_utterance gives for each row of the full-length phi.
        timing_coeffs / sharpening_coeffs / sampling_biases / speaker_weights / forced_frames / n_forced: as
        sample_model_device (with forcing outs has the seventh tensor, own_x, cut like the others; the rule reads phi only)."""
        from .utils import end_of_utterance_args
        ctl = self._check_row_controls(num_samples, timing_coeffs, sharpening_coeffs, sampling_biases, speaker_weights)
        forced = self._check_forced(num_samples, max_steps, forced_frames, n_forced)
        why = self._decode_stop_refusal(num_samples, extra)  # (before anything is keyed on `extra` or allocated)
        if why:
            raise ValueError("sample_until_end " + why)
        self.allocate()
        lm = torch.as_tensor(labels_mask)
        U = lm.shape[1]
        ws = self._sample_workspace(max_steps, num_samples, U, stop_extra=int(extra), forced=forced is not None)
        pos, ncmp = end_of_utterance_args(lm.detach().cpu().numpy(), U)
        ws['eou_pos'].copy_(torch.from_numpy(pos))
        ws['eou_ncmp'].copy_(torch.from_numpy(ncmp))
        outs = self._sample_device(ws, labels, labels_mask, speaker, num_samples, max_steps, unif, noise, seed, ctl, forced)
        steps = C.c_int(0)
        _lib.call('parrot_sample_steps_run', ws['plan'], C.byref(steps))
        first = ws['eou_first'].long()
        lengths = torch.where(first >= 0, (first + int(extra)).clamp(max=max_steps), torch.full_like(first, max_steps))
        steps_run = int(lengths.max().item())
        if steps.value != steps_run:
            raise RuntimeError(f"the decode machine completed {steps.value} frames, the rows' lengths ask for {steps_run}")
        return [o[:steps_run] for o in outs], lengths

    def sample_until_end(self, labels_tr, labels_mask_tr, features_mask_tr, speaker_tr, num_samples, max_steps, extra=40,
                         timing_coeffs=None, sharpening_coeffs=None, sampling_biases=None, speaker_weights=None,
                         forced_frames=None, n_forced=None):
        """numpy twin of sample_until_end_device (as sample_model is of sample_model_device): (list of numpy arrays,
        numpy lengths [N])."""
        kw = {k: v for k, v in locals().items() if k in _PER_UTTERANCE}
        outs, lengths = self.sample_until_end_device(labels_tr, labels_mask_tr, speaker_tr, num_samples, max_steps, extra, **kw)
        return [o.detach().cpu().numpy().copy() for o in outs], lengths.cpu().numpy()

    def sample_model_device(self, labels, labels_mask, speaker, num_samples, num_steps, unif=None, noise=None,
                            seed=None, timing_coeffs=None, sharpening_coeffs=None, sampling_biases=None, speaker_weights=None,
                            forced_frames=None, n_forced=None):
        """Device-resident version of sample_model: returns torch tensors
        [sample_x [S,N,O], k [S,N,A], w [S,N,E], pi, phi [S,N,U], pi_att [S,N,A]].
        GMM head: the component choice / Gaussian noise come from `unif` [S,N] and `noise` [S,N,O] if given,
        else from torch's generator (`seed`); Theano's MRG stream itself is not reproducible.
        Per utterance (all None: the model's scalars and the indexed speakers, bit for bit what the call was without them):
        timing_coeffs / sharpening_coeffs / sampling_biases -- N floats each, row b decodes with its own value in place of
        timing_coeff / sharpening_coeff / sampling_bias, on whichever path decodes the model (decode_path);
        speaker_weights [N, num_speakers] -- row b's speaker embedding is speaker_weights[b] @ lookuptable.W (one f32
        product) instead of the looked-up row; `speaker` is then not read.  ValueError (before anything is allocated) on a
        wrong length, non-finite values, timing / sharpening <= 0, biases on an MSE model, weights without use_speaker.
        Forced frames (priming; both None: the call as it is without them, on the same workspace): forced_frames [P, N, O]
        time-major, P <= num_steps, and n_forced, N ints with 0 <= n <= P.  While t < n_forced[b] the frame fed back into
        step t + 1 of row b is forced_frames[t, b] and not the model's (MSE: the output frame; GMM: the draw); from step
        n_forced[b] on the row decodes freely from the state the prompt left.  The list then has a seventh tensor, own_x
        [S, N, O]: what the model emitted or drew at every step; sample_x holds the fed-back (forced) frames in the forced
        region and equals own_x elsewhere.  Composes with the four arguments above.  ValueError (before anything is
        allocated) on a wrong shape, P > num_steps, non-finite frames, n outside 0 .. P, and with decode_dtype='bf16'."""
        ctl = self._check_row_controls(num_samples, timing_coeffs, sharpening_coeffs, sampling_biases, speaker_weights)
        forced = self._check_forced(num_samples, num_steps, forced_frames, n_forced)
        return self._sample_device(None, labels, labels_mask, speaker, num_samples, num_steps, unif, noise, seed, ctl, forced)

    def _sample_device(self, ws, labels, labels_mask, speaker, num_samples, num_steps, unif, noise, seed, ctl=None,
                       forced=None):
        """One decode call on the workspace `ws` (None: the plain workspace of the shape).  ctl: what _check_row_controls
        returned (None: no per-utterance arguments); forced: what _check_forced returned (None: no forced frames)."""
        controls, speaker_weights = ctl if ctl is not None else (None, None)
        self.allocate()
        dev = self._dev()
        labels = torch.as_tensor(labels).to(dev)
        labels_mask = torch.as_tensor(labels_mask).to(dev, torch.float32)
        N, U = labels.shape[0], labels.shape[1]
        assert N == num_samples
        S, L, H, O = num_steps, self.num_layers, self.rnn_h_dim, self.output_dim
        if ws is None:
            ws = self._sample_workspace(S, N, U, forced=forced is not None)
        if forced is not None:  # every call rewrites both arrays whole: nothing of an earlier prompt survives
            frames, n = forced
            ws['forced'].zero_()
            ws['forced'][:frames.shape[0], :, :O].copy_(torch.from_numpy(frames))
            ws['n_forced'].copy_(torch.from_numpy(n))
        ws['ctx'].copy_(self._encoder_forward(labels, labels_mask, None))
        self._sum_layer_biases(ws, extra_fb=not self.layer_norm)
        for l in range(1, L + 1):
            ws['h'][l - 1][0].copy_(self._p(f'/rnn{l}.initial_state').unsqueeze(0).expand(N, -1))
            if self.cell_type == 'lstm':
                ws['cwork'][l - 1][0].copy_(self._p(f'/rnn{l}.initial_cells').unsqueeze(0).expand(N, -1))
        ws['br'].copy_(self._p('/att_to_readout.b'))
        for l in range(1, L + 1):
            if not self.layer_norm:
                ws['br'].add_(self._p(f'/h{l}_to_readout.b'))
        self._write_row_controls(ws, controls)
        if self.use_speaker:
            if speaker_weights is not None:  # a blend of the table's rows in place of one of them
                with ops.gemm_precision(ops.PRECISION_F32):
                    emb = ops.gemm(torch.from_numpy(speaker_weights).to(dev).contiguous(), self._p('/lookuptable.W'))
            else:
                speaker = torch.as_tensor(speaker).to(dev)
                emb = self._p('/lookuptable.W')[speaker[:, 0].long()].contiguous()
            for l in range(1, L + 1):
                for key, wd, suf, mat, rec in self._groups:
                    ops.gemm(emb, self._p(f'/speaker_to_h{l}/fork_rnn{l}_{suf}.W'),
                             bias=self._p(f'/speaker_to_h{l}/fork_rnn{l}_{suf}.b'), out=ws['seq_' + key][l - 1])
                    if self.layer_norm:  # model.py:867
                        ops.simple_norm_fwd(ws['seq_' + key][l - 1])
            ops.gemm(emb, self._p('/speaker_to_readout.W'), bias=self._p('/speaker_to_readout.b'), out=ws['radd'])
            if self.which_cost == 'MSE':
                ops.gemm(emb, self._p('/speaker_to_output.W'), bias=self._p('/speaker_to_output.b'), out=ws['oadd'])
            else:
                for nm, key in _GMM_HEADS:
                    ops.gemm(emb, self._p(f'/speaker_to_output/fork_{key}.W'),
                             bias=self._p(f'/speaker_to_output/fork_{key}.b'), out=ws['add_' + nm])
        ws['x'][0].zero_()  # initial_x, model.py:834-835
        ws['w'][0].copy_(self._p('.initial_w').unsqueeze(0).expand(N, -1))
        ws['kappa'][0].zero_()
        if self.which_cost == 'GMM':
            if unif is None or noise is None:
                g = torch.Generator(device=dev)
                g.manual_seed(int(self.seed if seed is None else seed))
                unif = torch.rand(S, N, device=dev, generator=g)
                noise = torch.randn(S, N, O, device=dev, generator=g)
            ws['unif'].copy_(torch.as_tensor(unif).to(dev, torch.float32))
            ws['noise'].copy_(torch.as_tensor(noise).to(dev, torch.float32))
        if 'pm' in ws:
            self._refresh_sample_machine_weights(ws)
        _lib.call('parrot_sample_run', ws['plan'], ops._stream())
        if 'pm' in ws:  # persistent machine: a launch that gave up leaves invalid frames -- fail loudly (synchronises)
            _lib.call('parrot_sample_status', ws['plan'])
        self._decode_path = 'machine' if _lib.load().parrot_sample_is_persistent(ws['plan']) else 'launches'
        sx = ws['x'][1:, :, :O]
        pi = ws['pi_out'] if self.which_cost == 'GMM' else sx
        outs = [sx, ws['kappa'][1:], ws['w'][1:], pi, ws['phi'], ws['a']]
        return outs + [ws['own_x'][:, :, :O]] if forced is not None else outs

    @property
    def decode_path(self):
        """What the last decode call (sample_model*, sample_until_end*) ran on: 'machine' (the persistent phase machine), or
        'launches' (per-step launches); None before the first."""
        return getattr(self, '_decode_path', None)

    @staticmethod
    def _tile_machine_weight(W, out, lstm_H=0):
        """The fragment-major copy `out` of the matrix W (lstm_H = H: in the gate-interleaved column order of the LSTM units)."""
        bf16 = out.dtype == torch.bfloat16  # decode_dtype='bf16': rounded to nearest even, the machine's K order (mode 2)
        _lib.call('parrot_tile_weights_bf16' if bf16 else 'parrot_tile_weights', W.data_ptr(), W.shape[0], W.shape[1],
                  W.shape[1], out.data_ptr(), 2 if bf16 else 0, lstm_H, ops._stream())

    def _refresh_sample_machine_weights(self, ws):
        """Fragment-major weight copies of the decode machine from the current parameters."""
        pm, st = ws['pm'], self.store.storage
        H, E, L, O = self.rnn_h_dim, self.encoded_input_dim, self.num_layers, self.output_dim
        lstm_H = H if self.cell_type == 'lstm' else 0
        with torch.no_grad():
            for l in range(L):
                for key, wd, suf, mat, rec in self._groups:
                    cat = pm['cat'][(l, key)]
                    kl = H + E + l * H
                    cat[:kl].copy_(st[f'{mat}{l + 1}'])
                    if (l + 1) in self._fb_layers:
                        cat[kl:kl + O].copy_(self._p(f'/out_to_h{l + 1}/fork_rnn{l + 1}_{suf}.W'))
                    self._tile_machine_weight(cat, pm['tiled'][(l, key)], lstm_H)
            if 'Wrh_t' in pm:  # GMM head: Wr . [W_mu | W_sig | W_co] and its constant rows, composed in double, rounded once
                col, Wh, ch = 0, pm['Wh_pad'], pm['ch_pad']
                for nm, key in _GMM_HEADS:
                    W = self._p(f'/readout_to_output/fork_{key}.W')
                    n = W.shape[1]
                    Wh[:, col:col + n].copy_(W)
                    ch[:, col:col + n].copy_(self._p(f'/readout_to_output/fork_{key}.b').unsqueeze(0).expand(ch.shape[0], -1))
                    if self.use_speaker:
                        ch[:, col:col + n].add_(ws['add_' + nm])
                    col += n
                Wrh, c = compose_readout_output(st['dec.Wr'], Wh, ws['br'], ws['radd'], torch.zeros_like(ch[0]), ch, ch.shape[0])
                pm['Wrh'].copy_(Wrh)
                self._tile_machine_weight(pm['Wrh'], pm['Wrh_t'])
                pm['rh_const'].copy_(c)
            else:
                self._refresh_mse_head_weights(ws)

    def _refresh_mse_head_weights(self, ws):
        """The MSE head's part of _refresh_sample_machine_weights: readout stack, output projection, their composition, the
        folded attention projection and the composed feedback rows (called under no_grad)."""
        pm, st = ws['pm'], self.store.storage
        H, E, L, O = self.rnn_h_dim, self.encoded_input_dim, self.num_layers, self.output_dim
        self._tile_machine_weight(st['dec.Wr'], pm['Wr_t'])
        pm['Wo_pad'][:, :O].copy_(self._p('/readout_to_output.W'))
        self._tile_machine_weight(pm['Wo_pad'], pm['Wo_t'])
        pm['bo_pad'][:O].copy_(self._p('/readout_to_output.b'))
        if 'oadd_pad' in pm:
            pm['oadd_pad'][:, :O].copy_(ws['oadd'])
        Wro, c = compose_readout_output(st['dec.Wr'], pm['Wo_pad'], ws['br'], ws['radd'], pm['bo_pad'],
                                        pm.get('oadd_pad'), pm['ro_const'].shape[0])
        pm['Wro'].copy_(Wro)
        self._tile_machine_weight(pm['Wro'], pm['Wro_t'])
        pm['ro_const'].copy_(c)
        if 'Watt_t' in pm:
            A3 = 3 * self.attention_size
            pm['Watt_pad'][:, :A3].copy_(st['dec.WattT'].t())
            self._tile_machine_weight(pm['Watt_pad'], pm['Watt_t'])
        for key, wd, suf, mat, rec in self._groups:
            if ('x', key) not in pm['cat']:
                continue
            # x . Wf = x_pre . Wf + h_{L-1} . (A . Wf) with A = Wro[(L-1)H : L H]: composed in double, rounded once
            cat, base = pm['cat'][('x', key)], pm['cat'][(0, key)]
            cat[:H + E + 64].copy_(base)
            A_last = Wro[(L - 1) * H:L * H].double()
            cat[H + E + 64:].copy_((A_last @ base[H + E:H + E + 64].double()).float())
            self._tile_machine_weight(cat, pm['tiled'][('x', key)])

    def sample_model(self, labels_tr, labels_mask_tr, features_mask_tr, speaker_tr, num_samples, num_steps,
                     timing_coeffs=None, sharpening_coeffs=None, sampling_biases=None, speaker_weights=None,
                     forced_frames=None, n_forced=None):
        """Parrot.sample_model (model.py:1061-1083): numpy in, list of numpy arrays out
        [sample_x, k, w, pi, phi, pi_att], all time-major (the caller swaps axes, sample.py:142-143).  The keyword
        arguments: per utterance, as sample_model_device (forced_frames / n_forced: a seventh array, own_x)."""
        kw = {k: v for k, v in locals().items() if k in _PER_UTTERANCE}
        outs = self.sample_model_device(labels_tr, labels_mask_tr, speaker_tr, num_samples, num_steps, **kw)
        return [o.detach().cpu().numpy().copy() for o in outs]


def compose_readout_output(Wr, Wo_pad, br, radd, bo_pad, oadd_pad, n_rows):
    """readout -> output as ONE affine map of [h_0 .. h_{L-1} ; w] (model.py:992-1013 with the MSE head and no layer norm):
    x = (XR . Wr + br + radd) . Wo + bo + oadd = XR . (Wr . Wo) + [(br + radd) . Wo + bo + oadd].  Composed in float64 and
    rounded once.  Returns (Wr . Wo [K, 64], constant rows [n_rows, 64]) in float32."""
    Wo64 = Wo_pad.double()
    Wro = Wr.double() @ Wo64
    rows = br.double().unsqueeze(0)
    if radd is not None:
        rows = rows + radd.double()
    c = rows @ Wo64 + bo_pad.double()
    if oadd_pad is not None:
        c = c + oadd_pad.double()
    return Wro.float(), c.expand(n_rows, Wo_pad.shape[1]).float().contiguous()

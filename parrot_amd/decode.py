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
    def _sample_workspace(self, S, N, U, stop_extra=0, forced=False, carry=False):
        ws_key = self._sample_ws_key(S, N, U, stop_extra, forced, carry)
        ws = self._sample_ws.get(ws_key)
        if ws is not None:
            return ws
        why = self._decode_bf16_refusal(N) if self.decode_bf16 else ''
        if why:  # (before anything is allocated)
            raise ValueError("decode_dtype='bf16' " + why)
        ws = self._sample_buffers(S, N, U, stop_extra, forced)
        fd, d = self._sample_descriptor(ws, S, N, U, stop_extra, forced)
        self._sample_machine_operands(ws, d, fd, N, forced, carry)
        self._sample_create_plan(ws, d, fd, S, N, U, stop_extra)
        self._sample_ws[ws_key] = ws
        return ws

    @staticmethod
    def _sample_ws_key(S, N, U, stop_extra, forced, carry=False):
        """A plan that stops at the end of the utterance is another plan: a workspace key of its own; so is a plan with
        forced frames -- a call without them keeps the key, and the plan, it had -- and so is a carry plan (state= /
        return_state=, decode_segments): ('carry', ...) in front of the rest, 'forced' included."""
        key = ('stop', S, N, U, stop_extra) if stop_extra else (S, N, U)
        key = ('forced',) + key if forced else key
        return ('carry',) + key if carry else key

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

    def _sample_machine_operands(self, ws, d, fd, N, forced, carry=False):
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
            # (a forced plan keeps the frame on the chain and does not take them; nor does a carry plan: the first step of
            # a call takes x[0] . Wf, a step inside one x_pre . Wf + h_{L-1} . (A . Wf) -- a cut would show in the bits)
            if f32_gru and not forced and not carry and L >= 2 and self._fb_layers == [1] and env_int('PARROT_PM_FBC', 1) != 0:
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
                                speaker_weights=None, forced_frames=None, n_forced=None, state=None, return_state=False):
        """sample_model_device that stops at the end of the utterance INSIDE the decode kernel instead of decoding
        max_steps frames and cutting afterwards.  The rule is end_of_utterance's (reference sample.py:145-163): a row ends
        `extra` frames after the first step whose window weight on the position just past its text beats the weight on every
        real character.  Returns (outs, lengths): the six tensors of sample_model_device cut to steps_run = max(lengths)
        along time -- bit-identical to the first steps_run steps of sample_model_device(.., max_steps) -- and lengths [N]
        (int64, on the device) = what end_of_utterance gives for each row of the full-length phi.
        timing_coeffs / sharpening_coeffs / sampling_biases / speaker_weights / forced_frames / n_forced: as
        sample_model_device (with forcing outs has the seventh tensor, own_x, cut like the others; the rule reads phi only)."""
        from .utils import end_of_utterance_args
        if state is not None or return_state:
            raise ValueError("sample_until_end does not resume: the stop lives inside one launch of the machine and the frame "
                             "a state would be taken after need not exist; decode_segments(stop_at_end=True) stops between "
                             "segments instead")
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
                         forced_frames=None, n_forced=None, state=None, return_state=False):
        """numpy twin of sample_until_end_device (as sample_model is of sample_model_device): (list of numpy arrays,
        numpy lengths [N])."""
        kw = {k: v for k, v in locals().items() if k in _PER_UTTERANCE}
        outs, lengths = self.sample_until_end_device(labels_tr, labels_mask_tr, speaker_tr, num_samples, max_steps, extra,
                                                     state=state, return_state=return_state, **kw)
        return [o.detach().cpu().numpy().copy() for o in outs], lengths.cpu().numpy()

    def sample_model_device(self, labels, labels_mask, speaker, num_samples, num_steps, unif=None, noise=None,
                            seed=None, timing_coeffs=None, sharpening_coeffs=None, sampling_biases=None, speaker_weights=None,
                            forced_frames=None, n_forced=None, state=None, return_state=False):
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
        allocated) on a wrong shape, P > num_steps, non-finite frames, n outside 0 .. P, and with decode_dtype='bf16'.
        Resuming (both left alone: the call as it is without them, on the same workspace): state -- a DecodeState
        (initial_decode_state, or what an earlier call returned): the call decodes frames t .. t + num_steps - 1 of every row
        from it instead of starting at frame 0 from the learned initial states; unif / noise / forced_frames / n_forced then
        count from the call's first frame.  return_state=True, or a state given: returns (outs, DecodeState) -- the state
        after the call's last frame.  Such a call runs on a carry plan (workspace key ('carry', ...)), which keeps the
        fed-back frame on the step's chain, so calls chained over any cut give the bits of the one carry call over all the
        frames; for a two- or three-layer GRU stack with an MSE head that is the program of PARROT_PM_FBC=0, not the default
        call's, every other configuration keeps its program.  ValueError (before anything is allocated) on a state that is
        no DecodeState, of another N or W, on another device, or not finite."""
        ctl = self._check_row_controls(num_samples, timing_coeffs, sharpening_coeffs, sampling_biases, speaker_weights)
        forced = self._check_forced(num_samples, num_steps, forced_frames, n_forced)
        carry = state is not None or bool(return_state)
        self._check_state(num_samples, state)
        return self._sample_device(None, labels, labels_mask, speaker, num_samples, num_steps, unif, noise, seed, ctl, forced,
                                   state=state, carry=carry)

    def _sample_device(self, ws, labels, labels_mask, speaker, num_samples, num_steps, unif, noise, seed, ctl=None,
                       forced=None, state=None, carry=False):
        """One decode call on the workspace `ws` (None: the plain workspace of the shape; carry: the carry workspace).
        ctl: what _check_row_controls returned (None: no per-utterance arguments); forced: what _check_forced returned
        (None: no forced frames); state: the DecodeState the call enters through (None: the learned initial states).
        Two parts: what depends on the utterances and the parameters (_decode_setup), then the run (_decode_run) --
        decode_segments does the first once and the second per segment.  carry: returns (outs, DecodeState)."""
        self.allocate()
        N, U = int(numpy.shape(labels)[0]), int(numpy.shape(labels)[1])
        assert N == num_samples
        if ws is None:
            ws = self._sample_workspace(num_steps, N, U, forced=forced is not None, carry=carry)
        self._decode_setup(ws, labels, labels_mask, speaker, ctl)
        outs = self._decode_run(ws, num_steps, unif, noise, seed, forced, state)
        if not carry:
            return outs
        done = numpy.zeros(N, dtype=numpy.int64) if state is None else state.frames_done
        return outs, self._save_decode_state(ws, done + num_steps)

    def _decode_setup(self, ws, labels, labels_mask, speaker, ctl=None, weights=True):
        """Everything of a decode call that depends on the utterances and the parameters and not on where in the utterance
        the run starts: encoder, bias sums, row controls, speaker terms, the machine's weight copies and constant rows.
        weights=False (StreamingDecoder, when a slot gets a new utterance and the parameters are what they were): the
        fragment-major weight copies stay; only what depends on the utterances is written again."""
        controls, speaker_weights = ctl if ctl is not None else (None, None)
        dev = self._dev()
        labels = torch.as_tensor(labels).to(dev)
        labels_mask = torch.as_tensor(labels_mask).to(dev, torch.float32)
        L = self.num_layers
        ws['ctx'].copy_(self._encoder_forward(labels, labels_mask, None))
        self._sum_layer_biases(ws, extra_fb=not self.layer_norm)
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
        if 'pm' in ws:
            self._refresh_sample_machine_weights(ws, tiles=weights)

    def _write_initial_state(self, ws):
        """The learned initial states into the entering slots (slot 0) of the workspace; x[0] = 0, model.py:834-835."""
        N = ws['x'].shape[1]
        for l in range(1, self.num_layers + 1):
            ws['h'][l - 1][0].copy_(self._p(f'/rnn{l}.initial_state').unsqueeze(0).expand(N, -1))
            if self.cell_type == 'lstm':
                ws['cwork'][l - 1][0].copy_(self._p(f'/rnn{l}.initial_cells').unsqueeze(0).expand(N, -1))
        ws['x'][0].zero_()
        ws['w'][0].copy_(self._p('.initial_w').unsqueeze(0).expand(N, -1))
        ws['kappa'][0].zero_()

    def _decode_run(self, ws, num_steps, unif, noise, seed, forced=None, state=None, n_valid=None):
        """The run of a decode call on a workspace that _decode_setup has prepared: forced frames, the entering state,
        the randomness, the plan.  num_steps: the plan's S.  n_valid (decode_segments' last segment): unif / noise / the
        forced frames cover the first n_valid steps only, the rest run on zeros and are cut by the caller."""
        dev = self._dev()
        S, O = num_steps, self.output_dim
        if forced is not None:  # every call rewrites both arrays whole: nothing of an earlier prompt survives
            frames, n = forced
            ws['forced'].zero_()
            ws['forced'][:frames.shape[0], :, :O].copy_(torch.as_tensor(frames))
            ws['n_forced'].copy_(torch.as_tensor(n))
        if state is None:
            self._write_initial_state(ws)
        else:
            _lib.call('parrot_sample_load_state', ws['plan'], state.tensor.data_ptr(), ops._stream())
        if self.which_cost == 'GMM':
            if unif is None or noise is None:
                unif, noise = self._decode_randomness(S, ws['x'].shape[1], seed)
            k = S if n_valid is None else n_valid
            if k < S:
                ws['unif'][k:].zero_()
                ws['noise'][k:].zero_()
            ws['unif'][:k].copy_(torch.as_tensor(unif).to(dev, torch.float32))
            ws['noise'][:k].copy_(torch.as_tensor(noise).to(dev, torch.float32))
        _lib.call('parrot_sample_run', ws['plan'], ops._stream())
        if 'pm' in ws:  # persistent machine: a launch that gave up leaves invalid frames -- fail loudly (synchronises)
            _lib.call('parrot_sample_status', ws['plan'])
        self._decode_path = 'machine' if _lib.load().parrot_sample_is_persistent(ws['plan']) else 'launches'
        sx = ws['x'][1:, :, :O]
        pi = ws['pi_out'] if self.which_cost == 'GMM' else sx
        outs = [sx, ws['kappa'][1:], ws['w'][1:], pi, ws['phi'], ws['a']]
        return outs + [ws['own_x'][:, :, :O]] if forced is not None else outs

    def _decode_randomness(self, S, N, seed):
        """unif [S, N] and noise [S, N, O] of a GMM head from torch's generator (`seed`, else the model's)."""
        g = torch.Generator(device=self._dev())
        g.manual_seed(int(self.seed if seed is None else seed))
        unif = torch.rand(S, N, device=self._dev(), generator=g)
        return unif, torch.randn(S, N, self.output_dim, device=self._dev(), generator=g)

    # ---- resumable decoding: the state a call hands on (parrot_sample_save_state / _load_state) ----------------------------
    def _decode_state_pieces(self):
        """[(name, width)] of a decode state's row, in the library's order (include/parrot_hip.h): x (ldx) | kappa (A) | w (E)
        | h_0 .. h_{L-1} (H each) | c_0 .. c_{L-1} (H each, LSTM only)."""
        H, L = self.rnn_h_dim, self.num_layers
        pieces = [('x', (self.output_dim + 3) // 4 * 4), ('kappa', self.attention_size), ('w', self.encoded_input_dim)]
        pieces += [(('h', l), H) for l in range(L)]
        return pieces + [(('c', l), H) for l in range(L)] if self.cell_type == 'lstm' else pieces

    def decode_state_floats(self):
        """W: the floats one utterance carries from frame to frame (parrot_sample_state_floats of the decode descriptor)."""
        return sum(wd for _, wd in self._decode_state_pieces())

    def initial_decode_state(self, num_samples):
        """The DecodeState every utterance starts from: the learned initial states and cells, initial_w, zero kappa, zero x."""
        self.allocate()
        st = DecodeState(self, torch.zeros(int(num_samples), self.decode_state_floats(), device=self._dev(), dtype=torch.float32))
        st.reset_rows(range(int(num_samples)))
        return st

    def _check_state(self, N, state):
        """Refuses a state the call cannot enter through, without touching the workspace: ValueError on something that is no
        DecodeState, another N, another W, another device, a non-finite value."""
        if state is None:
            return
        if not isinstance(state, DecodeState):
            raise ValueError(f"state must be a DecodeState (Parrot.initial_decode_state, or what a call returned), "
                             f"got {type(state).__name__}")
        t, W, dev = state.tensor, self.decode_state_floats(), self._dev()
        if t.dim() != 2 or t.shape[0] != N:
            raise ValueError(f"state holds {tuple(t.shape)[0] if t.dim() else 0} utterances, the call decodes N = {N}")
        if t.shape[1] != W:
            raise ValueError(f"state rows hold {t.shape[1]} floats, this model carries W = {W} per utterance")
        if t.device.type != dev.type or (dev.index is not None and t.device.index != dev.index):
            raise ValueError(f"state lives on device {t.device}, the model decodes on {dev}")
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("state must be a contiguous float32 tensor [N, W]")
        if not bool(torch.isfinite(t).all()):
            raise ValueError("state must be finite")

    def _save_decode_state(self, ws, frames_done):
        """The state after the last frame of the workspace's last run, as a new DecodeState."""
        t = torch.empty(ws['x'].shape[1], self.decode_state_floats(), device=self._dev(), dtype=torch.float32)
        _lib.call('parrot_sample_save_state', ws['plan'], t.data_ptr(), ops._stream())
        return DecodeState(self, t, frames_done)

    def decode_segments(self, labels, labels_mask, speaker, num_samples, num_steps, segment_frames, unif=None, noise=None,
                        seed=None, timing_coeffs=None, sharpening_coeffs=None, sampling_biases=None, speaker_weights=None,
                        forced_frames=None, n_forced=None, stop_at_end=False, extra=40, state=None):
        """sample_model_device in segments of `segment_frames` frames, handed out as each completes: iterating yields
        (t0, outs) -- the tensors of sample_model_device for frames t0 .. t0 + len - 1 (own copies; with forcing the seventh,
        own_x).  One carry plan of segment_frames steps runs every segment; encoder, speaker terms and weight copies are made
        once, a boundary saves and loads the state and slices unif / noise / the forced frames (n_forced - t0, clamped to the
        segment).  The last, shorter segment runs whole and is cut.  The frames are, bit for bit, those of the one carry call
        over num_steps frames (sample_model_device(.., return_state=True)).
        The end-of-utterance rule runs per segment on the device (segment_end_of_utterance: end_of_utterance_args' strict
        predicate; the first firing step of a row is carried across segments): `.first` [N] (-1: not yet) and `.lengths` [N]
        (first + extra, at most num_steps; num_steps where the row never fired) are current after every segment.
        stop_at_end=True: the iteration ends after the segment in which the longest row's first + extra falls -- the
        overshoot is less than one segment.  `.state`: the DecodeState after the last segment RUN (a cut last segment has
        run segment_frames frames: .state.frames_done says so).  unif / noise: [num_steps, N(, O)], else from `seed` as
        sample_model_device draws them; state: enter through a DecodeState instead of the learned initial states.
        ValueError before anything is allocated, as sample_model_device, and on segment_frames < 1."""
        if int(segment_frames) < 1:
            raise ValueError(f"segment_frames must be >= 1, got {segment_frames}")
        ctl = self._check_row_controls(num_samples, timing_coeffs, sharpening_coeffs, sampling_biases, speaker_weights)
        forced = self._check_forced(num_samples, num_steps, forced_frames, n_forced)
        self._check_state(num_samples, state)
        return DecodeSegments(self, labels, labels_mask, speaker, int(num_samples), int(num_steps), int(segment_frames), unif,
                              noise, seed, ctl, forced, bool(stop_at_end), int(extra), state)

    def synthesize_segments(self, labels, labels_mask, speaker, num_samples, num_steps, segment_frames, stream_frames,
                            n_streams=32, temperature=0.0, seeds=None, draw_mode='sequential', top_k=0, top_p=0.0, min_p=0.0,
                            stop_at_end=True, extra=40, **decode_args):
        """Text to audio for a fixed batch: decode_segments(stop_at_end=...) whose segments feed a SampleRNN
        StreamingGenerator with open utterances (n_streams streams, segments of stream_frames frames) on the device, so the
        vocoder runs an utterance's first frames while the decoder is at its later ones.  Iterating yields (i, samples int32
        [80 k], done) for row i as they are produced; row i's first 80 samples are its Q/2 prefix, and its samples add up to
        80 * max(its length, 1), the length decode_segments' end-of-utterance rule gives.  Row i is closed as soon as the rule
        has fixed its length and the frames up to it are fed.  seeds = one per row: per-utterance draws at `temperature`
        (StreamingGenerator(utterance_draws=True)); draw_mode, top_k, top_p, min_p: the vocoder's.  decode_args:
        decode_segments' (the per-utterance controls, forced_frames / n_forced, unif / noise / seed).  The iteration has
        `.decode` (the DecodeSegments: .lengths, .first), `.outs` (every segment's output tensors, on the device),
        `.vocoder` and `.first_audio_s`.  Takes what decode_segments takes, the literal encoder included; ValueError before
        anything runs on what either half refuses, and on output_dim != the vocoder's FEAT_DIM."""
        F = _vocoder_feat_dim()
        if self.output_dim != F:
            raise ValueError(f"the vocoder is conditioned on frames of {F} floats, this model's output_dim is {self.output_dim}")
        if seeds is not None and len(seeds) != int(num_samples):
            raise ValueError(f"seeds needs one entry per utterance ({num_samples}), got {len(seeds)}")
        run = self.decode_segments(labels, labels_mask, speaker, num_samples, num_steps, segment_frames,
                                   stop_at_end=stop_at_end, extra=extra, **decode_args)
        return SynthesisSegments(run, int(stream_frames), int(n_streams), seeds,
                                 dict(temperature=temperature, draw_mode=draw_mode, top_k=top_k, top_p=top_p, min_p=min_p))

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

    def _refresh_sample_machine_weights(self, ws, tiles=True):
        """Fragment-major weight copies of the decode machine from the current parameters, and the constant rows that carry
        the speaker terms (ro_const / rh_const / oadd_pad).  tiles=False: the constant rows only."""
        pm, st = ws['pm'], self.store.storage
        H, E, L, O = self.rnn_h_dim, self.encoded_input_dim, self.num_layers, self.output_dim
        lstm_H = H if self.cell_type == 'lstm' else 0
        with torch.no_grad():
            for l in range(L if tiles else 0):
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
                if tiles:
                    pm['Wrh'].copy_(Wrh)
                    self._tile_machine_weight(pm['Wrh'], pm['Wrh_t'])
                pm['rh_const'].copy_(c)
            else:
                self._refresh_mse_head_weights(ws, tiles)

    def _refresh_mse_head_weights(self, ws, tiles=True):
        """The MSE head's part of _refresh_sample_machine_weights: readout stack, output projection, their composition, the
        folded attention projection and the composed feedback rows (called under no_grad)."""
        pm, st = ws['pm'], self.store.storage
        H, E, L, O = self.rnn_h_dim, self.encoded_input_dim, self.num_layers, self.output_dim
        if not tiles:  # the constant rows from the padded copies as they stand (the parameters have not changed)
            if 'oadd_pad' in pm:
                pm['oadd_pad'][:, :O].copy_(ws['oadd'])
            pm['ro_const'].copy_(compose_readout_output(st['dec.Wr'], pm['Wo_pad'], ws['br'], ws['radd'], pm['bo_pad'],
                                                        pm.get('oadd_pad'), pm['ro_const'].shape[0])[1])
            return
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
                     forced_frames=None, n_forced=None, state=None, return_state=False):
        """Parrot.sample_model (model.py:1061-1083): numpy in, list of numpy arrays out
        [sample_x, k, w, pi, phi, pi_att], all time-major (the caller swaps axes, sample.py:142-143).  The keyword
        arguments: per utterance, as sample_model_device (forced_frames / n_forced: a seventh array, own_x); state /
        return_state: as there -- (list of numpy arrays, DecodeState), the state stays on the device."""
        kw = {k: v for k, v in locals().items() if k in _PER_UTTERANCE}
        outs = self.sample_model_device(labels_tr, labels_mask_tr, speaker_tr, num_samples, num_steps, state=state,
                                        return_state=return_state, **kw)
        if state is not None or return_state:
            return [o.detach().cpu().numpy().copy() for o in outs[0]], outs[1]
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


class DecodeState:
    """What a decode call hands to the next: one packed float32 tensor [N, W] on the model's device, row b = everything
    utterance b carries from frame t to frame t + 1 (the library's layout, include/parrot_hip.h), so admitting or evicting
    an utterance is a row copy.  Named views into it: x [N, ldx], kappa [N, A], w [N, E], h[l] and (LSTM) c[l] [N, H].
    frames_done: int64 numpy array [N], the frames each row has decoded since its initial state."""

    def __init__(self, parrot, tensor, frames_done=None):
        self._parrot, self.tensor = parrot, tensor
        N = tensor.shape[0]
        self.frames_done = (numpy.zeros(N, dtype=numpy.int64) if frames_done is None
                            else numpy.array(frames_done, dtype=numpy.int64).reshape(N))
        self.h, self.c, col = [], [], 0
        for name, wd in parrot._decode_state_pieces():
            view = tensor[:, col:col + wd]
            col += wd
            if isinstance(name, tuple):
                getattr(self, name[0]).append(view)
            else:
                setattr(self, name, view)

    def reset_rows(self, rows):
        """The learned initial state into the given rows: initial states and cells, initial_w, zero kappa, zero x."""
        p = self._parrot
        rows = [int(r) for r in rows]
        idx = torch.as_tensor(rows, device=self.tensor.device, dtype=torch.long)
        with torch.no_grad():
            self.x[idx] = 0.
            self.kappa[idx] = 0.
            self.w[idx] = p._p('.initial_w').to(self.tensor.device)
            for l in range(len(self.h)):
                self.h[l][idx] = p._p(f'/rnn{l + 1}.initial_state').to(self.tensor.device)
            for l in range(len(self.c)):
                self.c[l][idx] = p._p(f'/rnn{l + 1}.initial_cells').to(self.tensor.device)
        self.frames_done[rows] = 0
        return self

    def clone(self):
        return DecodeState(self._parrot, self.tensor.clone(), self.frames_done.copy())


def segment_end_of_utterance(phi, pos, ncmp, first, t0):
    """The end-of-utterance rule on one segment, on phi's device: phi [F, N, U] are frames t0 .. t0 + F - 1 (t0: an int, or
    int64 [N] where every row counts its own frames), pos / ncmp [N]
    what utils.end_of_utterance_args gives, first [N] (int64) the first firing step of each row so far, -1: none.  A step
    fires when phi[pos] > phi[j] for EVERY j < ncmp (strict, as end_of_utterance and the decode machine's PmAtt).  Returns
    the new `first`: rows that had fired keep their step, the others get t0 + their first firing step of this segment."""
    F, N, U = phi.shape
    at = phi.gather(2, pos.long().view(1, N, 1).expand(F, N, 1))
    ignore = torch.arange(U, device=phi.device).view(1, U) >= ncmp.long().view(N, 1)
    fires = ((at > phi) | ignore.unsqueeze(0)).all(dim=2)                     # [F, N]
    step = torch.where(fires, torch.arange(F, device=phi.device).view(F, 1).expand(F, N),
                       torch.full((F, N), F, device=phi.device)).min(dim=0).values
    t0 = t0.to(phi.device).long() if torch.is_tensor(t0) else int(t0)  # (a tensor [N]: every row counts from its own frame)
    return torch.where((first < 0) & (step < F), step + t0, first)


class DecodeSegments:
    """The iteration Parrot.decode_segments returns: yields (t0, outs) per segment; .first / .lengths / .state follow it."""

    def __init__(self, parrot, labels, labels_mask, speaker, N, S, F, unif, noise, seed, ctl, forced, stop, extra, state):
        self._m, self._args = parrot, (labels, labels_mask, speaker, unif, noise, seed, ctl, forced, state)
        self.num_samples, self.num_steps, self.segment_frames, self.stop_at_end, self.extra = N, S, F, stop, extra
        self.state, self.first, self.frames = state, None, 0
        self._it = self._run()

    def __iter__(self):
        return self

    def __next__(self):
        return next(self._it)

    @property
    def lengths(self):
        """[N] int64 on the device: first + extra cut at num_steps, num_steps for a row that has not fired."""
        if self.first is None:
            return None
        S = self.num_steps
        return torch.where(self.first >= 0, (self.first + self.extra).clamp(max=S), torch.full_like(self.first, S))

    def _run(self):
        from .utils import end_of_utterance_args
        m, N, S, F = self._m, self.num_samples, self.num_steps, self.segment_frames
        labels, labels_mask, speaker, unif, noise, seed, ctl, forced, state = self._args
        m.allocate()
        dev = m._dev()
        lm = torch.as_tensor(labels_mask)
        U = lm.shape[1]
        ws = m._sample_workspace(F, N, U, forced=forced is not None, carry=True)
        m._decode_setup(ws, labels, labels_mask, speaker, ctl)
        gmm = m.which_cost == 'GMM'
        if gmm:  # the whole call's randomness once, as the one-piece call draws it; a segment takes its slice
            if unif is None or noise is None:
                unif, noise = m._decode_randomness(S, N, seed)
            unif, noise = torch.as_tensor(unif).to(dev, torch.float32), torch.as_tensor(noise).to(dev, torch.float32)
        pos, ncmp = (torch.from_numpy(a).to(dev) for a in end_of_utterance_args(lm.detach().cpu().numpy(), U))
        self.first = torch.full((N,), -1, device=dev, dtype=torch.long)
        done = numpy.zeros(N, dtype=numpy.int64) if state is None else state.frames_done
        for t0 in range(0, S, F):
            r = min(F, S - t0)
            seg_forced = None
            if forced is not None:
                frames, n = forced
                seg_forced = (frames[t0:t0 + r], numpy.clip(n.astype(numpy.int64) - t0, 0, r).astype(numpy.int32))
            outs = m._decode_run(ws, F, unif[t0:t0 + r] if gmm else None, noise[t0:t0 + r] if gmm else None, None,
                                 seg_forced, self.state, n_valid=r)
            self.state = m._save_decode_state(ws, done + t0 + F)
            outs = [o[:r].clone() for o in outs]  # (the next segment overwrites the workspace)
            self.first = segment_end_of_utterance(outs[4], pos, ncmp, self.first, t0)
            self.frames = t0 + r
            yield t0, outs
            if self.stop_at_end and bool((self.first >= 0).all()) and int(self.first.max()) + self.extra <= t0 + r:
                break


class SynthesisSegments:
    """The iteration Parrot.synthesize_segments returns: yields (i, samples, done); .decode, .outs, .vocoder, .first_audio_s."""

    def __init__(self, run, stream_frames, n_streams, seeds, vocoder_args):
        from .sampleRNN.generation.serving import StreamingGenerator
        self.decode, self.outs, self.first_audio_s, self._seeds = run, [], None, seeds
        self.vocoder = StreamingGenerator(n_streams, stream_frames, utterance_draws=seeds is not None, open_utterances=True,
                                          max_frames=run.num_steps, store_utterances=run.num_samples, **vocoder_args)
        self._it = self._run()

    def __iter__(self):
        return self

    def __next__(self):
        return next(self._it)

    def _feed(self, t0, frames, fed, closed):
        """The new frames of every open row into the vocoder; a row is closed with the last frame of its length."""
        run, S = self.decode, self.decode.num_steps
        first = run.first.cpu().tolist()
        for i in range(run.num_samples):
            if closed[i]:
                continue
            length = S if first[i] < 0 else max(min(first[i] + run.extra, S), 1)
            hi = min(t0 + frames.shape[0], length)
            closed[i] = hi == length
            self.vocoder.feed(i, frames[fed[i] - t0:hi - t0, i], last=closed[i])
            fed[i] = hi

    def _run(self):
        import time
        from .sampleRNN.generation.inputs import config
        start, sg, run, prefix = time.perf_counter(), self.vocoder, self.decode, config().BIG_FRAME_SIZE
        N = run.num_samples
        try:
            for i in range(N):
                assert sg.open(**({} if self._seeds is None else dict(seed=self._seeds[i]))) == i
            fed, closed, heard, decoding = [0] * N, [False] * N, set(), True
            while not sg.idle():
                while decoding and sg.short_of_segment():
                    seg = next(run, None)
                    decoding = seg is not None
                    if decoding:
                        self.outs.append(seg[1])
                        self._feed(seg[0], seg[1][0], fed, closed)
                assert decoding or all(closed), "the decoder ended with an utterance open"
                for i, chunk, done in sg.step():
                    if self.first_audio_s is None and chunk.size and (i in heard or chunk.size > prefix):
                        self.first_audio_s = time.perf_counter() - start
                    heard.add(i)
                    yield i, chunk, done
        finally:
            sg.close()


class StreamingDecoder:
    """Continuous admission for the decoder: `slots` utterances decode side by side on ONE carry plan of `segment_frames`
    steps; between segments a finished utterance is handed out and its slot goes to the next one queued.
      submit(labels, ...) -> id       queue one utterance (labels: 1 .. max_text label indices)
      run()                           yields (id, frames [length, O], phi [length, max_text]) as utterances end
      run_segments()                  yields (id, t0, frames [k, O], done) per utterance in flight after every segment
    An utterance ends `extra` frames after the end-of-utterance rule first fires on its phi (segment_end_of_utterance, per
    segment, on the device), at max_frames at the latest; length is what utils.end_of_utterance gives for its full phi with
    num_steps = max_frames.  A plain boundary saves and loads the state and slices the rows' randomness and prompts.  A
    boundary that admits utterances also writes the learned initial state into their rows (DecodeState.reset_rows), runs
    the encoder and the speaker products for the batch again -- with the batch size the plan has, so a row's context has
    the bits it would have in any other call of this shape; the rows in flight get their own values again -- and rewrites
    the label mask's indices, the constant rows and the row controls.  The fragment-major weight copies are made once; they
    are made again when the parameter buffer was written through torch since (its version counter), or after
    refresh_parameters().  Idle slots decode a one-character dummy whose frames nobody reads.  A row's frames are, bit for
    bit, those of Parrot.decode_segments with the utterance in the same slot of a batch of this shape.  Rows must not see one
    another: a model whose encoder recurs along the batch axis (encoder_literal=True, the reference's) is refused."""

    def __init__(self, parrot, slots, segment_frames, max_text, max_frames, extra=40):
        import collections
        for name, v in (('slots', slots), ('segment_frames', segment_frames), ('max_text', max_text), ('max_frames', max_frames)):
            if int(v) < 1:
                raise ValueError(f"{name} must be >= 1, got {v}")
        if int(extra) < 0:
            raise ValueError(f"extra must be >= 0, got {extra}")
        if parrot.encoder_type is not None and parrot.encoder_literal:
            raise ValueError("StreamingDecoder needs encoder_literal=False: the literal encoder (the reference's) recurs along "
                             "the batch axis, so a row's context depends on its neighbours and would change when one is admitted")
        self._m, self.slots, self.segment_frames = parrot, int(slots), int(segment_frames)
        self.max_text, self.max_frames, self.extra = int(max_text), int(max_frames), int(extra)
        self._queue, self._next_id, self._stale = collections.deque(), 0, True
        self.segments_run = self.setups_run = self.tilings_run = 0
        self.placements = {}   # id -> (slot, the segment it was admitted in front of)
        self._rows = []        # the utterances in flight, per slot, of the loop that is running

    @property
    def busy(self):
        """Whether an utterance is queued or in flight: whether another segment would decode anything."""
        return bool(self._queue) or any(r is not None for r in self._rows)

    def refresh_parameters(self):
        """The parameters were written behind torch's back (a fused optimiser step): tile the weights again at the next boundary."""
        self._stale = True

    def submit(self, labels, speaker=None, timing_coeff=None, sharpening_coeff=None, sampling_bias=None, speaker_weights=None,
               seed=None, unif=None, noise=None, forced_frames=None):
        """Queues one utterance; returns its id.  labels: 1 .. max_text label indices; speaker: its index (use_speaker);
        timing_coeff / sharpening_coeff / sampling_bias: its own value in place of the model's scalar; speaker_weights
        [num_speakers]: a blend of the speaker table in place of `speaker`; GMM head: unif [max_frames] and noise
        [max_frames, O], else drawn from `seed` (default: the model's seed + id); forced_frames [P, O], P <= max_frames:
        the utterance is primed with them.  ValueError on what the decode calls refuse (_check_row_controls, _check_forced)."""
        m, O = self._m, self._m.output_dim
        lab = numpy.asarray(_as_numpy(labels)).reshape(-1)
        if not 1 <= lab.shape[0] <= self.max_text:
            raise ValueError(f"labels needs 1 .. {self.max_text} entries (max_text), got {lab.shape[0]}")
        one = lambda v: None if v is None else [v]
        ctl, sw = m._check_row_controls(1, one(timing_coeff), one(sharpening_coeff), one(sampling_bias),
                                        None if speaker_weights is None else numpy.asarray(_as_numpy(speaker_weights))[None])
        if m.use_speaker and speaker is None and sw is None:
            raise ValueError("this model has speakers: submit needs speaker= or speaker_weights=")
        prompt = None
        if forced_frames is not None:
            fr = numpy.asarray(_as_numpy(forced_frames))
            if fr.ndim != 2:
                raise ValueError(f"forced_frames needs shape (P, {O}) = (frames, output_dim), got {tuple(fr.shape)}")
            prompt = m._check_forced(1, self.max_frames, fr[:, None, :], [fr.shape[0]])[0][:, 0]
        rnd = None
        if m.which_cost == 'GMM' and unif is not None and noise is not None:
            u, z = (numpy.asarray(_as_numpy(a), dtype=numpy.float32) for a in (unif, noise))
            if u.shape != (self.max_frames,) or z.shape != (self.max_frames, O):
                raise ValueError(f"unif / noise need shapes ({self.max_frames},) and ({self.max_frames}, {O}), "
                                 f"got {tuple(u.shape)} and {tuple(z.shape)}")
            rnd = (u, z)
        uid = self._next_id
        self._next_id += 1
        self._queue.append(dict(id=uid, labels=lab.astype(numpy.int64), speaker=0 if speaker is None else int(speaker),
                                ctl=ctl, sw=None if sw is None else sw[0], seed=seed, rnd=rnd, prompt=prompt))
        return uid

    def _admit(self, slot, u, host):
        """The queued utterance u into row `slot` of the host-side batch."""
        m, T = self._m, self.max_frames
        host['labels'][slot] = 0
        host['mask'][slot] = 0.
        host['labels'][slot, :len(u['labels'])] = u['labels']
        host['mask'][slot, :len(u['labels'])] = 1.
        host['speaker'][slot, 0] = u['speaker']
        for key, scalar in (('timing', m.timing_coeff), ('sharpening', m.sharpening_coeff), ('bias', m.sampling_bias)):
            if host[key] is not None:  # (no bias array without a GMM head: _check_row_controls has refused a bias)
                host[key][slot] = scalar if u['ctl'][key] is None else u['ctl'][key][0]
        if u['sw'] is not None or host['blend']:
            if not host['blend']:  # the first blended utterance: from here on every row is a row of weights (one-hot: the index)
                host['blend'] = True
                host['sw'][:] = 0.
                host['sw'][numpy.arange(self.slots), host['speaker'][:, 0]] = 1.
            host['sw'][slot] = 0.
            if u['sw'] is not None:
                host['sw'][slot] = u['sw']
            else:
                host['sw'][slot, u['speaker']] = 1.
        if m.which_cost == 'GMM':
            if u['rnd'] is None:
                a, b = m._decode_randomness(T, 1, m.seed + u['id'] if u['seed'] is None else u['seed'])
                u['rnd'] = (a[:, 0].cpu().numpy(), b[:, 0].cpu().numpy())
        return dict(u, t=0, first=-1, frames=[], phi=[])

    def run(self):
        """Decodes everything queued (utterances submitted while it runs included); yields (id, frames [length, O],
        phi [length, max_text]) -- device tensors -- as each utterance ends."""
        for batch in self._segments(False, True):
            yield from batch

    def run_segments(self, with_phi=False):
        """run(), handing the frames out as they are decoded: after every segment yields, for each utterance in flight,
        (id, t0, frames [k, O], done) -- the new device frames t0 .. t0 + k - 1 (k = segment_frames; in the utterance's last
        yield, done=True, they are trimmed so that the total is its length, run()'s rule: first + extra, at most
        max_frames).  with_phi=True: (id, t0, frames, phi [k, max_text], done).  Concatenated per id the frames (and phi) are
        run()'s, bit for bit."""
        for batch in self._segments(True, with_phi):
            yield from batch

    def _segments(self, per_segment, with_phi):
        """The loop behind run() and run_segments(): one list per decoder segment of what they yield for it."""
        from .utils import end_of_utterance_args
        m, N, F, U, T, O = self._m, self.slots, self.segment_frames, self.max_text, self.max_frames, self._m.output_dim
        m.allocate()
        dev = m._dev()
        forced, gmm = not m.decode_bf16, m.which_cost == 'GMM'   # (the bf16 programs have no kernels with forcing)
        ws = m._sample_workspace(F, N, U, forced=forced, carry=True)
        host = dict(labels=numpy.zeros((N, U), dtype=numpy.int64), mask=numpy.zeros((N, U), dtype=numpy.float32),
                    speaker=numpy.zeros((N, 1), dtype=numpy.int64), blend=False,
                    sw=numpy.zeros((N, m.num_speakers), dtype=numpy.float32) if m.use_speaker else None,
                    timing=numpy.full(N, m.timing_coeff, dtype=numpy.float32),
                    sharpening=numpy.full(N, m.sharpening_coeff, dtype=numpy.float32),
                    bias=numpy.full(N, m.sampling_bias, dtype=numpy.float32) if gmm else None)
        host['mask'][:, 0] = 1.   # idle slots: a one-character dummy
        rows = self._rows = [None] * N
        state = m.initial_decode_state(N)
        pos = ncmp = None
        version = None
        while self._queue or any(r is not None for r in rows):
            admitted = []
            for b in range(N):
                if rows[b] is None and self._queue:
                    u = self._queue.popleft()
                    if u['prompt'] is not None and not forced:
                        raise ValueError("forced_frames " + m._decode_forced_refusal())
                    rows[b] = self._admit(b, u, host)
                    self.placements[u['id']] = (b, self.segments_run)
                    admitted.append(b)
            if admitted or pos is None:
                stale = self._stale or version != m.store.flat._version
                ctl = dict(timing=host['timing'], sharpening=host['sharpening'], bias=host['bias'])
                m._decode_setup(ws, host['labels'], host['mask'], host['speaker'], (ctl, host['sw'] if host['blend'] else None),
                                weights=stale)
                self._stale, version = False, m.store.flat._version
                self.setups_run += 1
                self.tilings_run += int(stale)
                state.reset_rows(admitted)
                pos, ncmp = (torch.from_numpy(a).to(dev) for a in end_of_utterance_args(host['mask'], U))
            unif = noise = seg_forced = None
            if gmm:
                unif, noise = numpy.zeros((F, N), dtype=numpy.float32), numpy.zeros((F, N, O), dtype=numpy.float32)
            if forced:
                frames, n = numpy.zeros((F, N, O), dtype=numpy.float32), numpy.zeros(N, dtype=numpy.int32)
                seg_forced = (frames, n)
            t0 = numpy.zeros(N, dtype=numpy.int64)
            for b, r in enumerate(rows):
                if r is None:
                    continue
                t0[b] = t = r['t']
                k = min(F, T - t)
                if gmm:
                    unif[:k, b], noise[:k, b] = r['rnd'][0][t:t + k], r['rnd'][1][t:t + k]
                if r['prompt'] is not None and t < r['prompt'].shape[0]:
                    seg = r['prompt'][t:t + F]
                    frames[:seg.shape[0], b], n[b] = seg, seg.shape[0]
            outs = m._decode_run(ws, F, unif, noise, None, seg_forced, state)
            state = m._save_decode_state(ws, state.frames_done + F)
            self.segments_run += 1
            sx, phi = outs[0].clone(), outs[4].clone()
            first = torch.tensor([-1 if r is None else r['first'] for r in rows], device=dev, dtype=torch.long)
            first = segment_end_of_utterance(phi, pos, ncmp, first, torch.from_numpy(t0)).cpu().tolist()
            batch = []
            for b, r in enumerate(rows):
                if r is None:
                    continue
                t_seg = r['t']
                r['first'], r['t'] = first[b], t_seg + F
                length = T if r['first'] < 0 else min(r['first'] + self.extra, T)
                done = r['t'] >= length
                if per_segment:
                    k = max(0, min(F, length - t_seg)) if done else F
                    batch.append((r['id'], t_seg, sx[:k, b]) + ((phi[:k, b],) if with_phi else ()) + (done,))
                else:
                    r['frames'].append(sx[:, b])
                    r['phi'].append(phi[:, b])
                    if done:
                        batch.append((r['id'], torch.cat(r['frames'])[:length], torch.cat(r['phi'])[:length]))
                if done:
                    rows[b] = None
            yield batch


def _vocoder_feat_dim():
    from .sampleRNN.generation.inputs import config
    return config().FEAT_DIM


class TextToAudio:
    """Text to audio in one stream: a StreamingDecoder (`.decoder`) whose segments feed a SampleRNN StreamingGenerator with
    open utterances (`.vocoder`), so the audio of an utterance's first frames is out while its later frames are decoded.
      submit(labels, ...) -> id       StreamingDecoder.submit's arguments, and seed= / temperature= / top_k= / top_p= /
                                      min_p= of the vocoder's draws (StreamingGenerator.open's rules); the seed of a GMM
                                      head's own randomness, StreamingDecoder.submit's seed=, is decoder_seed= here
      run()                           yields (id, samples int32 [80 k], done) as they are produced; an utterance's first 80
                                      samples are its Q/2 prefix
    A decoded segment is copied on the device into the vocoder's frame store and fed as device tensors: no frame visits the
    host.  The policy is deterministic: before each vocoder step, decoder segments run until no utterance the vocoder is
    running or would place next is short of a full vocoder segment, or every such utterance is closed, or the decoder has
    nothing in flight; then one vocoder step runs.  A text enters the decoder only while the vocoder's store has a free row
    (pool_utterances rows, default decoder_slots + vocoder_streams; a row frees when the vocoder reports its utterance
    done).  `.decoder.placements[id]` and `.vocoder.record[.tickets[id]]` say where each utterance ran: its samples are those of the
    vocoder's standalone run, in that stream, of the frames Parrot.decode_segments gives it in that slot (temperature 0,
    or utterance_draws=True).  `.first_audio_s`: seconds from run()'s start to the first chunk that holds samples behind a
    prefix.  Refuses what its two halves refuse -- the literal encoder among them -- and a model whose output_dim is not
    the vocoder's FEAT_DIM."""

    def __init__(self, parrot, decoder_slots, decoder_segment_frames, max_text, max_frames, vocoder_streams,
                 vocoder_segment_frames, extra=40, pool_utterances=None, temperature=0.0, utterance_draws=False,
                 draw_mode='sequential', top_k=0, top_p=0.0, min_p=0.0, run_segment=None):
        import collections
        F = _vocoder_feat_dim()
        if parrot.output_dim != F:
            raise ValueError(f"the vocoder is conditioned on frames of {F} floats, this model's output_dim is {parrot.output_dim}")
        self.decoder = StreamingDecoder(parrot, decoder_slots, decoder_segment_frames, max_text, max_frames, extra=extra)
        pool = int(decoder_slots) + int(vocoder_streams) if pool_utterances is None else int(pool_utterances)
        if pool < 1:
            raise ValueError(f"pool_utterances must be >= 1, got {pool_utterances}")
        from .sampleRNN.generation.serving import StreamingGenerator
        self.vocoder = StreamingGenerator(vocoder_streams, vocoder_segment_frames, temperature=temperature,
                                          utterance_draws=utterance_draws, draw_mode=draw_mode, top_k=top_k, top_p=top_p,
                                          min_p=min_p, open_utterances=True, max_frames=max_frames, store_utterances=pool,
                                          run_segment=run_segment)
        self._pending = collections.deque()   # (the decoder's queue entry, the vocoder's draw arguments): not yet admitted
        self.tickets, self._uid = {}, {}      # id -> the vocoder's ticket (kept), and back from admission until done
        self._segments = None
        self.first_audio_s = None

    def submit(self, labels, speaker=None, seed=None, temperature=None, top_k=None, top_p=None, min_p=None,
               decoder_seed=None, **decoder_args):
        draws = dict(seed=seed, temperature=temperature, top_k=top_k, top_p=top_p, min_p=min_p)
        self.vocoder._check_draws(**draws)
        uid = self.decoder.submit(labels, speaker=speaker, seed=decoder_seed, **decoder_args)
        self._pending.append((self.decoder._queue.pop(), draws))  # (held back until a store row is free)
        return uid

    def _admit(self):
        while self._pending and self.vocoder.free_rows:
            u, draws = self._pending.popleft()
            ticket = self.vocoder.open(**draws)
            self.tickets[u['id']], self._uid[ticket] = ticket, u['id']
            self.decoder._queue.append(u)

    def _decode_segment(self):
        """One decoder segment, its frames fed to the vocoder; False when the decoder has nothing to decode."""
        if not self.decoder.busy:
            return False
        if self._segments is None:
            self._segments = self.decoder._segments(True, False)
        batch = next(self._segments, None)
        if batch is None:  # (the loop had ended before these texts were admitted: a new one)
            self._segments = self.decoder._segments(True, False)
            batch = next(self._segments)
        for uid, t0, frames, done in batch:
            self.vocoder.feed(self.tickets[uid], frames, last=done)
        return True

    def close(self):
        self.vocoder.close()

    def run(self):
        """Runs everything submitted (texts submitted while it runs included); yields (id, samples int32 [80 k], done)."""
        import time
        from .sampleRNN.generation.inputs import config
        start, heard, prefix = time.perf_counter(), set(), config().BIG_FRAME_SIZE
        self.first_audio_s = None
        while self._pending or self.decoder.busy or not self.vocoder.idle():
            self._admit()
            while self.vocoder.short_of_segment() and self._decode_segment():
                pass
            chunks = self.vocoder.step()
            if not chunks and self.vocoder.starved is not None:
                raise RuntimeError("the vocoder starves with nothing left to decode: " + self.vocoder.starved)
            for ticket, chunk, done in chunks:
                uid = self._uid[ticket]
                if self.first_audio_s is None and chunk.size and (uid in heard or chunk.size > prefix):
                    self.first_audio_s = time.perf_counter() - start
                heard.add(uid)
                if done:
                    del self._uid[ticket]
                yield uid, chunk, done

"""Secondary measurements (BASELINE configs[2] decode latency, the same loop with LSTM decoders -- persistent machine
with bf16 operands (decode_dtype='bf16') against the f32 machine against the per-step launches, alternating child
processes --, GRU decoders with bf16 operands (PARROT_PM_GRU_BF16=1) against the f32 machine from 2 x 1024 to 3 x 1536, alternating in one
process; the LSTM and GRU shapes with a GMM head (k_gmm = 20) on the machine (PARROT_PM_GMM=1) against the launches, the configs[2] decode that stops at the end of the utterance against the one that runs all its steps,
configs[4] SampleRNN sample loop, mu-law quantiser bandwidth).  Development / documentation aid; the driver's headline bench is bench.py.

  bench_extra.py                         everything, one JSON line
  bench_extra.py --only NAME[,NAME]      a subset (decode_cfg3, decode_stop, decode_lstm2_1024, decode_lstm3_1536,
                                         decode_gmm_gru2_1024, decode_gmm_lstm2_1024, decode_bf16_gru2_1024,
                                         decode_bf16_gru3_1024, decode_bf16_gru2_1536, decode_bf16_gru3_1536,
                                         samplernn_cfg5, samplernn_groups, samplernn_packed, samplernn_stream,
                                         samplernn_utt_draws, samplernn_draw_scan, samplernn_top_k, samplernn_top_p,
                                         samplernn_min_p, samplernn_forced, samplernn_skip, mulaw)
  bench_extra.py --only samplernn_groups [--reps N] [--groups-json FILE]
                                         SampleRNN at D = 1024 and B = 32 (anchor), 64, 128, 200: the persistent sample
                                         kernel in row groups (PARROT_SR_PERSIST_GROUPS=8) against the launch path, N
                                         alternations in one process; us per sample step, x real time per stream; the
                                         result also goes to FILE (default profiles/samplernn_groups.json)
  bench_extra.py --only samplernn_packed [--reps N] [--packed-json FILE]
                                         SampleRNN at D = 1024, 64 utterances of unequal length (fixed seed) on 32 streams:
                                         two rectangles of 32 at their own max(length) against ONE packed run
                                         (three_tier.pack_utterances, SampleRnnGenDesc::starts), and a packed plan whose
                                         starts are all zero against the plain plan (the cost of the extra launch per
                                         period); N alternations in one process; the result also goes to FILE (default
                                         profiles/samplernn_packed.json)
  bench_extra.py --only samplernn_stream [--reps N] [--stream-json FILE]
                                         SampleRNN at D = 1024 and B = 32, 201 frames: the run in one piece against
                                         three_tier.generate_stream in segments of 8 and of 40 frames (a plan of S + 1 slots
                                         used as a ring), N alternations in one process; every figure includes the host's
                                         copy of the samples and the synchronisation per segment; total time, us per sample
                                         step, the difference to the run in one piece per segment boundary, the time to the
                                         first chunk; the result also goes to FILE (default profiles/samplernn_stream.json)
  bench_extra.py --only samplernn_utt_draws [--reps N] [--utt-draws-json FILE]
                                         SampleRNN at D = 1024 and B = 32, 2000 samples per stream at temperature 1: the
                                         plan's key against per-utterance entries (DeviceGenerator(utterance_draws=True),
                                         with the seeds that reproduce the plan's key: bit identity is checked), and
                                         temperature 0 beside them; then the 64 utterances of samplernn_packed on one packed
                                         plan with temperatures 0 / 0.5 / 1 / 2 mixed inside every team against the same
                                         packing at temperature 0 and at 1 with the plan's key; N alternations in one
                                         process; the result also goes to FILE (default profiles/samplernn_utt_draws.json)
  bench_extra.py --only samplernn_draw_scan [--reps N] [--draw-scan-json FILE] [--parent-lib FILE]
                                         SampleRNN at D = 1024 and B = 32, 8000 samples per stream: argmax, the sequential
                                         draw at temperature 1 and the wave-parallel draw (draw_mode='scan') at temperature 1,
                                         N alternations in one process, each with its spread (max - min); the same three with
                                         per-utterance draws on; the two draws on the launch path at B = 33 and in two row
                                         groups (B = 64, PARROT_SR_PERSIST_GROUPS=8); with --parent-lib (the parent commit's
                                         libparrot_hip.so) the default path of both libraries at temperature 0 and 1 in the
                                         same alternation, bit identity included; the two bars of the mode are evaluated;
                                         the result also goes to FILE (default profiles/samplernn_draw_scan.json)
  bench_extra.py --only samplernn_top_k [--reps N] [--top-k-json FILE] [--parent-lib FILE]
                                         SampleRNN at D = 1024 and B = 32, 8000 samples per stream at temperature 1: the
                                         sequential and the wave-parallel draw, each among all codes (top_k = 0) and among
                                         the 64 most likely (DeviceGenerator(top_k=64)), with the plan's value and with
                                         per-utterance entries (generate(..., top_ks=)), argmax beside them; N alternations
                                         in one process, each with its spread; the cost of the selection per mode and the
                                         bar "scan at k = 64 stays faster than sequential at k = 0"; with --parent-lib (the
                                         parent commit's libparrot_hip.so) the default path of both libraries at temperature
                                         0 and 1 in the same alternation, bit identity included; the result also goes to
                                         FILE (default profiles/samplernn_top_k.json)
  bench_extra.py --only samplernn_top_p [--reps N] [--top-p-json FILE] [--parent-lib FILE]
                                         SampleRNN at D = 1024 and B = 32, 8000 samples per stream at temperature 1: the
                                         sequential and the wave-parallel draw, each among all codes, among the nucleus of
                                         top_p = 0.9 (DeviceGenerator(top_p=0.9)) and among the nucleus of the 64 most likely
                                         (top_k=64, top_p=0.9), with the plan's value and with per-utterance entries
                                         (generate(..., top_ps=)), argmax beside them; N alternations in one process, each
                                         with its spread; the cost of the selection per mode; with --parent-lib (the parent
                                         commit's libparrot_hip.so) the default path of both libraries at temperature 0 and 1
                                         in the same alternation, bit identity included, and the bar "scan at p = 0.9 stays
                                         faster than the parent's untruncated sequential draw"; the result also goes to FILE
                                         (default profiles/samplernn_top_p.json)
  bench_extra.py --only samplernn_min_p [--reps N] [--min-p-json FILE] [--parent-lib FILE]
                                         SampleRNN at D = 1024 and B = 32, 8000 samples per stream: argmax; at temperature 1
                                         the sequential and the wave-parallel draw, each among all codes, with min_p = 0.1
                                         (DeviceGenerator(min_p=0.1)) from the plan's value and from per-utterance entries
                                         (generate(..., min_ps=)), with top_k = 64 and with top_p = 0.9; a draw_stats=True plan
                                         beside a forcing=True, log_probs=True plan; N alternations in one process, each with
                                         its spread; the cost of each selection per mode and the bar "a min_p draw costs less
                                         than a top_k = 64 draw in the same mode"; with --parent-lib (the parent commit's
                                         libparrot_hip.so) the default path of both libraries at temperature 0 and 1 in the
                                         same alternation, bit identity included; the result also goes to FILE (default
                                         profiles/samplernn_min_p.json)
  bench_extra.py --only samplernn_forced [--reps N] [--forced-json FILE] [--parent-lib FILE]
                                         SampleRNN at D = 1024 and B = 32, 8000 samples per stream: the default plan at
                                         temperature 0 and 1, a forcing plan with every code -1, a forcing plan with every
                                         sample forced (DeviceGenerator(forcing=True)) and a plan with log_probs=True, the
                                         three at both temperatures; N alternations in one process, each with its spread; what
                                         forcing and the log-probability cost per sample step (no bar of their own); with
                                         --parent-lib (the parent commit's libparrot_hip.so) the default plan of both
                                         libraries at temperature 0 and 1 in the same alternation, bit identity included;
                                         the result also goes to FILE (default profiles/samplernn_forced.json)
  bench_extra.py --only samplernn_skip [--reps N] [--skip-json FILE] [--parent-lib FILE]
                                         SampleRNN at D = 1024 and B = 32 with PARROT_SR_SKIP_STACKS=1: a (GRU, 2) model with
                                         skip connections on the device loop (8000 samples per stream) against the literal
                                         three-function loop on the same model (160 samples per stream), the same plan against
                                         a (GRU, 2) plan without skip connections, and the default single-GRU plan at
                                         temperature 0 and 1; N alternations in one process, each with its spread; with
                                         --parent-lib (the parent commit's libparrot_hip.so) the default plan of both
                                         libraries in the same alternation, bit identity included; the result also goes to
                                         FILE (default profiles/samplernn_skip.json)
  bench_extra.py --only decode_row_controls [--reps N] [--row-controls-json FILE] [--parent-lib FILE]
                                         decode with per-utterance controls (Parrot.sample_model_device(timing_coeffs=, ..)):
                                         configs[2] and the 2 x LSTM-1024 plan at batch 16, 1000 frames -- the default call and
                                         the call with all controls given, N alternations in one process, each with its spread;
                                         with --parent-lib (the parent commit's libparrot_hip.so) the default call of both
                                         libraries in the same alternation, bit identity included; the result also goes to FILE
                                         (default profiles/decode_row_controls.json)
  bench_extra.py --only decode_forced [--reps N] [--forced-decode-json FILE] [--parent-lib FILE]
                                         decode with forced frames (Parrot.sample_model_device(forced_frames=, n_forced=)):
                                         configs[2] and the 2 x LSTM-1024 plan at batch 16, 1000 frames -- the default plan, the
                                         forced plan with n = 0 everywhere, the forced plan with 200 forced frames of 1000 and
                                         (GRU) the default plan under PARROT_PM_FBC=0, N alternations in one process, each with
                                         its spread; with --parent-lib (the parent commit's libparrot_hip.so) the default plan
                                         of both libraries in the same alternation, bit identity included; the result also goes
                                         to FILE (default profiles/decode_forced.json)
  bench_extra.py --only decode_segments [--reps N] [--segments-json FILE] [--parent-lib FILE]
                                         resumable decode (Parrot.decode_segments, sample_model_device(return_state=True)):
                                         configs[2] and the 2 x LSTM-1024 plan at batch 16, 1000 frames -- the plain call, the
                                         one-piece carry call, segments of 50 and of 10 frames, N >= 3 alternations in one
                                         process, each with its spread: total time, host time to the first segment, cost per
                                         boundary; with --parent-lib (the parent commit's libparrot_hip.so) the plain call of
                                         both libraries in the same alternation, bit identity included; the result also goes
                                         to FILE (default profiles/decode_segments.json)
  bench_extra.py --only text_to_audio [--text-to-audio-json FILE]
                                         text to audio in one stream (parrot_amd.decode.TextToAudio): configs[2] decoder, DIM
                                         1024 vocoder, 16 texts of 20 .. 100 characters (the end-of-utterance rule sets their
                                         frames, at most 1000), 16 decoder slots and 16 vocoder streams, vocoder segments of 8,
                                         decoder segments of 10 and of 50 -- time to first audio and total time against the
                                         staged path (StreamingDecoder.run() to the end, then StreamingGenerator.submit of whole
                                         utterances), the three alternating in one process, three runs each, with spreads; and
                                         the per-step cost of samplernn_generate_stage_features against the host-array upload
                                         it replaces; the result also goes to FILE (default profiles/text_to_audio.json)
  bench_extra.py --kappa-bias B          decode_stop: fork_kappa.b of the randomly initialised model (default -1.0: how fast
                                         the window walks over the text, i.e. after how many steps the utterance ends)
  bench_extra.py --dump-sample FILE      decode_cfg3 also saves sample_x (numpy) -- bit-identity checks between builds
  bench_extra.py --reps N                on / off alternations of the LSTM and GMM decode entries (default 3)
  bench_extra.py --gmm_head [--reps N]   this leg alone: the GMM head's cost and gradient, fused HIP kernels against the torch
                                         path (head alone at M = 51 200, O = 63, K = 20 and the configs[1] training step with
                                         that head; N >= 5 alternations, bytes moved, TB/s, peak memory)"""
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch


def _arg(name, dflt=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else dflt


ALL = ("decode_cfg3", "decode_stop", "decode_lstm2_1024", "decode_lstm3_1536", "decode_gmm_gru2_1024", "decode_gmm_lstm2_1024",
       "decode_bf16_gru2_1024", "decode_bf16_gru3_1024", "decode_bf16_gru2_1536", "decode_bf16_gru3_1536", "samplernn_cfg5", "samplernn_groups",
       "samplernn_packed", "samplernn_stream", "samplernn_utt_draws", "samplernn_draw_scan", "samplernn_top_k", "samplernn_top_p", "samplernn_min_p", "samplernn_forced", "samplernn_skip",
       "decode_row_controls", "decode_forced", "decode_segments", "text_to_audio", "mulaw")
only =tuple(_arg("--only", ",".join(ALL)).split(","))
assert all(n in ALL for n in only), only
LSTM_SHAPES = {  # configs[2]'s shape with LSTM cells; the 3 x LSTM-1536 model of BASELINE configs[3]
    "decode_lstm2_1024": dict(num_layers=2, rnn_h_dim=1024, readouts_dim=1024),
    "decode_lstm3_1536": dict(num_layers=3, rnn_h_dim=1536, readouts_dim=1536),
}
GRU_BF16_SHAPES = {  # configs[2] (2 x GRU-1024), a 3 x GRU-1536 stack whose f32 layer matrices no longer fit in LDS, and two
    # shapes between them (where bf16 operands start to pay)
    "decode_bf16_gru2_1024": dict(num_layers=2, rnn_h_dim=1024, readouts_dim=1024),
    "decode_bf16_gru3_1024": dict(num_layers=3, rnn_h_dim=1024, readouts_dim=1024),
    "decode_bf16_gru2_1536": dict(num_layers=2, rnn_h_dim=1536, readouts_dim=1536),
    "decode_bf16_gru3_1536": dict(num_layers=3, rnn_h_dim=1536, readouts_dim=1536),
}
GMM_SHAPES = {  # the decode_cfg3 / decode_lstm2_1024 shapes with the mixture-density head (which_cost='GMM', k_gmm=20)
    "decode_gmm_gru2_1024": dict(num_layers=2, rnn_h_dim=1024, readouts_dim=1024, cell_type='gru', which_cost='GMM', k_gmm=20),
    "decode_gmm_lstm2_1024": dict(num_layers=2, rnn_h_dim=1024, readouts_dim=1024, cell_type='lstm', which_cost='GMM', k_gmm=20),
}
dev = torch.device("cuda:0")
out = {}
g = torch.Generator().manual_seed(0)


def decode(kw, dump=None, decode_dtype='float32'):
    """Autoregressive decode, batch 16, 1000 frames, MSE head (greedy; a GMM head: fixed unif / noise), hipGraph: three
    runs, the last one reported."""
    from parrot_amd import _lib
    from parrot_amd.model import Parrot
    m = Parrot(device=dev, encoder_type='bidirectional', weak_feedback=True, use_graph=True, decode_dtype=decode_dtype,
               **kw).initialize()
    g = torch.Generator().manual_seed(0)
    N, U, S = 16, 100, 1000
    lab = torch.randint(0, 43, (N, U), generator=g)
    lm = torch.ones(N, U)
    rnd = {}
    if kw.get('which_cost') == 'GMM':
        rnd = dict(unif=torch.rand(S, N, generator=g).to(dev), noise=torch.randn(S, N, 63, generator=g).to(dev))
    for rep in range(3):
        torch.cuda.synchronize(); t0 = time.time()
        outs = m.sample_model_device(lab, lm, None, N, S, **rnd)
        torch.cuda.synchronize(); dt = time.time() - t0
    if dump:
        np.save(dump, outs[0].cpu().numpy())
    ws = m._sample_ws[(S, N, U)]
    res = {"batch": N, "frames": S, "seconds": round(dt, 4), "us_per_step": round(1e6 * dt / S, 2),
           "frames_per_s": round(N * S / dt, 1), "machine": int(_lib.load().parrot_sample_is_persistent(ws['plan'])),
           "bf16": int(_lib.load().parrot_sample_is_bf16(ws['plan']))}
    m.close()
    return res


def decode_stop(kappa_bias, reps):
    """configs[2] decode shape, max_steps 2048: the plain plan (all steps), the stopping plan with a predicate that never
    fires (all steps: what the stop costs per step) and the stopping plan with the rule of the text (leaves early),
    alternating in one process; whole-call wall times, every call listed."""
    from parrot_amd import _lib
    from parrot_amd.model import Parrot
    m = Parrot(device=dev, encoder_type='bidirectional', weak_feedback=True, use_graph=True, num_layers=2, rnn_h_dim=1024,
               readouts_dim=1024).initialize()
    m._p('/h1_to_att/fork_kappa.b').fill_(kappa_bias)
    g = torch.Generator().manual_seed(0)
    N, U, S, extra = 16, 100, 2048, 40
    lab = torch.randint(0, 43, (N, U), generator=g)
    lm = torch.ones(N, U)
    for i in range(N):  # texts of 100, 97, .. 55 characters
        lm[i, U - 3 * i:] = 0

    def timed(fn):
        torch.cuda.synchronize(); t0 = time.time()
        r = fn()
        torch.cuda.synchronize()
        return time.time() - t0, r

    def never():  # the stopping plan on the same inputs, its rows compare position 0 with itself: never true
        ws = m._sample_workspace(S, N, U, stop_extra=extra)
        ws['eou_pos'].zero_(); ws['eou_ncmp'].fill_(U - 1)
        return m._sample_device(ws, lab, lm, None, N, S, None, None, None)

    t = {"plain": [], "never": [], "stopped": []}
    for rep in range(reps + 1):  # (the first round builds the plans and captures the graphs: not listed)
        runs = (("plain", lambda: m.sample_model_device(lab, lm, None, N, S)), ("never", never),
                ("stopped", lambda: m.sample_until_end_device(lab, lm, None, N, S, extra=extra)))
        for key, fn in runs:
            dt, r = timed(fn)
            if rep:
                t[key].append(dt)
            if key == "plain":
                full = r
            if key == "never":
                same_never = all(torch.equal(a, b) for a, b in zip(r, full))
            if key == "stopped":
                outs, lengths = r
    steps = int(lengths.max())
    ws = m._sample_ws[('stop', S, N, U, extra)]
    us = lambda v: [round(1e6 * x / S, 2) for x in v]
    res = {"batch": N, "max_steps": S, "extra": extra, "kappa_bias": kappa_bias,
           "machine": int(_lib.load().parrot_sample_is_persistent(ws['plan'])),
           "lengths": lengths.tolist(), "steps_run": steps,
           "prefix_bit_identical": all(torch.equal(a, b[:steps]) for a, b in zip(outs, full)),
           "never_firing_bit_identical": same_never,
           "seconds_unstopped": [round(x, 4) for x in t["plain"]], "seconds_stopped": [round(x, 4) for x in t["stopped"]],
           "us_per_step_plain": us(t["plain"]), "us_per_step_stop_plan_never_firing": us(t["never"]),
           "us_per_step_stopped": [round(1e6 * x / steps, 2) for x in t["stopped"]]}
    m.close()
    return res


def decode_gru_bf16(kw, reps, whole_too):
    """GRU decode with bf16 operands (PARROT_PM_GRU_BF16=1, decode_dtype='bf16') against the f32 machine of the same model,
    batch 16, 1000 frames, alternating within one process; whole_too: also the bf16 whole-K phases (PARROT_PM_PIECES=0) beside
    the bf16 step cut along K.  The switches are read when a model's plan is built (its first call), so every model makes its
    first call under its own environment and keeps that plan.  Whole-call wall times around a device synchronise, every call
    listed; the first round (plans, graph capture) is not."""
    from parrot_amd import _lib
    from parrot_amd.model import Parrot
    g = torch.Generator().manual_seed(0)
    N, U, S = 16, 100, 1000
    lab = torch.randint(0, 43, (N, U), generator=g)
    lm = torch.ones(N, U)
    legs = [("bf16", "bf16", {}), ("f32", "float32", {})] + ([("bf16_whole_k", "bf16", {"PARROT_PM_PIECES": "0"})] if whole_too else [])
    saved = {k: os.environ.get(k) for k in ("PARROT_PM_GRU_BF16", "PARROT_PM_PIECES")}
    os.environ["PARROT_PM_GRU_BF16"] = "1"
    models, t, info = {}, {}, {}
    try:
        for key, dtype, env in legs:
            os.environ.update(env)
            m = models[key] = Parrot(device=dev, encoder_type='bidirectional', weak_feedback=True, use_graph=True, cell_type='gru',
                                     decode_dtype=dtype, **kw).initialize()
            m.sample_model_device(lab, lm, None, N, S)
            torch.cuda.synchronize()
            for k in env:
                os.environ.pop(k)
            ws = m._sample_ws[(S, N, U)]
            lib = _lib.load()
            info[key] = {"machine": int(lib.parrot_sample_is_persistent(ws['plan'])), "bf16": int(lib.parrot_sample_is_bf16(ws['plan']))}
            assert info[key]["machine"] != 0 and (info[key]["bf16"] != 0) == (dtype == "bf16"), (key, info[key])
            t[key] = []
        for rep in range(reps):
            for key, _, _ in legs:
                torch.cuda.synchronize(); t0 = time.time()
                models[key].sample_model_device(lab, lm, None, N, S)
                torch.cuda.synchronize()
                t[key].append(round(1e6 * (time.time() - t0) / S, 2))
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        for m in models.values():
            m.close()
    res = {"batch": N, "frames": S, "plans": info, "us_per_step": t,
           "spread_us": {k: round(max(v) - min(v), 2) for k, v in t.items()},
           "bf16_faster": max(t["bf16"]) < min(t["f32"]), "f32_faster": max(t["f32"]) < min(t["bf16"])}
    if whole_too:
        res["bf16_pieces_faster_than_whole_k"] = max(t["bf16"]) < min(t["bf16_whole_k"])
    return res


def gmm_head(reps):
    """The mixture-density head (which_cost='GMM', k_gmm=20) at the benchmark shape, the fused HIP kernels
    (PARROT_GMM_COST_FUSED=1) against the torch element-wise path (=0), alternating in one process: the head alone
    (forward + backward, device events) at M = 51 200, O = 63, K = 20, and the full training step of BASELINE configs[1]
    with that head.  Every repetition is listed; the spread is max - min of a path's repetitions."""
    from parrot_amd import ops
    from parrot_amd.model import Parrot, cost_gmm
    from parrot_amd.trainer import Trainer
    T, B, U, O, K, eps = 800, 64, 200, 63, 20, 1e-5
    M = T * B
    gen = torch.Generator().manual_seed(0)
    y, mu, co = (torch.randn(M, w, generator=gen).to(dev) for w in (O, O * K, K))
    sh = (0.5 * torch.randn(M, O * K, generator=gen)).to(dev)
    mask = torch.ones(M, device=dev)
    gscale = torch.ones((), device=dev)
    bufs = tuple(torch.empty(M, w, device=dev) for w in (O * K, O * K, K))

    def head_fused():
        nll, pi, logr = ops.gmm_cost_fwd(y, mu, sh, co, eps)
        msum = mask.sum() + 1e-5
        cost = (nll * mask).sum() / msum
        return cost, ops.gmm_cost_bwd(y, mu, sh, co, logr, (mask / msum * gscale).contiguous(), eps, out=bufs)

    def head_torch():  # Parrot.compute_cost's torch path and the copies of _readouts_factored_bwd
        leafs = [t.detach().requires_grad_(True) for t in (mu, sh, co)]
        with torch.enable_grad():
            cost = (cost_gmm(y, leafs[0], torch.exp(leafs[1]) + eps, torch.softmax(leafs[2], -1) + eps) * mask).sum() \
                / (mask.sum() + 1e-5)
        return cost, [d * gscale for d in torch.autograd.grad(cost, leafs)]

    def event_ms(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            r = fn()
        e1.record()
        torch.cuda.synchronize()
        del r
        return e0.elapsed_time(e1) / n

    res = {"shape": {"M": M, "O": O, "K": K}, "reps": reps}
    head = {"fused": [], "torch": []}
    peak = {}
    for key, fn in (("fused", head_fused), ("torch", head_torch)):  # warm, and the peak memory of one pass on its own
        fn(); torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn(); torch.cuda.synchronize()
        peak[key] = torch.cuda.max_memory_allocated() - base
    for rep in range(reps):
        for key, fn in (("fused", head_fused), ("torch", head_torch)):
            head[key].append(round(event_ms(fn, 5), 4))
    # the bytes the kernels must move: both [M, O*K] pre-activation arrays, y and co_hat once per direction, the two big
    # gradients once
    fwd_b = 4 * (2 * M * O * K + M * O + M * K)
    bwd_b = fwd_b + 4 * 2 * M * O * K
    e0 = lambda f: event_ms(f, 10)
    logr = ops.gmm_cost_fwd(y, mu, sh, co, eps)[2]
    rs = torch.ones(M, device=dev)
    fwd_all = [e0(lambda: ops.gmm_cost_fwd(y, mu, sh, co, eps)) for _ in range(3)]  # three means of 10 launches each;
    bwd_all = [e0(lambda: ops.gmm_cost_bwd(y, mu, sh, co, logr, rs, eps, out=bufs)) for _ in range(3)]
    t_fwd, t_bwd = min(fwd_all), min(bwd_all)  # the TB/s figures are of the best of the three
    tbs = lambda b, ms: round(b / (ms * 1e-3) * 1e-12, 3)
    res["head_ms"] = head
    res["head_spread_ms"] = {k: round(max(v) - min(v), 4) for k, v in head.items()}
    res["head_extra_bytes_peak"] = peak
    res["kernels"] = {"fwd_bytes": fwd_b, "bwd_bytes": bwd_b, "fwd_ms_all": [round(t, 4) for t in fwd_all], "bwd_ms_all": [round(t, 4) for t in bwd_all],
                      "fwd_ms": round(t_fwd, 4), "bwd_ms": round(t_bwd, 4), "TBps_of": "best of the three",
                      "fwd_TBps": tbs(fwd_b, t_fwd), "bwd_TBps": tbs(bwd_b, t_bwd),
                      "fwd_of_8TBps_peak": round(tbs(fwd_b, t_fwd) / 8.0, 3), "bwd_of_8TBps_peak": round(tbs(bwd_b, t_bwd) / 8.0, 3),
                      "fwd_of_6.3TBps_achievable": round(tbs(fwd_b, t_fwd) / 6.3, 3),
                      "bwd_of_6.3TBps_achievable": round(tbs(bwd_b, t_bwd) / 6.3, 3)}
    del y, mu, sh, co, bufs, logr
    torch.cuda.empty_cache()

    # the full training step (forward, backward, clip + Adam) of BASELINE configs[1] with the GMM head
    m = Parrot(device=dev, use_graph=True, seed=1234, num_layers=2, rnn_h_dim=1024, readouts_dim=1024,
               encoder_type='bidirectional', which_cost='GMM', k_gmm=K).initialize()
    with torch.no_grad():
        m.get_parameter_dict()['/parrot/h1_to_att/fork_kappa.b'].fill_(-1.5)
    tr = Trainer(m)
    feat = torch.randn(T + 1, B, O, generator=gen).to(dev)
    batch = (feat, torch.ones(T + 1, B, device=dev), torch.randint(0, 43, (B, U), generator=gen).to(dev),
             torch.ones(B, U, device=dev))
    step = {"fused": [], "torch": []}
    speak = {"fused": 0, "torch": 0}
    for rep in range(reps + 1):  # (the first round allocates the workspace and captures the graphs: not listed)
        for key, val in (("fused", "1"), ("torch", "0")):
            os.environ['PARROT_GMM_COST_FUSED'] = val
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            ms = event_ms(lambda: tr.step(*batch, None, 1), 3)
            assert m.gmm_cost_path == key, (m.gmm_cost_path, key)
            if rep:
                step[key].append(round(ms, 3))
                speak[key] = max(speak[key], torch.cuda.max_memory_allocated())
    os.environ.pop('PARROT_GMM_COST_FUSED', None)
    res["step_ms"] = step
    res["step_spread_ms"] = {k: round(max(v) - min(v), 3) for k, v in step.items()}
    res["step_max_memory_allocated"] = speak
    res["fused_faster_head"] = max(head["fused"]) < min(head["torch"])
    res["fused_faster_step"] = max(step["fused"]) < min(step["torch"])
    m.close()
    return res


def samplernn_d1024():
    """The three_tier module with the BASELINE configs[4] model in it: parameters deleted, D = 1024, and one dummy
    compute_cost that registers all parameters with the reference initialisation."""
    from parrot_amd.sampleRNN import lib
    from parrot_amd.sampleRNN.models.conditional import three_tier as tt
    lib.delete_all_params(); lib.set_device(dev)
    tt.configure(DIM=1024, EMB_SIZE=256)
    seq = torch.randint(0, 256, (2, 160 + 80), generator=g).to(dev)
    with torch.no_grad():
        tt.compute_cost(seq, torch.randn(2, 2, 63, device=dev), torch.zeros(2, 1, 1024, device=dev),
                        torch.zeros(2, 1, 1024, device=dev), 1, torch.ones(2, 240, device=dev))
    return tt


def alternate(gens, args, kw, reps):
    """Every plan's generate(*args[k], **kw.get(k, {})) reps + 1 times in turn, each round starting one plan further on (no
    plan always runs behind the same other one); the first round captures the graphs and is not counted.  Returns (call to
    device idle in seconds per plan and counted round, every plan's last samples)."""
    times, samples = {k: [] for k in gens}, {}
    keys = list(gens)
    for rep in range(reps + 1):
        for k in keys[rep % len(keys):] + keys[:rep % len(keys)]:
            torch.cuda.synchronize(); t0 = time.time()
            s = gens[k].generate(*args[k], **kw.get(k, {}))
            torch.cuda.synchronize(); dt = time.time() - t0
            samples[k] = s.cpu().numpy().copy()
            if rep:
                times[k].append(dt)
    return times, samples


def record(name, flag, res):
    """A SampleRNN section's result: into the JSON line, and into the file `flag` names (default profiles/<name>.json)."""
    out[name] = res
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(_arg(flag, os.path.join(root, "profiles", name + ".json")), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if "--gmm_head" in sys.argv:  # this leg alone, one JSON line
    print(json.dumps({"gmm_head": gmm_head(max(5, int(_arg("--reps", "5"))))}))
    sys.exit(0)

if "--child-gmm" in sys.argv:  # one GMM-head decode measurement under the caller's environment
    print(json.dumps(decode(GMM_SHAPES[_arg("--child-gmm")])))
    sys.exit(0)

if "--child" in sys.argv:  # one LSTM decode measurement under the caller's environment
    print(json.dumps(decode(dict(LSTM_SHAPES[_arg("--child")], cell_type='lstm'),
                            decode_dtype=_arg("--decode-dtype", "float32"))))
    sys.exit(0)

# ---- configs[2]: GRU decoder
if "decode_cfg3" in only:
    out["decode_cfg3"] = decode(dict(num_layers=2, rnn_h_dim=1024, readouts_dim=1024), _arg("--dump-sample"))

# ---- configs[2] again: stop at the end of the utterance inside the machine
if "decode_stop" in only:
    out["decode_stop"] = decode_stop(float(_arg("--kappa-bias", "-1.0")), int(_arg("--reps", "3")))

# ---- LSTM decoders: the persistent machine with bf16 operands and with f32 operands (PARROT_SAMPLE_PERSIST=1, the default)
# against the per-step launches (PARROT_SAMPLE_PERSIST=0), each run in a child process of its own, alternating so the
# spread is visible.  The bf16 machine's yardstick is the f32 machine of the SAME call.
for name in LSTM_SHAPES:
    if name not in only:
        continue
    runs = {"machine_bf16": [], "machine": [], "launches": []}
    for rep in range(int(_arg("--reps", "3"))):
        for key, val, dt_ in (("machine_bf16", "1", "bf16"), ("machine", "1", "float32"), ("launches", "0", "float32")):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--decode-dtype", dt_],
                               capture_output=True, text=True, env=dict(os.environ, PARROT_SAMPLE_PERSIST=val), timeout=600)
            if r.returncode != 0:  # (a fault in a child ends the measurement: nothing more is started on the device)
                sys.stderr.write(r.stdout + r.stderr)
                sys.exit(r.returncode)
            res = json.loads(r.stdout.strip().splitlines()[-1])
            assert (res["machine"] != 0) == (key != "launches") and (res["bf16"] != 0) == (key == "machine_bf16"), (key, res)
            runs[key].append(res["us_per_step"])
    out[name] = {"batch": 16, "frames": 1000, "us_per_step_machine_bf16": runs["machine_bf16"],
                 "us_per_step_machine": runs["machine"], "us_per_step_launches": runs["launches"],
                 "machine_faster": max(runs["machine"]) < min(runs["launches"]),
                 "bf16_faster": max(runs["machine_bf16"]) < min(runs["machine"])}

# ---- GMM head: the machine (PARROT_PM_GMM=1) against the per-step launches (the switch unset) of the same call, each run in a
# child process of its own, alternating; the yardstick is the launch path, every repetition is listed
for name in GMM_SHAPES:
    if name not in only:
        continue
    runs = {"machine": [], "launches": []}
    env_off = {k: v for k, v in os.environ.items() if k != "PARROT_PM_GMM"}
    for rep in range(int(_arg("--reps", "3"))):
        for key, env in (("machine", dict(env_off, PARROT_PM_GMM="1")), ("launches", env_off)):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-gmm", name], capture_output=True, text=True,
                               env=env, timeout=600)
            if r.returncode != 0:  # (a fault in a child ends the measurement: nothing more is started on the device)
                sys.stderr.write(r.stdout + r.stderr)
                sys.exit(r.returncode)
            res = json.loads(r.stdout.strip().splitlines()[-1])
            assert (res["machine"] != 0) == (key == "machine"), (key, res)
            runs[key].append(res["us_per_step"])
    out[name] = {"batch": 16, "frames": 1000, "k_gmm": 20, "us_per_step_machine": runs["machine"],
                 "us_per_step_launches": runs["launches"],
                 "spread_us": {k: round(max(v) - min(v), 2) for k, v in runs.items()},
                 "machine_faster": max(runs["machine"]) < min(runs["launches"])}

# ---- GRU decoders with bf16 operands (PARROT_PM_GRU_BF16=1) against the f32 machine, alternating in one process; at the
# configs[2] shape also the bf16 whole-K phases against the bf16 step cut along K
for name in GRU_BF16_SHAPES:
    if name in only:
        out[name] = decode_gru_bf16(GRU_BF16_SHAPES[name], int(_arg("--reps", "3")), whole_too=name == "decode_bf16_gru2_1024")

# ---- configs[4]: SampleRNN 3-tier GRU D=1024, batch 32, greedy, 16 kHz mu-law
if "samplernn_cfg5" in only:
    tt = samplernn_d1024()
    B, T = 32, 26  # 25 generated big frames = 2000 samples per stream
    gen = tt.DeviceGenerator(B, T, temperature=0.0)
    feats = torch.randn(T, B, 63, generator=g).numpy()
    for rep in range(2):
        torch.cuda.synchronize(); t0 = time.time()
        s = gen.generate(feats)
        torch.cuda.synchronize(); dt = time.time() - t0
    nsamp = (T - 1) * 80
    out["samplernn_cfg5"] = {"batch": B, "samples_per_stream": nsamp, "seconds": round(dt, 4),
                             "us_per_sample_step": round(1e6 * dt / nsamp, 2),
                             "samples_per_s": round(B * nsamp / dt, 1),
                             "x_realtime_per_stream": round(nsamp / dt / 16000.0, 3)}
    gen.close()

# ---- SampleRNN D=1024 above 32 streams: the persistent sample kernel in row groups (PARROT_SR_PERSIST_GROUPS) against the
# launch path, plans of both kinds alive in one process and run alternately; B = 32 is the anchor (one group: the same
# kernel instantiation with the switch set and unset)
if "samplernn_groups" in only:
    tt = samplernn_d1024()
    T, reps = 26, int(_arg("--reps", "5"))
    nsamp = (T - 1) * 80
    saved = {k: os.environ.get(k) for k in ("PARROT_SR_PERSIST", "PARROT_SR_PERSIST_GROUPS")}

    def plan(B, persist, groups):
        os.environ["PARROT_SR_PERSIST"] = str(persist)
        if groups is None:
            os.environ.pop("PARROT_SR_PERSIST_GROUPS", None)
        else:
            os.environ["PARROT_SR_PERSIST_GROUPS"] = str(groups)
        return tt.DeviceGenerator(B, T, temperature=0.0)

    res = {"dim": 1024, "samples_per_stream": nsamp, "alternations": reps, "batches": {}}
    for B in (32, 64, 128, 200):
        feats = torch.randn(T, B, 63, generator=g).numpy()
        gens = {"groups": plan(B, 1, 8), "launches": plan(B, 0, None)}
        if B == 32:
            gens["switch_unset"] = plan(B, 1, None)
        assert gens["groups"].persist_groups == -(-B // 32) and not gens["launches"].persistent
        times, samples = alternate(gens, {k: (feats,) for k in gens}, {}, reps)
        entry = {"row_groups": gens["groups"].persist_groups,
                 "rows_equal_to_launches": int((samples["groups"] == samples["launches"]).all(axis=1).sum())}
        for k, v in times.items():
            us = sorted(1e6 * dt / nsamp for dt in v)
            entry[k] = {"us_per_sample_step": round(us[len(us) // 2], 2), "spread_us": round(us[-1] - us[0], 2),
                        "x_realtime_per_stream": round(nsamp / sorted(v)[len(v) // 2] / 16000.0, 3)}
        entry["groups_faster"] = max(times["groups"]) < min(times["launches"])
        if B == 32:
            entry["bit_identical_to_switch_unset"] = bool((samples["groups"] == samples["switch_unset"]).all())
        res["batches"][str(B)] = entry
        for gen in gens.values():
            gen.close()
    for k, v in saved.items():
        os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    record("samplernn_groups", "--groups-json", res)

# ---- SampleRNN D=1024, 64 utterances of unequal length on 32 streams: (a) two rectangles of 32 in arrival order, each at
# its own max(length); (b) one packed run (longest first onto the least-loaded stream, utterance starts inside the loop);
# (c) the first rectangle on a packed plan whose starts are all zero against the plain plan of (a) -- what the extra launch
# per period costs.  All plans alive in one process and run alternately.
if "samplernn_packed" in only:
    tt = samplernn_d1024()
    B, N, LEN_SEED, reps = 32, 64, 1234, int(_arg("--reps", "5"))
    rs = np.random.RandomState(LEN_SEED)
    lengths = [int(n) for n in rs.randint(20, 201, size=N)]  # big frames of 5 ms: 0.1 .. 1 s of audio
    utts = [rs.randn(n, 63).astype(np.float32) for n in lengths]
    rect = []
    for k in range(N // B):
        Tk = max(lengths[k * B:(k + 1) * B])
        f = np.zeros((Tk, B, 63), dtype=np.float32)
        for b in range(B):
            f[:lengths[k * B + b], b] = utts[k * B + b]
        rect.append(f)
    stream, first, Tp = tt.pack_utterances(lengths, B)
    pf, ps = tt.build_packed_inputs(utts, stream, first, Tp, B)
    gens = {"rect0": tt.DeviceGenerator(B, rect[0].shape[0], temperature=0.0),
            "rect1": tt.DeviceGenerator(B, rect[1].shape[0], temperature=0.0),
            "packed": tt.DeviceGenerator(B, Tp, temperature=0.0, packed=True),
            "rect0_on_packed_plan": tt.DeviceGenerator(B, rect[0].shape[0], temperature=0.0, packed=True)}
    args = {"rect0": (rect[0],), "rect1": (rect[1],), "packed": (pf, ps),
            "rect0_on_packed_plan": (rect[0], np.zeros((rect[0].shape[0], B), dtype=np.int32))}
    assert all(gen.persistent for gen in gens.values())
    times, samples = alternate(gens, args, {}, reps)
    for gen in gens.values():
        gen.close()
    pieces = tt.unpack_samples(samples["packed"], lengths, stream, first)
    same = sum(int(np.array_equal(pieces[i], samples["rect%d" % (i // B)][i % B, :80 * lengths[i]])) for i in range(N))
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    periods = {k: gens[k].T - 1 for k in gens}
    res = {"dim": 1024, "streams": B, "utterances": N, "length_seed": LEN_SEED, "lengths": lengths, "alternations": reps,
           "periods": {"rectangles": periods["rect0"] + periods["rect1"], "packed": periods["packed"],
                       "ratio": round((periods["rect0"] + periods["rect1"]) / periods["packed"], 3)},
           "ms": {k: {"median": round(1e3 * med[k], 2), "spread": round(1e3 * (max(v) - min(v)), 2),
                      "us_per_period": round(1e6 * med[k] / periods[k], 2)} for k, v in times.items()},
           "ms_rectangles": round(1e3 * (med["rect0"] + med["rect1"]), 2),
           "ms_packed": round(1e3 * med["packed"], 2),
           "measured_ratio": round((med["rect0"] + med["rect1"]) / med["packed"], 3),
           "start_launch_us_per_period": round(1e6 * (med["rect0_on_packed_plan"] - med["rect0"]) / periods["rect0"], 2),
           "utterances_equal_to_rectangles": same,
           "zero_starts_bit_identical": bool((samples["rect0_on_packed_plan"] == samples["rect0"]).all())}
    record("samplernn_packed", "--packed-json", res)

# ---- SampleRNN D=1024, B=32, 201 frames: the run in one piece against the same run in segments of 8 and of 40 frames on a
# plan of S + 1 slots used as a ring (three_tier.generate_stream, samplernn_generate_run_segment).  All plans alive in one
# process and run alternately; every time includes the samples' way to the host (one copy for the run in one piece, one
# per segment -- behind samplernn_generate_status, which synchronises -- for the segmented runs).
if "samplernn_stream" in only:
    tt = samplernn_d1024()
    B, N, SEGS, reps = 32, 201, (8, 40), int(_arg("--reps", "5"))
    feats = torch.randn(N, B, 63, generator=g).numpy()
    gens = {"one_shot": tt.DeviceGenerator(B, N, temperature=0.0)}
    for S_ in SEGS:
        gens["segments_%d" % S_] = tt.DeviceGenerator(B, S_ + 1, temperature=0.0)
    assert all(gen.persistent for gen in gens.values())

    def run(k):
        torch.cuda.synchronize(); t0 = time.time()
        if k == "one_shot":
            s = gens[k].generate(feats).cpu().numpy().copy()
            return time.time() - t0, time.time() - t0, s
        chunks, first = [], None
        for c in tt.generate_stream(feats, gens[k].T - 1, gen=gens[k]):
            chunks.append(c)
            if first is None:
                first = time.time() - t0
        return time.time() - t0, first, np.concatenate(chunks, axis=1)

    times, firsts, samples = {k: [] for k in gens}, {k: [] for k in gens}, {}
    keys = list(gens)
    for rep in range(reps + 1):  # (the first alternation captures the graphs: not counted)
        for k in keys[rep % len(keys):] + keys[:rep % len(keys)]:  # (no plan always runs behind the same other one)
            dt, first, samples[k] = run(k)
            if rep:
                times[k].append(dt); firsts[k].append(first)
    for gen in gens.values():
        gen.close()
    nsamp = (N - 1) * 80
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    res = {"dim": 1024, "streams": B, "frames": N, "samples_per_stream": nsamp, "alternations": reps,
           "timed": "call to last sample on the host (device synchronisation and host copy per chunk included)", "runs": {}}
    for k in keys:
        S_ = gens[k].T - 1
        bounds = -(-(N - 1) // S_) - 1
        e = {"segment_frames": S_, "segments": bounds + 1, "ms": round(1e3 * med[k], 2),
             "spread_ms": round(1e3 * (max(times[k]) - min(times[k])), 2),
             "us_per_sample_step": round(1e6 * med[k] / nsamp, 3),
             "ms_to_first_chunk": round(1e3 * sorted(firsts[k])[len(firsts[k]) // 2], 2),
             "plan_sample_buffer_bytes": B * 80 * gens[k].T * 4}
        if k != "one_shot":
            e["us_per_boundary_over_one_shot"] = round(1e6 * (med[k] - med["one_shot"]) / bounds, 2)
            e["bit_identical_to_one_shot"] = bool(np.array_equal(samples[k], samples["one_shot"]))
        res["runs"][k] = e
    record("samplernn_stream", "--stream-json", res)

# ---- SampleRNN D=1024, B=32: per-utterance seeds and temperatures (samplernn_generate_set_utterance_draws) against the plan's
# key at temperature 1 -- the same draws, bit for bit, with seeds[b] = seed ^ K2 (b + 1) --, and a packed run whose teams mix
# arg-max rows with draws at 0.5 / 1 / 2.  All plans alive in one process and run alternately.
if "samplernn_utt_draws" in only:
    tt = samplernn_d1024()
    B, T, SEED, reps = 32, 26, 234, int(_arg("--reps", "3"))
    nsamp = (T - 1) * 80
    feats = torch.randn(T, B, 63, generator=g).numpy()
    key_seeds = [(SEED ^ (tt.DRAW_K2 * (b + 1))) & (2 ** 64 - 1) for b in range(B)]
    N, LEN_SEED = 64, 1234  # the utterances of samplernn_packed
    rs = np.random.RandomState(LEN_SEED)
    lengths = [int(n) for n in rs.randint(20, 201, size=N)]
    utts = [rs.randn(n, 63).astype(np.float32) for n in lengths]
    stream, first, Tp = tt.pack_utterances(lengths, B)
    pf, ps = tt.build_packed_inputs(utts, stream, first, Tp, B)
    # utterance i draws at MIX[stream % 4]: the four rows of every team of the persistent kernel differ
    MIX = (0.0, 0.5, 1.0, 2.0)
    mixed = [MIX[stream[i] % 4] for i in range(N)]
    useed, utemp = tt.build_packed_draws([tt.utterance_seed(SEED, i) for i in range(N)], mixed, stream, first, Tp, B)
    gens = {"plan_key_t1": tt.DeviceGenerator(B, T, temperature=1.0, seed=SEED),
            "utterance_draws_t1": tt.DeviceGenerator(B, T, utterance_draws=True),
            "plan_key_t0": tt.DeviceGenerator(B, T, temperature=0.0),
            "packed_t0": tt.DeviceGenerator(B, Tp, temperature=0.0, packed=True),
            "packed_plan_key_t1": tt.DeviceGenerator(B, Tp, temperature=1.0, seed=SEED, packed=True),
            "packed_mixed_temperatures": tt.DeviceGenerator(B, Tp, packed=True, utterance_draws=True)}
    args = {k: (pf, ps) if k.startswith("packed") else (feats,) for k in gens}
    kw = {"utterance_draws_t1": dict(seeds=key_seeds, temperatures=1.0),
          "packed_mixed_temperatures": dict(seeds=useed, temperatures=utemp)}
    assert all(gen.persistent for gen in gens.values())
    times, samples = alternate(gens, args, kw, reps)
    steps = {k: (gens[k].T - 1) * 80 for k in gens}
    for gen in gens.values():
        gen.close()
    pieces = {k: tt.unpack_samples(samples[k], lengths, stream, first) for k in ("packed_t0", "packed_mixed_temperatures")}
    argmax_rows = [i for i in range(N) if mixed[i] == 0.0]
    res = {"dim": 1024, "streams": B, "alternations": reps, "timed": "call to device idle (host-side input copies included)",
           "runs": {k: {"sample_steps": steps[k], "ms": [round(1e3 * dt, 2) for dt in v],
                        "us_per_sample_step": [round(1e6 * dt / steps[k], 3) for dt in v],
                        "us_per_sample_step_median": round(1e6 * sorted(v)[len(v) // 2] / steps[k], 3)}
                    for k, v in times.items()},
           "utterance_draws_bit_identical_to_plan_key": bool(np.array_equal(samples["utterance_draws_t1"], samples["plan_key_t1"])),
           "packed": {"utterances": N, "length_seed": LEN_SEED, "periods": Tp - 1, "temperatures_by_stream_mod_4": list(MIX),
                      "argmax_utterances": len(argmax_rows),
                      "argmax_utterances_equal_to_packed_t0": sum(int(np.array_equal(pieces["packed_mixed_temperatures"][i],
                                                                                     pieces["packed_t0"][i])) for i in argmax_rows)}}
    record("samplernn_utt_draws", "--utt-draws-json", res)

# ---- SampleRNN D=1024, B=32: the wave-parallel seeded draw (SampleRnnGenDesc::draw_mode = 1, DeviceGenerator(draw_mode='scan'))
# against the sequential draw and argmax; the same with per-utterance draws; the launch path at B = 33; two row groups at
# B = 64; and, with --parent-lib, the default path against the parent commit's library.  All plans alive in one process and
# run alternately.
if "samplernn_draw_scan" in only:
    import contextlib
    import ctypes
    from parrot_amd import _lib as plib
    tt = samplernn_d1024()
    T, SEED, reps = 101, 234, int(_arg("--reps", "5"))
    nsamp = (T - 1) * 80
    feats = {B: torch.randn(T, B, 63, generator=g).numpy() for B in (32, 33, 64)}
    key_seeds = [(SEED ^ (tt.DRAW_K2 * (b + 1))) & (2 ** 64 - 1) for b in range(32)]
    this_lib = plib.load()
    parent_path = _arg("--parent-lib")
    parent_lib = None
    if parent_path:
        parent_lib = ctypes.CDLL(os.path.abspath(parent_path))
        for name, (res_, args_) in plib.SIGNATURES.items():
            fn = getattr(parent_lib, name)
            fn.restype = res_
            fn.argtypes = args_

    @contextlib.contextmanager
    def under(which):  # every call of a plan goes to the library that made it
        plib._lib = which
        try:
            yield
        finally:
            plib._lib = this_lib

    saved = {k: os.environ.get(k) for k in ("PARROT_SR_PERSIST", "PARROT_SR_PERSIST_GROUPS")}

    def plan(B, groups=None, which=this_lib, **kw):
        if groups is None:
            os.environ.pop("PARROT_SR_PERSIST_GROUPS", None)
        else:
            os.environ["PARROT_SR_PERSIST_GROUPS"] = str(groups)
        with under(which):
            return tt.DeviceGenerator(B, T, seed=SEED, **kw)

    draws = dict(seeds=key_seeds, temperatures=1.0)
    # name: (plan, its library, generate's keywords)
    plans = {"argmax": (plan(32, temperature=0.0), this_lib, {}),
             "sequential_t1": (plan(32, temperature=1.0), this_lib, {}),
             "scan_t1": (plan(32, temperature=1.0, draw_mode='scan'), this_lib, {}),
             "utt_argmax": (plan(32, utterance_draws=True), this_lib, dict(seeds=key_seeds, temperatures=0.0)),
             "utt_sequential_t1": (plan(32, utterance_draws=True), this_lib, draws),
             "utt_scan_t1": (plan(32, utterance_draws=True, draw_mode='scan'), this_lib, draws),
             "launch_B33_sequential_t1": (plan(33, temperature=1.0), this_lib, {}),
             "launch_B33_scan_t1": (plan(33, temperature=1.0, draw_mode='scan'), this_lib, {}),
             "groups2_B64_sequential_t1": (plan(64, groups=8, temperature=1.0), this_lib, {}),
             "groups2_B64_scan_t1": (plan(64, groups=8, temperature=1.0, draw_mode='scan'), this_lib, {})}
    if parent_lib is not None:
        plans["parent_argmax"] = (plan(32, which=parent_lib, temperature=0.0), parent_lib, {})
        plans["parent_sequential_t1"] = (plan(32, which=parent_lib, temperature=1.0), parent_lib, {})
        # a second plan of each kind, created in the other order: what differs between two plans of ONE library (where their
        # buffers landed) is the floor under any difference between the libraries
        plans["argmax_again"] = (plan(32, temperature=0.0), this_lib, {})
        plans["sequential_t1_again"] = (plan(32, temperature=1.0), this_lib, {})
        plans["parent_sequential_t1_again"] = (plan(32, which=parent_lib, temperature=1.0), parent_lib, {})
        plans["parent_argmax_again"] = (plan(32, which=parent_lib, temperature=0.0), parent_lib, {})
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    for k, (gen, _, _) in plans.items():
        want = 0 if k.startswith("launch") else 2 if k.startswith("groups2") else 1
        assert gen.persist_groups == want, (k, gen.persist_groups)
    times, samples = {k: [] for k in plans}, {}
    keys = list(plans)
    for rep_ in range(reps + 1):  # (the first alternation captures the graphs: not counted)
        for k in keys[rep_ % len(keys):] + keys[:rep_ % len(keys)]:  # (no plan always runs behind the same other one)
            gen, which, kw = plans[k]
            with under(which):
                torch.cuda.synchronize(); t0 = time.time()
                s = gen.generate(feats[gen.B], **kw)
                torch.cuda.synchronize(); dt = time.time() - t0
                samples[k] = s.cpu().numpy().copy()
            if rep_:
                times[k].append(dt)
    for gen, which, _ in plans.values():
        with under(which):
            gen.close()
    us = {k: [1e6 * dt / nsamp for dt in v] for k, v in times.items()}
    med = {k: sorted(v)[len(v) // 2] for k, v in us.items()}
    spread = {k: max(v) - min(v) for k, v in us.items()}

    def faster(a, b):  # a faster than b by more than the sum of the two spreads
        return bool(med[b] - med[a] > spread[a] + spread[b])

    differ = int((samples["scan_t1"] != samples["sequential_t1"]).sum())
    res = {"dim": 1024, "alternations": reps, "samples_per_stream": nsamp,
           "timed": "call to device idle (host-side input copies included)",
           "runs": {k: {"streams": plans[k][0].B, "us_per_sample_step": [round(x, 3) for x in us[k]],
                        "us_per_sample_step_median": round(med[k], 3), "spread_max_minus_min": round(spread[k], 3)}
                    for k in plans},
           "scan_samples_that_differ_from_sequential": {"differ": differ, "of": int(samples["scan_t1"].size - 32 * 80)},
           "utt_scan_bit_identical_to_scan": bool(np.array_equal(samples["utt_scan_t1"], samples["scan_t1"])),
           "utt_sequential_bit_identical_to_sequential": bool(np.array_equal(samples["utt_sequential_t1"], samples["sequential_t1"])),
           "bar_scan_faster_than_sequential_by_more_than_both_spreads": {
               "persistent_B32": faster("scan_t1", "sequential_t1"),
               "persistent_B32_utterance_draws": faster("utt_scan_t1", "utt_sequential_t1"),
               "launch_B33": faster("launch_B33_scan_t1", "launch_B33_sequential_t1"),
               "groups2_B64": faster("groups2_B64_scan_t1", "groups2_B64_sequential_t1")},
           "not_measured": ["eight row groups", "the streaming generator's end-to-end time", "D = 256 and D = 512"]}
    if parent_lib is not None:
        def pair(t):  # medians of the two plans of each library, the gap between the libraries and inside each
            a, b = (med[t], med[t + "_again"]), (med["parent_" + t], med["parent_" + t + "_again"])
            four = sorted(spread[k] for k in (t, t + "_again", "parent_" + t, "parent_" + t + "_again"))
            inside = max(abs(a[0] - a[1]), abs(b[0] - b[1]), (four[1] + four[2]) / 2)  # (the median: one outlier is no spread)
            gap = sum(a) / 2 - sum(b) / 2
            return {"this_us": [round(x, 3) for x in a], "parent_us": [round(x, 3) for x in b],
                    "this_minus_parent_us": round(gap, 3), "largest_difference_inside_one_library_us": round(inside, 3),
                    "bar_default_within_its_spread_of_parent": bool(abs(gap) <= inside)}
        res["default_path_against_parent_commit"] = {
            "how": "this build and the parent commit's library loaded in one process, two plans of each per temperature (the "
                   "second pair created in the other order), all in the same alternation; the spread of the default path is "
                   "the larger of the four plans' median max - min and the difference between two plans of one library",
            "bit_identical_t0": bool(np.array_equal(samples["argmax"], samples["parent_argmax"])),
            "bit_identical_t1": bool(np.array_equal(samples["sequential_t1"], samples["parent_sequential_t1"])),
            "t0": pair("argmax"), "t1": pair("sequential_t1")}
    record("samplernn_draw_scan", "--draw-scan-json", res)

# ---- SampleRNN D=1024, B=32: top-k truncated draws (SampleRnnGenDesc::top_k, DeviceGenerator(top_k=)) at temperature 1 in both
# draw modes, k = 0 against k = 64, with the plan's value and with per-utterance entries; and, with --parent-lib, the default
# path (k = 0) against the parent commit's library.  All plans alive in one process and run alternately, as samplernn_draw_scan.
if "samplernn_top_k" in only:
    import contextlib
    import ctypes
    from parrot_amd import _lib as plib
    tt = samplernn_d1024()
    T, SEED, K, reps = 101, 234, 64, int(_arg("--reps", "5"))
    nsamp = (T - 1) * 80
    feats = torch.randn(T, 32, 63, generator=g).numpy()
    key_seeds = [(SEED ^ (tt.DRAW_K2 * (b + 1))) & (2 ** 64 - 1) for b in range(32)]
    this_lib = plib.load()
    parent_path = _arg("--parent-lib")
    parent_lib = None
    if parent_path:
        parent_lib = ctypes.CDLL(os.path.abspath(parent_path))
        for name, (res_, args_) in plib.SIGNATURES.items():
            if hasattr(parent_lib, name):  # (the parent has no samplernn_generate_set_utterance_top_k: its plans never call it)
                fn = getattr(parent_lib, name)
                fn.restype = res_
                fn.argtypes = args_

    @contextlib.contextmanager
    def under(which):  # every call of a plan goes to the library that made it
        plib._lib = which
        try:
            yield
        finally:
            plib._lib = this_lib

    def plan(which=this_lib, **kw):
        with under(which):
            return tt.DeviceGenerator(32, T, seed=SEED, **kw)

    draws = dict(seeds=key_seeds, temperatures=1.0)
    # name: (plan, its library, generate's keywords)
    plans = {"argmax": (plan(temperature=0.0), this_lib, {})}
    for mode in ("sequential", "scan"):
        plans[mode + "_t1"] = (plan(temperature=1.0, draw_mode=mode), this_lib, {})
        plans[mode + "_t1_k64"] = (plan(temperature=1.0, draw_mode=mode, top_k=K), this_lib, {})
        plans["utt_" + mode + "_t1"] = (plan(utterance_draws=True, draw_mode=mode), this_lib, draws)
        plans["utt_" + mode + "_t1_k64"] = (plan(utterance_draws=True, draw_mode=mode), this_lib, dict(draws, top_ks=[K] * 32))
    if parent_lib is not None:
        plans["parent_argmax"] = (plan(which=parent_lib, temperature=0.0), parent_lib, {})
        plans["parent_sequential_t1"] = (plan(which=parent_lib, temperature=1.0), parent_lib, {})
        # (a second plan of each kind, created in the other order: the floor under any difference between the libraries)
        plans["argmax_again"] = (plan(temperature=0.0), this_lib, {})
        plans["sequential_t1_again"] = (plan(temperature=1.0), this_lib, {})
        plans["parent_sequential_t1_again"] = (plan(which=parent_lib, temperature=1.0), parent_lib, {})
        plans["parent_argmax_again"] = (plan(which=parent_lib, temperature=0.0), parent_lib, {})
    assert all(gen.persist_groups == 1 for gen, _, _ in plans.values())
    times, samples = {k: [] for k in plans}, {}
    keys = list(plans)
    for rep_ in range(reps + 1):  # (the first alternation captures the graphs: not counted)
        for k in keys[rep_ % len(keys):] + keys[:rep_ % len(keys)]:  # (no plan always runs behind the same other one)
            gen, which, kw = plans[k]
            with under(which):
                torch.cuda.synchronize(); t0 = time.time()
                s = gen.generate(feats, **kw)
                torch.cuda.synchronize(); dt = time.time() - t0
                samples[k] = s.cpu().numpy().copy()
            if rep_:
                times[k].append(dt)
    for gen, which, _ in plans.values():
        with under(which):
            gen.close()
    us = {k: [1e6 * dt / nsamp for dt in v] for k, v in times.items()}
    med = {k: sorted(v)[len(v) // 2] for k, v in us.items()}
    spread = {k: max(v) - min(v) for k, v in us.items()}
    res = {"dim": 1024, "streams": 32, "top_k": K, "alternations": reps, "samples_per_stream": nsamp,
           "timed": "call to device idle (host-side input copies included)",
           "runs": {k: {"us_per_sample_step": [round(x, 3) for x in us[k]], "us_per_sample_step_median": round(med[k], 3),
                        "spread_max_minus_min": round(spread[k], 3)} for k in plans},
           "cost_of_truncation_us_per_sample_step": {
               m: round(med[m + "_t1_k64"] - med[m + "_t1"], 3)
               for m in ("sequential", "scan", "utt_sequential", "utt_scan")},
           "truncated_samples_that_differ_from_untruncated": {
               m: int((samples[m + "_t1_k64"] != samples[m + "_t1"]).sum()) for m in ("sequential", "scan")},
           "utt_k64_bit_identical_to_plan_k64": {
               m: bool(np.array_equal(samples["utt_" + m + "_t1_k64"], samples[m + "_t1_k64"])) for m in ("sequential", "scan")},
           "bar_scan_k64_faster_than_sequential_k0": {
               "scan_k64_us": round(med["scan_t1_k64"], 3), "sequential_k0_us": round(med["sequential_t1"], 3),
               "holds": bool(med["scan_t1_k64"] < med["sequential_t1"]),
               "by_more_than_both_spreads": bool(med["sequential_t1"] - med["scan_t1_k64"] >
                                                 spread["sequential_t1"] + spread["scan_t1_k64"])},
           "not_measured": ["row groups (two and eight)", "the launch path's timing", "the streaming generator end to end",
                            "D = 256 and D = 512", "k other than 64"]}
    if parent_lib is not None:
        def pair(t):  # medians of the two plans of each library, the gap between the libraries and inside each
            a, b = (med[t], med[t + "_again"]), (med["parent_" + t], med["parent_" + t + "_again"])
            four = sorted(spread[k] for k in (t, t + "_again", "parent_" + t, "parent_" + t + "_again"))
            inside = max(abs(a[0] - a[1]), abs(b[0] - b[1]), (four[1] + four[2]) / 2)  # (the median: one outlier is no spread)
            gap = sum(a) / 2 - sum(b) / 2
            return {"this_us": [round(x, 3) for x in a], "parent_us": [round(x, 3) for x in b],
                    "this_minus_parent_us": round(gap, 3), "largest_difference_inside_one_library_us": round(inside, 3),
                    "bar_default_within_its_spread_of_parent": bool(abs(gap) <= inside)}
        res["default_path_against_parent_commit"] = {
            "how": "this build and the parent commit's library loaded in one process, two plans of each per temperature (the "
                   "second pair created in the other order), all in the same alternation; the spread of the default path is "
                   "the larger of the four plans' median max - min and the difference between two plans of one library",
            "bit_identical_t0": bool(np.array_equal(samples["argmax"], samples["parent_argmax"])),
            "bit_identical_t1": bool(np.array_equal(samples["sequential_t1"], samples["parent_sequential_t1"])),
            "t0": pair("argmax"), "t1": pair("sequential_t1")}
    record("samplernn_top_k", "--top-k-json", res)

# ---- SampleRNN D=1024, B=32: top-p (nucleus) draws (samplernn_generate_set_top_p, DeviceGenerator(top_p=)) at temperature 1 in
# both draw modes -- untruncated, p = 0.9, and p = 0.9 behind k = 64 --, with the plan's value and with per-utterance entries; and,
# with --parent-lib, the default path (p = 0) and the scan draw at p = 0.9 against the parent commit's library.  All plans alive
# in one process and run alternately, as samplernn_top_k.
if "samplernn_top_p" in only:
    import contextlib
    import ctypes
    from parrot_amd import _lib as plib
    tt = samplernn_d1024()
    T, SEED, K, P, reps = 101, 234, 64, 0.9, int(_arg("--reps", "5"))
    nsamp = (T - 1) * 80
    feats = torch.randn(T, 32, 63, generator=g).numpy()
    key_seeds = [(SEED ^ (tt.DRAW_K2 * (b + 1))) & (2 ** 64 - 1) for b in range(32)]
    this_lib = plib.load()
    parent_path = _arg("--parent-lib")
    parent_lib = None
    if parent_path:
        parent_lib = ctypes.CDLL(os.path.abspath(parent_path))
        for name, (res_, args_) in plib.SIGNATURES.items():
            if hasattr(parent_lib, name):  # (the parent has neither top_p setter: its plans never call them)
                fn = getattr(parent_lib, name)
                fn.restype = res_
                fn.argtypes = args_

    @contextlib.contextmanager
    def under(which):  # every call of a plan goes to the library that made it
        plib._lib = which
        try:
            yield
        finally:
            plib._lib = this_lib

    def plan(which=this_lib, **kw):
        with under(which):
            return tt.DeviceGenerator(32, T, seed=SEED, **kw)

    draws = dict(seeds=key_seeds, temperatures=1.0)
    # name: (plan, its library, generate's keywords)
    plans = {"argmax": (plan(temperature=0.0), this_lib, {})}
    for mode in ("sequential", "scan"):
        plans[mode + "_t1"] = (plan(temperature=1.0, draw_mode=mode), this_lib, {})
        plans[mode + "_t1_p90"] = (plan(temperature=1.0, draw_mode=mode, top_p=P), this_lib, {})
        plans[mode + "_t1_k64_p90"] = (plan(temperature=1.0, draw_mode=mode, top_k=K, top_p=P), this_lib, {})
        plans["utt_" + mode + "_t1"] = (plan(utterance_draws=True, draw_mode=mode), this_lib, draws)
        plans["utt_" + mode + "_t1_p90"] = (plan(utterance_draws=True, draw_mode=mode), this_lib, dict(draws, top_ps=[P] * 32))
        plans["utt_" + mode + "_t1_k64_p90"] = (plan(utterance_draws=True, draw_mode=mode), this_lib,
                                                dict(draws, top_ks=[K] * 32, top_ps=[P] * 32))
    if parent_lib is not None:
        plans["parent_argmax"] = (plan(which=parent_lib, temperature=0.0), parent_lib, {})
        plans["parent_sequential_t1"] = (plan(which=parent_lib, temperature=1.0), parent_lib, {})
        # (a second plan of each kind, created in the other order: the floor under any difference between the libraries)
        plans["argmax_again"] = (plan(temperature=0.0), this_lib, {})
        plans["sequential_t1_again"] = (plan(temperature=1.0), this_lib, {})
        plans["parent_sequential_t1_again"] = (plan(which=parent_lib, temperature=1.0), parent_lib, {})
        plans["parent_argmax_again"] = (plan(which=parent_lib, temperature=0.0), parent_lib, {})
    assert all(gen.persist_groups == 1 for gen, _, _ in plans.values())
    times, samples = {k: [] for k in plans}, {}
    keys = list(plans)
    for rep_ in range(reps + 1):  # (the first alternation captures the graphs: not counted)
        for k in keys[rep_ % len(keys):] + keys[:rep_ % len(keys)]:  # (no plan always runs behind the same other one)
            gen, which, kw = plans[k]
            with under(which):
                torch.cuda.synchronize(); t0 = time.time()
                s = gen.generate(feats, **kw)
                torch.cuda.synchronize(); dt = time.time() - t0
                samples[k] = s.cpu().numpy().copy()
            if rep_:
                times[k].append(dt)
    for gen, which, _ in plans.values():
        with under(which):
            gen.close()
    us = {k: [1e6 * dt / nsamp for dt in v] for k, v in times.items()}
    med = {k: sorted(v)[len(v) // 2] for k, v in us.items()}
    spread = {k: max(v) - min(v) for k, v in us.items()}
    modes4 = ("sequential", "scan", "utt_sequential", "utt_scan")
    res = {"dim": 1024, "streams": 32, "top_p": P, "top_k": K, "alternations": reps, "samples_per_stream": nsamp,
           "timed": "call to device idle (host-side input copies included)",
           "runs": {k: {"us_per_sample_step": [round(x, 3) for x in us[k]], "us_per_sample_step_median": round(med[k], 3),
                        "spread_max_minus_min": round(spread[k], 3)} for k in plans},
           "cost_of_nucleus_us_per_sample_step": {m: round(med[m + "_t1_p90"] - med[m + "_t1"], 3) for m in modes4},
           "cost_of_top_k_and_nucleus_us_per_sample_step": {m: round(med[m + "_t1_k64_p90"] - med[m + "_t1"], 3) for m in modes4},
           "nucleus_samples_that_differ_from_untruncated": {
               m: int((samples[m + "_t1_p90"] != samples[m + "_t1"]).sum()) for m in ("sequential", "scan")},
           "utt_bit_identical_to_plan": {
               m + v: bool(np.array_equal(samples["utt_" + m + v], samples[m + v]))
               for m in ("sequential", "scan") for v in ("_t1_p90", "_t1_k64_p90")},
           "scan_p90_against_this_builds_sequential_untruncated": {
               "scan_p90_us": round(med["scan_t1_p90"], 3), "sequential_p0_us": round(med["sequential_t1"], 3),
               "faster_by_more_than_both_spreads": bool(med["sequential_t1"] - med["scan_t1_p90"] >
                                                        spread["sequential_t1"] + spread["scan_t1_p90"])},
           "not_measured": ["row groups (two and eight)", "the launch path's timing", "the streaming generator end to end",
                            "D = 256 and D = 512", "p other than 0.9, k other than 64"]}
    if parent_lib is not None:
        def pair(t):  # the bar of the issue (the two first plans, the sum of their spreads) and the four plans' picture beside it
            a, b = (med[t], med[t + "_again"]), (med["parent_" + t], med["parent_" + t + "_again"])
            both = spread[t] + spread["parent_" + t]
            return {"this_us": [round(x, 3) for x in a], "parent_us": [round(x, 3) for x in b],
                    "this_minus_parent_us": round(a[0] - b[0], 3), "sum_of_the_two_spreads_us": round(both, 3),
                    "bar_default_within_the_sum_of_both_spreads": bool(abs(a[0] - b[0]) <= both),
                    "mean_of_two_plans_this_minus_parent_us": round(sum(a) / 2 - sum(b) / 2, 3),
                    "largest_difference_between_two_plans_of_one_library_us": round(max(abs(a[0] - a[1]), abs(b[0] - b[1])), 3)}
        res["default_path_against_parent_commit"] = {
            "how": "this build and the parent commit's library loaded in one process, two plans of each per temperature (the "
                   "second pair created in the other order), all in the same alternation; the bar compares the first plan of "
                   "each library against the sum of their spreads (max - min over the alternations)",
            "bit_identical_t0": bool(np.array_equal(samples["argmax"], samples["parent_argmax"])),
            "bit_identical_t1": bool(np.array_equal(samples["sequential_t1"], samples["parent_sequential_t1"])),
            "t0": pair("argmax"), "t1": pair("sequential_t1")}
        both = spread["scan_t1_p90"] + spread["parent_sequential_t1"]
        res["bar_scan_p90_faster_than_parents_sequential_untruncated"] = {
            "scan_p90_us": round(med["scan_t1_p90"], 3), "parent_sequential_p0_us": round(med["parent_sequential_t1"], 3),
            "sum_of_the_two_spreads_us": round(both, 3),
            "holds": bool(med["parent_sequential_t1"] - med["scan_t1_p90"] > both)}
    record("samplernn_top_p", "--top-p-json", res)

# ---- SampleRNN D=1024, B=32: min-p draws (samplernn_generate_set_min_p, DeviceGenerator(min_p=)) at temperature 1 in both draw
# modes -- untruncated, min_p = 0.1 with the plan's value and with per-utterance entries, and in the same run top_k = 64 and
# top_p = 0.9 --; a draw_stats=True plan against a forcing=True, log_probs=True plan; and, with --parent-lib, the default path
# against the parent commit's library.  All plans alive in one process and run alternately, as samplernn_top_p.
if "samplernn_min_p" in only:
    import contextlib
    import ctypes
    from parrot_amd import _lib as plib
    tt = samplernn_d1024()
    T, SEED, K, P, M, reps = 101, 234, 64, 0.9, 0.1, int(_arg("--reps", "5"))
    nsamp = (T - 1) * 80
    feats = torch.randn(T, 32, 63, generator=g).numpy()
    free = np.full((32, 80 * T), -1, dtype=np.int32)
    key_seeds = [(SEED ^ (tt.DRAW_K2 * (b + 1))) & (2 ** 64 - 1) for b in range(32)]
    this_lib = plib.load()
    parent_path = _arg("--parent-lib")
    parent_lib = None
    if parent_path:
        parent_lib = ctypes.CDLL(os.path.abspath(parent_path))
        for name, (res_, args_) in plib.SIGNATURES.items():
            if hasattr(parent_lib, name):  # (the parent has none of the new setters: its plans never call them)
                fn = getattr(parent_lib, name)
                fn.restype = res_
                fn.argtypes = args_

    @contextlib.contextmanager
    def under(which):  # every call of a plan goes to the library that made it
        plib._lib = which
        try:
            yield
        finally:
            plib._lib = this_lib

    def plan(which=this_lib, **kw):
        with under(which):
            return tt.DeviceGenerator(32, T, seed=SEED, **kw)

    draws = dict(seeds=key_seeds, temperatures=1.0)
    # name: (plan, its library, generate's keywords)
    plans = {"argmax": (plan(temperature=0.0), this_lib, {})}
    for mode in ("sequential", "scan"):
        plans[mode + "_t1"] = (plan(temperature=1.0, draw_mode=mode), this_lib, {})
        plans[mode + "_t1_m10"] = (plan(temperature=1.0, draw_mode=mode, min_p=M), this_lib, {})
        plans[mode + "_t1_k64"] = (plan(temperature=1.0, draw_mode=mode, top_k=K), this_lib, {})
        plans[mode + "_t1_p90"] = (plan(temperature=1.0, draw_mode=mode, top_p=P), this_lib, {})
        plans["utt_" + mode + "_t1"] = (plan(utterance_draws=True, draw_mode=mode), this_lib, draws)
        plans["utt_" + mode + "_t1_m10"] = (plan(utterance_draws=True, draw_mode=mode), this_lib, dict(draws, min_ps=[M] * 32))
        plans[mode + "_t1_m10_draw_stats"] = (plan(temperature=1.0, draw_mode=mode, min_p=M, draw_stats=True), this_lib, {})
        plans[mode + "_t1_m10_forcing_log_probs"] = (plan(temperature=1.0, draw_mode=mode, min_p=M, forcing=True, log_probs=True),
                                                     this_lib, dict(forced=free))
    if parent_lib is not None:
        plans["parent_argmax"] = (plan(which=parent_lib, temperature=0.0), parent_lib, {})
        plans["parent_sequential_t1"] = (plan(which=parent_lib, temperature=1.0), parent_lib, {})
        # (a second plan of each kind, created in the other order: the floor under any difference between the libraries)
        plans["argmax_again"] = (plan(temperature=0.0), this_lib, {})
        plans["sequential_t1_again"] = (plan(temperature=1.0), this_lib, {})
        plans["parent_sequential_t1_again"] = (plan(which=parent_lib, temperature=1.0), parent_lib, {})
        plans["parent_argmax_again"] = (plan(which=parent_lib, temperature=0.0), parent_lib, {})
    assert all(gen.persist_groups == 1 for gen, _, _ in plans.values())
    times, samples, extra = {k: [] for k in plans}, {}, {}
    keys = list(plans)
    for rep_ in range(reps + 1):  # (the first alternation captures the graphs: not counted)
        for k in keys[rep_ % len(keys):] + keys[:rep_ % len(keys)]:  # (no plan always runs behind the same other one)
            gen, which, kw = plans[k]
            with under(which):
                torch.cuda.synchronize(); t0 = time.time()
                s = gen.generate(feats, **kw)
                torch.cuda.synchronize(); dt = time.time() - t0
                if isinstance(s, tuple):
                    s, extra[k] = s[0], [x.cpu().numpy().copy() for x in s[1:]]
                samples[k] = s.cpu().numpy().copy()
            if rep_:
                times[k].append(dt)
    for gen, which, _ in plans.values():
        with under(which):
            gen.close()
    us = {k: [1e6 * dt / nsamp for dt in v] for k, v in times.items()}
    med = {k: sorted(v)[len(v) // 2] for k, v in us.items()}
    spread = {k: max(v) - min(v) for k, v in us.items()}
    two = ("sequential", "scan")

    def cheaper(mode, other):  # bar (i): against something measured in this same run
        a, b = mode + "_t1_m10", mode + "_t1_" + other
        return {"min_p_us": round(med[a], 3), other + "_us": round(med[b], 3), "min_p_minus_" + other + "_us": round(med[a] - med[b], 3),
                "sum_of_the_two_spreads_us": round(spread[a] + spread[b], 3), "min_p_costs_less": bool(med[a] < med[b])}

    res = {"dim": 1024, "streams": 32, "min_p": M, "top_k": K, "top_p": P, "alternations": reps, "samples_per_stream": nsamp,
           "timed": "call to device idle (host-side input copies included)",
           "runs": {k: {"us_per_sample_step": [round(x, 3) for x in us[k]], "us_per_sample_step_median": round(med[k], 3),
                        "spread_max_minus_min": round(spread[k], 3)} for k in plans},
           "cost_of_the_selection_us_per_sample_step": {
               "min_p": {m: round(med[m + "_t1_m10"] - med[m + "_t1"], 3) for m in two + ("utt_sequential", "utt_scan")},
               "top_k": {m: round(med[m + "_t1_k64"] - med[m + "_t1"], 3) for m in two},
               "top_p": {m: round(med[m + "_t1_p90"] - med[m + "_t1"], 3) for m in two}},
           "bar_i_min_p_costs_less_than_top_k": {m: cheaper(m, "k64") for m in two},
           "min_p_against_top_p": {m: cheaper(m, "p90") for m in two},
           "min_p_samples_that_differ_from_untruncated": {m: int((samples[m + "_t1_m10"] != samples[m + "_t1"]).sum()) for m in two},
           "utt_bit_identical_to_plan": {m: bool(np.array_equal(samples["utt_" + m + "_t1_m10"], samples[m + "_t1_m10"])) for m in two},
           "draw_stats_against_forcing_and_log_probs": {
               m: {"draw_stats_us": round(med[m + "_t1_m10_draw_stats"], 3),
                   "forcing_log_probs_us": round(med[m + "_t1_m10_forcing_log_probs"], 3),
                   "plain_min_p_us": round(med[m + "_t1_m10"], 3),
                   "samples_bit_identical_to_plain": bool(np.array_equal(samples[m + "_t1_m10_draw_stats"], samples[m + "_t1_m10"])),
                   "kept_min_median_max": [int(np.min(extra[m + "_t1_m10_draw_stats"][1][:, 80:])),
                                           int(np.median(extra[m + "_t1_m10_draw_stats"][1][:, 80:])),
                                           int(np.max(extra[m + "_t1_m10_draw_stats"][1][:, 80:]))]} for m in two},
           "not_measured": ["row groups (two and eight)", "the launch path's timing", "the streaming generator end to end",
                            "D = 256 and D = 512", "min_p other than 0.1, combinations of the three truncations"]}
    if parent_lib is not None:
        def pair(t):  # the bar of the issue (the two first plans, the sum of their spreads) and the four plans' picture beside it
            a, b = (med[t], med[t + "_again"]), (med["parent_" + t], med["parent_" + t + "_again"])
            both = spread[t] + spread["parent_" + t]
            return {"this_us": [round(x, 3) for x in a], "parent_us": [round(x, 3) for x in b],
                    "this_minus_parent_us": round(a[0] - b[0], 3), "sum_of_the_two_spreads_us": round(both, 3),
                    "bar_default_within_the_sum_of_both_spreads": bool(abs(a[0] - b[0]) <= both),
                    "mean_of_two_plans_this_minus_parent_us": round(sum(a) / 2 - sum(b) / 2, 3),
                    "largest_difference_between_two_plans_of_one_library_us": round(max(abs(a[0] - a[1]), abs(b[0] - b[1])), 3)}
        res["default_path_against_parent_commit"] = {
            "how": "this build and the parent commit's library loaded in one process, two plans of each per temperature (the "
                   "second pair created in the other order), all in the same alternation; the bar compares the first plan of "
                   "each library against the sum of their spreads (max - min over the alternations)",
            "bit_identical_t0": bool(np.array_equal(samples["argmax"], samples["parent_argmax"])),
            "bit_identical_t1": bool(np.array_equal(samples["sequential_t1"], samples["parent_sequential_t1"])),
            "t0": pair("argmax"), "t1": pair("sequential_t1")}
    record("samplernn_min_p", "--min-p-json", res)

# ---- SampleRNN D=1024, B=32: forced samples and per-sample log-probabilities (samplernn_generate_set_forced / _set_log_probs,
# DeviceGenerator(forcing=, log_probs=)) -- the default plan at temperature 0 and 1, a forcing plan with every code -1, a
# forcing plan with every sample forced, a plan with log_probs=True, the three at both temperatures --; and, with
# --parent-lib, the default plan against the parent commit's library.  All plans alive in one process and run alternately,
# as samplernn_top_p.  No mode has a bar of its own: the leg reports what forcing and the log-probability cost per step.
if "samplernn_forced" in only:
    import contextlib
    import ctypes
    from parrot_amd import _lib as plib
    tt = samplernn_d1024()
    T, SEED, reps = 101, 234, int(_arg("--reps", "5"))
    nsamp = (T - 1) * 80
    feats = torch.randn(T, 32, 63, generator=g).numpy()
    free = np.full((32, 80 * T), -1, dtype=np.int32)
    codes = np.random.RandomState(SEED).randint(0, 256, size=(32, 80 * T)).astype(np.int32)
    this_lib = plib.load()
    parent_path = _arg("--parent-lib")
    parent_lib = None
    if parent_path:
        parent_lib = ctypes.CDLL(os.path.abspath(parent_path))
        for name, (res_, args_) in plib.SIGNATURES.items():
            if hasattr(parent_lib, name):  # (the parent has neither new setter: its plans never call them)
                fn = getattr(parent_lib, name)
                fn.restype = res_
                fn.argtypes = args_

    @contextlib.contextmanager
    def under(which):  # every call of a plan goes to the library that made it
        plib._lib = which
        try:
            yield
        finally:
            plib._lib = this_lib

    def plan(which=this_lib, **kw):
        with under(which):
            return tt.DeviceGenerator(32, T, seed=SEED, **kw)

    # name: (plan, its library, generate's keywords)
    plans = {}
    for tag, temp in (("argmax", 0.0), ("sequential_t1", 1.0)):
        plans[tag] = (plan(temperature=temp), this_lib, {})
        plans[tag + "_forcing_all_free"] = (plan(temperature=temp, forcing=True), this_lib, dict(forced=free))
        plans[tag + "_forcing_all_forced"] = (plan(temperature=temp, forcing=True), this_lib, dict(forced=codes))
        plans[tag + "_log_probs"] = (plan(temperature=temp, log_probs=True), this_lib, {})
    if parent_lib is not None:
        plans["parent_argmax"] = (plan(which=parent_lib, temperature=0.0), parent_lib, {})
        plans["parent_sequential_t1"] = (plan(which=parent_lib, temperature=1.0), parent_lib, {})
        # (a second plan of each kind, created in the other order: the floor under any difference between the libraries)
        plans["argmax_again"] = (plan(temperature=0.0), this_lib, {})
        plans["sequential_t1_again"] = (plan(temperature=1.0), this_lib, {})
        plans["parent_sequential_t1_again"] = (plan(which=parent_lib, temperature=1.0), parent_lib, {})
        plans["parent_argmax_again"] = (plan(which=parent_lib, temperature=0.0), parent_lib, {})
    assert all(gen.persist_groups == 1 for gen, _, _ in plans.values())
    times, samples, logps = {k: [] for k in plans}, {}, {}
    keys = list(plans)
    for rep_ in range(reps + 1):  # (the first alternation captures the graphs: not counted)
        for k in keys[rep_ % len(keys):] + keys[:rep_ % len(keys)]:  # (no plan always runs behind the same other one)
            gen, which, kw = plans[k]
            with under(which):
                torch.cuda.synchronize(); t0 = time.time()
                s = gen.generate(feats, **kw)
                torch.cuda.synchronize(); dt = time.time() - t0
                if isinstance(s, tuple):
                    s, logps[k] = s[0], s[1].cpu().numpy().copy()
                samples[k] = s.cpu().numpy().copy()
            if rep_:
                times[k].append(dt)
    for gen, which, _ in plans.values():
        with under(which):
            gen.close()
    us = {k: [1e6 * dt / nsamp for dt in v] for k, v in times.items()}
    med = {k: sorted(v)[len(v) // 2] for k, v in us.items()}
    spread = {k: max(v) - min(v) for k, v in us.items()}
    base = ("argmax", "sequential_t1")
    res = {"dim": 1024, "streams": 32, "alternations": reps, "samples_per_stream": nsamp,
           "timed": "call to device idle (host-side input copies included: a forcing plan also copies its [32, 8080] codes)",
           "runs": {k: {"us_per_sample_step": [round(x, 3) for x in us[k]], "us_per_sample_step_median": round(med[k], 3),
                        "spread_max_minus_min": round(spread[k], 3)} for k in plans},
           "cost_us_per_sample_step": {t: {m: round(med[t + "_" + m] - med[t], 3)
                                           for m in ("forcing_all_free", "forcing_all_forced", "log_probs")} for t in base},
           "all_free_bit_identical_to_default": {t: bool(np.array_equal(samples[t + "_forcing_all_free"], samples[t])) for t in base},
           "log_probs_bit_identical_to_default": {t: bool(np.array_equal(samples[t + "_log_probs"], samples[t])) for t in base},
           "all_forced_returns_the_codes": {t: bool(np.array_equal(samples[t + "_forcing_all_forced"][:, 80:], codes[:, 80:])) for t in base},
           "mean_bits_per_sample_of_the_default_runs": {t: round(float(-logps[t + "_log_probs"][:, 80:].mean() * np.log2(np.e)), 4) for t in base},
           "not_measured": ["row groups", "the launch path's timing", "the streaming generator end to end",
                            "D = 256 and D = 512", "both facilities on one plan, the scan draw and truncated draws with either"]}
    if parent_lib is not None:
        def pair(t):  # the bar of the issue (the two first plans, the sum of their spreads) and the four plans' picture beside it
            a, b = (med[t], med[t + "_again"]), (med["parent_" + t], med["parent_" + t + "_again"])
            both = spread[t] + spread["parent_" + t]
            return {"this_us": [round(x, 3) for x in a], "parent_us": [round(x, 3) for x in b],
                    "this_minus_parent_us": round(a[0] - b[0], 3), "sum_of_the_two_spreads_us": round(both, 3),
                    "bar_default_within_the_sum_of_both_spreads": bool(abs(a[0] - b[0]) <= both),
                    "mean_of_two_plans_this_minus_parent_us": round(sum(a) / 2 - sum(b) / 2, 3),
                    "largest_difference_between_two_plans_of_one_library_us": round(max(abs(a[0] - a[1]), abs(b[0] - b[1])), 3)}
        res["default_path_against_parent_commit"] = {
            "how": "this build and the parent commit's library loaded in one process, two plans of each per temperature (the "
                   "second pair created in the other order), all in the same alternation; the bar compares the first plan of "
                   "each library against the sum of their spreads (max - min over the alternations)",
            "bit_identical_t0": bool(np.array_equal(samples["argmax"], samples["parent_argmax"])),
            "bit_identical_t1": bool(np.array_equal(samples["sequential_t1"], samples["parent_sequential_t1"])),
            "t0": pair("argmax"), "t1": pair("sequential_t1")}
    record("samplernn_forced", "--forced-json", res)

# ---- SampleRNN D=1024, B=32: skip-connection stacks on the device loop (PARROT_SR_SKIP_STACKS=1,
# samplernn_generate_set_skip_stacks) -- a (GRU, 2) model with skip connections on the device loop and on the literal
# three-function loop, a (GRU, 2) model without them (the price of the extra K segments and the out-skip job), and the default
# single-GRU plan at temperature 0 and 1; with --parent-lib, that default plan against the parent commit's library.  All
# plans alive in one process and run alternately, as samplernn_forced; the three models' parameters are swapped in and out of
# the registry outside the timed region (a plan reads the learned h0 from it when a run starts).
if "samplernn_skip" in only:
    import contextlib
    import ctypes
    import io
    from parrot_amd import _lib as plib
    from parrot_amd.sampleRNN import lib as slib
    from parrot_amd.sampleRNN.models.conditional import three_tier as tt
    os.environ["PARROT_SR_SKIP_STACKS"] = "1"
    T, T_LIT, SEED, reps = 101, 3, 234, int(_arg("--reps", "5"))
    feats = torch.randn(T, 32, 63, generator=g).numpy()
    MODELS = {"skip_gru2": dict(RNN_TYPE='GRU', N_RNN=2, SKIP_CONN=True), "plain_gru2": dict(RNN_TYPE='GRU', N_RNN=2, SKIP_CONN=False),
              "default": dict(RNN_TYPE='GRU', N_RNN=1, SKIP_CONN=False)}
    registry = {}

    def select(model):
        """The model's configuration and parameters in place (created with the reference initialisation the first time)."""
        slib._params.clear()
        tt.configure(DIM=1024, EMB_SIZE=256, **MODELS[model])
        if model in registry:
            slib._params.update(registry[model])
            return
        slib.set_device(dev)
        n = MODELS[model]["N_RNN"]
        seq = torch.randint(0, 256, (2, 160 + 80), generator=g).to(dev)
        with torch.no_grad():
            tt.compute_cost(seq, torch.randn(2, 2, 63, device=dev), torch.zeros(2, n, 1024, device=dev),
                            torch.zeros(2, n, 1024, device=dev), 1, torch.ones(2, 240, device=dev))
        registry[model] = slib.named_params()

    this_lib = plib.load()
    parent_path = _arg("--parent-lib")
    parent_lib = None
    if parent_path:
        parent_lib = ctypes.CDLL(os.path.abspath(parent_path))
        for name, (res_, args_) in plib.SIGNATURES.items():
            if hasattr(parent_lib, name):  # (the parent has no samplernn_generate_set_skip_stacks: its plans never call it)
                fn = getattr(parent_lib, name)
                fn.restype = res_
                fn.argtypes = args_

    @contextlib.contextmanager
    def under(which):  # every call of a plan goes to the library that made it
        plib._lib = which
        try:
            yield
        finally:
            plib._lib = this_lib

    def plan(model, which=this_lib, **kw):
        select(model)
        with under(which):
            return tt.DeviceGenerator(32, T, seed=SEED, **kw)

    # name: (model, plan or None = the literal loop, its library)
    plans = {"skip_gru2_device": ("skip_gru2", plan("skip_gru2", temperature=0.0), this_lib),
             "skip_gru2_literal": ("skip_gru2", None, this_lib),
             "plain_gru2_device": ("plain_gru2", plan("plain_gru2", temperature=0.0), this_lib),
             "argmax": ("default", plan("default", temperature=0.0), this_lib),
             "sequential_t1": ("default", plan("default", temperature=1.0), this_lib)}
    if parent_lib is not None:
        plans["parent_argmax"] = ("default", plan("default", which=parent_lib, temperature=0.0), parent_lib)
        plans["parent_sequential_t1"] = ("default", plan("default", which=parent_lib, temperature=1.0), parent_lib)
        # (a second plan of each kind, created in the other order: the floor under any difference between the libraries)
        plans["argmax_again"] = ("default", plan("default", temperature=0.0), this_lib)
        plans["sequential_t1_again"] = ("default", plan("default", temperature=1.0), this_lib)
        plans["parent_sequential_t1_again"] = ("default", plan("default", which=parent_lib, temperature=1.0), parent_lib)
        plans["parent_argmax_again"] = ("default", plan("default", which=parent_lib, temperature=0.0), parent_lib)
    assert plans["skip_gru2_device"][1].skip and plans["skip_gru2_device"][1].persistent
    assert all(gen is None or gen.persist_groups == 1 for _, gen, _ in plans.values())
    nsamp = {k: ((T if gen is not None else T_LIT) - 1) * 80 for k, (_, gen, _) in plans.items()}
    times, samples = {k: [] for k in plans}, {}
    keys = list(plans)
    for rep_ in range(reps + 1):  # (the first alternation captures the graphs: not counted)
        for k in keys[rep_ % len(keys):] + keys[:rep_ % len(keys)]:  # (no plan always runs behind the same other one)
            model, gen, which = plans[k]
            select(model)
            with under(which):
                if gen is None:
                    fns = tt.getting_generation_functions()
                    with contextlib.redirect_stdout(io.StringIO()):
                        torch.cuda.synchronize(); t0 = time.time()
                        s = tt.generate_and_save_samples("bench", None, feats[:T_LIT], None, 0., *fns, temperature=0.0,
                                                         use_device_loop=False)
                        torch.cuda.synchronize(); dt = time.time() - t0
                    samples[k] = np.asarray(s).copy()
                else:
                    torch.cuda.synchronize(); t0 = time.time()
                    s = gen.generate(feats)
                    torch.cuda.synchronize(); dt = time.time() - t0
                    samples[k] = s.cpu().numpy().copy()
            if rep_:
                times[k].append(dt)
    for _, gen, which in plans.values():
        if gen is not None:
            with under(which):
                gen.close()
    slib._params.clear()
    tt.configure(DIM=1024, EMB_SIZE=256, RNN_TYPE='GRU', N_RNN=1, SKIP_CONN=False)
    us = {k: [1e6 * dt / nsamp[k] for dt in v] for k, v in times.items()}
    med = {k: sorted(v)[len(v) // 2] for k, v in us.items()}
    spread = {k: max(v) - min(v) for k, v in us.items()}
    lit, devs = samples["skip_gru2_literal"], samples["skip_gru2_device"][:, :80 * T_LIT]
    res = {"dim": 1024, "streams": 32, "alternations": reps, "samples_per_stream": nsamp,
           "timed": "call to device idle (host-side input copies included); the literal loop runs %d frames per call, the "
                    "device plans %d" % (T_LIT - 1, T - 1),
           "runs": {k: {"us_per_sample_step": [round(x, 3) for x in us[k]], "us_per_sample_step_median": round(med[k], 3),
                        "spread_max_minus_min": round(spread[k], 3)} for k in plans},
           "skip_gru2_device_loop_against_literal_loop": {
               "device_us": round(med["skip_gru2_device"], 3), "literal_us": round(med["skip_gru2_literal"], 3),
               "sum_of_the_two_spreads_us": round(spread["skip_gru2_device"] + spread["skip_gru2_literal"], 3),
               "literal_over_device": round(med["skip_gru2_literal"] / med["skip_gru2_device"], 1),
               "greedy_rows_identical_over_the_literal_loops_frames": int(sum(np.array_equal(a, b) for a, b in zip(lit, devs))),
               "rows": int(lit.shape[0])},
           "price_of_the_skip_connections_gru2": {
               "skip_us": round(med["skip_gru2_device"], 3), "plain_us": round(med["plain_gru2_device"], 3),
               "skip_minus_plain_us": round(med["skip_gru2_device"] - med["plain_gru2_device"], 3),
               "sum_of_the_two_spreads_us": round(spread["skip_gru2_device"] + spread["plain_gru2_device"], 3)},
           "not_measured": ["row groups", "the streaming generator end to end", "LSTM skip stacks at D = 1024",
                            "deeper stacks (N_RNN 3 .. 5)", "the launch path's timing"]}
    if parent_lib is not None:
        def pair(t):  # the standing bar (the two first plans, the sum of their spreads) and the four plans' picture beside it
            a, b = (med[t], med[t + "_again"]), (med["parent_" + t], med["parent_" + t + "_again"])
            both = spread[t] + spread["parent_" + t]
            return {"this_us": [round(x, 3) for x in a], "parent_us": [round(x, 3) for x in b],
                    "this_minus_parent_us": round(a[0] - b[0], 3), "sum_of_the_two_spreads_us": round(both, 3),
                    "bar_default_within_the_sum_of_both_spreads": bool(abs(a[0] - b[0]) <= both),
                    "mean_of_two_plans_this_minus_parent_us": round(sum(a) / 2 - sum(b) / 2, 3),
                    "largest_difference_between_two_plans_of_one_library_us": round(max(abs(a[0] - a[1]), abs(b[0] - b[1])), 3)}
        res["default_path_against_parent_commit"] = {
            "how": "this build and the parent commit's library loaded in one process, two plans of each per temperature (the "
                   "second pair created in the other order), all in the same alternation; the bar compares the first plan of "
                   "each library against the sum of their spreads (max - min over the alternations)",
            "bit_identical_t0": bool(np.array_equal(samples["argmax"], samples["parent_argmax"])),
            "bit_identical_t1": bool(np.array_equal(samples["sequential_t1"], samples["parent_sequential_t1"])),
            "t0": pair("argmax"), "t1": pair("sequential_t1")}
    record("samplernn_skip", "--skip-json", res)

# ---- decode with per-utterance controls (parrot_sample_set_row_controls): configs[2] (2 x GRU-1024) and 2 x LSTM-1024 at
# batch 16, 1000 frames.  Per shape a model whose calls pass no controls, a model whose calls pass all of them and, with
# --parent-lib, a model on the parent commit's library (which has no such entry: its plan decodes with the descriptor's
# scalars, as every plan did), all alive in one process and run alternately.
if "decode_row_controls" in only:
    import contextlib
    import ctypes
    from parrot_amd import _lib as plib
    from parrot_amd.model import Parrot
    reps = int(_arg("--reps", "5"))
    this_lib = plib.load()
    parent_path = _arg("--parent-lib")
    parent_lib = None
    if parent_path:
        parent_lib = ctypes.CDLL(os.path.abspath(parent_path))
        for name, (res_, args_) in plib.SIGNATURES.items():
            if hasattr(parent_lib, name):
                fn = getattr(parent_lib, name)
                fn.restype = res_
                fn.argtypes = args_
        parent_lib.parrot_sample_set_row_controls = lambda *a: 0  # (the parent's plans have no controls to be given)

    @contextlib.contextmanager
    def under(which):  # every call of a model goes to the library that made its plan
        plib._lib = which
        try:
            yield
        finally:
            plib._lib = this_lib

    N, U, S = 16, 100, 1000
    gen = torch.Generator().manual_seed(0)
    lab = torch.randint(0, 43, (N, U), generator=gen)
    lm = torch.ones(N, U)
    cyc = lambda v: (v * 4)[:N]
    rows = dict(timing_coeffs=cyc([1.0, 0.8, 1.25, 2.0, 0.5]), sharpening_coeffs=cyc([1.0, 1.5, 0.7, 1.0, 2.0]))
    shapes = {"cfg3_gru2_1024": dict(num_layers=2, rnn_h_dim=1024, readouts_dim=1024, cell_type='gru'),
              "lstm2_1024": dict(num_layers=2, rnn_h_dim=1024, readouts_dim=1024, cell_type='lstm')}
    res = {"batch": N, "frames": S, "alternations": reps, "timed": "call to device idle (host-side preparation included)",
           "controls": rows, "shapes": {}}
    for sname, kw in shapes.items():
        def model(which):
            with under(which):
                return Parrot(device=dev, encoder_type='bidirectional', weak_feedback=True, use_graph=True, seed=1234, **kw).initialize()
        runs = {"default": (model(this_lib), this_lib, {}), "row_controls": (model(this_lib), this_lib, rows)}
        if parent_lib is not None:
            runs["parent_default"] = (model(parent_lib), parent_lib, {})
            runs["default_again"] = (model(this_lib), this_lib, {})
            runs["parent_default_again"] = (model(parent_lib), parent_lib, {})
        times, frames = {k: [] for k in runs}, {}
        keys = list(runs)
        for rep_ in range(reps + 1):  # (the first alternation builds the plans and captures the graphs: not counted)
            for k in keys[rep_ % len(keys):] + keys[:rep_ % len(keys)]:
                m, which, ckw = runs[k]
                with under(which):
                    torch.cuda.synchronize(); t0 = time.time()
                    outs = m.sample_model_device(lab, lm, None, N, S, **ckw)
                    torch.cuda.synchronize(); dt = time.time() - t0
                    frames[k] = outs[0].cpu().numpy().copy()
                if rep_:
                    times[k].append(1e6 * dt / S)
        machine = {}
        for k, (m, which, _) in runs.items():
            with under(which):
                machine[k] = int(which.parrot_sample_is_persistent(m._sample_ws[(S, N, U)]['plan']))
                m.close()
        med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
        spread = {k: max(v) - min(v) for k, v in times.items()}
        one = {"runs": {k: {"machine": machine[k], "us_per_step": [round(x, 2) for x in times[k]], "us_per_step_median": round(med[k], 2),
                            "spread_max_minus_min": round(spread[k], 2)} for k in runs},
               "row_controls_minus_default_us": round(med["row_controls"] - med["default"], 2),
               "row_controls_frames_differ_from_default": bool((frames["row_controls"] != frames["default"]).any())}
        if parent_lib is not None:
            both = spread["default"] + spread["parent_default"]
            one["default_path_against_parent_commit"] = {
                "how": "this build and the parent commit's library loaded in one process, two models of each (the second pair "
                       "created in the other order), all in the same alternation; the bar compares the first model of each "
                       "library against the sum of their spreads (max - min over the alternations)",
                "bit_identical": bool(np.array_equal(frames["default"], frames["parent_default"])),
                "this_us": [round(med["default"], 2), round(med["default_again"], 2)],
                "parent_us": [round(med["parent_default"], 2), round(med["parent_default_again"], 2)],
                "this_minus_parent_us": round(med["default"] - med["parent_default"], 2),
                "sum_of_the_two_spreads_us": round(both, 2),
                "bar_default_not_slower_by_more_than_the_sum_of_both_spreads": bool(med["default"] - med["parent_default"] <= both)}
        res["shapes"][sname] = one
    res["not_measured"] = ["B > 16", "the H = 1536 LSTM plan with two units per workgroup", "the launch path's timing",
                           "a GMM head with per-utterance biases"]
    record("decode_row_controls", "--row-controls-json", res)

# ---- decode with forced frames (ParrotSampleForcedDesc::forced / n_forced / own_x): configs[2] (2 x GRU-1024) and 2 x LSTM-1024 at
# batch 16, 1000 frames.  Per shape a model whose calls force nothing (the default plan), a model on the forced plan with
# n = 0 everywhere, a model on the forced plan with 200 forced frames of 1000 (seeded N(0, 1) frames), a model on the default
# plan under PARROT_PM_FBC=0 (what the forced GRU plan is expected to cost) and, with --parent-lib, a model on the parent
# commit's library, all alive in one process and run alternately.  The switch is read when a plan is made: it is set around
# every call of its model and of no other.
if "decode_forced" in only:
    import contextlib
    import ctypes
    from parrot_amd import _lib as plib
    from parrot_amd.model import Parrot
    reps = int(_arg("--reps", "5"))
    this_lib = plib.load()
    parent_path = _arg("--parent-lib")
    parent_lib = None
    if parent_path:
        parent_lib = ctypes.CDLL(os.path.abspath(parent_path))
        for name, (res_, args_) in plib.SIGNATURES.items():
            if hasattr(parent_lib, name):
                fn = getattr(parent_lib, name)
                fn.restype = res_
                fn.argtypes = args_

    @contextlib.contextmanager
    def under(which, env):  # every call of a model goes to the library that made its plan, under the model's switches
        plib._lib = which
        saved = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            yield
        finally:
            plib._lib = this_lib
            for k, v in saved.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v

    N, U, S, P = 16, 100, 1000, 200
    gen = torch.Generator().manual_seed(0)
    lab = torch.randint(0, 43, (N, U), generator=gen)
    lm = torch.ones(N, U)
    prompt = torch.randn(P, N, 63, generator=gen)
    forced0 = dict(forced_frames=prompt, n_forced=[0] * N)
    forced200 = dict(forced_frames=prompt, n_forced=[P] * N)
    shapes = {"cfg3_gru2_1024": dict(num_layers=2, rnn_h_dim=1024, readouts_dim=1024, cell_type='gru'),
              "lstm2_1024": dict(num_layers=2, rnn_h_dim=1024, readouts_dim=1024, cell_type='lstm')}
    res = {"batch": N, "frames": S, "forced_frames": P, "alternations": reps,
           "timed": "call to device idle (host-side preparation included)", "shapes": {}}
    for sname, kw in shapes.items():
        def model(which):
            with under(which, {}):
                return Parrot(device=dev, encoder_type='bidirectional', weak_feedback=True, use_graph=True, seed=1234, **kw).initialize()
        runs = {"default": (model(this_lib), this_lib, {}, {}, False),
                "forced_n0": (model(this_lib), this_lib, forced0, {}, True),
                "forced_200_of_1000": (model(this_lib), this_lib, forced200, {}, True)}
        if kw['cell_type'] == 'gru':
            runs["default_fbc0"] = (model(this_lib), this_lib, {}, {"PARROT_PM_FBC": "0"}, False)
        if parent_lib is not None:
            runs["parent_default"] = (model(parent_lib), parent_lib, {}, {}, False)
            runs["default_again"] = (model(this_lib), this_lib, {}, {}, False)
            runs["parent_default_again"] = (model(parent_lib), parent_lib, {}, {}, False)
        times, frames = {k: [] for k in runs}, {}
        keys = list(runs)
        for rep_ in range(reps + 1):  # (the first alternation builds the plans and captures the graphs: not counted)
            for k in keys[rep_ % len(keys):] + keys[:rep_ % len(keys)]:
                m, which, ckw, env, _ = runs[k]
                with under(which, env):
                    torch.cuda.synchronize(); t0 = time.time()
                    outs = m.sample_model_device(lab, lm, None, N, S, **ckw)
                    torch.cuda.synchronize(); dt = time.time() - t0
                    frames[k] = outs[0].cpu().numpy().copy()
                if rep_:
                    times[k].append(1e6 * dt / S)
        machine = {}
        for k, (m, which, _, env, forced_) in runs.items():
            with under(which, env):
                key_ = (('forced',) if forced_ else ()) + (S, N, U)
                machine[k] = int(which.parrot_sample_is_persistent(m._sample_ws[key_]['plan']))
                m.close()
        med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
        spread = {k: max(v) - min(v) for k, v in times.items()}
        one = {"runs": {k: {"machine": machine[k], "us_per_step": [round(x, 2) for x in times[k]], "us_per_step_median": round(med[k], 2),
                            "spread_max_minus_min": round(spread[k], 2)} for k in runs},
               "forced_n0_minus_default_us": round(med["forced_n0"] - med["default"], 2),
               "forced_200_minus_default_us": round(med["forced_200_of_1000"] - med["default"], 2),
               "forced_n0_frames_equal_default": bool(np.array_equal(frames["forced_n0"], frames["default"])),
               "forced_200_prompt_is_in_the_frames": bool(np.array_equal(frames["forced_200_of_1000"][:P], prompt.numpy()))}
        if "default_fbc0" in runs:
            one["forced_n0_minus_default_fbc0_us"] = round(med["forced_n0"] - med["default_fbc0"], 2)
            one["forced_n0_frames_equal_default_fbc0"] = bool(np.array_equal(frames["forced_n0"], frames["default_fbc0"]))
        if parent_lib is not None:
            both = spread["default"] + spread["parent_default"]
            gap = med["default"] - med["parent_default"]
            one["default_path_against_parent_commit"] = {
                "how": "this build and the parent commit's library loaded in one process, two models of each (the second pair "
                       "created in the other order), all in the same alternation; the bar compares the first model of each "
                       "library against the sum of their spreads (max - min over the alternations)",
                "bit_identical": bool(np.array_equal(frames["default"], frames["parent_default"])),
                "this_us": [round(med["default"], 2), round(med["default_again"], 2)],
                "parent_us": [round(med["parent_default"], 2), round(med["parent_default_again"], 2)],
                "this_minus_parent_us": round(gap, 2),
                "sum_of_the_two_spreads_us": round(both, 2),
                "bar_default_within_the_sum_of_both_spreads": "met" if abs(gap) <= both else "not met"}
        res["shapes"][sname] = one
    res["not_measured"] = ["B > 16", "the H = 1536 LSTM plan with two units per workgroup", "the launch path's timing",
                           "a GMM head with forced frames", "forcing together with the end-of-utterance stop"]
    record("decode_forced", "--forced-decode-json", res)

# ---- resumable decode (parrot_sample_save_state / _load_state, Parrot.decode_segments): configs[2] (2 x GRU-1024) and
# 2 x LSTM-1024 at batch 16, 1000 frames.  Per shape a model for the plain call, one for the one-piece carry call
# (return_state=True), one decoding in segments of 50 frames and one in segments of 10, and, with --parent-lib, a model on the
# parent commit's library, all alive in one process and run alternately.  A segmented run is timed from the call to the last
# segment on the host side of the device (device idle), and to its FIRST segment (yielded and synchronised); the cost of a
# boundary is (segmented total - one-piece carry total) / (segments - 1).
if "decode_segments" in only:
    import contextlib
    import ctypes
    from parrot_amd import _lib as plib
    from parrot_amd.model import Parrot
    reps = max(3, int(_arg("--reps", "5")))
    this_lib = plib.load()
    parent_path = _arg("--parent-lib")
    parent_lib = None
    if parent_path:
        parent_lib = ctypes.CDLL(os.path.abspath(parent_path))
        for name, (res_, args_) in plib.SIGNATURES.items():
            if hasattr(parent_lib, name):
                fn = getattr(parent_lib, name)
                fn.restype = res_
                fn.argtypes = args_

    @contextlib.contextmanager
    def under(which):  # every call of a model goes to the library that made its plan
        plib._lib = which
        try:
            yield
        finally:
            plib._lib = this_lib

    N, U, S = 16, 100, 1000
    gen = torch.Generator().manual_seed(0)
    lab = torch.randint(0, 43, (N, U), generator=gen)
    lm = torch.ones(N, U)
    shapes = {"cfg3_gru2_1024": dict(num_layers=2, rnn_h_dim=1024, readouts_dim=1024, cell_type='gru'),
              "lstm2_1024": dict(num_layers=2, rnn_h_dim=1024, readouts_dim=1024, cell_type='lstm')}
    res = {"batch": N, "frames": S, "alternations": reps,
           "timed": "call to device idle, host-side preparation included; first_segment_ms: call to the first segment "
                    "yielded and the device idle", "shapes": {}}

    def whole(m, **kw):
        outs = m.sample_model_device(lab, lm, None, N, S, **kw)
        torch.cuda.synchronize()
        return (outs[0] if kw else outs)[0], None

    def segmented(F):
        def fn(m):
            t0, first, parts = time.time(), None, []
            for _, seg in m.decode_segments(lab, lm, None, N, S, F):
                if first is None:
                    torch.cuda.synchronize()
                    first = time.time() - t0
                parts.append(seg[0])
            torch.cuda.synchronize()
            return torch.cat(parts), first
        return fn

    for sname, kw in shapes.items():
        def model(which):
            with under(which):
                return Parrot(device=dev, encoder_type='bidirectional', weak_feedback=True, use_graph=True, seed=1234, **kw).initialize()
        runs = {"plain": (model(this_lib), this_lib, whole),
                "carry_one_piece": (model(this_lib), this_lib, lambda m: whole(m, return_state=True)),
                "segments_50": (model(this_lib), this_lib, segmented(50)),
                "segments_10": (model(this_lib), this_lib, segmented(10))}
        if parent_lib is not None:
            runs["parent_plain"] = (model(parent_lib), parent_lib, whole)
            runs["plain_again"] = (model(this_lib), this_lib, whole)
            runs["parent_plain_again"] = (model(parent_lib), parent_lib, whole)
        times, firsts, frames = {k: [] for k in runs}, {k: [] for k in runs}, {}
        keys = list(runs)
        for rep_ in range(reps + 1):  # (the first alternation builds the plans and captures the graphs: not counted)
            for k in keys[rep_ % len(keys):] + keys[:rep_ % len(keys)]:
                m, which, fn = runs[k]
                with under(which):
                    torch.cuda.synchronize(); t0 = time.time()
                    x, first = fn(m)
                    dt = time.time() - t0
                    frames[k] = x.cpu().numpy().copy()
                if rep_:
                    times[k].append(1e3 * dt)
                    if first is not None:
                        firsts[k].append(1e3 * first)
        machine = {}
        for k, (m, which, _) in runs.items():
            with under(which):
                machine[k] = sorted(int(which.parrot_sample_is_persistent(ws['plan'])) for ws in m._sample_ws.values())
                m.close()
        med = lambda v: sorted(v)[len(v) // 2]
        one = {"runs": {k: {"machine": machine[k], "total_ms": [round(x, 3) for x in times[k]], "total_ms_median": round(med(times[k]), 3),
                            "spread_max_minus_min_ms": round(max(times[k]) - min(times[k]), 3),
                            "us_per_step_median": round(1e3 * med(times[k]) / S, 2)} for k in runs}}
        for k, F_ in (("segments_50", 50), ("segments_10", 10)):
            one["runs"][k].update(first_segment_ms=[round(x, 3) for x in firsts[k]], first_segment_ms_median=round(med(firsts[k]), 3),
                                  segments=S // F_,
                                  us_per_boundary=round(1e3 * (med(times[k]) - med(times["carry_one_piece"])) / (S // F_ - 1), 2))
        one["carry_minus_plain_us_per_step"] = round(1e3 * (med(times["carry_one_piece"]) - med(times["plain"])) / S, 2)
        one["segments_equal_carry_one_piece"] = bool(np.array_equal(frames["segments_50"], frames["carry_one_piece"])
                                                     and np.array_equal(frames["segments_10"], frames["carry_one_piece"]))
        one["carry_frames_equal_plain"] = bool(np.array_equal(frames["carry_one_piece"], frames["plain"]))
        if parent_lib is not None:
            sp = lambda k: max(times[k]) - min(times[k])
            both, gap = sp("plain") + sp("parent_plain"), med(times["plain"]) - med(times["parent_plain"])
            one["default_path_against_parent_commit"] = {
                "how": "this build and the parent commit's library loaded in one process, two models of each (the second pair "
                       "created in the other order), all in the same alternation; the bar compares the first model of each "
                       "library against the sum of their spreads (max - min over the alternations)",
                "bit_identical": bool(np.array_equal(frames["plain"], frames["parent_plain"])),
                "this_us_per_step": [round(1e3 * med(times[k]) / S, 2) for k in ("plain", "plain_again")],
                "parent_us_per_step": [round(1e3 * med(times[k]) / S, 2) for k in ("parent_plain", "parent_plain_again")],
                "this_minus_parent_us_per_step": round(1e3 * gap / S, 2),
                "sum_of_the_two_spreads_us_per_step": round(1e3 * both / S, 2),
                "bar_default_within_the_sum_of_both_spreads": "met" if abs(gap) <= both else "not met"}
        res["shapes"][sname] = one
    res["not_measured"] = ["B > 16", "the H = 1536 LSTM plan with two units per workgroup", "the launch path's timing",
                           "StreamingDecoder: admission under load"]
    record("decode_segments", "--segments-json", res)

# ---- text to audio in one stream (parrot_amd.decode.TextToAudio): the decoder's segments feed the vocoder's ring on the device.
# Against the staged path of the parent commit: every frame decoded (StreamingDecoder.run()), copied to the host, then whole
# utterances submitted to a StreamingGenerator.  All three keep their plans alive in one process and alternate; a run is timed
# from its first call to the last chunk on the host, "first audio" to the first chunk that holds samples behind a prefix.
if "text_to_audio" in only:
    from parrot_amd import _lib as plib
    from parrot_amd import ops as hip
    from parrot_amd.decode import StreamingDecoder, TextToAudio
    from parrot_amd.model import Parrot
    tt = samplernn_d1024()
    N, U, T, Bv, Sv, extra, runs_each = 16, 100, 1000, 16, 8, 40, 3
    m = Parrot(device=dev, encoder_type='bidirectional', weak_feedback=True, use_graph=True, num_layers=2, rnn_h_dim=1024,
               readouts_dim=1024, encoder_literal=False, seed=1234).initialize()
    # (kappa bias -2.2: the window walks about 0.1 characters per frame, so texts of 20 .. 100 characters end after some 200 ..
    # 1000 frames; --kappa-bias B sets another pace)
    m._p('/h1_to_att/fork_kappa.b').fill_(float(_arg("--kappa-bias", "-2.2")))
    gen_ = torch.Generator().manual_seed(0)
    texts = [torch.randint(0, 43, (20 + (80 * i) // (N - 1),), generator=gen_) for i in range(N)]

    def pipeline(F):
        tta = TextToAudio(m, N, F, U, T, Bv, Sv, extra=extra)

        def run():
            for t in texts:
                tta.submit(t)
            pieces = {}
            for uid, chunk, done in tta.run():
                pieces.setdefault(uid, []).append(chunk)
            ids = sorted(pieces)
            return tta.first_audio_s, [np.concatenate(pieces[i]) for i in ids]
        return run, tta.close

    def staged(F):
        sd = StreamingDecoder(m, N, F, U, T, extra=extra)
        sg = tt.StreamingGenerator(Bv, Sv, temperature=0.0)

        def run():
            t0 = time.time()
            ids = [sd.submit(t) for t in texts]
            frames = {uid: fr.cpu().numpy() for uid, fr, _ in sd.run()}
            tickets = {sg.submit(frames[uid]): k for k, uid in enumerate(ids)}
            pieces, first = {}, None
            while not sg.idle():
                for ticket, chunk, done in sg.step():
                    if first is None and (ticket in pieces or chunk.size > 80):
                        first = time.time() - t0
                    pieces.setdefault(ticket, []).append(chunk)
            return first, [np.concatenate(pieces[t]) for t in sorted(pieces, key=tickets.get)]
        return run, sg.close

    legs = {"pipeline_decoder_segments_10": pipeline(10), "pipeline_decoder_segments_50": pipeline(50),
            "staged_decoder_segments_50": staged(50)}
    totals, firsts, samples = {k: [] for k in legs}, {k: [] for k in legs}, {}
    keys = list(legs)
    for rep_ in range(runs_each + 1):  # (the first round builds the plans and captures the graphs: not counted)
        for k in keys[rep_ % len(keys):] + keys[:rep_ % len(keys)]:
            torch.cuda.synchronize(); t0 = time.time()
            first, samples[k] = legs[k][0]()
            torch.cuda.synchronize(); dt = time.time() - t0
            if rep_:
                totals[k].append(1e3 * dt)
                firsts[k].append(1e3 * first)
    for run_, close_ in legs.values():
        close_()
    med = lambda v: sorted(v)[len(v) // 2]
    lengths = [int(s.size) // 80 for s in samples["staged_decoder_segments_50"]]
    res = {"decoder": "configs[2]: 2 x GRU-1024, MSE head, %d slots" % N, "vocoder": "DIM 1024, %d streams, segments of %d" % (Bv, Sv),
           "utterances": N, "frames_per_utterance": lengths, "runs_each": runs_each,
           "timed": "first submit to the last chunk on the host; first_audio_ms: to the first chunk with samples behind a prefix",
           "legs": {k: {"total_ms": [round(x, 2) for x in totals[k]], "total_ms_median": round(med(totals[k]), 2),
                        "total_spread_max_minus_min_ms": round(max(totals[k]) - min(totals[k]), 2),
                        "first_audio_ms": [round(x, 2) for x in firsts[k]], "first_audio_ms_median": round(med(firsts[k]), 2),
                        "first_audio_spread_max_minus_min_ms": round(max(firsts[k]) - min(firsts[k]), 2)} for k in legs},
           "pipeline_samples_equal_staged": {k: bool(all(a.shape == b.shape and np.array_equal(a, b) for a, b in
                                                         zip(samples[k], samples["staged_decoder_segments_50"])))
                                             for k in keys[:2]}}
    m.close()
    # the staging call against the host-array upload it replaces: one vocoder segment of Sv frames on Bv streams
    sgen = tt.DeviceGenerator(Bv, Sv + 1, temperature=0.0, packed=True)
    store = torch.randn(32 * T, 64, generator=g).to(dev)
    index = torch.randint(0, 32 * T, (Sv, Bv), generator=g, dtype=torch.int32).numpy()
    host = store.cpu().numpy()[index.reshape(-1), :63].reshape(Sv, Bv, 63).copy()
    fbuf = sgen.ws['features']

    def upload():
        fbuf[1:Sv + 1].copy_(torch.as_tensor(host).to(fbuf.device, torch.float32))

    def stage():
        idx = torch.from_numpy(index).to(dev)
        plib.call('samplernn_generate_stage_features', sgen.plan, store.data_ptr(), store.shape[0], 64, idx.data_ptr(), 1, Sv,
                  hip._stream())

    per_call = {"host_array_upload": [], "stage_features": []}
    for rep_ in range(runs_each + 1):
        for k, fn in (("host_array_upload", upload), ("stage_features", stage))[::1 if rep_ % 2 else -1]:
            torch.cuda.synchronize(); t0 = time.time()
            for _ in range(200):
                fn()
                torch.cuda.synchronize()
            if rep_:
                per_call[k].append(1e6 * (time.time() - t0) / 200)
    stage()
    torch.cuda.synchronize()
    res["staging_call"] = {"shape": "%d frames x %d streams x 63 floats, call to device idle, 200 calls per run" % (Sv, Bv),
                           "us_per_call": {k: [round(x, 1) for x in v] for k, v in per_call.items()},
                           "staged_rows_equal_uploaded": bool(np.array_equal(fbuf[1:Sv + 1].cpu().numpy(), host))}
    sgen.close()
    res["not_measured"] = ["admission under load (texts arriving while the pipeline runs)", "a pool smaller than the traffic",
                           "GMM-head decoders", "per-utterance draws at temperature > 0", "more than 16 utterances in flight"]
    record("text_to_audio", "--text-to-audio-json", res)

# ---- mu-law quantiser: x ~ N(0,1) [32, 16000*8]
if "mulaw" in only:
    from parrot_amd import ops
    x = torch.randn(32, 128000, device=dev)
    for rep in range(3):
        torch.cuda.synchronize(); t0 = time.time()
        for _ in range(20):
            q = ops.batch_quantize(x, 256, "mu-law")
        torch.cuda.synchronize(); dt = (time.time() - t0) / 20
    out["mulaw"] = {"elements": x.numel(), "us": round(1e6 * dt, 1), "GBps_alg": round(x.numel() * 6 / dt * 1e-9, 1)}
print(json.dumps(out))

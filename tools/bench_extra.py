"""Secondary measurements (BASELINE configs[2] decode latency, the same loop with LSTM decoders -- persistent machine
with bf16 operands (decode_dtype='bf16') against the f32 machine against the per-step launches, alternating child
processes --, the configs[2] decode that stops at the end of the utterance against the one that runs all its steps,
configs[4] SampleRNN sample loop, mu-law quantiser bandwidth).  Development / documentation aid; the driver's headline bench is bench.py.

  bench_extra.py                         everything, one JSON line
  bench_extra.py --only NAME[,NAME]      a subset (decode_cfg3, decode_stop, decode_lstm2_1024, decode_lstm3_1536,
                                         samplernn_cfg5, mulaw)
  bench_extra.py --kappa-bias B          decode_stop: fork_kappa.b of the randomly initialised model (default -1.0: how fast
                                         the window walks over the text, i.e. after how many steps the utterance ends)
  bench_extra.py --dump-sample FILE      decode_cfg3 also saves sample_x (numpy) -- bit-identity checks between builds
  bench_extra.py --reps N                on / off alternations of the LSTM decode entries (default 3)"""
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


ALL = ("decode_cfg3", "decode_stop", "decode_lstm2_1024", "decode_lstm3_1536", "samplernn_cfg5", "mulaw")
only = tuple(_arg("--only", ",".join(ALL)).split(","))
assert all(n in ALL for n in only), only
LSTM_SHAPES = {  # configs[2]'s shape with LSTM cells; the 3 x LSTM-1536 model of BASELINE configs[3]
    "decode_lstm2_1024": dict(num_layers=2, rnn_h_dim=1024, readouts_dim=1024),
    "decode_lstm3_1536": dict(num_layers=3, rnn_h_dim=1536, readouts_dim=1536),
}
dev = torch.device("cuda:0")
out = {}
g = torch.Generator().manual_seed(0)


def decode(kw, dump=None, decode_dtype='float32'):
    """Autoregressive decode, batch 16, 1000 frames, MSE head (greedy), hipGraph: three runs, the last one reported."""
    from parrot_amd import _lib
    from parrot_amd.model import Parrot
    m = Parrot(device=dev, encoder_type='bidirectional', weak_feedback=True, use_graph=True, decode_dtype=decode_dtype,
               **kw).initialize()
    g = torch.Generator().manual_seed(0)
    N, U, S = 16, 100, 1000
    lab = torch.randint(0, 43, (N, U), generator=g)
    lm = torch.ones(N, U)
    for rep in range(3):
        torch.cuda.synchronize(); t0 = time.time()
        outs = m.sample_model_device(lab, lm, None, N, S)
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

# ---- configs[4]: SampleRNN 3-tier GRU D=1024, batch 32, greedy, 16 kHz mu-law
if "samplernn_cfg5" in only:
    from parrot_amd.sampleRNN import lib
    from parrot_amd.sampleRNN.models.conditional import three_tier as tt
    lib.delete_all_params(); lib.set_device(dev)
    tt.configure(DIM=1024, EMB_SIZE=256)
    B, T = 32, 26  # 25 generated big frames = 2000 samples per stream
    seq = torch.randint(0, 256, (2, 160 + 80), generator=g).to(dev)
    with torch.no_grad():  # registers all parameters with the reference initialisation
        tt.compute_cost(seq, torch.randn(2, 2, 63, device=dev), torch.zeros(2, 1, 1024, device=dev),
                        torch.zeros(2, 1, 1024, device=dev), 1, torch.ones(2, 240, device=dev))
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

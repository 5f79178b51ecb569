"""Headline benchmark: acoustic feature frames/sec of one training step (fwd + bwd + gradient
all-reduce + clip/Adam) of the attention-GRU decoder at BASELINE.json configs[1]:
2-layer attention-GRU h=1024, batch=64 per GPU, T_enc=200, T_dec=800, fp32, synthetic data.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
    (N > 1: launched by torch.distributed.run, one rank per GPU, RCCL all-reduce of the flat gradient)

Prints ONE JSON line on rank 0 (see the driver contract).  A plain run sets up, warms up, times the K steps and prints
the line; --dump-outputs DIR also writes what the last timed step computed as DIR/<name>.npy (dump_outputs).  Everything
else is measured only with --full, and the line's fields for it are null otherwise.  With --full the line also carries
  roofline     -- the recurrent-step kernel family (sk_kernel): algorithmic flops of all its dispatches
                  in one training step / summed dispatch time, measured with HIP events attached to
                  every dispatch (hipExtLaunchKernelGGL) on the stream they run on, vs the f32 MFMA peak;
  cpu_baseline -- the oracle restatement of the reference (torch-CPU fp32, all host cores) timed on
                  a bounded sample of the same workload, on rank 0 at N=1 only;
and allreduce_ms, dense, value_f32_mfma, parity_check and secondary (see main()).
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed as DIR/<name>.npy (at most 64 MB)")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check everything beside the headline figure (all-reduce time, roofline, dense "
                         "and f32-MFMA runs, CPU baseline, parity, secondary configurations); the --no-* switches "
                         "below thin this out")
    ap.add_argument("--T", type=int, default=800, help="decoder frames per window (T_dec)")
    ap.add_argument("--B", type=int, default=64, help="batch per GPU")
    ap.add_argument("--U", type=int, default=200, help="encoder timesteps (T_enc)")
    ap.add_argument("--H", type=int, default=1024)
    ap.add_argument("--L", type=int, default=2)
    ap.add_argument("--config", choices=("cfg2", "cfg4"), default="cfg2",
                    help="cfg2 = BASELINE configs[1] (the headline; default).  cfg4 = BASELINE configs[3] per GPU: 3-layer "
                         "LSTM h=1536 + attention, batch 64 per GPU (global 512 on 8), bf16 operands; sets --L/--H/--cell/--dtype")
    ap.add_argument("--cell", choices=("gru", "lstm"), default="gru")
    ap.add_argument("--dtype", choices=("f32", "bf16"), default="f32",
                    help="bf16: MFMA operands (weights and activations) rounded to bf16, f32 accumulation, f32 master "
                         "weights / states / gradients")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--cpu-baseline-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--cpu-T", type=int, default=100, help="decoder frames per window of the CPU-baseline sample")
    ap.add_argument("--cpu-iters", type=int, default=10, help="timed CPU-baseline iterations (after 3 warm-ups)")
    ap.add_argument("--kappa-bias", type=float, default=-1.5,
                    help="bias of the attention's kappa projection: exp(-1.5) = 0.22 positions per frame keeps the "
                         "window inside the 200-character context for all 800 frames (with the plain N(0, 0.01) init "
                         "kappa advances ~1 per frame and leaves the text after ~210 frames, after which no context row "
                         "is read at all -- a favourable, unrealistic case)")
    ap.add_argument("--no-dense", action="store_true", help="skip the second timed run that reads all context rows")
    ap.add_argument("--no-f32-gemm", action="store_true",
                    help="skip the extra timed run with the batched products on the f32-input MFMA kernel (value_f32_mfma)")
    ap.add_argument("--no-secondary", action="store_true",
                    help="skip the `secondary` object (decode configs[2], SampleRNN configs[4], configs[3] bf16 step), "
                         "measured after the headline region in child processes")
    ap.add_argument("--no-parity", action="store_true", help="skip the `parity_check` object (HIP step vs fp64 oracle)")
    ap.add_argument("--secondary-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--parity-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--plumbing-only", action="store_true",
                    help="N > 1 launch + collectives only (no GPU step, value null): what the CPU/gloo test of the "
                         "self-launch path runs")
    a = ap.parse_args()
    if a.config == "cfg4":
        a.L, a.H, a.cell = 3, 1536, "lstm"
        if "--dtype" not in sys.argv:
            a.dtype = "bf16"
    return a


def host_cores():
    """Usable host cores: min(affinity, cgroup CPU quota).  The GPU boxes show 256 logical CPUs but
    run the container under a 16-CPU quota; oversubscribing that stalls torch-CPU for minutes."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except Exception:
        pass
    return max(1, n)


def gemm_mode_name():
    from parrot_amd import ops as pops
    return {pops.PRECISION_F32: "f32 (v_mfma_f32_32x32x2_f32)",
            pops.PRECISION_BF16X3: "bf16x3 (f32 operands split into three bf16 terms in-kernel, six "
                                   "v_mfma_f32_32x32x16_bf16 per block, f32 accumulate: f32-grade results)"}[pops.full_precision()]


def make_batch(a, dev, seed):
    g = torch.Generator().manual_seed(seed)
    feat = torch.randn(a.T + 1, a.B, 63, generator=g).to(dev)
    fmask = torch.ones(a.T + 1, a.B, device=dev)
    labels = torch.randint(0, 43, (a.B, a.U), generator=g).to(dev)
    lmask = torch.ones(a.B, a.U, device=dev)
    return feat, fmask, labels, lmask


def model_kwargs(a):
    return dict(num_layers=a.L, rnn_h_dim=a.H, readouts_dim=a.H, encoder_type='bidirectional', cell_type=a.cell)


def build_model(a, dev, use_graph=True):
    """BASELINE configs[1] model: train.py's init (N(0, 0.01) weights, zero biases) except the kappa bias (--kappa-bias)."""
    from parrot_amd.model import Parrot
    m = Parrot(device=dev, use_graph=use_graph, seed=1234,
               compute_dtype='bf16' if a.dtype == 'bf16' else 'float32', **model_kwargs(a)).initialize()
    with torch.no_grad():
        m.get_parameter_dict()['/parrot/h1_to_att/fork_kappa.b'].fill_(a.kappa_bias)
    return m


DUMP_BYTES = 64_000_000  # --dump-outputs: all files together stay below this


def dump_outputs(path, cost, model, batch_size):
    """What the last timed Trainer.step hands its caller, as .npy files: the cost it returned (float64), the parameters
    after its clip + Adam update, the gradient it applied, and the TBPTT carry (h and c of every layer, w, kappa) the next
    step starts from (float32).  Each array gets an equal share of DUMP_BYTES; a larger one is written as a fixed sample:
    the sorted distinct flat indices drawn with seed 0, so two runs with the same arguments write the same elements."""
    import numpy as np
    carry = model._carry[batch_size]
    arrays = {"cost": cost.detach().double().reshape(1), "parameters": model.flat_parameters,
              "gradients": model.flat_gradients}
    for l, (h, c) in enumerate(zip(carry['h'], carry['c'])):
        arrays[f"state_h{l + 1}"], arrays[f"state_c{l + 1}"] = h, c
    arrays["state_w"], arrays["state_k"] = carry['w'], carry['k']
    share = DUMP_BYTES // (len(arrays) + 1)  # (the spare share covers the .npy headers)
    os.makedirs(path, exist_ok=True)
    for name, t in arrays.items():
        t = t.detach()
        cap = share // t.element_size()
        if t.numel() > cap:
            idx = np.unique(np.random.default_rng(0).integers(0, t.numel(), size=cap))
            t = t.reshape(-1)[torch.from_numpy(idx).to(t.device)]
        np.save(os.path.join(path, name + ".npy"), t.cpu().numpy())


def kernel_source_digest(root=ROOT):
    """sha256 over the sources of the step kernels and their schedules: what a PMC traffic figure is valid for."""
    import hashlib
    hd = hashlib.sha256()
    for name in ("skinny.hip", "skinny.h", "plans.hip", "plans_common.h", "att_fwd_body.h"):
        hd.update(open(os.path.join(root, "parrot_amd", "csrc", name), "rb").read())
    return hd.hexdigest()


def secondary_source_digest(root=ROOT):
    """sha256 over the sources of the decode machine and the SampleRNN sample kernel: what profiles/rNN_pmc_secondary.json
    is valid for."""
    import hashlib
    hd = hashlib.sha256()
    for name in ("persist.hip", "persist.h", "plans_decode.hip", "sr_persist.hip", "sr_persist.h", "sr_common.h", "samplernn.hip"):
        hd.update(open(os.path.join(root, "parrot_amd", "csrc", name), "rb").read())
    return hd.hexdigest()


def pmc_secondary_figure(which, root=ROOT, names=("r06_pmc_secondary.json",)):
    """(counter bytes per step | None, note): HBM-side bytes per decode step / per SampleRNN sample step from the committed
    counter passes (tools/pmc_secondary.py), refused when the kernels' sources changed after they were measured."""
    for name in names:
        path = os.path.join(root, "profiles", name)
        if not os.path.exists(path):
            continue
        try:
            blob = json.load(open(path))
        except Exception:
            return None, f"profiles/{name} is unreadable"
        if blob.get("source_digest") != secondary_source_digest(root):
            return None, f"profiles/{name} is stale: the kernel sources changed after it was measured"
        rec = blob.get(which)
        if not rec:
            return None, f"profiles/{name} has no {which} record"
        return rec["bytes_per_step"], f"profiles/{name} ({blob.get('session', '?')}; tools/pmc_secondary.py; separate --pmc passes)"
    return None, "no committed counter passes"


def trace_launch_figure(root=ROOT, names=("r06_bench_kernel_stats.csv",), kernels=("sk_kernel<",)):
    """(average launch duration in us | None, note) of the plain step-GEMM launches in the committed rocprofv3 --kernel-trace
    --stats summary of the headline command: the figure the HIP-event leg of this run should agree with."""
    import csv
    for name in names:
        path = os.path.join(root, "profiles", name)
        if not os.path.exists(path):
            continue
        tot_ns, calls = 0.0, 0
        try:
            for r in csv.DictReader(open(path)):
                if any(k in r["Name"] for k in kernels) and "ska_kernel" not in r["Name"] and "skb_kernel" not in r["Name"]:
                    tot_ns += float(r["TotalDurationNs"]); calls += int(r["Calls"])
        except Exception:
            return None, f"profiles/{name} is unreadable"
        if calls:
            return round(tot_ns / calls * 1e-3, 3), f"profiles/{name} ({calls} launches in the trace)"
    return None, "no committed kernel trace"


def pmc_traffic_figure(root=ROOT, names=("r06_pmc_traffic.json", "r05_pmc_traffic.json"), key="hbm_bytes_per_launch"):
    """(bytes per launch | None, source note).  HBM-side bytes per step-kernel launch come from separate rocprofv3 --pmc
    passes (FETCH_SIZE / WRITE_SIZE cannot share a pass with the timed run), so the number is a committed measurement,
    not one of this run -- and it is only reported while the kernel sources it was measured on are unchanged (digest
    stored by tools/pmc_traffic.py); otherwise `traffic` is null and the note says which file went stale."""
    for name in names:
        tpath = os.path.join(root, "profiles", name)
        if not os.path.exists(tpath):
            continue
        try:
            blob = json.load(open(tpath))
        except Exception:
            return None, f"profiles/{name} is unreadable"
        if blob.get("source_digest") == kernel_source_digest(root):
            return blob.get(key, blob.get("hbm_bytes_per_launch")), (f"profiles/{name} ({blob.get('session', '?')}; tools/pmc_traffic.py; "
                                                      "separate --pmc passes)")
        return None, f"profiles/{name} is stale: the kernel sources changed after it was measured"
    return None, None



def roofline_leg(a, dev, flat_params):
    """One extra, untimed training step with eager launches, every recurrent-step dispatch timed."""
    from parrot_amd import _lib, ops
    from parrot_amd import dist as pdist
    from parrot_amd.model import Parrot
    from parrot_amd.trainer import Trainer
    with pdist.local_only():  # rank 0 measures alone: no collective may be issued here (N > 1)
        return _roofline_leg(a, dev, flat_params, _lib, Parrot, Trainer)


def _roofline_leg(a, dev, flat_params, _lib, Parrot, Trainer):
    m = build_model(a, dev, use_graph=False)
    m.flat_parameters.copy_(flat_params)
    tr = Trainer(m)
    batch = make_batch(a, dev, 4321)
    tr.step(*batch, None, 1)  # warm (allocations, caches)
    torch.cuda.synchronize()
    lib = _lib.load()
    lib.parrot_profile_begin()
    tr.step(*batch, None, 1)
    torch.cuda.synchronize()
    us, fl, by = C.c_double(), C.c_double(), C.c_double()
    plain = (C.c_double * 4)()
    n = lib.parrot_profile_end2(C.byref(us), C.byref(fl), C.byref(by), plain)
    m.close()
    if n <= 0 or us.value <= 0:
        return None
    ach = fl.value / us.value * 1e-6  # TFLOP/s
    # the whole step-kernel family (heterogeneous launches carry the attention forward / backward chains beside their GEMM
    # workgroups: their time counts, the chains have no flops) -- reported beside the dominant kernel's own figure
    family = {"launches_per_step": int(n), "avg_launch_us": round(us.value / n, 3),
              "kernel_time_ms_per_step": round(us.value * 1e-3, 3), "alg_TFLOPs": round(ach, 2),
              "alg_GBps": round(by.value / us.value * 1e-3, 1),
              "note": "all step launches incl. the heterogeneous ones (attention forward / backward row blocks in the grid)"}
    p_us, p_fl, p_by, p_n = (float(plain[i]) for i in range(4))
    if a.dtype == "bf16":
        # bf16 operands: 16 x the f32 matrix rate, half the weight bytes -- the step GEMMs (M = 64 rows per weight
        # element) are bound by how fast the weights and the f32 activations arrive, so the roof is HBM / L2 bandwidth
        gbps = by.value / us.value * 1e-3
        traffic4, traffic4_src = pmc_traffic_figure(names=("r06_pmc_traffic_cfg4.json", "r05_pmc_traffic_cfg4.json"))
        return {
            "kernel": "wk_kernel family (fused LSTM step GEMM, bf16 operands, fwd + bwd ticks as one launch each)",
            "bound": "hbm", "achieved": round(gbps, 1), "peak": 8000, "unit": "GB/s", "frac": round(gbps / 8000, 4),
            "traffic": traffic4, "traffic_source": traffic4_src,
            "launches_per_step": int(n), "avg_launch_us": round(us.value / n, 3),
            "alg_flops_per_launch": round(fl.value / n), "alg_bytes_per_launch": round(by.value / n),
            "alg_TFLOPs": round(ach, 2), "bf16_mfma_peak_TFLOPs": 2516.6,
            "kernel_time_ms_per_step": round(us.value * 1e-3, 3),
        }
    peak = 157.3  # f32-input MFMA peak, /opt/skills/guides/MI355X_MICROARCH.md
    # HBM-side bytes per launch come from separate rocprofv3 --pmc passes (FETCH_SIZE / WRITE_SIZE cannot share a pass
    # with the timed run); the number is the committed measurement of the session named next to it, not of this run
    traffic, traffic_src = pmc_traffic_figure(key="hbm_bytes_per_plain_launch")  # (the plain launches' own traffic)
    if p_n > 0 and p_us > 0:  # the dominant kernel: the plain step-GEMM launches (sk_kernel<2,2> / <2,1>)
        us_d, fl_d, by_d, n_d = p_us, p_fl, p_by, p_n
    else:
        us_d, fl_d, by_d, n_d = us.value, fl.value, by.value, float(n)
    ach_d = fl_d / us_d * 1e-6
    trace_us, trace_src = trace_launch_figure()
    return {
        "kernel": "sk_kernel (fused GRU gate/candidate/backward step GEMM: the plain launches, fwd + bwd)",
        "bound": "mfma", "achieved": round(ach_d, 2), "peak": peak, "unit": "TFLOP/s",
        "frac": round(ach_d / peak, 4), "frac_plain": round(ach_d / peak, 4), "frac_family": round(ach / peak, 4),
        "frac_note": "frac = frac_plain: the plain step-GEMM launches alone (the dominant kernel); frac_family: every step "
                     "launch incl. the heterogeneous ones, whose time contains the attention forward / backward chains and "
                     "whose flops do not (the reading of rounds 1-3)",
        "traffic": traffic, "traffic_source": traffic_src,
        "launches_per_step": int(n_d), "avg_launch_us": round(us_d / n_d, 3),
        "trace_avg_launch_us": trace_us, "trace_source": trace_src,
        "frac_trace": (round(fl_d / n_d / trace_us * 1e-6 / peak, 4) if trace_us else None),
        "alg_flops_per_launch": round(fl_d / n_d), "alg_bytes_per_launch": round(by_d / n_d),
        "alg_GBps": round(by_d / us_d * 1e-3, 1), "hbm_peak_GBps": 8000,
        "kernel_time_ms_per_step": round(us_d * 1e-3, 3),
        "peak_at_sustained_clock": 136.9, "frac_at_sustained_clock": round(ach_d / 136.9, 4),
        "clock_note": "the chip sustains 2.09 GHz under f32 MFMA load (profiles/r04_gemm_clock.txt): 136.9 TFLOP/s, not the data-sheet 157.3",
        "family": family,
    }


def cpu_baseline_leg(a):
    """Oracle (port of the reference equations, torch-CPU fp32, all cores): fwd + bwd + clip/Adam, BASELINE.md section 2
    protocol: the cfg2 shapes at T_dec = --cpu-T (100) timed directly -- 3 warm-ups, >= 10 iterations, median + IQR --
    and configs[0] (1-layer GRU h=256, batch 4, 50-frame windows) exactly."""
    from oracle import parrot_ref as R
    nthreads = host_cores()
    torch.set_num_threads(nthreads)

    def time_config(kw, B, U, Tc, iters, warm):
        cfg = R.default_config(**kw)
        p = R.init_params(cfg, seed=1234, dtype=torch.float32)
        p['/parrot/h1_to_att/fork_kappa.b'].fill_(a.kappa_bias)
        for v in p.values():
            v.requires_grad_()
        mom = {k: torch.zeros_like(v) for k, v in p.items()}
        var = {k: torch.zeros_like(v) for k, v in p.items()}
        g = torch.Generator().manual_seed(99)
        lab = torch.randint(0, 43, (B, U), generator=g)
        lm = torch.ones(B, U)
        feat, fm = torch.randn(Tc + 1, B, 63, generator=g), torch.ones(Tc + 1, B)
        times = []
        for it in range(warm + iters):
            t0 = time.perf_counter()
            for v in p.values():
                v.grad = None
            cost, _, _, _ = R.compute_cost(p, cfg, feat, fm, lab, lm, None, 1)
            cost.backward()
            with torch.no_grad():
                R.clip_adam_step({k: v.data for k, v in p.items()}, {k: v.grad for k, v in p.items()}, mom, var, it + 1)
            if it >= warm:
                times.append(time.perf_counter() - t0)
        times.sort()
        n = len(times)
        med = times[n // 2] if n % 2 else 0.5 * (times[n // 2 - 1] + times[n // 2])
        q1, q3 = times[n // 4], times[(3 * n) // 4]
        return dict(frames_per_s=round(B * Tc / med, 1), median_s=round(med, 4), iqr_s=round(q3 - q1, 4), iters=n,
                    cpu_work_s=round(sum(times), 1))

    t_all = time.time()
    main = time_config(model_kwargs(a), a.B, a.U, a.cpu_T, a.cpu_iters, 3)
    cfg1 = time_config(dict(num_layers=1, rnn_h_dim=256, readouts_dim=256, encoder_type='bidirectional'), 4, 15, 50,
                       a.cpu_iters, 3)
    return {"value": main["frames_per_s"], "unit": "frames/s", "cores": nthreads, "kind": "port",
            "median_s": main["median_s"], "iqr_s": main["iqr_s"], "iters": main["iters"],
            "configs0": {"frames_per_s": cfg1["frames_per_s"], "median_s": cfg1["median_s"], "iqr_s": cfg1["iqr_s"],
                         "workload": "BASELINE configs[0]: 1-layer GRU h=256, batch 4, 50-frame windows, T_enc=15"},
            "sample": f"{main['iters']} training steps (after 3 warm-ups) of the cfg2 shapes (L={a.L}, H={a.H}, B={a.B}, "
                      f"T_enc={a.U}) at T_dec={a.cpu_T}, timed directly, median + IQR ({time.time() - t_all:.0f} s of CPU "
                      f"work incl. configs[0]); the per-window costs (encoder, optimiser) are amortised over {a.cpu_T} "
                      f"instead of {a.T} frames, which understates the CPU rate at T_dec={a.T} by a few percent; "
                      f"oracle/parrot_ref.py (torch-CPU fp32, autograd backward, clip+Adam), {nthreads} threads"}


def parity_leg(a):
    """The HIP training step against the fp64 oracle ON THE CPU-BASELINE LEG'S OWN BATCH (the cfg2 shapes at T_dec =
    --cpu-T, seed 99, the same initialisation): relative errors of the cost, the predicted frames, kappa and the worst
    parameter gradient.  The oracle is the checker here, never the thing timed or shipped."""
    from oracle import parrot_ref as R
    from parrot_amd.model import Parrot
    torch.set_num_threads(host_cores())
    dev = torch.device("cuda", 0)
    kw = model_kwargs(a)
    cfg = R.default_config(**kw)
    p = R.init_params(cfg, seed=1234)  # float64
    p['/parrot/h1_to_att/fork_kappa.b'].fill_(a.kappa_bias)
    g = torch.Generator().manual_seed(99)
    lab = torch.randint(0, 43, (a.B, a.U), generator=g)
    lm = torch.ones(a.B, a.U, dtype=torch.float64)
    feat = torch.randn(a.cpu_T + 1, a.B, 63, generator=g).double()
    fm = torch.ones(a.cpu_T + 1, a.B, dtype=torch.float64)
    m = Parrot(device=dev, use_graph=True, compute_dtype='bf16' if a.dtype == 'bf16' else 'float32', **kw).allocate()
    m.set_parameter_values(p)
    m.zero_grad()
    cost, _, av, _ = m.compute_cost(feat.float().to(dev), fm.float().to(dev), lab.to(dev), lm.float().to(dev), None, 1, a.B)
    cost.backward()
    grads = m.get_gradient_dict()
    for v in p.values():
        v.requires_grad_()
    rc, rav = R.cost_and_grads_checkpointed(p, cfg, feat, fm, lab, lm, None, chunk=50)

    def rel(x, y):
        x, y = torch.as_tensor(x).detach().double().cpu(), torch.as_tensor(y).detach().double().cpu()
        return float((x - y).abs().max() / y.abs().max())
    worst = ("", 0.0)
    for name, ref in p.items():
        if ref.grad is None or float(ref.grad.abs().max()) < 1e-12:
            continue
        e = rel(grads[name], ref.grad)
        if e > worst[1]:
            worst = (name, e)
    m.close()
    out = {"against": "oracle/parrot_ref.py in float64 (checkpointed BPTT)", "T_dec": a.cpu_T, "batch": a.B,
           "cost_hip": float(cost), "cost_oracle": float(rc),
           "cost_rel_err": abs(float(cost) - float(rc)) / abs(float(rc)),
           "frames_rel_err": rel(av[0], rav[0]), "kappa_rel_err": rel(av[1], rav[1]),
           "grad_rel_err_max": worst[1], "grad_worst": worst[0],
           "norm": "max|hip - oracle| / max|oracle| per tensor"}
    if a.dtype != "f32" or a.config != "cfg2":
        return out
    # ---- the `secondary` figures' own parity: every number of the line has its check beside it
    try:  # BASELINE configs[2]: 100 decode steps of the benchmarked decode configuration vs the float64 oracle
        kw3 = dict(num_layers=2, encoder_type='bidirectional', rnn_h_dim=1024, readouts_dim=1024, weak_feedback=True)
        cfg3 = R.default_config(**kw3)
        p3 = R.init_params(cfg3, seed=29, scale_by_fan_in=True)
        p3['/parrot/h1_to_att/fork_kappa.b'].fill_(-2.3)
        N3, U3, S3 = 16, 100, 100
        g3 = torch.Generator().manual_seed(31)
        lab3 = torch.randint(0, 43, (N3, U3), generator=g3)
        lm3 = torch.ones(N3, U3, dtype=torch.float64)
        m3 = Parrot(device=dev, use_graph=True, **kw3).allocate()
        m3.set_parameter_values(p3)
        with torch.no_grad():
            ref3 = R.sample_model(p3, cfg3, lab3, lm3, None, S3)
        outs3 = m3.sample_model(lab3.numpy(), lm3.float().numpy(), None, None, N3, S3)
        from parrot_amd import _lib as _plib
        kind = int(_plib.load().parrot_sample_is_persistent(next(iter(m3._sample_ws.values()))['plan']))
        m3.close()
        errs = {n: rel(torch.from_numpy(o), r) for o, r, n in zip(outs3, ref3, ("sample_x", "k", "w", "pi", "phi", "pi_att"))}
        out["decode_cfg3"] = {"against": "oracle/parrot_ref.py sample_model in float64", "steps": S3, "batch": N3, "T_enc": U3,
                              "plan_kind": kind, "rel_err": {k: float(v) for k, v in errs.items()},
                              "worst": max(errs.values()), "tolerance": 1e-4}
    except Exception as e:
        out["decode_cfg3"] = {"error": repr(e)[:300]}
    try:  # BASELINE configs[4]: 160 greedy samples per stream (two big frames) at the benchmarked widths vs the float64 oracle
        import numpy as np
        from oracle import samplernn_ref as S
        from parrot_amd.sampleRNN import lib
        from parrot_amd.sampleRNN.models.conditional import three_tier as tt
        lib.delete_all_params(); lib.set_device(dev)
        tt.configure(DIM=1024, EMB_SIZE=256, RNN_TYPE='GRU', N_RNN=1)
        c5 = S.config()
        p5 = S.init_params(c5, seed=5, perturb=0.2)
        lib.set_params(p5)
        B5, T5 = 32, 3
        g5 = torch.Generator().manual_seed(2)
        feats5 = torch.randn(T5, B5, 63, generator=g5, dtype=torch.float64)
        with torch.no_grad():
            ref5, ref_logits = S.generate(p5, c5, feats5, return_logits=True)
        gen = tt.DeviceGenerator(B5, T5, temperature=0.0, use_graph=True)
        out5 = gen.generate(feats5.float().numpy()).cpu().numpy()
        gen.close()
        lib.delete_all_params()
        ref5 = ref5.numpy()
        exact, ties = 0, 0
        for b in range(B5):
            diff = np.nonzero(out5[b] != ref5[b])[0]
            if diff.size == 0:
                exact += 1
                continue
            lg = ref_logits[b, int(diff[0]) - 80]
            top2 = torch.topk(lg, 2).values
            ties += int(float(top2[0] - top2[1]) < 2e-5 * float(lg.abs().max()))
        out["samplernn_cfg5"] = {"against": "oracle/samplernn_ref.py generate in float64 (greedy)", "streams": B5,
                                 "samples_per_stream": int(out5.shape[1]) - 80, "rows_bit_exact": exact,
                                 "rows_left_at_an_oracle_tie": ties, "rows_wrong": B5 - exact - ties,
                                 "criterion": "sample indices bit-exact; a row may leave the oracle only where the oracle's own "
                                              "top-2 logits tie within fp32 resolution (2e-5 of the largest logit)"}
    except Exception as e:
        out["samplernn_cfg5"] = {"error": repr(e)[:300]}
    return out


def secondary_leg(a):
    """BASELINE configs[2] (decode latency) and configs[4] (SampleRNN sample loop) on the device, a few seconds each,
    each against its own algorithmic-bytes roofline (58.5 MB of weights per decode step, 27.4 MB per
    SampleRNN sample step; HBM peak 8 TB/s)."""
    import numpy  # noqa: F401
    dev = torch.device("cuda", 0)
    out = {}
    from parrot_amd.model import Parrot
    m = Parrot(device=dev, num_layers=2, rnn_h_dim=1024, readouts_dim=1024, encoder_type='bidirectional',
               weak_feedback=True, use_graph=True).initialize()
    g = torch.Generator().manual_seed(0)
    N, U, S = 16, 100, 1000
    lab, lm = torch.randint(0, 43, (N, U), generator=g), torch.ones(N, U)
    best = None
    for rep in range(4):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        m.sample_model_device(lab, lm, None, N, S)
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
        if rep > 0:
            best = dt if best is None else min(best, dt)
    from parrot_amd import _lib as _plib
    kind = int(_plib.load().parrot_sample_is_persistent(next(iter(m._sample_ws.values()))['plan']))
    m.close()
    alg = 58.5e6
    cb, cb_src = pmc_secondary_figure("decode_cfg3")
    out["decode_cfg3"] = {"workload": "BASELINE configs[2]: greedy decode, batch 16, 1000 frames, 2-layer GRU h=1024, feedback on",
                          "us_per_step": round(1e6 * best / S, 2), "frames_per_s": round(N * S / best, 1),
                          "counter_bytes_per_step": cb, "counter_source": cb_src,
                          "frac_counter": (round(cb * S / best / 8e12, 4) if cb else None),
                          "frac": (round(cb * S / best / 8e12, 4) if cb else None),
                          "frac_note": "frac = frac_counter: HBM-side bytes the resident kernel actually moves per step (committed "
                                       "counter passes) / time / 8 TB/s; frac_ref_formulation divides SURVEY 8d's 58.5 MB of the "
                                       "reference's formulation, which the plan no longer reads (composed weights, stationary slabs)",
                          "alg_bytes_per_step_ref_formulation": int(alg), "alg_GBps_ref_formulation": round(alg * S / best * 1e-9, 1),
                          "frac_ref_formulation": round(alg * S / best / 8e12, 4), "bound": "hbm", "peak_GBps": 8000,
                          "plan": {3: "resident kernel, 5 phases per step (products cut along K by operand age, "
                                      "readout.output composed, the fed-back frame out of the chain: x = x_pre + h_last.A)",
                                   2: "resident kernel, 6 phases per step (products cut along K by operand age, "
                                      "readout.output composed)",
                                   1: "resident kernel, 7 whole-K phases per step", 0: "per-step launches"}.get(kind, str(kind))}
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
    best = None
    for rep in range(6):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        gen.generate(feats)
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
        if rep > 0:
            best = dt if best is None else min(best, dt)
    gen.close()
    nsamp = (T - 1) * 80
    alg = 27.4e6
    cb, cb_src = pmc_secondary_figure("samplernn_cfg5")
    out["samplernn_cfg5"] = {"workload": "BASELINE configs[4]: 3-tier GRU h=1024, batch 32, greedy, 2000 samples per stream",
                             "us_per_sample_step": round(1e6 * best / nsamp, 2),
                             "samples_per_s": round(B * nsamp / best, 1),
                             "x_realtime_per_stream": round(nsamp / best / 16000.0, 3),
                             "counter_bytes_per_sample_step": cb, "counter_source": cb_src,
                             "frac_counter": (round(cb * nsamp / best / 8e12, 4) if cb else None),
                             "frac": (round(cb * nsamp / best / 8e12, 4) if cb else None),
                             "frac_note": "frac = frac_counter: HBM-side bytes the sample kernel moves per sample step (weights live in "
                                          "VGPRs / LDS: polls, hand-offs and the per-frame weight prologue) / time / 8 TB/s -- a latency "
                                          "chain, not a bandwidth figure; frac_ref_formulation divides SURVEY 8d's 27.4 MB of the reference's "
                                          "formulation (three sample-MLP products per sample + the tiers' share), which the kernel no longer reads",
                             "alg_bytes_per_sample_step_ref_formulation": int(alg),
                             "alg_GBps_ref_formulation": round(alg * nsamp / best * 1e-9, 1),
                             "frac_ref_formulation": round(alg * nsamp / best / 8e12, 4), "bound": "hbm", "peak_GBps": 8000}
    # ---- SampleRNN TRAINING (three_tier.py:534-636): one truncated-BPTT window, forward + backward of cost + ip_cost
    try:
        S = 4000
        gs = torch.Generator().manual_seed(1)
        seq = torch.randint(0, 256, (B, S + 80), generator=gs).to(dev)
        feats_t = torch.randn(B, S // 80, 63, generator=gs).to(dev)
        h0 = torch.zeros(B, 1, 1024, device=dev)
        mask = torch.ones(B, S + 80, device=dev)

        def train_step():
            cost, ip_cost, params = tt.compute_cost(seq, feats_t, h0, h0, 1, mask)[:3]
            for p_ in params:
                p_.grad = None
            (cost + ip_cost).backward()
            return float(cost)
        best = None
        for rep in range(3):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            c_ = train_step()
            torch.cuda.synchronize(); dt = time.perf_counter() - t0
            if rep > 0:
                best = dt if best is None else min(best, dt)
        rows = B * S
        mlp = 2.0 * rows * (2560 * 1024 + 2 * 1024 * 1024 + 1024 * 256)  # sample-level MLP, forward (three_tier.py:452-515)
        ip = 2.0 * B * (S // 80) * 1024 * (256 * 80)                      # IndependentPreds projection
        out["samplernn_train"] = {"workload": "configs[4] training window: 3-tier GRU h=1024, batch 32, SEQ_LEN 4000, "
                                              "cost + ip_cost forward + backward (no optimiser)",
                                  "ms_per_window": round(1e3 * best, 2), "samples_per_s": round(rows / best, 1),
                                  "cost_bits": round(c_, 4),
                                  "mlp_fwd_TFLOP": round(mlp * 1e-12, 3),
                                  "executed_TFLOPs": round(3.0 * (mlp - 2.0 * rows * 2560 * 1024 + ip) / best * 1e-12, 1),
                                  "ref_formulation_TFLOPs": round(3.0 * (mlp + ip) / best * 1e-12, 1),
                                  "gemm_mode": gemm_mode_name(),
                                  "note": "frac = executed_TFLOPs / 157.3 (the f32-input MFMA roof; in bf16x3 mode the products "
                                          "run on the bf16 pipe at six MFMAs per block, so the same roof is the honest "
                                          "f32-equivalent yardstick): 3 x the forward flops of the products that still run "
                                          "(sample-MLP L2 / L3 / Output + IndependentPreds).  frac_ref_formulation also counts the "
                                          "K = 2560 product behind the Embedding (three_tier.py:452-515), which since round 5 is a "
                                          "gather-sum / segmented sum over the folded table (parrot_gather_sum_*) and no longer runs",
                                  "frac": round(3.0 * (mlp - 2.0 * rows * 2560 * 1024 + ip) / best * 1e-12 / 157.3, 4),
                                  "frac_ref_formulation": round(3.0 * (mlp + ip) / best * 1e-12 / 157.3, 4), "bound": "mfma",
                                  "peak_TFLOPs": 157.3}
    except Exception as e:  # a secondary figure must never take the headline line down with it
        out["samplernn_train"] = {"error": repr(e)[:300]}
    return out


def child_json(a, flag, extra=(), timeout=420):
    """Runs `bench.py <flag>` in a child process (own HIP context, hard wall-clock limit) and returns its JSON line."""
    import subprocess
    cmd = [sys.executable, os.path.abspath(__file__), flag, "--T", str(a.T), "--B", str(a.B), "--U", str(a.U),
           "--H", str(a.H), "--L", str(a.L), "--cell", a.cell, "--dtype", a.dtype, "--cpu-T", str(a.cpu_T),
           "--kappa-bias", str(a.kappa_bias)] + list(extra)
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
        for line in reversed(r.stdout.strip().splitlines()):
            if line.startswith("{"):
                return json.loads(line)
        return {"error": (r.stderr or r.stdout)[-300:]}
    except subprocess.TimeoutExpired:
        return {"error": f"exceeded its {timeout} s limit"}


def secondary_subprocess(a):
    sec = child_json(a, "--secondary-only", timeout=300)
    if a.config == "cfg2":  # BASELINE configs[3] per GPU (the 8-GPU line's workload), bf16 operands
        d = child_json(a, "--full", ["--no-secondary", "--config", "cfg4", "--no-cpu-baseline", "--no-dense", "--no-f32-gemm",
                                     "--no-parity", "--steps", "3", "--warmup", "1", "--L", "3", "--H", "1536",
                                     "--cell", "lstm", "--dtype", "bf16"], timeout=420)
        sec["cfg4_bf16"] = ({"workload": d["config"]["workload"], "ms_per_step": d["ms_per_step"],
                             "frames_per_s": d["value"], "roofline": d.get("roofline")}
                            if "ms_per_step" in d else d)
        # the reference's own decoder depth (model.py:312-347: three GatedRecurrent layers, h = 1024), literal batch-axis
        # encoder, fp32: the one instance where "the reference's model" is literally defined
        d = child_json(a, "--full", ["--no-secondary", "--L", "3", "--H", "1024", "--cell", "gru", "--dtype", "f32",
                                     "--no-cpu-baseline", "--no-dense", "--no-f32-gemm", "--no-parity", "--steps", "3",
                                     "--warmup", "1"], timeout=420)
        if "ms_per_step" in d:
            fwd_bytes = 99.9e6  # 21.26 M weights per decoder timestep, forward
            sec["ref_literal_3gru"] = {
                "workload": "reference-literal decoder: 3 x GRU h=1024 + attention, batch 64, T_enc 200, T_dec 800, fp32, "
                            "encoder_literal=True (train fwd+bwd+clip/Adam)",
                "ms_per_step": d["ms_per_step"], "frames_per_s": d["value"], "roofline": d.get("roofline"),
                "alg_bytes_per_step_fwd": int(fwd_bytes),
                "hbm_frac_weights_fwd_plus_bwd": round(2.0 * fwd_bytes * a.T / (d["ms_per_step"] * 1e-3) / 8e12, 4)}
        else:
            sec["ref_literal_3gru"] = d
    return sec


def cpu_baseline_subprocess(a):
    """Runs the CPU leg in a child process with a hard wall-clock limit so a mis-sized thread pool can
    never stall the GPU job."""
    import subprocess
    cmd = [sys.executable, os.path.abspath(__file__), "--cpu-baseline-only", "--T", str(a.T), "--B", str(a.B),
           "--U", str(a.U), "--H", str(a.H), "--L", str(a.L), "--cell", a.cell, "--cpu-T", str(a.cpu_T), "--cpu-iters", str(a.cpu_iters),
           "--kappa-bias", str(a.kappa_bias)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        for line in reversed(r.stdout.strip().splitlines()):
            if line.startswith("{"):
                return json.loads(line)
        return {"value": None, "unit": "frames/s", "cores": host_cores(), "kind": "port",
                "sample": "cpu leg produced no result: " + r.stderr[-200:]}
    except subprocess.TimeoutExpired:
        return {"value": None, "unit": "frames/s", "cores": host_cores(), "kind": "port",
                "sample": "cpu leg exceeded its 300 s limit"}


def self_launch(a):
    """`python bench.py --gpus N` with N > 1 outside torchrun: start the N ranks ourselves (one process per GPU, the
    same command line under torch.distributed.run on 127.0.0.1) and hand back their exit code.  Rank 0's JSON line goes
    to our stdout unchanged."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # the host driver only supports dmabuf IPC (RCCL needs it)
    env.setdefault("OMP_NUM_THREADS", str(max(1, host_cores() // a.gpus)))
    return subprocess.call(cmd, env=env)


def ranks_seen(dev):
    """All-reduce of ones: how many ranks the collective really spans (1 outside a process group)."""
    from parrot_amd import dist as pdist
    t = torch.ones(1, device=dev, dtype=torch.float32)
    if pdist.is_distributed():
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.SUM)
    return int(round(float(t)))


def allreduce_ms(flat_groups, dev, reps=5):
    """The gradient exchange alone: median wall time of the sum-all-reduce of the flat gradient bucket(s), as
    Trainer.step issues it (blocking, on the compute stream), bracketed by barrier + synchronize; max over ranks."""
    from parrot_amd import dist as pdist
    if not pdist.is_distributed():
        return None
    times = []
    for rep in range(reps + 1):
        pdist.barrier()
        if dev.type == "cuda":
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        for g_ in flat_groups:
            pdist.allreduce_flat_(g_)
        if dev.type == "cuda":
            torch.cuda.synchronize()
        t = torch.tensor([time.perf_counter() - t0], device=dev, dtype=torch.float64)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        if rep > 0:
            times.append(float(t))
    times.sort()
    return round(1e3 * times[len(times) // 2], 3)


def plumbing_only(a):
    """The N > 1 control flow without a GPU step: process group, ranks_seen, the timed bucket all-reduce, one line."""
    from parrot_amd import dist as pdist
    rank, local_rank, world = pdist.init_process_group()
    assert world == a.gpus, f"--gpus {a.gpus} but WORLD_SIZE={world}"
    dev = torch.device("cpu")
    seen = ranks_seen(dev)
    bucket = torch.full((1 << 16,), float(rank + 1), dtype=torch.float32)
    ar = allreduce_ms([bucket], dev, reps=2)
    pdist.barrier()
    if rank == 0:
        print(json.dumps({"metric": "plumbing only (no GPU step)", "value": None, "n_gpus": world, "ranks_seen": seen,
                          "allreduce_ms": ar, "steps": a.steps, "warmup": a.warmup, "plumbing_only": True}), flush=True)
    if world > 1:
        torch.distributed.destroy_process_group()


def main():
    a = parse()
    torch.set_num_threads(host_cores())
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(a))
    if a.plumbing_only:
        plumbing_only(a)
        return
    if a.cpu_baseline_only:
        print(json.dumps(cpu_baseline_leg(a)), flush=True)
        return
    if a.secondary_only:
        print(json.dumps(secondary_leg(a)), flush=True)
        return
    if a.parity_only:
        print(json.dumps(parity_leg(a)), flush=True)
        return
    from parrot_amd import dist as pdist
    rank, local_rank, world = pdist.init_process_group()
    assert world == a.gpus, f"--gpus {a.gpus} but WORLD_SIZE={world}"
    assert torch.cuda.is_available(), "bench.py needs a GPU"
    # (ranks wrap around the visible devices only in the gloo plumbing test, PARROT_DIST_BACKEND=gloo)
    dev = torch.device("cuda", (local_rank % torch.cuda.device_count()) if world > 1 else 0)
    torch.cuda.set_device(dev)

    from parrot_amd.trainer import Trainer

    model = build_model(a, dev)
    trainer = Trainer(model)
    batch = make_batch(a, dev, 1234 + rank)

    def timed(steps, warmup):
        for _ in range(warmup):
            trainer.step(*batch, None, 1)
        pdist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            c = trainer.step(*batch, None, 1)
        torch.cuda.synchronize()
        pdist.barrier()
        t = torch.tensor([time.perf_counter() - t0], device=dev, dtype=torch.float64)
        if world > 1:
            torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        return float(t), c

    el, cost = timed(a.steps, a.warmup)
    final_cost = float(cost)
    if a.dump_outputs and rank == 0:  # before the --full runs below step the same model further
        dump_outputs(a.dump_outputs, cost, model, a.B)
    seen = ranks_seen(dev)
    ar_ms = allreduce_ms([g_ for _, g_ in trainer.groups], dev) if a.full else None
    try:  # the launch schedule the plan actually ran (after the library's fall-backs)
        from parrot_amd import _lib
        sched_id = int(_lib.load().parrot_decoder_schedule(next(iter(model._train_ws.values()))['plan']))
    except Exception:
        sched_id = None
    sched_names = {0: "0 (merged wavefront launches)", 2: "2 (chunked layer pipeline)", 3: "3 (chunk-skewed wavefront)",
                   5: "5 (balanced wavefront: attention + upper layers' input projections in one heterogeneous launch)",
                   6: "6 (attention inside the gate launch, in-launch hand-off)",
                   7: "7 (LSTM: one launch per tick, the attention at its head, layer 0's w rows behind an in-launch flag)"}
    kappa_end = float(model._carry[a.B]['k'].mean()) if a.B in model._carry else None
    # extra timed run, outside the headline region: the batched products (readouts, deferred weight gradients) on the
    # f32-input matrix instructions instead of the split-bf16 kernel (the same f32 operands, f32-grade results either way)
    from parrot_amd import ops as pops
    gemm_mode = gemm_mode_name()
    if a.dtype == "bf16":
        gemm_mode = "bf16 operands (bf16-in kernels)"
    f32run = None
    if a.full and not a.no_f32_gemm and a.dtype == "f32" and pops.full_precision() == pops.PRECISION_BF16X3:
        prev_mode = pops.set_full_precision(pops.PRECISION_F32)
        el_f, _ = timed(a.steps, 1)
        pops.set_full_precision(prev_mode)
        f32run = {"value": round(world * a.B * a.T * a.steps / el_f, 1), "ms_per_step": round(1e3 * el_f / a.steps, 3)}
    # second timed run, outside the headline region: the attention kernels read ALL context rows (no window support)
    dense = None
    if a.full and not a.no_dense and os.environ.get("PARROT_ATT_DENSE", "0") in ("", "0"):
        os.environ["PARROT_ATT_DENSE"] = "1"
        model.close()  # plans read the switch when they are built
        el_d, _ = timed(a.steps, 1)
        os.environ["PARROT_ATT_DENSE"] = "0"
        dense = {"value": round(world * a.B * a.T * a.steps / el_d, 1), "ms_per_step": round(1e3 * el_d / a.steps, 3)}
        model.close()

    roof = cpu = parity = secondary = None
    if a.full and rank == 0:
        if not a.no_roofline:
            roof = roofline_leg(a, dev, model.flat_parameters)
    model.close()
    if a.full and rank == 0 and world == 1:
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        if not a.no_cpu_baseline:
            cpu = cpu_baseline_subprocess(a)
        if not a.no_parity:
            parity = child_json(a, "--parity-only", timeout=480)
        if not a.no_secondary:
            secondary = secondary_subprocess(a)
    if world > 1:
        pdist.barrier()
    if rank == 0:
        frames = world * a.B * a.T * a.steps
        out = {
            "metric": "acoustic feature frames/sec (train fwd+bwd+allreduce+clip/Adam)",
            "value": round(frames / el, 1), "unit": "frames/s", "n_gpus": world, "ranks_seen": seen,
            "allreduce_ms": ar_ms, "allreduce_bytes": int(sum(g_.numel() * 4 for _, g_ in trainer.groups)),
            "steps": a.steps,
            "warmup": a.warmup, "ms_per_step": round(1e3 * el / a.steps, 3), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": a.dtype, "data": "synthetic",
            "config": {"workload": ("BASELINE configs[3] per GPU: 3-layer attention-LSTM decoder, h=1536, batch=64 per GPU "
                                    "(global 512 on 8 GPUs), T_enc=200, T_dec=800, bf16 MFMA operands / f32 accumulate / "
                                    "f32 master weights" if a.config == "cfg4" else
                                    "BASELINE configs[1]: 2-layer attention-GRU decoder, h=1024, "
                                    "batch=64 per GPU, T_enc=200, T_dec=800, fp32"),
                       "cell": a.cell,
                       "layers": a.L, "hidden": a.H, "batch_per_gpu": a.B, "global_batch": a.B * world,
                       "T_enc": a.U, "T_dec": a.T, "parallelism": f"dp{world}",
                       "params": int(model.store.numel),
                       "init": f"train.py:30-31 (N(0,0.01) weights, zero biases) with the kappa bias at {a.kappa_bias}: the "
                               f"window ends the 800 frames at mean position {kappa_end and round(kappa_end, 1)} of "
                               f"{a.U}, i.e. inside the text, as for a trained model",
                       "attention_rows": ("all U context rows (PARROT_ATT_DENSE=1)"
                                          if os.environ.get("PARROT_ATT_DENSE", "0") not in ("", "0") else
                                          "support: rows whose window weight phi is exactly 0.0f are not read "
                                          "(bit-identical results); `dense` = the same step reading all rows"),
                       "scan_schedule": sched_names.get(sched_id, str(sched_id))},
            "dense": dense,
            "gemm_mode": gemm_mode,
            "value_f32_mfma": f32run and f32run["value"], "ms_per_step_f32_mfma": f32run and f32run["ms_per_step"],
            "final_cost": round(final_cost, 5),
            "roofline": roof, "cpu_baseline": cpu, "parity_check": parity, "secondary": secondary,
        }
        print(json.dumps(out), flush=True)
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()

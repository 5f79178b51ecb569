"""The cases of the step-kernel launch-mode tests: which job descriptor a workgroup picks (grid.z = job, or the prefix table
along x) and which epilogue fields it then sees.

The step kernels (sk_kernel, ska_kernel, skb_kernel of skinny.hip) are driven through the C ABI and the decoder entry
points only.  Every family runs at H = 48 (three 16-column tiles: not a multiple of the 32-column workgroup), E = 16,
U = 7, T = 4 and B in (5, 33, 64): a ragged single row block, two row blocks with a ragged second one, and full ones.

  family      entry point                                  launches it reaches
  linear      parrot_gemm (M <= 64)                        z-mode, grid.z = 1: LINEAR without / with bias, accumulate, relu,
                                                           tanh, sigmoid; K = 63: the generic one-tile path
  gru_step    parrot_gru_step_fwd / _bwd                   z-mode, grid.z = 1: GRU gates, candidate (with o1, with and without a
                                                           step mask, both with the additive input), BWD_RH
  gru_seq     parrot_gru_seq_* on the launch path          1, 2 and 4 chains of one width: z-mode with grid.z = 1, 2, 4
  lstm_seq    parrot_lstm_seq_*                            z-mode, grid.z = 1: the LSTM cell
  dec_*       Parrot.compute_cost + backward               the decoder's plans: z-mode launches with grid.z = layers, prefix-mode
                                                           launches of 2 jobs up to the most a plan makes (three GRU layers on
                                                           schedule 5 with the K-balanced backward tick), ska_kernel / skb_kernel
                                                           beside the attention and state row blocks, LINEAR with the additive
                                                           input, LSTM cell and gate-ordered LINEAR jobs in prefix mode;
                                                           dec_lstm2_s7: the flagged last segment of ska_kernel
  sample_gru2 Parrot.sample_model, launch path             the GRU candidate without o1, LINEAR with bias and additive input

`run(family, B, dev)` returns (written, refs): every buffer the launches wrote (host tensors, in a fixed order) and, for the
buffers a float64 restatement exists for, (reference, tolerance) with the tolerance the neighbouring test file uses for the
same kernel.  tests/golden/step_launch_modes.json holds the SHA-256 of every written buffer as the parent of the commit
that introduced this file computed it, tests/golden/step_launch_modes_b5.npz the arrays themselves for the B = 5 runs of
the C-ABI families (tools/record_step_launch_golden.py writes both).  The kernels are atomic-free and deterministic, so
the comparison is equality of bits."""
import contextlib
import ctypes as C
import hashlib
import json
import math
import os
from collections import OrderedDict

import numpy as np
import torch

from tests import gemm_cases as GC
from tests import gru_scan_cases as GS

H, E, U, T = 48, 16, 7, 4
BS = (5, 33, 64)
FAMILIES = ("linear", "gru_step", "gru_seq", "lstm_seq", "dec_gru1", "dec_gru2", "dec_gru3", "dec_lstm2", "dec_lstm2_s7",
            "sample_gru2")
ARRAY_FAMILIES = ("linear", "gru_step", "lstm_seq")  # stored as arrays at B = 5, besides their digests

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN_JSON = os.path.join(GOLDEN_DIR, "step_launch_modes.json")
GOLDEN_NPZ = os.path.join(GOLDEN_DIR, "step_launch_modes_b5.npz")

SWITCHES = ("PARROT_SCHEDULE", "PARROT_WK", "PARROT_BWD_HETERO", "PARROT_CHUNK", "PARROT_S5_WSTEP", "PARROT_GRU_ROWWISE",
            "PARROT_SAMPLE_PERSIST", "PARROT_ATT_DENSE")


def case_id(family, B):
    return "%s-B%d" % (family, B)


@contextlib.contextmanager
def switches(**values):
    """Every switch that picks a launch path unset, except the ones given; restored afterwards."""
    old = {k: os.environ.get(k) for k in SWITCHES}
    try:
        for k in SWITCHES:
            os.environ.pop(k, None)
        for k, v in values.items():
            os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ---- the host's layout of a launch ------------------------------------------------------------------------------------------
def launch_mode(jobs):
    """parrot_step_launch_mode for jobs = [(M, N, K) or (M, N, K, lstm_H), ...]: dict(zmode, mb, nb, grid, ends)."""
    from parrot_amd import _lib
    n = len(jobs)
    arr = lambda i: (C.c_int * n)(*[(j[i] if len(j) > i else 0) for j in jobs])
    info = (C.c_int * (5 + n))()
    _lib.call("parrot_step_launch_mode", n, arr(0), arr(1), arr(2), arr(3), info)
    return dict(zmode=bool(info[0]), mb=info[1] // 10, nb=info[1] % 10, grid=(info[2], info[3], info[4]),
                ends=[info[5 + q] for q in range(n)])


def expected_mode(jobs):
    """The rule of sk_prepare restated: with the tile shape the host picked, z-mode iff every job has the same number of
    workgroups; then grid = (that number, row blocks, jobs), else (the sum, row blocks, 1) with the prefix of workgroups."""
    got = launch_mode(jobs)
    nb, mb = got["nb"], got["mb"]
    wgs = [-(-(j[3] // 4 if len(j) > 3 and j[3] else -(-j[1] // 16)) // nb) for j in jobs]
    rows = -(-max(j[0] for j in jobs) // (16 * mb))
    ends = [sum(wgs[:q + 1]) for q in range(len(jobs))]
    if len(set(wgs)) == 1:
        return dict(zmode=True, mb=mb, nb=nb, grid=(wgs[0], rows, len(jobs)), ends=ends)
    return dict(zmode=False, mb=mb, nb=nb, grid=(ends[-1], rows, 1), ends=ends)


def plan_launches(plan, which):
    """parrot_decoder_trace_jobs of a decoder plan: {launch index: [(M, N, K, epilogue code), ...]} for the forward (0) or
    the backward (1) scan; epilogue -1 / -2 = the attention forward / backward row blocks of a heterogeneous launch."""
    from parrot_amd import _lib
    lib = _lib.load()
    n = lib.parrot_decoder_trace_jobs(plan, which, None, 0)
    assert n > 0, n
    buf = (C.c_longlong * (6 * n))()
    assert lib.parrot_decoder_trace_jobs(plan, which, buf, n) == n
    out = OrderedDict()
    for i in range(n):
        launch, _, M, N, K, epi = buf[6 * i:6 * i + 6]
        out.setdefault(int(launch), []).append((int(M), int(N), int(K), int(epi)))
    return out


def plan_modes(plan):
    """The launch kinds of a decoder plan's two scans: set of (kernel, z-mode, step-GEMM jobs) with kernel "sk" (plain), "ska" /
    "skb" (the launch carries attention forward / backward row blocks: always the prefix table)."""
    kinds = set()
    for which in (0, 1):
        for jobs in plan_launches(plan, which).values():
            gemm = [j for j in jobs if j[3] >= 0]
            if not gemm:
                continue
            hetero = [j[3] for j in jobs if j[3] < 0]
            if hetero:
                kinds.add(("ska" if -1 in hetero else "skb", False, len(gemm)))
            else:
                mode = launch_mode([(M, N, K, N // 4 if epi == 4 else 0) for M, N, K, epi in gemm])
                kinds.add(("sk", mode["zmode"], len(gemm)))
    return kinds


# ---- golden ---------------------------------------------------------------------------------------------------------------
def digest(t):
    a = np.ascontiguousarray(t.detach().cpu().numpy())
    return dict(sha256=hashlib.sha256(a.tobytes()).hexdigest(), shape=list(a.shape), dtype=str(a.dtype))


def load_golden():
    with open(GOLDEN_JSON) as f:
        digests = json.load(f)
    return digests, np.load(GOLDEN_NPZ)


def check_golden(cid, written, golden):
    """Every written buffer bit for bit what the recorded build wrote; returns the list of differences."""
    digests, arrays = golden
    want = digests[cid]
    bad = []
    if list(written) != list(want):
        return ["buffers %s, recorded %s" % (list(written), list(want))]
    for name, t in written.items():
        key = cid + "/" + name
        if key in arrays.files:
            a, b = np.ascontiguousarray(t.numpy()), arrays[key]
            if a.shape != b.shape or a.dtype != b.dtype:
                bad.append("%s: %s %s, recorded %s %s" % (name, a.dtype, a.shape, b.dtype, b.shape))
                continue
            ne = a.view(np.uint8).reshape(-1) != b.view(np.uint8).reshape(-1)
            if ne.any():
                first = int(np.flatnonzero(ne)[0]) // a.itemsize
                bad.append("%s: %d bytes differ, first at element %d: %r, recorded %r" % (
                    name, int(ne.sum()), first, a.reshape(-1)[first], b.reshape(-1)[first]))
        if digest(t) != want[name]:
            bad.append("%s: %s, recorded %s" % (name, digest(t), want[name]))
    return bad


# ---- families ---------------------------------------------------------------------------------------------------------------
def _gen(*key):
    return GS._gen("step_launch", *key)


def _host(t):
    return t.detach().cpu().clone()


LINEAR_VARIANTS = (  # name, K, bias, accumulate, activation
    ("plain", 64, False, False, GC.NONE), ("bias", 64, True, False, GC.NONE), ("bias-acc", 64, True, True, GC.NONE),
    ("acc", 64, False, True, GC.NONE), ("bias-relu", 64, True, False, GC.RELU), ("bias-tanh", 64, True, False, GC.TANH),
    ("sigmoid", 64, False, False, GC.SIGMOID), ("generic-K63-bias", 63, True, False, GC.NONE))


def run_linear(B, dev):
    from parrot_amd import ops
    written, refs = OrderedDict(), {}
    for name, K, bias, acc, act in LINEAR_VARIANTS:
        g = _gen("linear", B, K)
        a = (torch.randn(B, K, generator=g, dtype=torch.float64) / math.sqrt(K)).float()
        b = torch.randn(K, H, generator=g, dtype=torch.float64).float()
        bv = torch.randn(H, generator=g, dtype=torch.float64).float()
        c0 = torch.randn(B, H, generator=g, dtype=torch.float64).float()
        ad, bd, out = a.to(dev), b.to(dev), (c0.clone() if acc else torch.full((B, H), float("nan"))).to(dev)
        kw = dict(bias=bv.to(dev) if bias else None, out=out, accumulate=acc, act=act)
        assert ops.gemm_route(ad, bd, **kw) == (ops.ROUTE_STEP, 1), name
        ops.gemm(ad, bd, **kw)
        mode = launch_mode([(B, H, K)])
        assert mode["zmode"] and mode["grid"][2] == 1 and (K % 16 == 0 or mode["nb"] == 1), (name, mode)
        v = a.double() @ b.double() + (bv.double() if bias else 0.0) + (c0.double() if acc else 0.0)
        v = {GC.NONE: v, GC.RELU: torch.relu(v), GC.TANH: torch.tanh(v), GC.SIGMOID: torch.sigmoid(v)}[act]
        written[name] = _host(out)
        refs[name] = (v, GC.TOL_STEP_ACT if act in (GC.TANH, GC.SIGMOID) else GC.TOL_STEP)
    return written, refs


def run_gru_step(B, dev):
    """Tolerances: tests/test_gpu_kernels.py::test_gru_step_fwd_bwd (1e-5 on the new state, 5e-5 backward); the saved
    activations, which that test does not compare, at tests/gru_scan_cases.py's TOL_FWD for the same buffers of a scan."""
    from parrot_amd import ops
    written, refs = OrderedDict(), {}
    g = _gen("gru_step", B)
    r32 = lambda *s, scale=1.0: (torch.randn(*s, generator=g, dtype=torch.float64) * scale).float()
    h, inp, gin = r32(B, H), r32(B, H), r32(B, 2 * H)
    Wc, Wg = r32(H, H, scale=1 / math.sqrt(H)), r32(H, 2 * H, scale=1 / math.sqrt(H))
    gout = r32(B, H)
    mask = (torch.rand(B, generator=g) > 0.3).float()
    for tag, m in (("nomask", None), ("mask", mask)):
        dv = [x.to(dev) for x in (h, inp, gin, Wg, Wc)]
        md = None if m is None else m.to(dev)
        out, saved = ops.gru_step_fwd(*dv, md)
        dh, dC, dG = ops.gru_step_bwd(gout.to(dev), dv[0], dv[3], dv[4], saved, md)
        got = dict(zip(("h_new", "z", "r", "rh", "c", "dh", "d_inputs", "d_gate_inputs"), (out,) + tuple(saved) + (dh, dC, dG)))
        hd, ind, gd = (x.double().requires_grad_() for x in (h, inp, gin))
        gt = torch.sigmoid(hd @ Wg.double() + gd)
        z, r = gt[:, :H], gt[:, H:]
        rh = r * hd
        c = torch.tanh(rh @ Wc.double() + ind)
        hn = z * c + (1 - z) * hd
        if m is not None:
            hn = m.double()[:, None] * hn + (1 - m.double()[:, None]) * hd
        (hn * gout.double()).sum().backward()
        want = dict(h_new=hn, z=z, r=r, rh=rh, c=c, dh=hd.grad, d_inputs=ind.grad, d_gate_inputs=gd.grad)
        for k, v in got.items():
            written[tag + "/" + k] = _host(v)
            refs[tag + "/" + k] = (want[k].detach(), 5e-5 if k.startswith("d") else (1e-5 if k == "h_new" else GS.TOL_FWD))
    for jobs in ([(B, 2 * H, H)], [(B, H, H)]):
        mode = launch_mode(jobs)
        assert mode["zmode"] and mode["grid"][2] == 1, mode
    return written, refs


def run_gru_seq(B, dev):
    """Tolerances: tests/gru_scan_cases.py (TOL_FWD, TOL_BWD), whose data and float64 scan these runs use."""
    from parrot_amd import ops
    written, refs = OrderedDict(), {}
    for reverse in ((False,), (False, True), (False, True, True, False)):
        n = len(reverse)
        with switches(PARROT_GRU_ROWWISE=0):
            run = ops.GruSeqRunner(T, B, H, n, list(reverse), dev)
            data = [GS.chain_data(T, B, H, i) for i in range(n)]
            mask = GS.mask_data(T, B, "random").to(dev)
            for i, d in enumerate(data):
                run.inputs[i].copy_(d["inp"])
                run.gate_inputs[i].copy_(d["gin"])
                run.h[i][0].copy_(d["h0"])
                run.h[i][1:].fill_(float("nan"))
                run.dh[i].copy_(d["dh_in"])
                for k in ("z", "r", "rh", "c", "dG", "dC"):
                    getattr(run, k)[i].fill_(float("nan"))
            run.bind([d["Wg"].to(dev) for d in data], [d["Wc"].to(dev) for d in data], mask)
            assert run.route() == dict(rowwise=False, waves=0, nch=0, reason="switch")
        run.forward()
        run.backward()
        torch.cuda.synchronize()
        for i in range(n):
            ref = GS.reference(T, B, H, i, reverse[i], "random")
            for k in GS.NAMES:
                name = "chains%d/%d/%s" % (n, i, k)
                written[name] = _host(getattr(run, k)[i])
                refs[name] = (ref[k], GS.TOL_FWD if k in GS.FWD_NAMES else GS.TOL_BWD)
        run.close()
        for width in (2 * H, H):  # the gate and candidate launches of a step (and the backward's products of that width)
            mode = launch_mode([(B, width, H)] * n)
            assert mode["zmode"] and mode["grid"][2] == n, mode
    return written, refs


def run_lstm_seq(B, dev):
    from parrot_amd import _lib, ops
    d = GS.lstm_data(T, B, H)
    f = dict(device=dev, dtype=torch.float32)
    nan = float("nan")
    ws = dict(W=d["W"].to(dev), pre_in=d["pre_in"].to(dev), s=torch.full((T + 1, B, H), nan, **f),
              c=torch.full((T + 1, B, H), nan, **f), gates=torch.full((T, B, 4 * H), nan, **f), dS=d["dS_in"].to(dev),
              dc=d["dc_in"].to(dev), dP=torch.full((T, B, 4 * H), nan, **f))
    ws["s"][0].copy_(d["s0"])
    ws["c"][0].copy_(d["c0"])
    desc = _lib.LstmSeqDesc()
    desc.T, desc.B, desc.H, desc.use_graph = T, B, H, 0
    for k, v in ws.items():
        setattr(desc, k, v.data_ptr())
    plan = C.c_void_p()
    _lib.call("parrot_lstm_seq_create", C.byref(desc), C.byref(plan))
    try:
        _lib.call("parrot_lstm_seq_fwd", plan, ops._stream())
        _lib.call("parrot_lstm_seq_bwd", plan, ops._stream())
        torch.cuda.synchronize()
    finally:
        _lib.load().parrot_lstm_seq_destroy(plan)
    ref = GS.lstm_reference(T, B, H)
    written, refs = OrderedDict(), {}
    for k in GS.LSTM_NAMES_FWD + GS.LSTM_NAMES_BWD:
        written[k] = _host(ws[k])
        refs[k] = (ref[k], GS.TOL_FWD if k in GS.LSTM_NAMES_FWD else GS.TOL_BWD)
    mode = launch_mode([(B, 4 * H, H, H)])
    assert mode["zmode"] and mode["grid"][2] == 1, mode
    return written, refs


MODEL_KW = dict(rnn_h_dim=H, readouts_dim=H, encoder_dim=E // 2, input_dim=24, encoder_type="bidirectional")
# launch kinds: (kernel, z-mode, step-GEMM jobs) as plan_modes reports them; tests/test_step_launch_modes_cpu.py checks on
# dry-run plans of the same descriptors that the plans make them, 9 = SK_MAXJOB being the longest prefix table there is
DECODERS = {  # family: (model keywords, switches, schedule the plan must pick, launch kinds it must contain)
    "dec_gru1": (dict(num_layers=1), {}, 0, [("sk", True, 1), ("sk", False, 2)]),
    "dec_gru2": (dict(num_layers=2), {}, 5, [("sk", True, 2), ("sk", False, 2), ("ska", False, 2), ("skb", False, 4)]),
    "dec_gru3": (dict(num_layers=3, full_feedback=True), {}, 5,
                 [("sk", True, 3), ("sk", True, 4), ("sk", False, 9), ("ska", False, 4), ("skb", False, 9)]),
    "dec_lstm2": (dict(num_layers=2, cell_type="lstm"), dict(PARROT_SCHEDULE=5), 5,
                  [("sk", True, 2), ("sk", False, 5), ("ska", False, 1)]),
    "dec_lstm2_s7": (dict(num_layers=2, cell_type="lstm"), dict(PARROT_SCHEDULE=7), 7, [("sk", False, 5), ("ska", False, 2)]),
}
# the same plans as descriptors of tests/test_schedule_cpu.py::_make_plan: (cell, layers, PARROT_SCHEDULE, all accumulators, seq_init)
DECODER_PLANS = {"dec_gru1": (0, 1, None, False, 0), "dec_gru2": (0, 2, None, True, 0), "dec_gru3": (0, 3, None, True, 7),
                 "dec_lstm2": (1, 2, 5, False, 0), "dec_lstm2_s7": (1, 2, 7, False, 0)}
A = 10  # attention_size of the model's default configuration
WS_BUFFERS = ("h", "w", "kappa", "a", "b", "phi", "z", "r", "rh", "c", "cst", "gate4", "dh", "dw", "dw0", "dhup", "dG", "dC", "dp")


def build_model(dev, kw, use_graph=False):
    from oracle import parrot_ref as R
    from parrot_amd.model import Parrot
    base = dict(MODEL_KW)
    base.update(kw)
    cfg = R.default_config(**base)
    p = R.init_params(cfg, seed=7, scale_by_fan_in=True)
    m = Parrot(device=dev, use_graph=use_graph, **base).allocate()
    m.set_parameter_values(p)
    return cfg, p, m


def run_decoder(family, B, dev):
    """Tolerances: tests/test_gpu_parrot.py (1e-4 on the cost and the scan's outputs, 1e-3 norm-wise per gradient)."""
    from oracle import parrot_ref as R
    from parrot_amd import _lib
    from tests.util import make_batch
    kw, env, schedule, kinds = DECODERS[family]
    with switches(**env):
        cfg, p, m = build_model(dev, kw)
        feat, fm, lab, lm, _ = make_batch(cfg, T, B, U, seed=3, ragged=True)
        for v in p.values():
            v.requires_grad_()
        rc, _, rav, _ = R.compute_cost(p, cfg, feat, fm, lab, lm, None, 1)
        rc.backward()
        m.zero_grad()
        cost, _, av, _ = m.compute_cost(feat.float().to(dev), fm.float().to(dev), lab.to(dev), lm.float().to(dev), None, 1, B)
        cost.backward()
        torch.cuda.synchronize()
        ws = next(iter(m._train_ws.values()))
        assert int(_lib.load().parrot_decoder_schedule(ws["plan"])) == schedule
        found = plan_modes(ws["plan"])
    written, refs = OrderedDict(), {}
    written["cost"] = _host(cost).reshape(1)
    refs["cost"] = (rc.detach().reshape(1), 1e-4)
    for i, name in ((0, "frames"), (1, "kappa"), (2, "w"), (4, "phi"), (5, "pi_att")):
        written[name] = _host(av[i])
        refs[name] = (rav[i].detach(), 1e-4)
    grads = m.get_gradient_dict()
    for name in sorted(grads):
        written["grad" + name] = _host(grads[name])
        if p[name].grad is not None and float(p[name].grad.abs().max()) >= 1e-12:
            refs["grad" + name] = (p[name].grad, 1e-3)
    for k in WS_BUFFERS:
        v = ws.get(k)
        for i, t in enumerate(v if isinstance(v, (list, tuple)) else [v]):
            if t is not None:
                written["ws/%s%s" % (k, i if isinstance(v, (list, tuple)) else "")] = _host(t)
    m.close()
    return written, refs, found, kinds


def run_sample(B, dev):
    """Tolerance: tests/test_gpu_parrot.py::test_sample_model_parity (1e-4)."""
    from oracle import parrot_ref as R
    from tests.util import make_batch
    S = T
    with switches(PARROT_SAMPLE_PERSIST=0):
        cfg, p, m = build_model(dev, dict(num_layers=2, weak_feedback=True), use_graph=True)
        _, _, lab, lm, _ = make_batch(cfg, 2, B, U, seed=9)
        with torch.no_grad():
            ref = R.sample_model(p, cfg, lab, lm, None, S)
        outs = m.sample_model(lab.numpy(), lm.float().numpy(), None, None, B, S)
        m.close()
    written, refs = OrderedDict(), {}
    for o, r, n in zip(outs, ref, ("sample_x", "k", "w", "pi", "phi", "pi_att")):
        written[n] = torch.from_numpy(np.ascontiguousarray(o))
        refs[n] = (r, 1e-4)
    return written, refs


def run(family, B, dev):
    """-> (written, refs, launch kinds found, launch kinds required); the last two are None outside the decoder families."""
    if family in DECODERS:
        return run_decoder(family, B, dev)
    fn = dict(linear=run_linear, gru_step=run_gru_step, gru_seq=run_gru_seq, lstm_seq=run_lstm_seq, sample_gru2=run_sample)[family]
    return fn(B, dev) + (None, None)

"""The case table and the float64 reference of the decoder scan edge tests (`parrot_decoder_seq_fwd` / `_seq_bwd`).

A case is the smallest shape at which one branch of the training scan is live -- a forward schedule (0, 3, 5, 7 or the
persistent schedule 4), a backward tick (0 or 8), a set of accumulators, scratch-or-caller `seq_*` buffers, an attention
window -- together with the route the plan must report (`expected_route`, a restatement of DecoderPlan::resolve() in
csrc/plans.hip) and the switches it runs under (`environment`; every path switch a case does not name is unset).

Data depends on the shape, the cell, the number of layers, the `seq` mode and the window kind only -- never on the path --
so every path of one shape shares one reference and the paths can be compared with each other.

The reference works at the level of ParrotDecoderDesc (include/parrot_hip.h), from packed operands: `Wg[l]` / `Wc[l]` with
rows `[h_l ; w ; h_0 .. h_{l-1}]`, `bg`, `bc`, `WattT`, `batt`, `ctx`, slot 0 of `h[l]`, `w`, `kappa` (and `cst`), and
the per-step inputs `seq_g` / `seq_c` where the case gives caller data.  Layer 0 consumes `w[t]`, layers >= 1 consume
`w[t+1]` and `h_j[t+1]` (j < l); the GRU algebra is that of oracle.parrot_ref.gru_step (z = first half of the gates), the
LSTM algebra that of oracle.parrot_ref.lstm_cell (i|f|o|g), the window is oracle.parrot_ref.attention_step with the
training coefficients (the reference tests/test_gpu_kernels.py `_att_reference` uses); `a` is saved with epsilon added and
`b = exp(b_hat) * sharpening + epsilon` (csrc/att_fwd_body.h).  tests/test_decoder_scan_cases_cpu.py holds this
reference to oracle.parrot_ref.decoder_step at 1e-12.

Backward: autograd on the surrogate
    S = sum_l sum_s <dh_in[l][s], h_l[s]> + sum_s <dw_in[s], w[s]> + <dkappa_in, kappa[T]> (+ sum_l <dcell_in[l], cst_l[T]>)
over all T+1 slots.  `dG`, `dC`, `dp` are its gradients wrt the pre-activations, `dh[l][0]`, `dkappa`, `dcell[l]` wrt what
entered the window.  Every in-value the header documents is honoured by the code (slot 0 of `dh` and `dw`, `dkappa`,
`dcell` are accumulated into, never overwritten), so all of them are random and non-zero here.

What the backward schedules leave in slots >= 1 (read from plans.hip `bwd`, `bwd8`, `bwd_skew` and the state-backward
chains of csrc/elementwise.h, whose `dh` operand is const):

  * `dw[s]`, s >= 1: the TOTAL gradient wrt w[s].  The attention backward of step s-1 adds every share (`dw0[s]`, and
    `dw_b`, `dw_c`, `dw0_b`, `dw0_c` where given) and writes the sum back; model.py reads it for d ctx.  Compared.
  * `dw[0]` is never written: it keeps `dw_in[0]`.  The total wrt w[0] is `dw[0] + dw0[0]` plus slot 0 of whichever of
    `dw_b`, `dw_c`, `dw0_b`, `dw0_c` the plan was given, as Parrot._backward_f adds them.  Compared as that sum.
  * `dh[l][s]`, s >= 1, is NOT the total (the header said "out: total"; corrected): the state backward of step s-1 reads
    `dh[l][s]` plus the shares in `dhup[l][s]` (from the layers above; every schedule, the hoisted projections of schedule
    3 included) and, on the K-balanced tick, `dh_b[l][s]`, `dhup_b[l][s]`, `dhup_c[l][s]`, and does not write the sum
    back.  What is defined is the SUM of those buffers: it is the total gradient wrt h_l[s] (for the top layer on tick 0,
    `dh[L-1][s]` alone).  Compared as that sum ("dhT"); the single buffers are partial sums and are not compared.
  * `dw0[s]`, `dw0_b[s]`, `dw0_c[s]`, `dw_b[s]`, `dw_c[s]`, s >= 1: shares already folded into `dw[s]`; not compared.

This module imports no GPU code.  tests/test_gpu_decoder_scan_edges.py runs the cases."""
import functools
import json
import math
import os
import zlib
from collections import namedtuple

import torch

# The project's scan tolerances (norm-wise, tests.util.assert_close against float64), set for scans without the
# attention's exponentials.  A buffer whose float32-reference noise floor (tests/golden/decoder_scan_noise.json: the same
# reference evaluated in float32 against float64, per data set and buffer) exceeds a quarter of its tolerance is held to
# 4 x that floor instead: the kernels sum K in another order than torch's float32 matmul.  Nothing here is derived from
# what the kernels produce.
from tests.gru_scan_cases import TOL_BWD, TOL_FWD, TOL_PATHS  # noqa: F401

NOISE_MARGIN = 4.0
NOISE_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decoder_scan_noise.json")
MAX_ELEMENTS = 200000  # T * B * max(4H, U) of a case
EPS, ALIGNMENT = 1e-5, 1.0
PM_ATT_MAXU, PM_ATT_MAXA = 800, 32  # csrc/persist.h
GRU, LSTM = 0, 1
ELEMENTWISE = ("phi", "a", "b", "kappa")  # also compared with tests.util.rel_err_elem

# every switch that picks a path of the scan; a case names the ones it sets, the others are unset
SWITCHES = ("PARROT_SCHEDULE", "PARROT_WK", "PARROT_BWD_HETERO", "PARROT_CHUNK", "PARROT_S5_WSTEP", "PARROT_ATT_DENSE",
            "PARROT_PM_DATAFLOW", "PARROT_ATT_BWD_NARROW")

# seq: "none" = no caller data (seq_*[0] NULL, layers >= 1 scratch), "l0" = caller data at layer 0, "all" = at every layer
# accum: 0 = no second / third accumulators, 2 = all of them;  tiled: the fragment-major copies are given
# window: "" = U positions around a small kappa, "wide" = U = 200 with windows that underflow a dozen positions from kappa,
# "past" = kappa[0] past the text
Case = namedtuple("Case", "id group cell L T B H E A U att_type seq accum tiled persist env window")
DataKey = namedtuple("DataKey", "cell L T B H E A U seq window")

CASES = {}
GROUPS = {}


def _case(group, tag, cell, L, T, B, H=32, E=16, A=3, U=7, att_type=0, seq="l0", accum=2, tiled=True, env=(), window=""):
    env = tuple(sorted(dict(env).items()))
    assert all(k in SWITCHES for k, _ in env), env
    persist = dict(env).get("PARROT_SCHEDULE") == "4"
    name = "%s-%s-%s-L%d-T%d-B%d-H%d-E%d-U%d" % (group, tag, "lstm" if cell else "gru", L, T, B, H, E, U)
    assert name not in CASES, name
    CASES[name] = Case(name, group, cell, L, T, B, H, E, A, U, att_type, seq, accum, bool(tiled), persist, env, window)
    GROUPS.setdefault(group, []).append(name)


S = "PARROT_SCHEDULE"
# rows: one row, one short of a block, a full block, a block and a row, the last shape bwd8 / schedule 7 / the persistent
# scan accept, the first they refuse
for _B in (1, 15, 16, 17, 64, 65):
    _case("rows", "default", GRU, 2, 2, _B)
    _case("rows", "persist", GRU, 2, 2, _B, env={S: "4"})
    _case("rows", "default", LSTM, 2, 2, _B)
    _case("rows", "s7", LSTM, 2, 2, _B, env={S: "7"})
# steps: T = 1 has no previous tick to overlap with; L = 3 at T = 2 makes bwd8's lead of the upper layers longer than the
# window; one layer runs schedule 0 whatever is asked
for _L in (1, 2, 3):
    for _T in (1, 2, 5):
        _case("steps", "default", GRU, _L, _T, 5)
        _case("steps", "default", LSTM, _L, _T, 5)
_case("steps", "s5", GRU, 1, 2, 5, env={S: "5"})
# widths: three 16-column tiles against the 32-column workgroup; H = 64 with E = 32; K segments that are no multiples of
# 16 (no fragment-major copies can exist: the generic K loop, no bwd8); the same kernels on plain matrices
for _cell in (GRU, LSTM):
    _case("widths", "default", _cell, 2, 3, 17, H=48, E=16)
    _case("widths", "default", _cell, 2, 3, 17, H=64, E=32)
    _case("widths", "plain", _cell, 2, 3, 17, H=20, E=12, tiled=False)
    _case("widths", "plain", _cell, 2, 3, 17, H=32, E=16, tiled=False)
# paths, all on one data set per (cell, L)
for _L in (2, 3):
    _p = dict(cell=GRU, L=_L, T=5, B=17)
    _case("paths", "default", **_p)
    _case("paths", "hetero0", env={"PARROT_BWD_HETERO": "0"}, **_p)
    _case("paths", "noacc", accum=0, **_p)
    _case("paths", "s0", env={S: "0"}, **_p)
    _case("paths", "s0-noacc", env={S: "0"}, accum=0, **_p)
    _case("paths", "wstep0", env={"PARROT_S5_WSTEP": "0"}, **_p)
    _case("paths", "s3-chunk2", env={S: "3", "PARROT_CHUNK": "2"}, accum=0, **_p)  # three chunks, the last ragged
    _case("paths", "s3-chunk2-acc", env={S: "3", "PARROT_CHUNK": "2"}, **_p)  # ... given accumulators it does not use
    _case("paths", "persist-df0", env={S: "4", "PARROT_PM_DATAFLOW": "0"}, **_p)
    _case("paths", "persist-df1", env={S: "4", "PARROT_PM_DATAFLOW": "1"}, **_p)
    _case("paths", "wk2", env={"PARROT_WK": "2"}, **_p)
    _p["cell"] = LSTM
    _case("paths", "default", **_p)
    _case("paths", "s7", env={S: "7"}, **_p)
    _case("paths", "s5", env={S: "5"}, **_p)
# seq: seq_init and the per-step buffers
for _cell in (GRU, LSTM):
    for _seq in ("none", "l0", "all"):
        for _s in ("0", "3", "5"):
            _case("seq", "%s-s%s" % (_seq, _s), _cell, 3, 3, 5, seq=_seq, env={S: _s}, accum=0 if _s == "3" else 2)
# window: the attention support
for _at in (0, 1):
    for _dense in ("0", "1"):
        _case("window", "at%d-dense%s" % (_at, _dense), GRU, 2, 6, 17, U=200, att_type=_at, window="wide",
              env={"PARROT_ATT_DENSE": _dense})
    _case("window", "at%d-one" % _at, GRU, 2, 3, 5, U=1, att_type=_at)
    _case("window", "at%d-past" % _at, GRU, 2, 3, 5, U=3, att_type=_at, window="past")


def gate_width(case):
    return (4 if case.cell == LSTM else 2) * case.H


def krows(case, l):
    return case.H + case.E + l * case.H


def seq_init(case):
    return {"none": 0, "l0": 1, "all": (1 << case.L) - 1}[case.seq]


def environment(case):
    """The switches a case runs under: name -> value, None = unset."""
    env = dict.fromkeys(SWITCHES)
    env.update(dict(case.env))
    return env


def expected_route(case):
    """dict(schedule, tick, persistent) a plan for the case must report: DecoderPlan::resolve(), restated.  The upper
    layers' seq buffers are always given here (scratch or caller data), so the pipelined schedules need L >= 2 only.
    `persistent` assumes a device whose persistent grid has at least 64 workgroups."""
    env = dict(case.env)
    aligned = case.H % 16 == 0 and case.E % 16 == 0
    tiled = aligned and case.tiled
    pipe_ok = case.L >= 2
    want = int(env.get("PARROT_SCHEDULE", -1))
    want_persist = want == 4
    if want_persist:
        want = -1
    if want < 0:
        want = 5 if (pipe_ok and case.cell == GRU) else 0
    if want not in (0, 3, 5, 7):
        want = 0
    if want >= 2 and want != 7 and not pipe_ok:
        want = 0
    if want == 7 and case.cell != LSTM:
        want = 5 if pipe_ok else 0
    if want == 7 and not (tiled and case.B <= 64):
        want = 0
    tick = 8 if (case.cell == GRU and case.L in (2, 3) and tiled and case.B <= 64 and case.accum == 2 and want != 3
                 and int(env.get("PARROT_BWD_HETERO", 1)) != 0) else 0  # (schedule 3 has a backward of its own)
    persistent = int(want_persist and case.cell == GRU and tiled and case.B <= 64 and case.U <= PM_ATT_MAXU
                     and case.A <= PM_ATT_MAXA)
    return dict(schedule=want, tick=tick, persistent=persistent)


def data_key(case):
    return DataKey(case.cell, case.L, case.T, case.B, case.H, case.E, case.A, case.U, case.seq, case.window)


def key_name(key):
    return "%s-L%d-T%d-B%d-H%d-E%d-A%d-U%d-%s%s" % (("gru", "lstm")[key.cell], key.L, key.T, key.B, key.H, key.E, key.A,
                                                    key.U, key.seq, "-" + key.window if key.window else "")


def twins(case):
    """Ids of the cases that run the same data with the same window type on another path."""
    return [c.id for c in CASES.values() if c.id != case.id and data_key(c) == data_key(case) and c.att_type == case.att_type]


# ---- fake-address descriptors (schedule tracing, route queries: nothing is launched) -------------------------------------
class Arena:
    """Fake device address space: distinct, 4 KB aligned ranges; name -> (lo, hi)."""

    def __init__(self):
        self.top = 0x10000000
        self.ranges = {}

    def take(self, name, nbytes):
        lo = self.top
        self.top = (lo + max(nbytes, 16) + 4095) // 4096 * 4096 + 4096
        self.ranges[name] = (lo, lo + nbytes)
        return lo


def arena_descriptor(L, cell, nl, seq_init, T=5, B=20, H=32, E=16, A=4, U=7, bf16=0, layer_norm=0, ln_buffers=True, accum=0,
                     tiled=True, seq_upper=True, att_type=0, persist_floats=0):
    """A ParrotDecoderDesc (`L` = the parrot_amd._lib module) on fake addresses.  accum: 0 / 1 / 2 = no / second / second
    and third accumulators; seq buffers: layers >= 1 when `seq_upper`, layer l when bit l of seq_init is set; tiled:
    fragment-major copies given; persist_floats > 0: a persist_ws of that many floats.  Returns (arena, descriptor)."""
    ar = Arena()
    d = L.DecoderDesc()
    d.T, d.B, d.H, d.E, d.A, d.U, d.L = T, B, H, E, A, U, nl
    d.cell, d.use_graph, d.seq_init, d.bf16, d.layer_norm, d.att_type = cell, 0, seq_init, bf16, layer_norm, att_type
    d.eps, d.alignment, d.sharpening, d.timing = 1e-5, 1.0, 1.0, 1.0
    f = 4
    gw = 4 * H if cell == 1 else 2 * H
    for l in range(nl):
        K = H + E + l * H
        d.Wg[l] = ar.take(f"Wg{l}", K * gw * f)
        d.bg[l] = ar.take(f"bg{l}", gw * f)
        if tiled:
            d.Wg_f[l] = ar.take(f"Wg_f{l}", K * gw * f)
            d.Wg_r[l] = ar.take(f"Wg_r{l}", K * gw * f)
        d.h[l] = ar.take(f"h{l}", (T + 1) * B * H * f)
        d.dh[l] = ar.take(f"dh{l}", (T + 1) * B * H * f)
        d.dG[l] = ar.take(f"dG{l}", T * B * gw * f)
        if l < nl - 1:
            d.dhup[l] = ar.take(f"dhup{l}", (T + 1) * B * H * f)
        if bf16 and cell == 1:  # bf16 copies of the pre-activation gradients, written by the fused backward tick (round 5)
            d.dG16[l] = ar.take(f"dG16_{l}", T * B * gw * 2)
        if accum >= 1:  # second (and third) accumulators: the backward products run as K parts
            d.dh_b[l] = ar.take(f"dh_b{l}", (T + 1) * B * H * f)
            if l < nl - 1:
                d.dhup_b[l] = ar.take(f"dhup_b{l}", (T + 1) * B * H * f)
                if accum >= 2:
                    d.dhup_c[l] = ar.take(f"dhup_c{l}", (T + 1) * B * H * f)
        has_seq = (l >= 1 and seq_upper) or (seq_init >> l) & 1
        if has_seq:
            d.seq_g[l] = ar.take(f"seq_g{l}", T * B * gw * f)
        if cell == 0:
            d.Wc[l] = ar.take(f"Wc{l}", K * H * f)
            d.bc[l] = ar.take(f"bc{l}", H * f)
            if tiled:
                d.Wc_f[l] = ar.take(f"Wc_f{l}", K * H * f)
                d.Wc_r[l] = ar.take(f"Wc_r{l}", K * H * f)
            for n in ("z", "r", "rh", "c"):
                getattr(d, n)[l] = ar.take(f"{n}{l}", T * B * H * f)
            d.dC[l] = ar.take(f"dC{l}", T * B * H * f)
            if has_seq:
                d.seq_c[l] = ar.take(f"seq_c{l}", T * B * H * f)
        else:
            d.cst[l] = ar.take(f"cst{l}", (T + 1) * B * H * f)
            d.gate4[l] = ar.take(f"gate4{l}", T * B * 4 * H * f)
            d.dcell[l] = ar.take(f"dcell{l}", B * H * f)
        for j in range(l if (layer_norm and ln_buffers) else 0):  # layer_norm: the normalised projection of h_j into layer l
            pj = l * len(d.Wg) + j
            for g, wd in (("g", gw),) + ((("c", H),) if cell == 0 else ()):
                getattr(d, f"ln_y{g}")[pj] = ar.take(f"ln_y{g}{l}{j}", T * B * wd * f)
                getattr(d, f"ln_s{g}")[pj] = ar.take(f"ln_s{g}{l}{j}", T * B * f)
                getattr(d, f"ln_b{g}")[pj] = ar.take(f"ln_b{g}{l}{j}", wd * f)
    d.WattT = ar.take("WattT", 3 * A * H * f)
    d.batt = ar.take("batt", 3 * A * f)
    d.ctx = ar.take("ctx", B * U * E * f)
    d.w = ar.take("w", (T + 1) * B * E * f)
    d.kappa = ar.take("kappa", (T + 1) * B * A * f)
    d.a = ar.take("a", T * B * A * f)
    d.b = ar.take("b", T * B * A * f)
    d.phi = ar.take("phi", T * B * U * f)
    d.dw = ar.take("dw", (T + 1) * B * E * f)
    d.dw0 = ar.take("dw0", (T + 1) * B * E * f)
    if accum >= 1:
        d.dw_b = ar.take("dw_b", (T + 1) * B * E * f)
        d.dw0_b = ar.take("dw0_b", (T + 1) * B * E * f)
        if accum >= 2:
            d.dw_c = ar.take("dw_c", (T + 1) * B * E * f)
            d.dw0_c = ar.take("dw0_c", (T + 1) * B * E * f)
    d.dkappa = ar.take("dkappa", B * A * f)
    d.dp = ar.take("dp", T * B * 3 * A * f)
    d.att_sup = ar.take("att_sup", T * B * 2 * 4)
    if persist_floats > 0:
        d.persist_ws = ar.take("persist_ws", persist_floats * f)
        d.persist_ws_floats = persist_floats
    return ar, d


def case_arena_descriptor(L, case, **over):
    kw = dict(T=case.T, B=case.B, H=case.H, E=case.E, A=case.A, U=case.U, accum=case.accum, tiled=case.tiled,
              att_type=case.att_type)
    kw.update(over)
    return arena_descriptor(L, case.cell, case.L, seq_init(case), **kw)


# ---- data ---------------------------------------------------------------------------------------------------------------
def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


@functools.lru_cache(maxsize=None)
def data(key, variant=0):
    """float32 operands of a data set (`variant` = another draw of everything: the second window through one plan).
    Lists are per layer.  Weights uniform in +-1/sqrt(K_l); slot-0 states random (a TBPTT carry, not the start of an
    utterance), kappa[0] random and positive; the consumers' gradients random in every slot; batt near zero, so that
    b ~ 1 and kappa advances by about 1 per step."""
    cell, L, T, B, H, E, A, U = key[:8]
    g = _gen("decoder", tuple(key), variant)
    gw = (4 if cell == LSTM else 2) * H

    def rn(*shape, scale=1.0):
        return torch.randn(*shape, generator=g) * scale

    def un(*shape, bound=1.0):
        return (torch.rand(*shape, generator=g) * 2 - 1) * bound

    d = dict(Wg=[], Wc=[], bg=[], bc=[], h0=[], cst0=[], seq_g=[], seq_c=[], dh_in=[], dcell_in=[])
    for l in range(L):
        K = H + E + l * H
        d["Wg"].append(un(K, gw, bound=1 / math.sqrt(K)))
        d["bg"].append(rn(gw, scale=0.1))
        d["h0"].append(rn(B, H, scale=0.5))
        d["dh_in"].append(rn(T + 1, B, H))
        caller = (key.seq == "all") or (key.seq == "l0" and l == 0)
        d["seq_g"].append(rn(T, B, gw, scale=0.5) if caller else None)
        if cell == GRU:
            d["Wc"].append(un(K, H, bound=1 / math.sqrt(K)))
            d["bc"].append(rn(H, scale=0.1))
            d["seq_c"].append(rn(T, B, H, scale=0.5) if caller else None)
        else:
            d["cst0"].append(rn(B, H, scale=0.5))
            d["dcell_in"].append(rn(B, H))
    d["WattT"] = un(3 * A, H, bound=0.5 / math.sqrt(H))
    d["batt"] = rn(3 * A, scale=0.05)
    d["ctx"] = rn(B, U, E)
    d["w0"] = rn(B, E)
    if key.window == "wide":
        # even rows: the mixtures of a row within a few positions of each other (a support of some 30 rows);
        # odd rows: spread over the text (a support wider than the narrow backward path takes)
        centre = 20 + 150 * torch.rand(B, 1, generator=g)
        near = centre + 3 * torch.rand(B, A, generator=g)
        far = 20 + 150 * torch.rand(B, A, generator=g)
        d["kappa0"] = torch.where((torch.arange(B) % 2 == 0)[:, None], near, far)
    elif key.window == "past":
        d["kappa0"] = U + 15 + torch.rand(B, A, generator=g)
    else:
        d["kappa0"] = 0.25 + 2 * torch.rand(B, A, generator=g)
    d["dw_in"] = rn(T + 1, B, E)
    d["dkappa_in"] = rn(B, A)
    return d


# ---- reference ----------------------------------------------------------------------------------------------------------
def forward_names(cell, L):
    per = ("h", "z", "r", "rh", "c") if cell == GRU else ("h", "cst", "gate4")
    return tuple("%s%d" % (n, l) for l in range(L) for n in per) + ("w", "kappa", "a", "b", "phi")


def backward_names(cell, L):
    """dh0_l = dh[l][0]; dhT_l = the total of slots 1..T (see the module docstring); dw0 = the total wrt w[0];
    dw = dw[1:]; dctx = sum_t phi[t]^T . dw[t+1]."""
    per = ("dG", "dC", "dh0_", "dhT_") if cell == GRU else ("dG", "dcell", "dh0_", "dhT_")
    return tuple("%s%d" % (n, l) for l in range(L) for n in per) + ("dp", "dkappa", "dw0", "dw", "dctx")


def scan_reference(d, cell, L, att_type, dtype=torch.float64):
    """The scan over the operands `d` (data()'s keys) in `dtype`: every forward buffer of the descriptor (histories with
    T+1 slots) and the backward buffers of backward_names, by autograd on the surrogate S."""
    from oracle import parrot_ref as R
    T, B, H = d["dh_in"][0].shape[0] - 1, d["h0"][0].shape[0], d["h0"][0].shape[1]
    A = d["kappa0"].shape[1]
    cfg = R.default_config(attention_type="softmax" if att_type else "graves", attention_size=A,
                           attention_alignment=ALIGNMENT, epsilon=EPS)

    def cv(t):
        return t.to(dtype)

    def leaf(t):
        return cv(t).clone().requires_grad_()

    Wg, bg = [cv(x) for x in d["Wg"]], [cv(x) for x in d["bg"]]
    Wc, bc = [cv(x) for x in d["Wc"]], [cv(x) for x in d["bc"]]
    seq_g = [None if x is None else cv(x) for x in d["seq_g"]]
    seq_c = [None if x is None else cv(x) for x in d["seq_c"]]
    WattT, batt, ctx = cv(d["WattT"]), cv(d["batt"]), leaf(d["ctx"])
    h = [[leaf(x)] for x in d["h0"]]
    cst = [[leaf(x)] for x in d["cst0"]]
    w, kappa = [leaf(d["w0"])], [leaf(d["kappa0"])]
    saved = {n: [[] for _ in range(L)] for n in ("z", "r", "rh", "c", "gate4", "pg", "pc")}
    att = {n: [] for n in ("a", "b", "phi", "p")}

    def layer_step(l, t, x_rest):
        hp = h[l][t]
        pg = torch.cat([hp, x_rest], 1) @ Wg[l] + bg[l]
        if seq_g[l] is not None:
            pg = pg + seq_g[l][t]
        pg.retain_grad()
        saved["pg"][l].append(pg)
        if cell == LSTM:
            i, f, o = torch.sigmoid(pg[:, :H]), torch.sigmoid(pg[:, H:2 * H]), torch.sigmoid(pg[:, 2 * H:3 * H])
            gg = torch.tanh(pg[:, 3 * H:])
            cn = f * cst[l][t] + i * gg
            hn = torch.tanh(cn) * o
            cst[l].append(cn)
            saved["gate4"][l].append(torch.cat([i, f, o, gg], 1))
        else:
            gact = torch.sigmoid(pg)
            z, r = gact[:, :H], gact[:, H:]
            rh = hp * r
            pc = torch.cat([rh, x_rest], 1) @ Wc[l] + bc[l]
            if seq_c[l] is not None:
                pc = pc + seq_c[l][t]
            pc.retain_grad()
            saved["pc"][l].append(pc)
            c = torch.tanh(pc)
            hn = c * z + hp * (1 - z)
            for n, v in (("z", z), ("r", r), ("rh", rh), ("c", c)):
                saved[n][l].append(v)
        hn.retain_grad()
        h[l].append(hn)

    for t in range(T):
        layer_step(0, t, w[t])
        p = h[0][t + 1] @ WattT.t() + batt
        p.retain_grad()
        a, k, phi, wn = R.attention_step(cfg, p[:, :A], p[:, A:2 * A], p[:, 2 * A:], kappa[t], ctx)
        wn.retain_grad()
        att["p"].append(p)
        att["a"].append(a)
        att["b"].append(torch.exp(p[:, A:2 * A]) + EPS)
        att["phi"].append(phi)
        w.append(wn)
        kappa.append(k)
        for l in range(1, L):
            layer_step(l, t, torch.cat([w[t + 1]] + [h[j][t + 1] for j in range(l)], 1))

    S = sum((h[l][s] * cv(d["dh_in"][l][s])).sum() for l in range(L) for s in range(T + 1))
    S = S + sum((w[s] * cv(d["dw_in"][s])).sum() for s in range(T + 1)) + (kappa[T] * cv(d["dkappa_in"])).sum()
    if cell == LSTM:
        S = S + sum((cst[l][T] * cv(d["dcell_in"][l])).sum() for l in range(L))
    S.backward()

    out = {}
    for l in range(L):
        out["h%d" % l] = torch.stack([x.detach() for x in h[l]])
        if cell == LSTM:
            out["cst%d" % l] = torch.stack([x.detach() for x in cst[l]])
            out["gate4%d" % l] = torch.stack([x.detach() for x in saved["gate4"][l]])
            out["dcell%d" % l] = cst[l][0].grad
        else:
            for n in ("z", "r", "rh", "c"):
                out["%s%d" % (n, l)] = torch.stack([x.detach() for x in saved[n][l]])
            out["dC%d" % l] = torch.stack([x.grad for x in saved["pc"][l]])
        out["dG%d" % l] = torch.stack([x.grad for x in saved["pg"][l]])
        out["dh0_%d" % l] = h[l][0].grad
        out["dhT_%d" % l] = torch.stack([x.grad for x in h[l][1:]])
    out["w"] = torch.stack([x.detach() for x in w])
    out["kappa"] = torch.stack([x.detach() for x in kappa])
    for n in ("a", "b", "phi"):
        out[n] = torch.stack([x.detach() for x in att[n]])
    out["dp"] = torch.stack([x.grad for x in att["p"]])
    out["dkappa"] = kappa[0].grad
    out["dw0"] = w[0].grad
    out["dw"] = torch.stack([x.grad for x in w[1:]])
    out["dctx"] = ctx.grad
    return out


@functools.lru_cache(maxsize=None)
def reference(key, att_type, variant=0):
    """The float64 reference of a data set; computed once, shared by every case on it.  Read-only."""
    return scan_reference(data(key, variant), key.cell, key.L, att_type)


def case_reference(case, variant=0):
    return reference(data_key(case), case.att_type, variant)


def representable(t):
    """A float64 reference buffer as float32 can hold it: magnitudes below the smallest denormal (a window weight past the
    text is 1e-100 in float64 and exactly 0.0f in the kernels) are zero; everything else is unchanged."""
    return torch.where(t.abs() < 2.0 ** -150, torch.zeros_like(t), t)


# ---- noise floors and tolerances ------------------------------------------------------------------------------------------
def noise_name(case):
    return "%s-at%d" % (key_name(data_key(case)), case.att_type)


def noise_row(case):
    """name -> rel_err of the reference evaluated in float32 against float64 (ELEMENTWISE buffers also as "<name>:elem",
    with rel_err_elem)."""
    from tests.util import rel_err, rel_err_elem
    key = data_key(case)
    ref = case_reference(case)
    f32 = scan_reference(data(key), key.cell, key.L, case.att_type, dtype=torch.float32)
    row = {n: rel_err(f32[n], representable(ref[n])) for n in ref}
    for n in ELEMENTWISE:
        row[n + ":elem"] = rel_err_elem(f32[n], representable(ref[n]))
    return row


@functools.lru_cache(maxsize=None)
def noise_table():
    with open(NOISE_FILE) as f:
        return json.load(f)


def tolerance(case, name, base=None, elem=False):
    """The bound of buffer `name` of a case: the project's scan tolerance, or 4 x the buffer's float32 noise floor where
    that floor exceeds a quarter of it."""
    if base is None:
        base = TOL_FWD if name in forward_names(case.cell, case.L) else TOL_BWD
    floor = noise_table()[noise_name(case)][name + (":elem" if elem else "")]
    return NOISE_MARGIN * floor if floor > base / NOISE_MARGIN else base

"""The case table and the float64 reference of the GRU scan edge tests (`parrot_gru_seq_*`).

A GRU scan plan runs on one of two paths: the row-wise sequence kernels of rowgru.hip (`rg_fwd_kernel` / `rg_bwd_kernel`,
one launch per direction, instantiated per H / 16 = 1..8 and per block width of 4 or 8 waves), or the per-step launches of
the step kernel.  A case is `(T, B, H, reverse list, mask kind, waves, path)` with an id and a group: the smallest shape at
which one branch of those kernels is live, and the path the plan must report (`parrot_gru_seq_route`).  `path` is
"rowwise", "switch" (the launch path under PARROT_GRU_ROWWISE=0) or "shape" (the launch path because the row-wise
kernels refuse the shape); `waves` is 0 on the launch path.

Data depends on the shape and the chain's index only -- not on the path, the width, the mask kind or the other chains
of the plan -- so one reference serves every case that shares a chain, a chain alone can be compared with the same
chain as one of four, and an all-ones mask with no mask.

The reference works at the level of the descriptor (include/parrot_hip.h): per chain, slot-indexed states `h[T+1]` and
their total gradients `dh[T+1]`, time-indexed saved activations `z`, `r`, `rh`, `c` and gradients `dC`, `dG`; a reversed
chain's step s consumes and writes time T-1-s.  Same algebra as `oracle.parrot_ref.gru_step`, mask blend included.

This module imports no GPU code.  tests/test_gru_scan_cases_cpu.py checks the reference against the oracle and the
premises of the table; tests/test_gpu_gru_scan_edges.py runs the cases."""
import functools
import math
import zlib
from collections import namedtuple

import torch

# The project's norm-wise tolerances for these kernels (tests.util.assert_close against float64;
# tests/test_gpu_kernels.py test_gru_seq_rowwise_vs_step_launches, test_lstm_seq_fwd_bwd)
TOL_FWD = 2e-5    # h, z, r, rh, c (LSTM: s, c, gates)
TOL_BWD = 1e-4    # dC, dG, dh (LSTM: dP, dS, dc)
TOL_PATHS = 2e-5  # the row-wise path against the launch path
FWD_NAMES = ("h", "z", "r", "rh", "c")
BWD_NAMES = ("dC", "dG", "dh")
NAMES = FWD_NAMES + BWD_NAMES

ROWWISE, SWITCH, SHAPE = "rowwise", "switch", "shape"
MASKS = ("none", "random", "row", "ones", "frac")
RG_MAXH = 128  # rowgru.hip

Case = namedtuple("Case", "id group T B H reverse mask waves path")

CASES = {}
GROUPS = {}


def _case(group, T, B, H, reverse, mask, waves, path):
    assert mask in MASKS and path in (ROWWISE, SWITCH, SHAPE) and waves in ((4, 8) if path == ROWWISE else (0,))
    name = "%s-T%d-B%d-H%d-%s-%s-%s" % (group, T, B, H, "".join("fr"[int(x)] for x in reverse), mask,
                                        ("w%d" % waves) if path == ROWWISE else path)
    assert name not in CASES, name
    CASES[name] = Case(name, group, T, B, H, tuple(int(x) for x in reverse), mask, waves, path)
    GROUPS.setdefault(group, []).append(name)


def _both_widths(group, T, B, H, reverse, mask):
    for waves in (4, 8):
        _case(group, T, B, H, reverse, mask, waves, ROWWISE)


def _rows_chains_masks(add):
    # rows: one row, one short of a block, a full block, a block and one row -- at an even and an odd chunk count
    # (H / 16 = 5 at 8 waves: the partial last round of the backward's element-wise half)
    for H in (48, 80):
        for B in (1, 15, 16, 17):
            add("rows", 2, B, H, (0, 1), "frac")
    # chains: one alone in either direction, the four-chain limit, three reversed -- the encoder's shared 0/1 mask
    for reverse in ((0,), (1,), (0, 1, 1, 0), (1, 1, 1)):
        add("chains", 4, 17, 32, reverse, "random")
    for mask in MASKS:
        add("masks", 5, 17, 64, (0, 1), mask)


# width sweep: every instantiation of the two kernels; 21 rows = two blocks, the second with 5 rows
for _H in range(16, RG_MAXH + 1, 16):
    _both_widths("width", 3, 21, _H, (0, 1), "random")
_rows_chains_masks(_both_widths)
# steps: T = 1 prefetches no next step, T = 2 exactly one
for _T in (1, 2, 9):
    _both_widths("steps", _T, 5, 112, (0, 1), "random")
# launch path: the same rows, chains and masks with the switch off ...
_rows_chains_masks(lambda g, T, B, H, rev, m: _case("launch-" + g, T, B, H, rev, m, 0, SWITCH))
# ... and the shapes the row-wise kernels refuse, under the default switch
for _H in (8, 100, 144, 256):
    _case("refused", 3, 20, _H, (0, 1), "random", 0, SHAPE)


def shape_supported(T, B, H, nchain):
    """The boundary the table assumes (rowgru_supported; the CPU test compares it with the library's predicate)."""
    return T >= 1 and B >= 1 and 16 <= H <= RG_MAXH and H % 16 == 0 and 1 <= nchain <= 4


def expected_route(case):
    """What GruSeqRunner.route() must return for the case."""
    if case.path == ROWWISE:
        return dict(rowwise=True, waves=case.waves, nch=case.H // 16, reason="rowwise")
    return dict(rowwise=False, waves=0, nch=0, reason=case.path)


def environment(case):
    """The switches a case runs under: name -> value, None = unset."""
    return {"PARROT_GRU_ROWWISE": "0" if case.path == SWITCH else None,
            "PARROT_RG_WAVES": str(case.waves) if case.path == ROWWISE else None}


def twin(case, path, waves=0):
    """The id of the same scan on another path, or None if the table does not hold it."""
    for other in CASES.values():
        if (other.T, other.B, other.H, other.reverse, other.mask, other.path, other.waves) == \
                (case.T, case.B, case.H, case.reverse, case.mask, path, waves):
            return other.id
    return None


# ---- data ---------------------------------------------------------------------------------------------------------------
def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


@functools.lru_cache(maxsize=None)
def chain_data(T, B, H, index, variant=0):
    """float32 operands of chain `index` of a (T, B, H) scan: inputs, gate_inputs, h0, Wg, Wc and the consumers' gradients
    dh_in [T+1, B, H] (non-zero in every slot 1..T, zero in slot 0: the header's contract).  `variant` = another draw of
    the weights alone (the optimiser step of the replay test)."""
    g = _gen("chain", T, B, H, index)
    d = dict(inp=torch.randn(T, B, H, generator=g), gin=torch.randn(T, B, 2 * H, generator=g),
             h0=torch.randn(B, H, generator=g), dh_in=torch.randn(T + 1, B, H, generator=g))
    d["dh_in"][0].zero_()
    gw = _gen("weights", T, B, H, index, variant)
    d["Wg"] = torch.randn(H, 2 * H, generator=gw) / math.sqrt(H)
    d["Wc"] = torch.randn(H, H, generator=gw) / math.sqrt(H)
    return d


@functools.lru_cache(maxsize=None)
def mask_data(T, B, kind):
    """The step mask [T, B] (float32) shared by the chains of a plan, or None."""
    if kind == "none":
        return None
    if kind == "ones":
        return torch.ones(T, B)
    if kind == "row":  # one batch row masked at every step
        m = torch.ones(T, B)
        m[:, B // 2] = 0.0
        return m
    if kind == "frac":  # strictly inside (0, 1): both terms of the blend carry weight in every element
        return 0.05 + 0.9 * torch.rand(T, B, generator=_gen("frac", T, B))
    # random 0/1: the first seed that puts a 0 and a 1 into every time step
    for seed in range(64):
        m = (torch.rand(T, B, generator=_gen("random", T, B, seed)) > 0.5).float()
        if bool(((m == 0).any(1) & (m == 1).any(1)).all()):
            break
    assert bool(((m == 0).any(1) & (m == 1).any(1)).all()), ("no seed gives a 0 and a 1 in every step", T, B)
    return m


# ---- reference ----------------------------------------------------------------------------------------------------------
def reference_chain(d, mask, reverse):
    """float64 scan of one chain over the float32 operands `d` (chain_data's keys): dict of h [T+1,B,H] and dh [T+1,B,H]
    by slot, z / r / rh / c / dC [T,B,H] and dG [T,B,2H] by time.  dh = the gradient of sum_s <h[s+1], dh_in[s+1]> wrt
    every slot's state (retained), dC / dG = its gradient wrt inputs / gate_inputs."""
    T, B, H = d["inp"].shape
    inp = d["inp"].double().requires_grad_()
    gin = d["gin"].double().requires_grad_()
    Wg, Wc = d["Wg"].double(), d["Wc"].double()
    m = None if mask is None else mask.double()
    dh_in = d["dh_in"].double()
    assert not bool(dh_in[0].any()) and all(bool(dh_in[s].any()) for s in range(1, T + 1))
    h = [d["h0"].double().requires_grad_()]
    saved = {k: [None] * T for k in ("z", "r", "rh", "c")}
    for s in range(T):
        t = T - 1 - s if reverse else s
        hp = h[s]
        g = torch.sigmoid(hp @ Wg + gin[t])
        z, r = g[:, :H], g[:, H:]
        rh = hp * r
        c = torch.tanh(rh @ Wc + inp[t])
        hn = c * z + hp * (1 - z)
        if m is not None:
            hn = m[t][:, None] * hn + (1 - m[t][:, None]) * hp
        hn.retain_grad()
        h.append(hn)
        for k, v in (("z", z), ("r", r), ("rh", rh), ("c", c)):
            saved[k][t] = v.detach()
    loss = sum((h[s + 1] * dh_in[s + 1]).sum() for s in range(T))
    loss.backward()
    out = {k: torch.stack(v) for k, v in saved.items()}
    out["h"] = torch.stack([x.detach() for x in h])
    out["dh"] = torch.stack([x.grad for x in h])
    out["dC"], out["dG"] = inp.grad, gin.grad
    return out


@functools.lru_cache(maxsize=None)
def reference(T, B, H, index, reverse, mask_kind, variant=0):
    """The reference of chain `index` of a case's scan; computed once, shared by every case with that chain.  Read-only."""
    return reference_chain(chain_data(T, B, H, index, variant), mask_data(T, B, mask_kind), bool(reverse))


def case_reference(case):
    return [reference(case.T, case.B, case.H, i, rev, case.mask) for i, rev in enumerate(case.reverse)]


# ---- LSTM scan ------------------------------------------------------------------------------------------------------------
LSTM_SHAPES = [(T, B, H) for H in (4, 20, 100, 256) for B in (1, 17, 65) for T in (1, 6)]
LSTM_NAMES_FWD = ("s", "c", "gates")
LSTM_NAMES_BWD = ("dP", "dS", "dc")


@functools.lru_cache(maxsize=None)
def lstm_data(T, B, H):
    """float32 operands of an LSTM scan: pre_in, W, s0, c0, the consumers' gradients dS_in [T+1,B,H] (slots 1..T, slot 0
    zero) and a non-zero gradient dc_in [B,H] wrt the final cell."""
    g = _gen("lstm", T, B, H)
    d = dict(pre_in=torch.randn(T, B, 4 * H, generator=g), W=torch.randn(H, 4 * H, generator=g) / math.sqrt(H),
             s0=torch.randn(B, H, generator=g), c0=torch.randn(B, H, generator=g),
             dS_in=torch.randn(T + 1, B, H, generator=g), dc_in=torch.randn(B, H, generator=g))
    d["dS_in"][0].zero_()
    return d


@functools.lru_cache(maxsize=None)
def lstm_reference(T, B, H):
    """float64 loop of the header's LSTM algebra (gate order i | f | o | g): s, c [T+1,B,H], gates [T,B,4H] after the
    non-linearity, dP [T,B,4H], the total dS of every slot and dc wrt the initial cell."""
    d = lstm_data(T, B, H)
    pre = d["pre_in"].double().requires_grad_()
    W = d["W"].double()
    s = [d["s0"].double().requires_grad_()]
    c = [d["c0"].double().requires_grad_()]
    gates = []
    for t in range(T):
        a = s[t] @ W + pre[t]
        i, f, o = torch.sigmoid(a[:, :H]), torch.sigmoid(a[:, H:2 * H]), torch.sigmoid(a[:, 2 * H:3 * H])
        g = torch.tanh(a[:, 3 * H:])
        cn = c[t] * f + g * i
        sn = torch.tanh(cn) * o
        sn.retain_grad()
        s.append(sn)
        c.append(cn)
        gates.append(torch.cat([i, f, o, g], 1).detach())
    dS_in, dc_in = d["dS_in"].double(), d["dc_in"].double()
    loss = sum((s[t + 1] * dS_in[t + 1]).sum() for t in range(T)) + (c[T] * dc_in).sum()
    loss.backward()
    return dict(s=torch.stack([x.detach() for x in s]), c=torch.stack([x.detach() for x in c]), gates=torch.stack(gates),
                dP=pre.grad, dS=torch.stack([x.grad for x in s]), dc=c[0].grad)

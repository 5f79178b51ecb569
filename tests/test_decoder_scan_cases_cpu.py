"""Premises of the decoder scan edge tests, checked without a GPU: the float64 reference of tests/decoder_scan_cases.py
equals the oracle's decoder_step, every case's expected route is what the library resolves for such a descriptor, the
attention-window cases do what the table says, the committed noise floors are the ones the reference gives, and the
create call refuses what the header says it refuses."""
import ctypes as C

import pytest
import torch

from tests import decoder_scan_cases as D
from tests.step_launch_cases import switches
from tests.util import rel_err

BADARG = 10001


def _lib():
    from parrot_amd import _lib as L
    try:
        return L, L.load()
    except L.HipLibraryMissing:
        pytest.skip("libparrot_hip.so not built")


def _find(group, tag, cell, **fields):
    hits = [c for c in D.CASES.values() if c.group == group and c.id.startswith("%s-%s-%s-" % (group, tag, ("gru", "lstm")[cell]))
            and all(getattr(c, k) == v for k, v in fields.items())]
    assert len(hits) == 1, (group, tag, cell, fields, [c.id for c in hits])
    return hits[0]


# ---- the reference is the oracle's step --------------------------------------------------------------------------------------
def _oracle_params(d, cell, L, H, E, A):
    p = {}
    for l in range(L):
        ll = l + 1
        Wg, Wc = d["Wg"][l].double(), (d["Wc"][l].double() if cell == D.GRU else None)
        if cell == D.LSTM:
            p[f"/parrot/rnn{ll}.W_state"] = Wg[:H]
            groups = [(f"rnn{ll}_inputs", Wg, d["bg"][l].double())]
        else:
            p[f"/parrot/rnn{ll}.state_to_state"] = Wc[:H]
            p[f"/parrot/rnn{ll}.state_to_gates"] = Wg[:H]
            groups = [(f"rnn{ll}_inputs", Wc, d["bc"][l].double()), (f"rnn{ll}_gates", Wg, d["bg"][l].double())]
        for name, W, b in groups:
            p[f"/parrot/inp_to_h{ll}/fork_{name}.W"] = W[H:H + E]
            p[f"/parrot/inp_to_h{ll}/fork_{name}.b"] = b
            for j in range(l):
                p[f"/parrot/h{j + 1}_to_h{ll}/fork_{name}.W"] = W[H + E + j * H:H + E + (j + 1) * H]
                p[f"/parrot/h{j + 1}_to_h{ll}/fork_{name}.b"] = torch.zeros_like(b)
    Watt, batt = d["WattT"].double().t(), d["batt"].double()
    for i, n in enumerate(("alpha", "beta", "kappa")):
        p[f"/parrot/h1_to_att/fork_{n}.W"] = Watt[:, i * A:(i + 1) * A]
        p[f"/parrot/h1_to_att/fork_{n}.b"] = batt[i * A:(i + 1) * A].clone().requires_grad_()
    return p


@pytest.mark.parametrize("cell", [D.GRU, D.LSTM], ids=["gru", "lstm"])
def test_reference_is_the_oracles_decoder_step(cell):
    """L = 3 with caller data at every layer: oracle.parrot_ref.decoder_step over the window, from the equivalent parameter
    dictionary, gives the reference's forward buffers and -- by autograd on the same surrogate -- its gradients, to 1e-12.
    (dG / dC are the gradients wrt the additive per-step inputs, dp is held through its column sums = d batt, z / r / rh /
    c / b through the gradients they enter.)"""
    from oracle import parrot_ref as R
    case = _find("seq", "all-s0", cell)
    key, L, T, H, E, A = D.data_key(case), case.L, case.T, case.H, case.E, case.A
    d, ref = D.data(key), D.case_reference(case)
    cfg = R.default_config(rnn_h_dim=H, num_layers=L, attention_size=A, cell_type="lstm" if cell else "gru",
                           attention_type="graves", attention_alignment=D.ALIGNMENT, epsilon=D.EPS)
    p = _oracle_params(d, cell, L, H, E, A)

    def leaf(t):
        return t.double().clone().requires_grad_()

    seq_g, seq_c = [leaf(x) for x in d["seq_g"]], [leaf(x) for x in d["seq_c"]]
    h0, c0 = [leaf(x) for x in d["h0"]], [leaf(x) for x in d["cst0"]]
    w0, k0, ctx = leaf(d["w0"]), leaf(d["kappa0"]), leaf(d["ctx"])
    states = [(h0[l], c0[l]) for l in range(L)] if cell else list(h0)
    hs, cs, ws, ks, phis, avs = [[x] for x in h0], [[x] for x in c0], [w0], [k0], [], []
    for t in range(T):
        seq_in = [[seq_g[l][t]] if cell else [seq_c[l][t], seq_g[l][t]] for l in range(L)]
        states, outs, k, w, phi, a = R.decoder_step(p, cfg, seq_in, states, ks[t], ws[t], ctx)
        for l in range(L):
            outs[l].retain_grad()
            hs[l].append(outs[l])
            if cell:
                cs[l].append(states[l][1])
        w.retain_grad()
        ws.append(w); ks.append(k); phis.append(phi); avs.append(a)
    S = sum((hs[l][s] * d["dh_in"][l][s].double()).sum() for l in range(L) for s in range(T + 1))
    S = S + sum((ws[s] * d["dw_in"][s].double()).sum() for s in range(T + 1)) + (ks[T] * d["dkappa_in"].double()).sum()
    if cell:
        S = S + sum((cs[l][T] * d["dcell_in"][l].double()).sum() for l in range(L))
    S.backward()
    got = dict(w=torch.stack(ws), kappa=torch.stack(ks), phi=torch.stack(phis), a=torch.stack(avs), dkappa=k0.grad,
               dw0=w0.grad, dw=torch.stack([x.grad for x in ws[1:]]), dctx=ctx.grad)
    for l in range(L):
        got["h%d" % l] = torch.stack(hs[l])
        got["dh0_%d" % l] = h0[l].grad
        got["dhT_%d" % l] = torch.stack([x.grad for x in hs[l][1:]])
        got["dG%d" % l] = seq_g[l].grad
        if cell:
            got["cst%d" % l] = torch.stack(cs[l])
            got["dcell%d" % l] = c0[l].grad
        else:
            got["dC%d" % l] = seq_c[l].grad
    for n, v in got.items():
        assert rel_err(v.detach(), ref[n]) <= 1e-12, (n, rel_err(v.detach(), ref[n]))
    dbatt = torch.cat([p[f"/parrot/h1_to_att/fork_{n}.b"].grad for n in ("alpha", "beta", "kappa")])
    assert rel_err(ref["dp"].sum((0, 1)), dbatt) <= 1e-12
    # the buffers the oracle's step does not return: the reference's own identities
    A_ = slice(A, 2 * A)
    pre = torch.stack([ref["h0"][t + 1] @ d["WattT"].double().t() + d["batt"].double() for t in range(T)])
    assert rel_err(ref["b"], torch.exp(pre[..., A_]) + D.EPS) <= 1e-12
    if not cell:
        for l in range(L):
            assert rel_err(ref["rh%d" % l], ref["r%d" % l] * ref["h%d" % l][:-1]) <= 1e-12
            hn = ref["c%d" % l] * ref["z%d" % l] + ref["h%d" % l][:-1] * (1 - ref["z%d" % l])
            assert rel_err(hn, ref["h%d" % l][1:]) <= 1e-12
    assert set(ref) == set(D.forward_names(cell, L) + D.backward_names(cell, L))


# ---- routes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(D.CASES))
def test_expected_route_is_what_the_library_resolves(monkeypatch, name):
    """Schedule and backward tick of a descriptor like the case's, on fake addresses (nothing is launched).  Whether the
    persistent scan takes a plan depends on the device's grid: tests/test_gpu_decoder_scan_edges.py asserts it."""
    L, lib = _lib()
    case = D.CASES[name]
    monkeypatch.setenv("PARROT_TRACE_ONLY", "1")
    with switches(**{k: v for k, v in D.environment(case).items() if v is not None}):
        ar, d = D.case_arena_descriptor(L, case)
        plan = C.c_void_p()
        assert lib.parrot_decoder_create(C.byref(d), C.byref(plan)) == 0
    try:
        want = D.expected_route(case)
        assert (lib.parrot_decoder_schedule(plan), lib.parrot_decoder_backward_tick(plan)) == (want["schedule"], want["tick"])
    finally:
        lib.parrot_decoder_destroy(plan)


def test_routes_the_table_claims_to_visit():
    routes = {(c.cell, r["schedule"], r["tick"], r["persistent"]) for c in D.CASES.values() for r in [D.expected_route(c)]}
    for want in [(D.GRU, 0, 0, 0), (D.GRU, 0, 8, 0), (D.GRU, 3, 0, 0), (D.GRU, 5, 0, 0), (D.GRU, 5, 8, 0), (D.GRU, 5, 8, 1),
                 (D.GRU, 5, 0, 0), (D.LSTM, 0, 0, 0), (D.LSTM, 3, 0, 0), (D.LSTM, 5, 0, 0), (D.LSTM, 7, 0, 0)]:
        assert want in routes, want
    rows = {c.B: D.expected_route(c) for c in D.CASES.values() if c.group == "rows" and c.persist}
    assert rows[64] == dict(schedule=5, tick=8, persistent=1) and rows[65] == dict(schedule=5, tick=0, persistent=0)
    s7 = {c.B: D.expected_route(c)["schedule"] for c in D.CASES.values() if c.group == "rows" and "-s7-" in c.id}
    assert s7[64] == 7 and s7[65] == 0
    one = [D.expected_route(c) for c in D.CASES.values() if c.L == 1]
    assert one and all(r["schedule"] == 0 and r["tick"] == 0 for r in one)
    plain = [D.expected_route(c) for c in D.CASES.values() if not c.tiled]
    assert plain and all(r["tick"] == 0 for r in plain)


@pytest.mark.parametrize("what,kw", [("T = 0", dict(T=0)), ("B = 0", dict(B=0)), ("L = 0", dict(nl=0)), ("L = 4", dict(nl=4)),
                                     ("bf16 without fragment-major copies", dict(bf16=1, tiled=False, H=64, E=32, cell=1))])
def test_create_refuses(monkeypatch, what, kw):
    L, lib = _lib()
    monkeypatch.setenv("PARROT_TRACE_ONLY", "1")
    kw = dict(kw)
    nl, cell = kw.pop("nl", 2), kw.pop("cell", 0)
    with switches():
        ar, d = D.arena_descriptor(L, cell, min(max(nl, 1), 3), 0, **kw)
        d.L = nl
        plan = C.c_void_p()
        assert lib.parrot_decoder_create(C.byref(d), C.byref(plan)) == BADARG, what


# ---- the table ---------------------------------------------------------------------------------------------------------------
def test_table_premises():
    assert set(D.GROUPS) == {"rows", "steps", "widths", "paths", "seq", "window"} and all(D.GROUPS.values())
    assert len(set(D.CASES)) == len(D.CASES) == sum(len(v) for v in D.GROUPS.values())
    for c in D.CASES.values():
        assert c.T * c.B * max(4 * c.H, c.U) <= D.MAX_ELEMENTS, c.id
        assert 1 <= c.L <= 3 and c.accum in (0, 2) and c.seq in ("none", "l0", "all")
    assert {c.B for c in D.CASES.values() if c.group == "rows"} == {1, 15, 16, 17, 64, 65}
    assert {(c.L, c.T) for c in D.CASES.values() if c.group == "steps"} == {(l, t) for l in (1, 2, 3) for t in (1, 2, 5)}
    for c in D.CASES.values():  # every path of a data set is compared with another one, or the data set has one path
        for other in D.twins(c):
            assert D.data_key(D.CASES[other]) == D.data_key(c)


def test_data_does_what_the_table_says():
    for c in D.CASES.values():
        d = D.data(D.data_key(c))
        assert bool((d["kappa0"] > 0).all())
        for l in range(c.L):
            assert all(bool(d["dh_in"][l][s].any()) for s in range(c.T + 1))
            K = D.krows(c, l)
            assert float(d["Wg"][l].abs().max()) <= 1 / K ** 0.5 and d["Wg"][l].shape == (K, D.gate_width(c))
            assert (d["seq_g"][l] is not None) == bool((D.seq_init(c) >> l) & 1)
        assert all(bool(d["dw_in"][s].any()) for s in range(c.T + 1)) and bool(d["dkappa_in"].all())
    a, b = D.data(D.data_key(c)), D.data(D.data_key(c), 1)
    assert not torch.equal(a["Wg"][0], b["Wg"][0]) and not torch.equal(a["h0"][0], b["h0"][0])


@pytest.mark.parametrize("att_type", [0, 1])
def test_window_cases_leave_and_keep_their_support(att_type):
    """The reference evaluated in float32: every (t, row) of the U = 200 case has at least 100 exactly-zero phi entries and
    at least 3 non-zero ones, kappa stays below U, b ~ 1 and kappa advances by about 1 per step; past the text phi is
    exactly zero everywhere."""
    wide = _find("window", "at%d-dense0" % att_type, D.GRU)
    key = D.data_key(wide)
    f32 = D.scan_reference(D.data(key), key.cell, key.L, att_type, dtype=torch.float32)
    phi = f32["phi"]
    assert phi.dtype == torch.float32 and phi.shape == (wide.T, wide.B, 200)
    assert int((phi == 0).sum(-1).min()) >= 100 and int((phi != 0).sum(-1).min()) >= 3
    assert float(f32["kappa"].max()) < wide.U
    step = f32["kappa"][1:] - f32["kappa"][:-1]
    assert 0.5 < float(step.min()) and float(step.max()) < 2.0 and 0.5 < float(f32["b"].min()) and float(f32["b"].max()) < 2.0
    width = (phi != 0).float().argmax(-1)  # first non-zero position; the last one from the flipped row
    last = phi.shape[-1] - 1 - (phi.flip(-1) != 0).float().argmax(-1)
    span = last - width + 1
    assert int(span.min()) <= 64 < int(span.max())  # supports on either side of the narrow backward path's cap
    past = _find("window", "at%d-past" % att_type, D.GRU)
    key = D.data_key(past)
    f32 = D.scan_reference(D.data(key), key.cell, key.L, att_type, dtype=torch.float32)
    assert not bool(f32["phi"].any()) and float(D.data(key)["kappa0"].min()) > past.U


# ---- noise floors ------------------------------------------------------------------------------------------------------------
def test_noise_table_covers_every_case():
    table = D.noise_table()
    for c in D.CASES.values():
        row = table[D.noise_name(c)]
        names = set(D.forward_names(c.cell, c.L) + D.backward_names(c.cell, c.L)) | {n + ":elem" for n in D.ELEMENTWISE}
        assert set(row) == names, c.id
        assert all(0 <= v < 1e-2 for v in row.values()), (c.id, row)
        for n in names:
            t = D.tolerance(c, n.split(":")[0], elem=n.endswith(":elem"))
            assert t >= (D.TOL_FWD if n.split(":")[0] in D.forward_names(c.cell, c.L) else D.TOL_BWD)
            assert t <= 1e-2


@pytest.mark.parametrize("group,tag,cell", [("paths", "default", D.GRU), ("window", "at0-dense0", D.GRU)])
def test_noise_row_is_what_the_recorder_wrote(group, tag, cell):
    """One row recomputed (tools/record_decoder_scan_noise.py): a float32 evaluation on another build of torch may sum in
    another order, so every entry is held to a factor of 3 of the file, not to its digits."""
    torch.set_num_threads(1)
    case = _find(group, tag, cell, L=2)
    row, want = D.noise_row(case), D.noise_table()[D.noise_name(case)]
    for n, v in row.items():
        assert want[n] / 3 <= v <= want[n] * 3 or max(v, want[n]) < 1e-9, (n, v, want[n])

"""The premises of tests/test_gpu_trainops_edges.py, checked without a GPU: every group of tests/trainops_cases.py has
the structure its name claims, the integer cases are exact in float32, the references agree with torch float64 autograd
of the straightforward formulation, and the buffers stay small."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import trainops_cases as TC


def _group(table, group):
    hits = [c for c in table.values() if c.group == group]
    assert hits, group
    return hits


# ---- the tables as such -------------------------------------------------------------------------------------------------
def test_ids_are_unique_and_keyed():
    tables = (TC.FWD, TC.BWD, TC.CE, TC.WN, TC.QUANT)
    ids = [k for t in tables for k in t]
    assert len(ids) == len(set(ids))
    for t in tables:
        assert all(k == c.id for k, c in t.items())
    assert set(TC.WN_ACC_CASES) <= set(TC.WN)


def test_size_cap():
    for c in TC.FWD.values():
        assert max(c.J * c.Q * c.D, c.N * c.ldy, c.N * c.ldadd, c.N * c.J) <= TC.MAX_FLOATS, c.id
    for c in TC.BWD.values():
        ws = c.J * (-(-c.N // TC.GS_CH) + c.Q) * c.D
        assert max(c.J * c.Q * c.D, c.N * c.lddy, ws) <= TC.MAX_FLOATS, c.id
    for c in TC.CE.values():
        assert c.rows * max(c.ld, c.ldd) <= TC.MAX_FLOATS
    for c in TC.WN.values():
        assert c.K * max(c.ld, c.ldo, c.ldd, c.lddw) <= TC.MAX_FLOATS
    big = [c for c in TC.QUANT.values() if c.rows * max(c.ld, c.ldo) > TC.MAX_FLOATS]
    assert len(big) <= 3 and all(c.group in TC.QUANT_CLAMP_GROUPS for c in big)
    assert max(TC.RELU_N) <= TC.MAX_FLOATS


def test_data_is_seeded_from_the_key():
    c = TC.BWD[sorted(TC.BWD)[0]]
    a, b = TC.bwd_data(c), TC.bwd_data(c)
    assert all(torch.equal(a[k], b[k]) for k in a)
    c = TC.WN["wn-K-K65-N65"]
    a, b = TC.wn_data(c), TC.wn_data(c)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert not torch.equal(TC.wn_data(TC.WN["wn-K-K64-N65"])["g"], a["g"])


# ---- gather-sum forward -------------------------------------------------------------------------------------------------
def test_fwd_groups():
    cols = _group(TC.FWD, "fwd-cols")
    assert {c.D for c in cols} == {4, 12, 20, 1020, 1024, 1028}
    assert all(256 % (D // 4) != 0 for D in (12, 20, 1020)) and all(256 % (D // 4) == 0 for D in (4, 1024))
    assert 1028 // 4 == 257                                   # a second column pass with one live lane
    for c in cols:
        assert c.N == 2 * TC.rows_per_block(c.D) + 1          # two full blocks and one row
    J = {c.J for c in _group(TC.FWD, "fwd-J")}
    assert {1, 4, 8} <= J and any(j > 4 and j % 4 for j in J)
    assert {(c.D, c.J) for c in _group(TC.FWD, "fwd-J") if c.D == 4} == {(4, 1), (4, 4), (4, 8)}
    rows = _group(TC.FWD, "fwd-rows")
    rpb = TC.rows_per_block(32)
    assert {rpb - 1, rpb, rpb + 1, 1} <= {c.N for c in rows if c.D == 32}
    assert all(c.Q == 1 for c in _group(TC.FWD, "fwd-Q1"))
    for c in TC.FWD.values():
        assert c.D % 4 == 0 and c.ldy % 4 == 0 and c.ldadd % 4 == 0 and c.ldy > c.D and c.ldadd > c.D
        twin = c.id.replace("-add", "-noadd") if c.has_add else c.id.replace("-noadd", "-add")
        assert TC.FWD[twin].has_add == 1 - c.has_add
        idx = TC.fwd_data(c)["idx"]
        assert int(idx.min()) == 0 and int(idx.max()) == c.Q - 1
        if c.N >= 2:
            assert bool((idx == 0).any(0).all()) and bool((idx == c.Q - 1).any(0).all()), "0 and Q - 1 at every j"


# ---- segmented-sum backward ---------------------------------------------------------------------------------------------
def test_bwd_groups():
    for c in _group(TC.BWD, "bwd-aligned"):
        assert bool((TC.bwd_data(c)["offs"] % TC.GS_CH == 0).all())
    for c in _group(TC.BWD, "bwd-shifted"):
        assert bool((TC.bwd_data(c)["offs"][:, 1:] % TC.GS_CH == 1).all())
    for c in _group(TC.BWD, "bwd-before"):
        assert bool((TC.bwd_data(c)["offs"][:, 1:-1] % TC.GS_CH == TC.GS_CH - 1).all())
    for c in _group(TC.BWD, "bwd-runs"):
        for r in c.runs:
            assert {7, 8, 9, 16, 17} <= set(r)
    assert any(c.N == c.Q == 256 and all(set(r) == {1} for r in c.runs) for c in _group(TC.BWD, "bwd-one-per-bin"))
    for c in _group(TC.BWD, "bwd-sparse"):
        for r in c.runs:
            assert r[0] == 0 and r[-1] == 0 and sum(1 for v in r if v) * 4 < c.Q
    for c in _group(TC.BWD, "bwd-long"):
        offs = TC.bwd_data(c)["offs"]
        for j, r in enumerate(c.runs):
            q = max(range(c.Q), key=lambda k: r[k])
            a, b = int(offs[j, q]), int(offs[j, q + 1])
            assert (b - 1) // TC.GS_CH - a // TC.GS_CH + 1 >= 3, "a run across three or more chunks"
            assert 0 < r[q - 1] < 8 and 0 < r[q + 1] < 8, "short neighbours"
    assert all(c.D > 1024 for c in _group(TC.BWD, "bwd-D"))
    assert all(c.Q == 1 or c.N == 1 for c in _group(TC.BWD, "bwd-Q1"))
    for c in TC.BWD.values():
        twin = c.id[:-3] + ("set" if c.accumulate else "acc")
        assert TC.BWD[twin].accumulate == 1 - c.accumulate
        assert c.D % 4 == 0 and c.lddy % 4 == 0 and c.lddy > c.D


def test_histogram_builder_follows_the_recipe():
    for c in TC.BWD.values():
        d = TC.bwd_data(c)
        idx, perm, offs = d["idx"], d["perm"].long(), d["offs"].long()
        assert idx.shape == (c.N, c.J) and d["perm"].dtype is torch.int32 and d["offs"].dtype is torch.int32
        for j in range(c.J):
            assert torch.equal(torch.bincount(idx[:, j], minlength=c.Q), torch.tensor(c.runs[j]))
            assert torch.equal(offs[j, 1:] - offs[j, :-1], torch.tensor(c.runs[j]))
            assert int(offs[j, 0]) == 0 and int(offs[j, c.Q]) == c.N
            assert torch.equal(torch.sort(perm[j])[0], torch.arange(c.N))
            for q in range(c.Q):
                rows = perm[j, offs[j, q]:offs[j, q + 1]]
                assert bool((idx[rows, j] == q).all()) and bool((rows[1:] > rows[:-1]).all()), "sorted by (index, row)"
        if c.Q > 1 and c.N > 4:
            assert not torch.equal(perm[0], torch.arange(c.N)), "the rows of a bin are scattered"


def test_integer_cases_are_exact_in_float32():
    """Every partial sum, in any order, is an integer of magnitude at most (addends) * 8 (and for the squares 64)."""
    for c in TC.FWD.values():
        d = TC.fwd_data(c)
        for t in (d["tbl"], d["add"]):
            assert torch.equal(t, t.round()) and float(t.abs().max()) <= 8
        assert 8 * (c.J + 1) < 2 ** 24
    for c in TC.BWD.values():
        d = TC.bwd_data(c)
        for t in (d["dy"], d["old"]):
            assert torch.equal(t, t.round()) and float(t.abs().max()) <= 8
        assert 8 * (max(max(r) for r in c.runs) + 1) < 2 ** 24
    for c in _group(TC.WN, "wn-int"):
        d = TC.wn_data(c)
        for t in d.values():
            assert torch.equal(t, t.round()) and float(t.abs().max()) <= 8
        assert 64 * c.K < 2 ** 24
        ss = (d["W"].double() ** 2).sum(0)
        assert bool((ss > 0).all()) and bool((d["g"] != 0).all())
        sq = TC.wn_is_square_column(c.N)
        root = ss[sq].sqrt().round()
        assert bool(sq.any()) and torch.equal(root * root, ss[sq]), "perfect squares"
        assert bool((ss[~sq].sqrt().round() ** 2 != ss[~sq]).any()) or c.K == 1


def test_gather_sum_references_against_autograd():
    """Embedding, reshape, matmul in float64 autograd: the forward is the gather-sum over the folded table, and the
    gradient with respect to that table is the segmented sum."""
    for name in ("fwd-J-N70-J5-Q7-D36-add", "fwd-cols-N171-J3-Q5-D12-noadd"):
        c = TC.FWD[name]
        d = TC.fwd_data(c)
        EMB = 3
        g = TC._gen("emb", name)
        E = torch.randn(c.Q, EMB, generator=g, dtype=torch.float64)
        W1 = torch.randn(c.J * EMB, c.D, generator=g, dtype=torch.float64)
        tbl = torch.stack([E @ W1[j * EMB:(j + 1) * EMB] for j in range(c.J)])
        add = d["add"] if c.has_add else None
        want = torch.nn.functional.embedding(d["idx"], E).reshape(c.N, c.J * EMB) @ W1
        if add is not None:
            want = want + add.double()
        got = TC.gather_sum_reference(tbl, d["idx"], add)
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    for name in ("bwd-runs-a-N109-J2-Q9-D12-set", "bwd-sparse-a-N334-J2-Q64-D8-acc"):
        c = TC.BWD[name]
        d = TC.bwd_data(c)
        tbl = torch.zeros(c.J, c.Q, c.D, dtype=torch.float64, requires_grad=True)
        y = sum(tbl[j][d["idx"][:, j]] for j in range(c.J))
        y.backward(d["dy"].double())
        old = d["old"] if c.accumulate else None
        want = tbl.grad + (old.double() if old is not None else 0.0)
        assert torch.equal(TC.segmented_sum_reference(d["idx"], d["dy"], c.Q, old), want)


# ---- cross-entropy ------------------------------------------------------------------------------------------------------
def test_ce_groups():
    assert {c.Q for c in _group(TC.CE, "ce-Q")} == {1, 2, 63, 64, 65, 127, 129, 257}
    assert {c.rows for c in _group(TC.CE, "ce-rows")} == {1, 2, 3, 4, 5}
    assert all(c.ld > c.Q and c.ldd > c.Q and c.ld != c.ldd for c in TC.CE.values() if c.group != "ce-dense")
    for c in _group(TC.CE, "ce-Q"):
        d = TC.ce_data(c)
        x, t, rs = d["x"], d["target"], d["rowscale"]
        assert c.rows >= 16 and int(t.min()) == 0 and int(t.max()) == c.Q - 1
        assert float(x[0].min()) > 60 and float(x[1].max()) < -60
        fin = torch.where(torch.isinf(x), torch.zeros_like(x), x)
        assert bool(torch.isfinite(x.gather(1, t[:, None])).all()), "-inf only away from the target"
        if c.Q >= 2:
            assert float(x[2].max() - x[2].min()) > 200 and bool(torch.isinf(x[3]).any())
            am = fin.argmax(1)
            assert bool((t == am)[2::4].all()) and not bool((t == am)[3::4].any()), "at the argmax and away from it"
        assert {float(v) for v in rs} == {float(np.float32(v)) for v in TC.CE_ROWSCALES}
        pairs = {(float(rs[i]), float(rs[i + 1])) for i in range(c.rows - 1)}
        assert (float(np.float32(1e-3)), 1.0) in pairs and any(a == 0.0 for a, _ in pairs)
    assert TC.ce_chain_length(1) == 11 and TC.ce_chain_length(64) == 11 and TC.ce_chain_length(257) == 15


def test_ce_reference_against_autograd():
    for c in TC.CE.values():
        d = TC.ce_data(c)
        ref = TC.ce_reference(d["x"], d["target"], d["rowscale"])
        x = d["x"].double().requires_grad_()
        ce = F.cross_entropy(x, d["target"], reduction="none")
        (ce * d["rowscale"].double()).sum().backward()
        assert bool(torch.isfinite(ref["ce"]).all()) and bool(torch.isfinite(ref["dlogits"]).all())
        assert float((ce.detach() - ref["ce"]).abs().max()) <= 1e-12 * (1 + float(ref["ce"].abs().max()))
        assert float((x.grad - ref["dlogits"]).abs().max()) <= 1e-14
        inf = torch.isinf(d["x"])
        assert bool((ref["dlogits"][inf] == 0).all()) and bool((ref["dlogits"][d["rowscale"] == 0] == 0).all())
        b = TC.dlogits_bound(c, d["x"], d["rowscale"], ref)
        assert bool(torch.isfinite(b).all()) and bool((b[d["rowscale"] == 0] == 0).all())


# ---- ReLU gate ----------------------------------------------------------------------------------------------------------
def test_relu_data():
    assert TC.RELU_N == (0, 4, 1020, 1024, 1028) and float(TC.DENORM_MIN) > 0
    for n in TC.RELU_N:
        dy, gate = TC.relu_data(n)
        ref = TC.relu_reference(dy, gate)
        assert dy.dtype == gate.dtype == ref.dtype == np.float32 and ref.shape == (n,)
        if n == 0:
            continue
        bits = gate.view(np.int32)
        assert (bits == 1).any() and (bits == 0).any() and (bits == np.int32(-2 ** 31)).any() and np.isnan(gate).any()
        closed = ~(gate > 0)
        assert (ref[closed].view(np.int32) == 0).all(), "+0.0 where the gate is closed"
        assert np.isnan(dy[closed]).any() and not np.isnan(ref).any()
        assert (ref[bits == 1] == dy[bits == 1]).all() and (dy[bits == 1] != 0).all(), "the smallest denormal is open"
        if n >= 1020:
            assert np.isinf(gate).any() and (gate < 0).any() and np.isinf(dy[closed]).any()
            assert (gate[-len(TC.RELU_GATES):].view(np.int32) == gate[:len(TC.RELU_GATES)].view(np.int32)).all()


# ---- weight-norm --------------------------------------------------------------------------------------------------------
def test_wn_groups():
    Ks = {c.K for c in _group(TC.WN, "wn-K")}
    for edge in (4, TC.WN_KS, TC.WN_RC):
        assert {edge - 1, edge, edge + 1} <= Ks
    for K in (1, 17):                              # slices that start past K
        assert K in Ks and (TC.WN_KS - 1) * TC.wn_slice_rows(K) >= K
    rounds = {TC.wn_unrolled_rounds(K) for K in Ks}
    assert {0, 1} <= rounds and max(rounds) >= 2
    assert {1, 63} <= {c.N for c in _group(TC.WN, "wn-N")} and any(c.N > 128 for c in TC.WN.values())
    for c in TC.WN.values():
        assert min(c.ld, c.ldo, c.ldd, c.lddw) > c.N and len({c.ld, c.ldo, c.ldd, c.lddw}) == 4
    for c in TC.WN.values():
        if c.kind != "float":
            continue
        d = TC.wn_data(c)
        nrm = d["W"].double().norm(dim=0)
        assert abs(float(nrm[0]) / 1e-3 - 1) < 1e-6 and abs(abs(float(d["g"][0])) / 1e3 - 1) < 1e-6
        if c.N > 1:
            assert abs(float(nrm[-1]) / 1e3 - 1) < 1e-6 and abs(abs(float(d["g"][-1])) / 1e-3 - 1) < 1e-6
    assert TC.wn_chain_length(1) == 1 + 4 + 16 and TC.wn_chain_length(529) == 9 + 4 + 16


def test_wn_reference_against_autograd():
    for name in ("wn-K-K65-N65", "wn-N-K70-N130", "wn-int-K17-N63", "wn-K-K1-N65"):
        c = TC.WN[name]
        d = TC.wn_data(c)
        ref = TC.wn_reference(d["W"], d["g"], d["dWe"])
        W, g = d["W"].double().requires_grad_(), d["g"].double().requires_grad_()
        out = W * (g / W.norm(dim=0))
        out.backward(d["dWe"].double())
        for got, want, scale in ((ref["W_eff"], out.detach(), out.detach().abs()),
                                 (ref["dg"], g.grad, ref["absdot"] / ref["norm"]),
                                 (ref["dW"], W.grad, (d["g"].double() / ref["norm"]).abs() * (d["dWe"].double().abs() + 1))):
            assert bool(((got - want).abs() <= 1e-12 * scale + 1e-300).all()), name
        b = TC.wn_bounds(c, d["W"], d["g"], d["dWe"], ref, d["old_dW"], d["old_dg"])
        assert all(bool(torch.isfinite(v).all()) and bool((v >= 0).all()) for v in b.values())
        assert all(bool((v > 0).all()) for v in b.values()) or c.kind == "int"


# ---- quantisers ---------------------------------------------------------------------------------------------------------
def test_quant_groups():
    clamps = {"q-clamp-minmax": TC.Q_MINMAX_CLAMP, "q-clamp-quantize": TC.Q_QUANT_CLAMP, "q-clamp-mu2linear": TC.MU2LIN_CLAMP}
    assert (TC.Q_MINMAX_CLAMP, TC.Q_QUANT_CLAMP, TC.MU2LIN_CLAMP) == (131072, 262144, 1048576)
    assert tuple(clamps) == TC.QUANT_CLAMP_GROUPS
    for group, clamp in clamps.items():
        for c in _group(TC.QUANT, group):
            assert c.n - 2 >= clamp, "the extremes lie past what the clamped grid reads in its full rounds"
            x = TC.quant_data(c)
            assert (x.argmin(1) == c.n - 1).all() and (x.argmax(1) == c.n - 2).all()
    for c in TC.QUANT.values():
        assert c.ld > c.n and c.ldo > c.n and c.ldo % 2 == 1
        x = TC.quant_data(c)
        assert x.shape == (c.rows, c.n) and x.dtype == np.float32
        const = [r for r in range(c.rows) if x[r].max() == x[r].min()]
        assert tuple(const) == TC.quant_constant_rows(c)
    rows = _group(TC.QUANT, "q-rows")
    assert any((TC.quant_data(c).max(1) < 0).any() for c in rows) and any(c.n == 2 for c in rows)
    assert any(TC.quant_constant_rows(c) for c in rows)

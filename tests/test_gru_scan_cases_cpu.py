"""The premises of tests/test_gpu_gru_scan_edges.py, checked without a GPU: the float64 reference of
tests/gru_scan_cases.py against the oracle (values through `gru_scan`, gradients through autograd -- which is what pins
the hand indexing of time t against step s for a reversed chain), the shape boundary of the row-wise kernels against the
library's own predicate, and every premise of the case table."""
import pytest
import torch

from tests import gru_scan_cases as G


@pytest.fixture(scope="module")
def lib():
    from parrot_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


REF_SHAPES = [(1, 3, 16, "none"), (4, 5, 16, "random"), (5, 3, 32, "frac"), (3, 4, 48, "row"), (2, 2, 16, "ones")]


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("T,B,H,mask_kind", REF_SHAPES)
def test_reference_matches_oracle(T, B, H, mask_kind, reverse):
    from oracle import parrot_ref as R
    d = G.chain_data(T, B, H, 0)
    mask = G.mask_data(T, B, mask_kind)
    ref = G.reference_chain(d, mask, reverse)
    inp, gin, h0 = (d[k].double().requires_grad_() for k in ("inp", "gin", "h0"))
    m = None if mask is None else mask.double()
    # a reversed chain = the oracle's scan over the flipped sequence; its output s is the state of slot s + 1
    flip = (lambda x: x.flip(0)) if reverse else (lambda x: x)
    hs = R.gru_scan(flip(inp), flip(gin), h0, d["Wc"].double(), d["Wg"].double(), None if m is None else flip(m))
    assert hs.shape == (T, B, H)
    assert float((ref["h"][1:] - hs.detach()).abs().max()) <= 1e-12
    assert torch.equal(ref["h"][0], d["h0"].double())
    (hs * d["dh_in"].double()[1:]).sum().backward()
    for name, got, want in (("dC", ref["dC"], inp.grad), ("dG", ref["dG"], gin.grad), ("dh[0]", ref["dh"][0], h0.grad)):
        assert float((got - want).abs().max()) <= 1e-12, name
    # saved activations sit at the time their step consumed: recompute them from the states, by hand
    for s in range(T):
        t = T - 1 - s if reverse else s
        hp = ref["h"][s]
        g = torch.sigmoid(hp @ d["Wg"].double() + d["gin"].double()[t])
        assert float((ref["z"][t] - g[:, :H]).abs().max()) <= 1e-12
        assert float((ref["r"][t] - g[:, H:]).abs().max()) <= 1e-12
        assert float((ref["rh"][t] - hp * g[:, H:]).abs().max()) <= 1e-12
        assert float((ref["c"][t] - torch.tanh(ref["rh"][t] @ d["Wc"].double() + d["inp"].double()[t])).abs().max()) <= 1e-12


def test_reference_slot_gradients_are_totals():
    """dh[s] of the reference = what flows into slot s from everything after it plus the consumers' own dh_in[s]:
    cutting the scan at slot s and restarting from there gives the same dh[s] - dh_in[s]."""
    T, B, H = 4, 3, 16
    d = G.chain_data(T, B, H, 1)
    mask = G.mask_data(T, B, "random")
    full = G.reference_chain(d, mask, False)
    for s in (1, 2, 3):
        tail = dict(d, inp=d["inp"][s:], gin=d["gin"][s:], h0=full["h"][s].float(), dh_in=d["dh_in"][s:].clone())
        tail["dh_in"][0].zero_()
        sub = G.reference_chain(tail, mask[s:], False)
        # (h0 of the restart is the float32 rounding of the state: agreement to float32 resolution, not float64)
        want = full["dh"][s] - d["dh_in"][s].double()
        assert float((sub["dh"][0] - want).abs().max()) <= 1e-5 * float(want.abs().max())


def test_rowwise_supported_boundary(lib):
    from parrot_amd import ops
    for H in range(16, 129, 16):
        for nchain in (1, 2, 3, 4):
            assert ops.gru_rowwise_supported(3, 21, H, nchain), (H, nchain)
    for H in (8, 24, 100, 144, 256):
        assert not ops.gru_rowwise_supported(3, 21, H, 2), H
    for nchain in (0, 5):
        assert not ops.gru_rowwise_supported(3, 21, 64, nchain), nchain
    assert not ops.gru_rowwise_supported(0, 21, 64, 2)
    assert not ops.gru_rowwise_supported(3, 0, 64, 2)
    assert ops.gru_rowwise_supported(1, 1, 16, 1)
    for T, B, H, n in [(1, 1, 16, 1), (3, 21, 128, 4), (3, 21, 129, 1), (3, 21, 15, 1), (0, 1, 16, 1), (3, 21, 0, 1), (3, 21, -16, 1)]:
        assert ops.gru_rowwise_supported(T, B, H, n) == G.shape_supported(T, B, H, n), (T, B, H, n)


def test_route_query_rejects_null(lib):
    import ctypes as C
    info = (C.c_int * 4)()
    assert lib.parrot_gru_seq_route(None, info) == 10001


@pytest.mark.parametrize("name", sorted(G.CASES))
def test_case_premise(lib, name):
    from parrot_amd import ops
    c = G.CASES[name]
    n = len(c.reverse)
    supported = ops.gru_rowwise_supported(c.T, c.B, c.H, n)
    assert supported == G.shape_supported(c.T, c.B, c.H, n)
    assert supported == (c.path in (G.ROWWISE, G.SWITCH)), "the case's path against the predicate"
    env = G.environment(c)
    assert (env["PARROT_GRU_ROWWISE"] == "0") == (c.path == G.SWITCH)
    want = G.expected_route(c)
    assert want["rowwise"] == (c.path == G.ROWWISE) and (want["reason"] == "rowwise") == want["rowwise"]
    if c.path == G.ROWWISE:
        assert env["PARROT_RG_WAVES"] == str(c.waves) and want["waves"] in (4, 8) and want["nch"] * 16 == c.H
    # the mask conditions
    m = G.mask_data(c.T, c.B, c.mask)
    if c.mask == "none":
        assert m is None
    else:
        assert m.shape == (c.T, c.B) and m.dtype == torch.float32
    if c.mask == "random":
        assert bool(((m == 0) | (m == 1)).all())
        assert bool((m == 0).any(1).all()) and bool((m == 1).any(1).all()), "a 0 and a 1 in every time step"
    if c.mask == "row":
        assert int((m == 0).all(0).sum()) == 1 and int((m == 1).all(0).sum()) == c.B - 1
    if c.mask == "ones":
        assert bool((m == 1).all())
    if c.mask == "frac":
        assert bool(((m > 0) & (m < 1)).all())
    # the header's contract for the consumers' gradients
    for i in range(n):
        dh_in = G.chain_data(c.T, c.B, c.H, i)["dh_in"]
        assert not bool(dh_in[0].any()) and all(bool(dh_in[s].any()) for s in range(1, c.T + 1))


def test_table_covers_what_it_claims():
    C = G.CASES.values()
    row = [c for c in C if c.path == G.ROWWISE]
    # every instantiation of the two kernels: H / 16 = 1..8 at 4 and 8 waves, on two blocks with a partial second one
    assert {(c.H // 16, c.waves) for c in row if c.group == "width"} == {(q, w) for q in range(1, 9) for w in (4, 8)}
    assert all(c.B == 21 and c.T == 3 and c.reverse == (0, 1) and c.mask == "random" for c in row if c.group == "width")
    assert {(c.B, c.H) for c in row if c.group == "rows"} == {(b, h) for b in (1, 15, 16, 17) for h in (48, 80)}
    assert {c.T for c in row if c.group == "steps"} == {1, 2, 9} and all(c.H == 112 and c.B == 5 for c in row if c.group == "steps")
    assert {c.reverse for c in row if c.group == "chains"} == {(0,), (1,), (0, 1, 1, 0), (1, 1, 1)}
    assert {c.mask for c in row if c.group == "masks"} == set(G.MASKS)
    assert all(c.H == 64 and c.B == 17 and c.T == 5 for c in row if c.group == "masks")
    # every row-wise rows / chains / masks case has its twin under the switch, and both widths
    for c in row:
        assert G.twin(c, G.ROWWISE, 12 - c.waves) is not None
        if c.group in ("rows", "chains", "masks"):
            assert G.twin(c, G.SWITCH) is not None, c.id
    assert {c.H for c in C if c.path == G.SHAPE} == {8, 100, 144, 256}
    assert all(c.B == 20 and c.T == 3 for c in C if c.path == G.SHAPE)
    assert len(G.CASES) < 200
    # a chain alone against the same chain as one of four: the data of chain 0 does not depend on the plan
    assert G.chain_data(4, 17, 32, 0) is G.chain_data(4, 17, 32, 0)
    assert not torch.equal(G.chain_data(4, 17, 32, 0)["inp"], G.chain_data(4, 17, 32, 1)["inp"])
    assert not torch.equal(G.chain_data(4, 17, 64, 0, 1)["Wg"], G.chain_data(4, 17, 64, 0)["Wg"])
    assert torch.equal(G.chain_data(4, 17, 64, 0, 1)["inp"], G.chain_data(4, 17, 64, 0)["inp"])


@pytest.mark.parametrize("T,B,H", [(1, 1, 4), (6, 3, 20)])
def test_lstm_reference_matches_oracle_cell(T, B, H):
    from oracle import parrot_ref as R
    d = G.lstm_data(T, B, H)
    ref = G.lstm_reference(T, B, H)
    s, c = d["s0"].double(), d["c0"].double()
    for t in range(T):
        s, c = R.lstm_cell(d["pre_in"].double()[t], s, c, d["W"].double())
        assert float((ref["s"][t + 1] - s).abs().max()) <= 1e-12
        assert float((ref["c"][t + 1] - c).abs().max()) <= 1e-12
    assert ref["gates"].shape == (T, B, 4 * H) and ref["dS"].shape == (T + 1, B, H) and ref["dc"].shape == (B, H)
    assert not bool(d["dS_in"][0].any()) and bool(d["dc_in"].any())
    assert len(G.LSTM_SHAPES) == 24


def test_lstm_create_rejects_bad_width(lib):
    import ctypes as C
    from parrot_amd import _lib
    for H, ok in ((6, False), (2, False), (0, False), (4, True), (20, True)):
        d = _lib.LstmSeqDesc()
        d.T, d.B, d.H, d.use_graph = 3, 2, H, 0
        plan = C.c_void_p()
        rc = lib.parrot_lstm_seq_create(C.byref(d), C.byref(plan))
        assert (rc == 0) == ok and (ok or rc == 10001), (H, rc)
        if rc == 0:
            assert lib.parrot_lstm_seq_destroy(plan) == 0

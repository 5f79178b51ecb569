"""Edge tests of the recurrent scans (`parrot_gru_seq_*`, `parrot_lstm_seq_*`): every buffer the kernels write against a
float64 reference of the descriptor's contract, at the shapes of tests/gru_scan_cases.py, on the path the case names.

Every buffer of a plan is a view into a larger allocation with a frame of PAD floats on either side.  Frames hold a NaN
with a payload of their own and must be bit-identical after the run (a write past the last partial 16-row block lands
in one); operands sit in such frames too, so a read outside them poisons the result, and must be unchanged as a whole,
like slot 0 of the states.  Everything the kernels must write starts as NaN.

Every test asserts the plan's route (`GruSeqRunner.route()`) before it asserts a value: a scan that silently fell back to
the other path would otherwise be compared with itself.  Results of table cases are computed once per session and shared
by the tests that need them."""
import contextlib
import ctypes as C
import os

import pytest
import torch

from tests import gru_scan_cases as G
from tests.util import FRAME_BITS, PAD, Framed, _bits, assert_close, rel_err  # noqa: F401

pytestmark = pytest.mark.gpu

BADARG = 10001
PATHS = [(G.ROWWISE, 4), (G.ROWWISE, 8), (G.SWITCH, 0)]
PATH_IDS = ["rowwise-w4", "rowwise-w8", "launch"]


def SHAPES(T, B, H):
    return dict(h=(T + 1, B, H), z=(T, B, H), r=(T, B, H), rh=(T, B, H), c=(T, B, H), inputs=(T, B, H),
                gate_inputs=(T, B, 2 * H), dh=(T + 1, B, H), dG=(T, B, 2 * H), dC=(T, B, H))


@contextlib.contextmanager
def _env(values):
    """Sets (None: unsets) the switches for the creation of a plan, and restores what it found."""
    old = {k: os.environ.get(k) for k in values}
    try:
        for k, v in values.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _path_env(path, waves):
    return {"PARROT_GRU_ROWWISE": "0" if path == G.SWITCH else None, "PARROT_RG_WAVES": str(waves) if waves else None}


def _route_of(path, waves, H):
    return G.expected_route(G.Case("", "", 0, 0, H, (), "none", waves, path))


def _bind_with_null(run, Wg, Wc, mask, null):
    """GruSeqRunner.bind with NULL `inputs` and / or `gate_inputs` in the descriptor."""
    from parrot_amd import _lib
    d = _lib.GruSeqDesc()
    d.T, d.B, d.H, d.nchain, d.use_graph = run.T, run.B, run.H, run.nchain, int(run.use_graph)
    for i in range(run.nchain):
        d.reverse[i] = int(run.reverse[i])
        d.Wg[i], d.Wc[i] = Wg[i].data_ptr(), Wc[i].data_ptr()
        d.inputs[i] = None if null[0] else run.inputs[i].data_ptr()
        d.gate_inputs[i] = None if null[1] else run.gate_inputs[i].data_ptr()
        for k in ("h", "z", "r", "rh", "c", "dh", "dG", "dC"):
            getattr(d, k)[i] = getattr(run, k)[i].data_ptr()
    d.mask = mask.data_ptr() if mask is not None else None
    plan = C.c_void_p()
    _lib.call("parrot_gru_seq_create", C.byref(d), C.byref(plan))
    run._plan, run._weights, run._keep = plan, None, (Wg, Wc, mask)


class Scan:
    """A GruSeqRunner whose buffers, weights and mask sit in frames.  `null` / `zero` = (inputs, gate_inputs): NULL in the
    descriptor / zero-filled; `unaligned`: names of weights placed one float past an aligned address."""

    def __init__(self, dev, T, B, H, reverse, mask_kind, env, use_graph=False, null=(False, False), zero=(False, False),
                 unaligned=()):
        from parrot_amd import ops
        self.T, self.B, self.H, self.reverse, self.mask_kind = T, B, H, tuple(reverse), mask_kind
        self.null, self.zero = null, zero
        n = len(reverse)
        self.run = ops.GruSeqRunner(T, B, H, n, list(reverse), dev, use_graph=use_graph)
        self.fr = {k: [Framed(s, dev) for _ in range(n)] for k, s in SHAPES(T, B, H).items()}
        for k in SHAPES(T, B, H):
            setattr(self.run, k, [f.view for f in self.fr[k]])
        self.fr["Wg"] = [Framed((H, 2 * H), dev, int("Wg" in unaligned)) for _ in range(n)]
        self.fr["Wc"] = [Framed((H, H), dev, int("Wc" in unaligned)) for _ in range(n)]
        self.fr["mask"] = [Framed((T, B), dev)] if mask_kind != "none" else []
        self.fill()
        Wg, Wc = [f.view for f in self.fr["Wg"]], [f.view for f in self.fr["Wc"]]
        mask = self.fr["mask"][0].view if self.fr["mask"] else None
        with _env(env):
            if any(null):
                _bind_with_null(self.run, Wg, Wc, mask, null)
            else:
                self.run.bind(Wg, Wc, mask)
        self.route = self.run.route()

    def data(self, i, variant=0):
        """The operands of chain i as the reference takes them (a NULL operand = zeros)."""
        d = dict(G.chain_data(self.T, self.B, self.H, i, variant))
        if self.null[0] or self.zero[0]:
            d["inp"] = torch.zeros_like(d["inp"])
        if self.null[1] or self.zero[1]:
            d["gin"] = torch.zeros_like(d["gin"])
        return d

    def fill(self, variant=0):
        """Operands in, NaN into everything the kernels must write, frames remembered.  Same addresses every time."""
        nan = float("nan")
        for i in range(len(self.reverse)):
            d = self.data(i, variant)
            fr = {k: v[i].view for k, v in self.fr.items() if k != "mask"}
            fr["inputs"].copy_(torch.full_like(d["inp"], nan) if self.null[0] else d["inp"])  # (NULL: never read)
            fr["gate_inputs"].copy_(torch.full_like(d["gin"], nan) if self.null[1] else d["gin"])
            fr["h"][0].copy_(d["h0"])
            fr["h"][1:].fill_(nan)
            fr["dh"].copy_(d["dh_in"])
            for k in ("z", "r", "rh", "c", "dG", "dC"):
                fr[k].fill_(nan)
            fr["Wg"].copy_(d["Wg"])
            fr["Wc"].copy_(d["Wc"])
        if self.fr["mask"]:
            self.fr["mask"][0].view.copy_(G.mask_data(self.T, self.B, self.mask_kind))
        for frames in self.fr.values():
            for f in frames:
                f.snapshot()

    def go(self):
        """Forward, backward; returns (per chain {name: tensor on the host}, the names of frames and operands touched)."""
        self.run.forward()
        self.run.backward()
        torch.cuda.synchronize()
        out = [{k: getattr(self.run, k)[i].detach().cpu().clone() for k in G.NAMES} for i in range(len(self.reverse))]
        touched = []
        for k, frames in self.fr.items():
            for i, f in enumerate(frames):
                if k in G.NAMES:
                    ok = f.frame_untouched()
                    if k == "h":  # the initial state is the caller's
                        ok = ok and torch.equal(_bits(f.view[0]), f.before[f.lo:f.lo + self.B * self.H])
                else:
                    ok = f.untouched()
                if not ok:
                    touched.append("%s[%d]" % (k, i))
        return out, touched

    def close(self):
        self.run.close()


def _check_values(out, refs, what):
    for ch, (o, ref) in enumerate(zip(out, refs)):
        for k in G.NAMES:
            assert not bool(torch.isnan(o[k]).any()), "%s: %s of chain %d has elements the kernels did not write" % (what, k, ch)
    for ch, (o, ref) in enumerate(zip(out, refs)):
        for k in G.NAMES:
            tol = G.TOL_FWD if k in G.FWD_NAMES else G.TOL_BWD
            print("ratio %s chain %d %s %.4f" % (what, ch, k, rel_err(o[k], ref[k]) / tol))
            assert_close(o[k], ref[k], tol, "%s: %s of chain %d" % (what, k, ch))


def _assert_equal(a, b, what):
    for ch, (x, y) in enumerate(zip(a, b)):
        for k in G.NAMES:
            assert not bool(torch.isnan(x[k]).any()) and not bool(torch.isnan(y[k]).any()), (what, k, ch)
            assert torch.equal(x[k], y[k]), "%s: %s of chain %d differs, max |diff| %.3e" % (
                what, k, ch, float((x[k] - y[k]).abs().max()))


_RESULTS = {}


def _result(dev, case):
    """The table case, run once: dict(route, out, touched)."""
    if case.id not in _RESULTS:
        scan = Scan(dev, case.T, case.B, case.H, case.reverse, case.mask, G.environment(case))
        out, touched = scan.go()
        _RESULTS[case.id] = dict(route=scan.route, out=out, touched=touched)
        scan.close()
    return _RESULTS[case.id]


def _find(group, path, waves, **fields):
    hits = [c for c in G.CASES.values() if c.group.endswith(group) and (c.path, c.waves) == (path, waves)
            and all(getattr(c, k) == v for k, v in fields.items())]
    assert len(hits) == 1, (group, path, waves, fields)
    return hits[0]


# ---- a. every buffer against float64, inside frames -----------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(G.CASES))
def test_every_buffer_against_float64(dev, name):
    case = G.CASES[name]
    res = _result(dev, case)
    assert res["route"] == G.expected_route(case)
    assert res["touched"] == [], "written outside a buffer, or into an operand"
    _check_values(res["out"], G.case_reference(case), name)


# ---- b. path against path ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(c.id for c in G.CASES.values() if c.path == G.ROWWISE and G.twin(c, G.SWITCH)))
def test_rowwise_against_launch_path(dev, name):
    a = G.CASES[name]
    b = G.CASES[G.twin(a, G.SWITCH)]
    ra, rb = _result(dev, a), _result(dev, b)
    assert ra["route"] == G.expected_route(a) and ra["route"]["rowwise"]
    assert rb["route"] == G.expected_route(b) and not rb["route"]["rowwise"]
    for ch, (x, y) in enumerate(zip(ra["out"], rb["out"])):
        for k in G.NAMES:
            assert not bool(torch.isnan(x[k]).any()) and not bool(torch.isnan(y[k]).any()), (k, ch)
            assert_close(x[k], y[k], G.TOL_PATHS, "row-wise vs step launches: %s of chain %d" % (k, ch))


# ---- c. metamorphic checks, bit for bit, on one path ------------------------------------------------------------------------
@pytest.mark.parametrize("path,waves", PATHS, ids=PATH_IDS)
def test_all_ones_mask_is_no_mask(dev, path, waves):
    ones, none = _find("masks", path, waves, mask="ones"), _find("masks", path, waves, mask="none")
    ro, rn = _result(dev, ones), _result(dev, none)
    assert ro["route"] == G.expected_route(ones) and rn["route"] == G.expected_route(none)
    _assert_equal(ro["out"], rn["out"], "all-ones mask vs no mask")


@pytest.mark.parametrize("path,waves", PATHS, ids=PATH_IDS)
def test_chain_alone_is_chain_among_four(dev, path, waves):
    for alone, among in (((0,), (0, 1, 1, 0)), ((1,), (1, 1, 1))):
        a, b = _find("chains", path, waves, reverse=alone), _find("chains", path, waves, reverse=among)
        ra, rb = _result(dev, a), _result(dev, b)
        assert ra["route"] == G.expected_route(a) and rb["route"] == G.expected_route(b)
        _assert_equal(ra["out"], rb["out"][:1], "chain %s alone vs first of %s" % (alone, among))


@pytest.mark.parametrize("null", [(True, False), (False, True), (True, True)], ids=["inputs", "gate_inputs", "both"])
@pytest.mark.parametrize("path,waves", PATHS, ids=PATH_IDS)
def test_null_operands_are_zeros(dev, path, waves, null):
    T, B, H, reverse = 5, 17, 64, (0, 1)
    got = {}
    for kind, kw in (("null", dict(null=null)), ("zero", dict(zero=null))):
        scan = Scan(dev, T, B, H, reverse, "random", _path_env(path, waves), **kw)
        assert scan.route == _route_of(path, waves, H)
        out, touched = scan.go()
        assert touched == [], kind
        got[kind] = out
        refs = [G.reference_chain(scan.data(i), G.mask_data(T, B, "random"), bool(rev)) for i, rev in enumerate(reverse)]
        scan.close()
    _check_values(got["null"], refs, "null %s on %s" % (null, path))
    _assert_equal(got["null"], got["zero"], "NULL operand vs zero-filled")


@pytest.mark.parametrize("path,waves", PATHS, ids=PATH_IDS)
def test_same_plan_twice(dev, path, waves):
    scan = Scan(dev, 4, 17, 64, (0, 1), "random", _path_env(path, waves))
    assert scan.route == _route_of(path, waves, 64)
    first, touched = scan.go()
    assert touched == []
    scan.fill()
    second, touched = scan.go()
    assert touched == []
    scan.close()
    _assert_equal(first, second, "second run of the plan")


# ---- d. weights change between the runs of a captured plan ------------------------------------------------------------------
@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "nograph"])
@pytest.mark.parametrize("path,waves", PATHS, ids=PATH_IDS)
def test_second_run_sees_new_weights(dev, path, waves, use_graph):
    """An optimiser step between two runs of one plan: same pointers, new values.  The row-wise plan reads fragment-major
    COPIES of the weights, made at the head of every forward scan: a captured graph must hold the copies' refresh (a
    replay that skipped it would return the old result), and a plan without a graph must make them on every call, not
    on its first one alone."""
    T, B, H, reverse = 4, 17, 64, (0, 1)
    scan = Scan(dev, T, B, H, reverse, "random", _path_env(path, waves), use_graph=use_graph)
    assert scan.route == _route_of(path, waves, H)
    old, touched = scan.go()
    assert touched == []
    _check_values(old, [G.reference(T, B, H, i, rev, "random") for i, rev in enumerate(reverse)], "first run")
    scan.fill(variant=1)  # in place
    new, touched = scan.go()
    assert touched == []
    scan.close()
    _check_values(new, [G.reference(T, B, H, i, rev, "random", 1) for i, rev in enumerate(reverse)], "replay, new weights")
    fresh = Scan(dev, T, B, H, reverse, "random", _path_env(path, waves), use_graph=False)
    fresh.fill(variant=1)
    assert fresh.route == _route_of(path, waves, H)
    want, touched = fresh.go()
    assert touched == []
    fresh.close()
    _assert_equal(new, want, "replay vs a fresh plan on the new weights")
    assert not torch.equal(new[0]["h"], old[0]["h"])


# ---- e. weights at a 4-byte aligned address -----------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["Wg", "Wc"])
def test_unaligned_weights_take_the_launch_path(dev, which):
    """The row-wise path needs 16-byte aligned weights (its tiling kernel loads vectors) and steps aside.  The launch path
    reads a row-major weight operand element by element wherever its address is not 16-byte aligned: forward (weights
    [K][N], skinny.hip sk_fetch_fast BM = 0 and sk_fetch) with four scalar loads per lane, backward (K contiguous) on the
    generic path with guarded scalar loads, which sk_finalize_job selects from the operand's address."""
    T, B, H, reverse = 3, 17, 64, (0, 1)
    scan = Scan(dev, T, B, H, reverse, "random", _path_env(G.ROWWISE, 8), unaligned=(which,))
    assert all(f.view.data_ptr() % 16 == 4 for f in scan.fr[which])
    assert scan.route == dict(rowwise=False, waves=0, nch=0, reason="unaligned")
    out, touched = scan.go()
    scan.close()
    assert touched == []
    _check_values(out, [G.reference(T, B, H, i, rev, "random") for i, rev in enumerate(reverse)], "unaligned " + which)


# ---- LSTM scan ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,B,H", G.LSTM_SHAPES)
def test_lstm_every_buffer_against_float64(dev, T, B, H):
    from parrot_amd import _lib, ops
    d = G.lstm_data(T, B, H)
    shapes = dict(W=(H, 4 * H), pre_in=(T, B, 4 * H), s=(T + 1, B, H), c=(T + 1, B, H), gates=(T, B, 4 * H),
                  dS=(T + 1, B, H), dc=(B, H), dP=(T, B, 4 * H))
    fr = {k: Framed(s, dev) for k, s in shapes.items()}
    nan = float("nan")
    fr["W"].view.copy_(d["W"])
    fr["pre_in"].view.copy_(d["pre_in"])
    for k, first in (("s", d["s0"]), ("c", d["c0"])):
        fr[k].view[0].copy_(first)
        fr[k].view[1:].fill_(nan)
    fr["gates"].view.fill_(nan)
    fr["dP"].view.fill_(nan)
    fr["dS"].view.copy_(d["dS_in"])
    fr["dc"].view.copy_(d["dc_in"])
    for f in fr.values():
        f.snapshot()
    desc = _lib.LstmSeqDesc()
    desc.T, desc.B, desc.H, desc.use_graph = T, B, H, 0
    for k, f in fr.items():
        setattr(desc, k, f.view.data_ptr())
    plan = C.c_void_p()
    _lib.call("parrot_lstm_seq_create", C.byref(desc), C.byref(plan))
    try:
        _lib.call("parrot_lstm_seq_fwd", plan, ops._stream())
        _lib.call("parrot_lstm_seq_bwd", plan, ops._stream())
        torch.cuda.synchronize()
    finally:
        _lib.load().parrot_lstm_seq_destroy(plan)
    for k, f in fr.items():
        assert f.untouched() if k in ("W", "pre_in") else f.frame_untouched(), k + ": written outside the buffer, or into an operand"
    for k in ("s", "c"):
        assert torch.equal(_bits(fr[k].view[0]), fr[k].before[PAD:PAD + B * H]), k + "[0] is the caller's"
    ref = G.lstm_reference(T, B, H)
    out = {k: fr[k].view.detach().cpu() for k in G.LSTM_NAMES_FWD + G.LSTM_NAMES_BWD}
    for k in out:
        assert not bool(torch.isnan(out[k]).any()), k + " has elements the kernels did not write"
    for k in out:
        tol = G.TOL_FWD if k in G.LSTM_NAMES_FWD else G.TOL_BWD
        print("ratio lstm T%d-B%d-H%d %s %.4f" % (T, B, H, k, rel_err(out[k], ref[k]) / tol))
        assert_close(out[k], ref[k], tol, k)


def test_lstm_create_rejects_width_6(dev):
    from parrot_amd import _lib
    desc = _lib.LstmSeqDesc()
    desc.T, desc.B, desc.H, desc.use_graph = 3, 2, 6, 0
    plan = C.c_void_p()
    assert _lib.load().parrot_lstm_seq_create(C.byref(desc), C.byref(plan)) == BADARG

"""Edge tests of the training scan plan (`parrot_decoder_seq_fwd` / `parrot_decoder_seq_bwd`): every buffer the scan
writes against the float64 reference of the descriptor's contract, at the cases of tests/decoder_scan_cases.py, on the
route each case names.

Every buffer of the descriptor -- operands and the fragment-major weight copies included -- is a view into a larger
allocation with a frame of PAD floats on either side.  Frames hold a NaN with a payload of their own and must be
bit-identical after each scan; operands must be unchanged as a whole, like slot 0 of the histories, and the forward
buffers after the backward scan.  Everything the scan must write starts as NaN; what the header says the caller
zero-fills is zero-filled exactly when the header says (once: persist_ws, dh_b, dw0_b, dw0_c; before every seq_bwd: dw0,
dhup, dhup_b, dhup_c, dw_b, dw_c); `seq_*` buffers are refilled before every seq_fwd (caller data, or NaN where the
descriptor calls them scratch).

Every test asserts the plan's route before any value: a scan that fell back would otherwise be compared with itself.
A case runs three windows through one plan -- its data, the same data again, other data -- once per session; the tests
share the results."""
import contextlib
import ctypes as C
import os

import pytest
import torch

from tests import decoder_scan_cases as D
from tests.util import Framed, _bits, rel_err, rel_err_elem

pytestmark = pytest.mark.gpu

NAN = float("nan")
SCALARS = ("WattT", "batt", "ctx", "w", "kappa", "a", "b", "phi", "dw", "dw0", "dkappa", "dp", "att_sup", "dw_b", "dw0_b", "dw_c",
           "dw0_c")  # the descriptor's fields that are one buffer; every other buffer is one of a per-layer array


@contextlib.contextmanager
def _env(values):
    """Sets (None: unsets) the switches, and restores what it found."""
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


def _sync():
    """Waits for the device.  A fault ends the session: nothing more is started on a device that has faulted."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("the device reported %s" % e, returncode=3)


class Scan:
    """A decoder plan for a case whose every buffer sits in a frame."""

    def __init__(self, dev, case, use_graph=0, sup=True):
        from parrot_amd import _lib
        self.L, self.lib, self.plan = _lib, _lib.load(), None
        self.case, self.dev, self.env = case, dev, D.environment(case)
        c = case
        T, B, H, E, A, U, nl = c.T, c.B, c.H, c.E, c.A, c.U, c.L
        gw = D.gate_width(c)
        lstm = c.cell == D.LSTM
        self.tiled = c.tiled and H % 16 == 0 and E % 16 == 0
        sh = dict(WattT=(3 * A, H), batt=(3 * A,), ctx=(B, U, E), w=(T + 1, B, E), kappa=(T + 1, B, A), a=(T, B, A),
                  b=(T, B, A), phi=(T, B, U), dw=(T + 1, B, E), dw0=(T + 1, B, E), dkappa=(B, A), dp=(T, B, 3 * A))
        self.operands = ["WattT", "batt", "ctx"]
        self.fwd_out = ["w", "kappa", "a", "b", "phi"]
        self.histories = {"w": B * E, "kappa": B * A}  # name -> words of slot 0 (the caller's)
        self.bwd_out = ["dw", "dw0", "dkappa", "dp"]
        self.zero_once, self.zero_each, self.seq = [], ["dw0"], []
        if sup:
            sh["att_sup"] = (T, B, 2)
            self.fwd_out.append("att_sup")
        if c.accum >= 2:
            for n in ("dw_b", "dw0_b", "dw_c", "dw0_c"):
                sh[n] = (T + 1, B, E)
            self.bwd_out += ["dw_b", "dw0_b", "dw_c", "dw0_c"]
            self.zero_once += ["dw0_b", "dw0_c"]
            self.zero_each += ["dw_b", "dw_c"]
        for l in range(nl):
            K = D.krows(c, l)
            sh.update({f"Wg{l}": (K, gw), f"bg{l}": (gw,), f"h{l}": (T + 1, B, H), f"dh{l}": (T + 1, B, H), f"dG{l}": (T, B, gw)})
            self.operands += [f"Wg{l}", f"bg{l}"]
            self.fwd_out.append(f"h{l}")
            self.histories[f"h{l}"] = B * H
            self.bwd_out += [f"dh{l}", f"dG{l}"]
            if self.tiled:
                sh.update({f"Wg_f{l}": (K, gw), f"Wg_r{l}": (K, gw)})
                self.operands += [f"Wg_f{l}", f"Wg_r{l}"]
            if lstm:
                sh.update({f"cst{l}": (T + 1, B, H), f"gate4{l}": (T, B, 4 * H), f"dcell{l}": (B, H)})
                self.fwd_out += [f"cst{l}", f"gate4{l}"]
                self.histories[f"cst{l}"] = B * H
                self.bwd_out.append(f"dcell{l}")
            else:
                sh.update({f"Wc{l}": (K, H), f"bc{l}": (H,), f"dC{l}": (T, B, H)})
                sh.update({f"{n}{l}": (T, B, H) for n in ("z", "r", "rh", "c")})
                self.operands += [f"Wc{l}", f"bc{l}"]
                self.fwd_out += [f"{n}{l}" for n in ("z", "r", "rh", "c")]
                self.bwd_out.append(f"dC{l}")
                if self.tiled:
                    sh.update({f"Wc_f{l}": (K, H), f"Wc_r{l}": (K, H)})
                    self.operands += [f"Wc_f{l}", f"Wc_r{l}"]
            if l >= 1 or (D.seq_init(c) >> l) & 1:
                sh[f"seq_g{l}"] = (T, B, gw)
                self.seq.append(f"seq_g{l}")
                if not lstm:
                    sh[f"seq_c{l}"] = (T, B, H)
                    self.seq.append(f"seq_c{l}")
            if l < nl - 1:
                sh[f"dhup{l}"] = (T + 1, B, H)
                self.bwd_out.append(f"dhup{l}")
                self.zero_each.append(f"dhup{l}")
            if c.accum >= 2:
                sh[f"dh_b{l}"] = (T + 1, B, H)
                self.bwd_out.append(f"dh_b{l}")
                self.zero_once.append(f"dh_b{l}")
                if l < nl - 1:
                    for n in (f"dhup_b{l}", f"dhup_c{l}"):
                        sh[n] = (T + 1, B, H)
                        self.bwd_out.append(n)
                        self.zero_each.append(n)
        self.fr = {n: Framed(s, dev) for n, s in sh.items()}
        d = _lib.DecoderDesc()
        d.T, d.B, d.H, d.E, d.A, d.U, d.L = T, B, H, E, A, U, nl
        d.att_type, d.use_graph, d.cell, d.seq_init = c.att_type, int(use_graph), c.cell, D.seq_init(c)
        d.eps, d.alignment, d.sharpening, d.timing = D.EPS, D.ALIGNMENT, 1.0, 1.0
        for n, f in self.fr.items():
            if n in SCALARS:
                setattr(d, n, f.view.data_ptr())
            else:  # per layer: "<field><l>"
                getattr(d, n[:-1])[int(n[-1])] = f.view.data_ptr()
        with _env(self.env):
            if c.persist:
                n = int(self.lib.parrot_decoder_persist_floats(C.byref(d)))
                if n > 0:
                    self.fr["persist_ws"] = Framed((n,), dev)
                    self.fwd_out.append("persist_ws")
                    self.zero_once.append("persist_ws")
                    d.persist_ws, d.persist_ws_floats = self.fr["persist_ws"].view.data_ptr(), n
            for n in self.fwd_out + self.bwd_out + self.seq:
                if n not in self.zero_once:
                    self.fr[n].view.fill_(NAN)
            for n in self.zero_once:
                self.fr[n].view.zero_()
            self.load(0)
            plan = C.c_void_p()
            _lib.call("parrot_decoder_create", C.byref(d), C.byref(plan))
        self.plan, self.desc = plan, d
        self.route = dict(schedule=self.lib.parrot_decoder_schedule(plan), tick=self.lib.parrot_decoder_backward_tick(plan),
                          persistent=self.lib.parrot_decoder_is_persistent(plan))

    def load(self, variant):
        """The operands and the slot-0 states of a data set (the weights' fragment-major copies refreshed)."""
        from parrot_amd import ops
        c = self.case
        x = self.x = D.data(D.data_key(c), variant)
        v = {n: f.view for n, f in self.fr.items()}
        for n in ("WattT", "batt", "ctx"):
            v[n].copy_(x[n])
        v["w"][0].copy_(x["w0"])
        v["kappa"][0].copy_(x["kappa0"])
        for l in range(c.L):
            v[f"Wg{l}"].copy_(x["Wg"][l])
            v[f"bg{l}"].copy_(x["bg"][l])
            v[f"h{l}"][0].copy_(x["h0"][l])
            mats = [("Wg", 0 if c.cell == D.GRU else c.H)]
            if c.cell == D.GRU:
                v[f"Wc{l}"].copy_(x["Wc"][l])
                v[f"bc{l}"].copy_(x["bc"][l])
                mats.append(("Wc", 0))
            else:
                v[f"cst{l}"][0].copy_(x["cst0"][l])
            for m, lstm_h in mats if self.tiled else []:
                W = v[f"{m}{l}"]
                self.L.call("parrot_tile_weights", W.data_ptr(), W.shape[0], W.shape[1], W.shape[1],
                            v[f"{m}_f{l}"].data_ptr(), 0, lstm_h, ops._stream())
                self.L.call("parrot_tile_weights", W.data_ptr(), W.shape[0], W.shape[1], W.shape[1],
                            v[f"{m}_r{l}"].data_ptr(), 1, 0, ops._stream())

    def _snapshot(self):
        for f in self.fr.values():
            f.snapshot()

    def _touched(self, written):
        """Names of the buffers whose frame changed, or that changed at all without being in `written`; a history in
        `written` keeps its slot 0."""
        bad = []
        for n, f in self.fr.items():
            if n not in written:
                ok = f.untouched()
            else:
                ok = f.frame_untouched()
                if n in self.histories:
                    ok = ok and torch.equal(_bits(f.view[0]), f.before[f.lo:f.lo + self.histories[n]])
            if not ok:
                bad.append(n)
        return bad

    def window(self):
        """One window: refills, seq_fwd, per-window zero fills, seq_bwd.  Returns (every buffer on the host after the
        backward scan, names touched out of turn by the forward scan, by the backward scan, the persistent status)."""
        from parrot_amd import ops
        c, x = self.case, self.x
        v = {n: f.view for n, f in self.fr.items()}
        for n in self.seq:
            l, src = int(n[-1]), x[n[:-1]][int(n[-1])]
            v[n].copy_(src) if (src is not None and (D.seq_init(c) >> l) & 1) else v[n].fill_(NAN)
        for l in range(c.L):
            v[f"dh{l}"].copy_(x["dh_in"][l])
            if c.cell == D.LSTM:
                v[f"dcell{l}"].copy_(x["dcell_in"][l])
        v["dw"].copy_(x["dw_in"])
        v["dkappa"].copy_(x["dkappa_in"])
        _sync()
        self._snapshot()
        with _env(self.env):
            self.L.call("parrot_decoder_seq_fwd", self.plan, ops._stream())
            status = self.lib.parrot_decoder_status(self.plan)
            _sync()
            bad_fwd = self._touched(set(self.fwd_out) | set(self.seq))
            fwd = {n: self.fr[n].view.detach().cpu().clone() for n in self.fwd_out if n != "persist_ws"}
            for n in self.zero_each:
                v[n].zero_()
            _sync()
            self._snapshot()
            self.L.call("parrot_decoder_seq_bwd", self.plan, ops._stream())
            _sync()
        bad_bwd = self._touched(set(self.bwd_out))
        out = {n: f.view.detach().cpu().clone() for n, f in self.fr.items() if n not in self.operands and n != "persist_ws"}
        for n, t in fwd.items():
            assert torch.equal(_bits(t), _bits(out[n])), n  # (the same check as _touched, on the host copies)
        return out, bad_fwd, bad_bwd, status

    def close(self):
        if self.plan is not None:
            self.lib.parrot_decoder_destroy(self.plan)
            self.plan = None


def results_of(case, out):
    """The raw buffers of a window as the reference names them (float64 on the host): forward buffers as they are;
    dh0_l, dhT_l, dw0 with the accumulators added the way Parrot._backward_f adds slot 0; dw = dw[1:]; dctx =
    sum_t phi[t]^T . dw[t+1]."""
    r = {n: out[n].double() for n in D.forward_names(case.cell, case.L)}
    for l in range(case.L):
        r["dG%d" % l] = out["dG%d" % l].double()
        if case.cell == D.LSTM:
            r["dcell%d" % l] = out["dcell%d" % l].double()
        else:
            r["dC%d" % l] = out["dC%d" % l].double()
        tot = sum(out[n % l].double() for n in ("dh%d", "dhup%d", "dh_b%d", "dhup_b%d", "dhup_c%d") if n % l in out)
        r["dhT_%d" % l] = tot[1:]
        r["dh0_%d" % l] = sum(out[n % l][0].double() for n in ("dh%d", "dh_b%d") if n % l in out)
    r["dp"], r["dkappa"] = out["dp"].double(), out["dkappa"].double()
    r["dw0"] = sum(out[n][0].double() for n in ("dw", "dw0", "dw_b", "dw_c", "dw0_b", "dw0_c") if n in out)
    r["dw"] = out["dw"][1:].double()
    r["dctx"] = torch.einsum("tbu,tbe->bue", out["phi"].double(), out["dw"][1:].double())
    return r


_RESULTS = {}


def _result(dev, case, **kw):
    """The case run once: dict(route, windows = [(out, bad_fwd, bad_bwd, status)] for its data, the same data again and the
    data of variant 1 through the same plan)."""
    key = (case.id,) + tuple(sorted(kw.items()))
    if key not in _RESULTS:
        scan = Scan(dev, case, **kw)
        try:
            res = dict(route=scan.route, windows=[])
            if scan.route == D.expected_route(case):  # (a plan on another route is not run: its values prove nothing)
                res["windows"].append(scan.window())
                res["windows"].append(scan.window())
                scan.load(1)
                res["windows"].append(scan.window())
        finally:
            scan.close()
        _RESULTS[key] = res
    return _RESULTS[key]


def _assert_route(case, res):
    assert res["route"] == D.expected_route(case), (case.id, res["route"], D.expected_route(case))


def _against_reference(case, window, variant, what):
    out, bad_fwd, bad_bwd, status = window
    assert status == 0, "%s: the persistent scan gave up (status %d)" % (what, status)
    ref = D.case_reference(case, variant)
    got = results_of(case, out)
    problems = []
    for n, t in out.items():
        # (att_sup holds integers; a scratch `seq_*` buffer is the scan's to use or to leave: schedule 0 never touches it,
        # and a NaN read from it would show in the values below)
        scratch = n.startswith("seq_") and not (D.seq_init(case) >> int(n[-1])) & 1
        if n != "att_sup" and not scratch and bool(torch.isnan(t).any()):
            problems.append("%s has %d elements the scan did not write" % (n, int(torch.isnan(t).sum())))
    for n in D.forward_names(case.cell, case.L) + D.backward_names(case.cell, case.L):
        want = D.representable(ref[n])
        checks = [(rel_err, D.tolerance(case, n), "")]
        if n in D.ELEMENTWISE:
            checks.append((rel_err_elem, D.tolerance(case, n, elem=True), ":elem"))
        for fn, tol, tag in checks:
            e = fn(got[n], want)
            print("ratio %s %s%s %.4f" % (what, n, tag, e / tol))
            if not e <= tol:
                problems.append("%s%s: relative error %.3e > %.1e" % (n, tag, e, tol))
    if bad_fwd:
        problems.append("the forward scan touched frames / operands / slot 0 of %s" % bad_fwd)
    if bad_bwd:
        problems.append("the backward scan touched frames / operands / forward buffers of %s" % bad_bwd)
    if "att_sup" in out:
        phi, sup = out["phi"], out["att_sup"].view(torch.int32)
        nz = phi != 0
        U = phi.shape[-1]
        lo = torch.where(nz.any(-1), nz.float().argmax(-1), torch.full(nz.shape[:2], U)).int()
        hi = torch.where(nz.any(-1), U - 1 - nz.flip(-1).float().argmax(-1), torch.full(nz.shape[:2], -1)).int()
        if D.environment(case)["PARROT_ATT_DENSE"] == "1":  # (the header: dense mode saves the full range)
            lo, hi = torch.zeros_like(lo), torch.full_like(hi, U - 1)
        if not (torch.equal(sup[..., 0], lo) and torch.equal(sup[..., 1], hi)):
            problems.append("att_sup is not the support of the kernel's own phi at %d (t, row) pairs" %
                            int(((sup[..., 0] != lo) | (sup[..., 1] != hi)).sum()))
    assert not problems, "%s:\n  " % what + "\n  ".join(problems)


def _assert_same_bits(a, b, what, names=None):
    diff = [n for n in (names or a) if not torch.equal(_bits(a[n]), _bits(b[n]))]
    assert not diff, "%s: %s differ" % (what, diff)


# ---- a. every buffer against float64, inside frames, on the route the case names --------------------------------------------
@pytest.mark.parametrize("name", sorted(D.CASES))
def test_every_buffer_against_float64(dev, name):
    case = D.CASES[name]
    res = _result(dev, case)
    _assert_route(case, res)
    _against_reference(case, res["windows"][0], 0, name)


# ---- b. two windows through one plan -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(D.CASES))
def test_two_windows_through_one_plan(dev, name):
    """The same data again after the per-window zero fills and refills only: every buffer bit-identical.  Then other data
    (weights included) through the same plan, against its own reference: a value that survives from the previous window in
    the once-zeroed accumulators, the plan's flags or persist_ws shows here."""
    case = D.CASES[name]
    res = _result(dev, case)
    _assert_route(case, res)
    first, again, other = res["windows"]
    assert again[1:] == first[1:], (again[1:], first[1:])
    _assert_same_bits(first[0], again[0], name + " run again")
    _against_reference(case, other, 1, name + " window2")


# ---- c. across paths -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(n for n, c in D.CASES.items() if D.twins(c)))
def test_paths_agree(dev, name):
    case = D.CASES[name]
    res = _result(dev, case)
    _assert_route(case, res)
    mine = results_of(case, res["windows"][0][0])
    problems = []
    for other in D.twins(case):
        if other < name:
            continue
        oc = D.CASES[other]
        ores = _result(dev, oc)
        _assert_route(oc, ores)
        theirs = results_of(oc, ores["windows"][0][0])
        for n in mine:
            tol = D.tolerance(case, n, base=D.TOL_PATHS)
            e = rel_err(mine[n], theirs[n])
            print("ratio %s~%s %s %.4f" % (name, other, n, e / tol))
            if not e <= tol:
                problems.append("%s vs %s: %s differs by %.3e > %.1e" % (name, other, n, e, tol))
    assert not problems, "\n  ".join(problems)


# ---- d. the support is an optimisation: NULL gives the same ------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(D.GROUPS["window"]) + [n for n in D.GROUPS["paths"] if "-default-" in n])
def test_without_att_sup_the_scan_gives_the_same(dev, name):
    case = D.CASES[name]
    res, bare = _result(dev, case), _result(dev, case, sup=False)
    _assert_route(case, res)
    _assert_route(case, bare)
    _against_reference(case, bare["windows"][0], 0, name + " sup=NULL")
    a, b = results_of(case, res["windows"][0][0]), results_of(case, bare["windows"][0][0])
    for n in a:
        tol = D.tolerance(case, n, base=D.TOL_PATHS)
        print("ratio %s sup~NULL %s %.4f" % (name, n, rel_err(b[n], a[n]) / tol))
        assert rel_err(b[n], a[n]) <= tol, n


# ---- e. captured plans -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(n for n in D.GROUPS["paths"] if "-L2-" in n))
def test_graph_replay_equals_eager(dev, name):
    """use_graph = 1: the first window (capture), the second (replay) and the window of other data are bit-identical to the
    eager plan's."""
    case = D.CASES[name]
    eager, graph = _result(dev, case), _result(dev, case, use_graph=1)
    _assert_route(case, eager)
    _assert_route(case, graph)
    for i, what in enumerate(("capture", "replay", "replay on other data")):
        assert graph["windows"][i][1:] == eager["windows"][i][1:], what
        _assert_same_bits(eager["windows"][i][0], graph["windows"][i][0], "%s %s" % (name, what))


# ---- f. the persistent machine's two synchronisation modes -------------------------------------------------------------------
@pytest.mark.parametrize("L", [2, 3])
def test_persistent_dataflow_equals_barriers(dev, L):
    a = [c for c in D.CASES.values() if c.group == "paths" and "persist-df0" in c.id and c.L == L][0]
    b = [c for c in D.CASES.values() if c.group == "paths" and "persist-df1" in c.id and c.L == L][0]
    ra, rb = _result(dev, a), _result(dev, b)
    _assert_route(a, ra)
    _assert_route(b, rb)
    assert ra["route"]["persistent"] == 1
    for i in range(3):
        _assert_same_bits(ra["windows"][i][0], rb["windows"][i][0], "window %d" % i)


# ---- g. the caller's side of the slot-0 contract -------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [2, 3])
def test_model_adds_slot_0_of_every_accumulator(dev, L):
    """Parrot._backward_f is the caller the header's rule on slot 0 speaks to: on the K-balanced tick the gradient wrt what
    entered the window is dh[l][0] + dh_b[l][0] and dw[0] + dw0[0] + slot 0 of dw_b, dw_c, dw0_b, dw0_c.  With the learned
    initial states (start_flag = 1) their column sums are the gradients of `initial_state` and `initial_w`, held here to the
    scan's backward tolerance against the float64 oracle (the model-level suite holds them to 1e-3)."""
    from oracle import parrot_ref as R
    from parrot_amd import _lib
    from tests.test_gpu_parrot import _build
    from tests.util import make_batch
    T, B, U = 6, 4, 9
    cfg, p, m = _build(dev, num_layers=L, encoder_type="bidirectional")
    try:
        feat, fm, lab, lm, spk = make_batch(cfg, T, B, U, seed=3)
        for v in p.values():
            v.requires_grad_()
        rc = R.compute_cost(p, cfg, feat, fm, lab, lm, spk, 1)[0]
        rc.backward()
        m.zero_grad()
        cost = m.compute_cost(feat.float().to(dev), fm.float().to(dev), lab.to(dev), lm.float().to(dev), None, 1, B)[0]
        cost.backward()
        ws = next(v for k, v in m._train_ws.items() if k[0] == "dec")
        assert "dw0_c" in ws and int(_lib.load().parrot_decoder_backward_tick(ws["plan"])) == 8
        assert bool(ws["dw0_c"][0].any()) and bool(ws["dw0_b"][0].any()) and bool(ws["dh_b"][0][0].any())
        grads = m.get_gradient_dict()
        for name in ["/parrot.initial_w"] + ["/parrot/rnn%d.initial_state" % (l + 1) for l in range(L)]:
            e = rel_err(grads[name], p[name].grad)
            print("ratio model-L%d %s %.4f" % (L, name, e / D.TOL_BWD))
            assert e <= D.TOL_BWD, (name, e)
    finally:
        m.close()

"""The training and decode paths with the attention window at the edges of the text and past it (tests/attention_cases.py).

P1-P4 (and P2W, P2 at widths the wide bf16 kernel takes) raise `fork_kappa.b` so that within a few frames kappa passes the
end of the short ragged texts: phi underflows to exactly 0.0f on every position, the forward step saves the empty support
(U, -1), and the backward step runs its clamped preload and its mixture loop of zero trips -- on every training schedule.
W1-W3 keep the window inside a long text and cross the forward kernels' thresholds on U instead (one thread per position
in the 512-thread block for U > 256, a second pass over the positions in the persistent machine for U > 512, the
backward without its context preload for U > 256).

Every run is compared with the fp64 oracle exactly as tests/test_gpu_parrot.py compares: cost, frames, kappa, w, phi,
pi_att at 1e-4 and every gradient norm-wise at 1e-3.  tests/test_attention_edges_cpu.py checks the premises (how many rows
are empty, that float32 arithmetic itself stays two orders inside these bounds) without a GPU."""
import pytest
import torch

from tests import attention_cases as AC
from tests.test_gpu_parrot import _build, _check_cost_and_grads
from tests.test_gpu_persist import _is_persistent
from tests.util import assert_close, rel_err

pytestmark = pytest.mark.gpu

SWITCHES = ("PARROT_SCHEDULE", "PARROT_CHUNK", "PARROT_BWD_HETERO", "PARROT_S5_WSTEP", "PARROT_WK", "PARROT_ATT_DENSE",
            "PARROT_SAMPLE_PERSIST")


def _env(monkeypatch, **env):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, str(value))


def _to_dev(batch, dev):
    feat, fm, lab, lm, spk = batch
    return (feat.float().to(dev), fm.float().to(dev), lab.to(dev), lm.float().to(dev), None if spk is None else spk.to(dev))


def _schedule(m):
    from parrot_amd import _lib
    ws = next(v for k, v in m._train_ws.items() if isinstance(k, tuple) and k[0] == 'dec')
    return int(_lib.load().parrot_decoder_schedule(ws['plan']))


def _run_case(dev, name, use_graph, expect_schedule, persistent=False):
    """One training step of a case against its shared fp64 oracle: the comparison of _check_cost_and_grads, and the
    kernel's phi has at least as many all-zero rows as the oracle has rows below 1e-60."""
    o = AC.oracle(name)
    T, B, U = AC.shape(name)
    cfg, p, m = _build(dev, use_graph=use_graph, param_overrides=AC.overrides(name), **AC.model_kwargs(name))
    for k, v in p.items():
        assert torch.equal(v, o['params'][k]), k  # the oracle shared by the tests is the oracle of this model
    feat, fm, lab, lm, spk = _to_dev(o['batch'], dev)
    worst_out = worst_grad = 0.0
    for rep in range(2 if use_graph else 1):  # the second pass replays the captured graph
        m.zero_grad()
        cost, _, av, _ = m.compute_cost(feat, fm, lab, lm, spk, 1, B)
        cost.backward()
        assert _schedule(m) == expect_schedule  # no silent fall-back
        if persistent:
            assert _is_persistent(m, T, B, U)
        errs = {"cost": rel_err(cost, o['cost'])}
        for i, n in ((0, "frames"), (1, "kappa"), (2, "w"), (4, "phi"), (5, "pi_att")):
            errs[n] = rel_err(av[i], o['av'][i])
        grads = m.get_gradient_dict()
        gerrs = {}
        for k, ref in o['grads'].items():
            if float(ref.abs().max()) < 1e-12:
                assert float(grads[k].abs().max()) < 1e-6, k
                continue
            assert torch.isfinite(grads[k]).all(), k
            gerrs[k] = rel_err(grads[k], ref)
        worst = max(gerrs, key=gerrs.get)
        empty_ref, empty_got = AC.count_empty(o['av'][4]), int((av[4].abs().amax(-1) == 0).sum())
        print(f"{name} schedule {expect_schedule} graph={use_graph} pass {rep}: " +
              " ".join(f"{n}={e:.2e}" for n, e in errs.items()) +
              f" worst grad {gerrs[worst]:.2e} ({worst}); all-zero phi rows {empty_got} (oracle: {empty_ref} empty)")
        for n, e in errs.items():
            assert e <= 1e-4, f"{n}: relative error {e:.3e}"
        for k, e in gerrs.items():
            assert e <= 1e-3, f"grad {k}: rel err {e:.3e}"
        assert len(gerrs) >= 10
        assert empty_got >= empty_ref
        worst_out, worst_grad = max(worst_out, max(errs.values())), max(worst_grad, gerrs[worst])
    m.close()
    return worst_out, worst_grad


# ----------------------------------------------------------------------------- the window leaves the text: every schedule
LAUNCH_SCHEDULES = [("0", {}), ("3", dict(PARROT_CHUNK=3)), ("5", {})]


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("sched,env", LAUNCH_SCHEDULES)
@pytest.mark.parametrize("name", ["P1", "P2", "P3", "P4"])
def test_empty_support_on_the_launch_schedules(dev, monkeypatch, name, sched, env, use_graph):
    """Schedules 0 (att_fwd_kernel; att_state_bwd_kernel, or skb_kernel for the GRU stacks), 3 (chunks of 3 frames, a
    ragged last one) and 5 (att_fwd_block<512> in ska_kernel), eager and graph."""
    _env(monkeypatch, PARROT_SCHEDULE=sched, **env)
    _run_case(dev, name, use_graph, int(sched))


@pytest.mark.parametrize("use_graph", [False, True])
def test_empty_support_one_launch_per_tick_lstm(dev, monkeypatch, use_graph):
    """Schedule 7 on f32 operands (LSTM layers: the attention of step q - 1 inside the launch of tick q)."""
    _env(monkeypatch, PARROT_SCHEDULE=7)
    _run_case(dev, "P2", use_graph, 7)


@pytest.mark.parametrize("name", ["P1", "P3"])
def test_empty_support_on_the_persistent_machine(dev, monkeypatch, name):
    """Schedule 4: pm_att_row saves the empty support, the launch-schedule backward reads it."""
    _env(monkeypatch, PARROT_SCHEDULE=4)
    _run_case(dev, name, True, 5, persistent=True)


@pytest.mark.parametrize("switch", ["PARROT_BWD_HETERO", "PARROT_S5_WSTEP"])
@pytest.mark.parametrize("name", ["P1", "P2", "P3", "P4"])
def test_empty_support_schedule_5_variants(dev, monkeypatch, name, switch):
    """Schedule 5 without the K-balanced backward tick (att_state_bwd_kernel instead of skb_kernel) and with the upper
    layers' w rows in the attention launch's projection jobs."""
    _env(monkeypatch, PARROT_SCHEDULE=5, **{switch: 0})
    for use_graph in (False, True):
        _run_case(dev, name, use_graph, 5)


# ----------------------------------------------------------------------------- long texts: the thresholds on U
def test_long_text_one_layer(dev, monkeypatch):
    """W1 (U = 260): three passes of the phi loop in att_fwd_kernel, the backward without its context preload.  A
    one-layer decoder has nothing to run the attention beside: asked for 5, the plan runs schedule 0 (as in
    test_balanced_wavefront_schedules); W3 below is the same case with two layers."""
    T, B, U = AC.shape("W1")
    for sched in ("0", "5"):
        _env(monkeypatch, PARROT_SCHEDULE=sched)
        _check_cost_and_grads(dev, T, B, U, ragged=True, use_graph=True, expect_schedule=0,
                              param_overrides=AC.overrides("W1"), **AC.model_kwargs("W1"))


@pytest.mark.parametrize("sched", ["0", "5"])
def test_long_text_two_layers(dev, monkeypatch, sched):
    """W3 (U = 260, two layers): on schedule 5 the 512-thread block takes one thread per position (U > 256)."""
    _env(monkeypatch, PARROT_SCHEDULE=sched)
    _run_case(dev, "W3", True, int(sched))


def test_long_text_on_the_persistent_machine(dev, monkeypatch):
    """W2 (U = 520): a second pass over the positions in pm_att_row, training forward."""
    _env(monkeypatch, PARROT_SCHEDULE=4)
    _run_case(dev, "W2", True, 5, persistent=True)


@pytest.mark.parametrize("persist", ["1", "0"])
def test_long_text_decode(dev, monkeypatch, persist):
    """W2's text decoded on the machine (pm_att_row) and step by step (att_fwd_kernel, three passes of the phi loop)
    against R.sample_model at the 1e-4 of test_decode_on_the_persistent_machine."""
    from oracle import parrot_ref as R
    from parrot_amd import _lib
    _env(monkeypatch, PARROT_SAMPLE_PERSIST=persist)
    o = AC.oracle("W2")
    T, N, U = AC.shape("W2")
    S = 6
    _, _, lab, lm, spk = o['batch']
    with torch.no_grad():
        ref = R.sample_model(o['params'], o['cfg'], lab, lm, spk, S)
    cfg, p, m = _build(dev, use_graph=True, param_overrides=AC.overrides("W2"), **AC.model_kwargs("W2"))
    for rep in range(2):
        outs = m.sample_model_device(lab, lm.float(), spk, N, S)
        for got, r, n in zip(outs, ref, ("sample_x", "k", "w", "pi", "phi", "pi_att")):
            assert_close(got, r, 1e-4, f"persist={persist} pass {rep}: {n}")
    ws = m._sample_ws.get((S, N, U))
    assert (_lib.load().parrot_sample_is_persistent(ws['plan']) != 0) == (persist == "1")
    if persist == "1":
        assert int(ws['pm']['ws'][832:833].view(torch.int32).item()) == 0, "a spin timed out inside the machine"
    assert float(AC.row_max(ref[4]).min()) > 1e-3  # the window stays inside the text while decoding
    m.close()


# ----------------------------------------------------------------------------- bf16 operands
def test_empty_support_bf16(dev, monkeypatch):
    """P2 with bf16 operands against the oracle at the mode's tolerances (tests/test_gpu_bf16.py), on the schedule the
    plan picks for these widths (0), and P2W under PARROT_WK=2, where it picks 7 and the backward tick is wkb_kernel."""
    from tests.test_gpu_bf16 import _bf16_check
    T, B, U = AC.shape("P2")
    _env(monkeypatch)
    kw = {k: v for k, v in AC.model_kwargs("P2").items()}
    _bf16_check(dev, kw, T, B, U, seed=7, kappa_bias=1.0)
    _env(monkeypatch, PARROT_WK=2)
    _bf16_check(dev, dict(AC.model_kwargs("P2W")), T, B, U, seed=7, kappa_bias=1.0)


def test_empty_support_bf16_one_launch_per_tick_agrees_with_schedule_0(dev, monkeypatch):
    """Schedule 7 on the wide bf16 kernel (att_bwd_row with late() in wkb_kernel) against schedule 0 on P2W, compared as
    test_bf16_lstm_one_launch_per_tick_agrees_with_schedule_0 compares them; both see the windows leave the text."""
    from parrot_amd.model import Parrot
    o = AC.oracle("P2W")
    T, B, U = AC.shape("P2W")
    batch = _to_dev(o['batch'], dev)
    got = {}
    for sched in ("0", "7"):
        _env(monkeypatch, PARROT_WK=2, PARROT_SCHEDULE=sched)
        m = Parrot(device=dev, compute_dtype='bf16', use_graph=True, **AC.model_kwargs("P2W")).allocate()
        m.set_parameter_values(o['params'])
        for rep in range(2):
            m.zero_grad()
            cost, _, av, _ = m.compute_cost(*batch, 1, B)
            cost.backward()
        assert _schedule(m) == int(sched)
        assert int((av[4].abs().amax(-1) == 0).sum()) >= 10
        got[sched] = (cost.detach().clone(), av[0].detach().clone(), av[2].detach().clone(),
                      {k: v.detach().clone() for k, v in m.get_gradient_dict().items()})
        m.close()
    assert abs(float(got["0"][0]) - float(got["7"][0])) <= 1e-4 * abs(float(got["0"][0]))
    for i, n in ((1, "frames"), (2, "w")):
        assert_close(got["7"][i], got["0"][i].double().cpu(), 2e-3, n)
    for k, v in got["0"][3].items():
        if float(v.abs().max()) > 1e-12:
            assert rel_err(got["7"][3][k], v) < 5e-3, (k, rel_err(got["7"][3][k], v))


# ----------------------------------------------------------------------------- saved support vs every context row
@pytest.mark.parametrize("sched", ["0", "4", "5"])
@pytest.mark.parametrize("name", ["P1", "P3"])
def test_support_vs_dense_with_empty_rows(dev, monkeypatch, name, sched):
    """Reading only the window support == reading all context rows (bitwise: cost, frames, kappa; gradients to the
    summation-order noise of the split-K atomics) -- the property of test_full_size_cfg2_properties, here with rows whose
    saved support is empty (the backward skips them altogether) next to rows that read the whole text."""
    o = AC.oracle(name)
    T, B, U = AC.shape(name)
    batch = _to_dev(o['batch'], dev)
    res = {}
    for dense in ("0", "1"):
        _env(monkeypatch, PARROT_SCHEDULE=sched, PARROT_ATT_DENSE=dense)
        cfg, p, m = _build(dev, use_graph=True, param_overrides=AC.overrides(name), **AC.model_kwargs(name))
        m.zero_grad()
        cost, _, av, _ = m.compute_cost(*batch, 1, B)
        cost.backward()
        assert _schedule(m) == (5 if sched == "4" else int(sched))
        assert _is_persistent(m, T, B, U) == (sched == "4")
        res[dense] = (cost.detach().clone(), av[0].clone(), av[1].clone(), m.flat_gradients.clone(), av[4].clone())
        m.close()
    assert int((res["0"][4].abs().amax(-1) == 0).sum()) >= AC.count_empty(o['av'][4]) >= 10
    assert torch.equal(res["0"][0], res["1"][0]), "support vs dense: cost"
    assert torch.equal(res["0"][1], res["1"][1]), "support vs dense: frames"
    assert torch.equal(res["0"][2], res["1"][2]), "support vs dense: kappa"
    assert_close(res["1"][3], res["0"][3], 1e-6, "support vs dense: gradients")

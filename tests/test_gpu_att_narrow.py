"""The attention backward row block on its narrow path (only the support's context rows, the Watt column requested at
entry) against the fp64 oracle and against its wide path, bit for bit.  Cases and recipe: tests/att_narrow_cases.py;
their premises (every row's support and route) are checked without a GPU in tests/test_att_narrow_cpu.py."""
import pytest
import torch

from tests import att_narrow_cases as NC
from tests.test_gpu_attention_edges import _schedule, _to_dev
from tests.test_gpu_kernels import ATT_ALIGN, ATT_EPS, ATT_SHARP, ATT_TIMING, ATT_TOL, PLACEMENT_TOL, _att_parity
from tests.test_gpu_parrot import _build
from tests.util import assert_close, rel_err

pytestmark = pytest.mark.gpu

SWITCHES = ("PARROT_SCHEDULE", "PARROT_CHUNK", "PARROT_BWD_HETERO", "PARROT_S5_WSTEP", "PARROT_WK", "PARROT_ATT_DENSE",
            "PARROT_ATT_BWD_NARROW")


def _env(monkeypatch, **env):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, str(value))


def _step(monkeypatch, att_type, x, narrow, with_support):
    """Forward and backward step through the stand-alone entry points; the forward step's saved support is handed to the
    backward step (with_support) or not."""
    from parrot_amd import ops
    _env(monkeypatch, PARROT_ATT_BWD_NARROW=narrow)
    at = 1 if att_type == "softmax" else 0
    WattT = x['Watt'].t().contiguous()
    a, b, k, phi, w, sup = ops.gmm_attention_fwd(x['h1'], WattT, x['batt'], x['kprev'], x['ctx'], at, ATT_EPS, ATT_ALIGN,
                                                 ATT_SHARP, ATT_TIMING, return_support=True)
    dkappa = x['gk'].clone()
    dh1 = torch.zeros_like(x['h1'])
    dp = ops.gmm_attention_bwd(x['gw'], x['ctx'], a, b, k, x['kprev'], WattT, dkappa, dh1, at, ATT_EPS,
                               support=sup if with_support else None)
    return dict(a=a, b=b, kappa=k, phi=phi, w=w, dh1=dh1, dkappa=dkappa, dp=dp, sup=sup)


@pytest.mark.parametrize("att_type", NC.ATT_TYPES)
@pytest.mark.parametrize("name", sorted(NC.STEP_CASES))
def test_one_step_narrow_vs_wide_vs_oracle(dev, monkeypatch, name, att_type):
    """Every row of the case: the forward step saves the support the case claims, the route query names the path the case
    states for it, every output meets the oracle at the bounds of test_attention_fwd_bwd / the placement test (dp row by
    row as well) -- with the narrow path on, with PARROT_ATT_BWD_NARROW=0 and without a support handed in -- and dp, dh1,
    dkappa of the narrow path equal those of PARROT_ATT_BWD_NARROW=0 bit for bit."""
    from parrot_amd import ops
    (B, H, A, U, E), rows = NC.STEP_CASES[name]
    xc, ref = NC.step_case(name, att_type)
    x = {k: v.to(dev) for k, v in xc.items()}
    tol = PLACEMENT_TOL.get((att_type, U))
    runs = {"narrow": _step(monkeypatch, att_type, x, 1, True), "wide": _step(monkeypatch, att_type, x, 0, True),
            "nosup": _step(monkeypatch, att_type, x, 1, False)}
    _env(monkeypatch)
    sup = runs["narrow"]["sup"].cpu().tolist()
    assert len(sup) == B
    for r, row in enumerate(rows):  # no row left out
        assert tuple(sup[r]) == NC.claimed_support(row, U), (r, sup[r])
        assert ops.att_bwd_route(U, E, sup[r]) == row[-1], r
    assert ops.att_bwd_route(U, E, None) == NC.WIDE
    for what, got in runs.items():
        _att_parity(got, ref, f"{name} {att_type} {what}", tol)
        bound = {**ATT_TOL, **(tol or {})}['dp']
        for r in range(B):
            e = rel_err(got['dp'][r], ref['dp'][r])
            print(f"{name} {att_type} {what} dp row {r}: {e:.2e}")
            assert e <= bound, f"{what} dp row {r}: relative error {e:.3e} > {bound:.1e}"
    # (a backward step without a support sums the mixtures' terms over lanes that start at u = 0, not at u_lo: same path as
    # "wide" for the context rows, other bits in the mixture sums, so it is held to the oracle only)
    for n in ("dp", "dh1", "dkappa"):
        assert torch.equal(runs["narrow"][n], runs["wide"][n]), f"narrow vs wide: {n}"


def _train_step(dev, monkeypatch, name, env, narrow, dtype=None):
    """One captured training step of a model case under the switches `env`; everything a later step depends on."""
    from parrot_amd.model import Parrot
    o = NC.model_oracle(name)
    B = NC.MODEL_CASES[name][2]
    _env(monkeypatch, PARROT_ATT_BWD_NARROW=narrow, **env)
    if dtype is None:
        cfg, p, m = _build(dev, use_graph=True, param_overrides=NC.model_overrides(name), **NC.model_kwargs(name))
        for k, v in p.items():
            assert torch.equal(v, o['params'][k]), k
    else:
        m = Parrot(device=dev, compute_dtype=dtype, use_graph=True, **NC.model_kwargs(name)).allocate()
        m.set_parameter_values(o['params'])
    batch = _to_dev(o['batch'], dev)
    m.zero_grad()
    cost, updates, av, _ = m.compute_cost(*batch, 1, B)
    cost.backward()
    sched = _schedule(m)
    res = dict(cost=cost.detach().clone(), av=[x.detach().clone() for x in av],
               carried=[src.detach().clone() for _, src in updates],  # the scan's final states, (destination, value) pairs
               flat=m.flat_gradients.detach().clone(),
               grads={k: v.detach().clone() for k, v in m.get_gradient_dict().items()})
    m.close()
    return res, sched


def _same_bits(a, b):
    assert torch.equal(a['cost'], b['cost']), "cost"
    assert len(a['av']) == len(b['av']) and len(a['carried']) == len(b['carried']) >= 1
    for i, (u, v) in enumerate(zip(a['av'], b['av'])):
        assert torch.equal(u, v), f"attention_vars[{i}]"
    for i, (u, v) in enumerate(zip(a['carried'], b['carried'])):
        assert torch.equal(u, v), f"carried state {i}"
    assert torch.equal(a['flat'], b['flat']), "gradients"


@pytest.mark.parametrize("hetero", [1, 0])
@pytest.mark.parametrize("sched", [0, 5])
@pytest.mark.parametrize("name", ["IN", "OUT"])
def test_training_step_narrow_equals_wide(dev, monkeypatch, name, sched, hetero):
    """Whole training steps (skb_kernel with PARROT_BWD_HETERO=1, att_state_bwd_kernel without): gradients and carried
    states with the narrow path on equal those with it off bit for bit, and both meet the oracle at the bounds of
    tests/test_gpu_attention_edges.py (outputs 1e-4, gradients norm-wise 1e-3)."""
    o = NC.model_oracle(name)
    env = dict(PARROT_SCHEDULE=sched, PARROT_BWD_HETERO=hetero)
    res = {}
    for narrow in (1, 0):
        res[narrow], got_sched = _train_step(dev, monkeypatch, name, env, narrow)
        assert got_sched == sched
        r = res[narrow]
        errs = {"cost": rel_err(r['cost'], o['cost'])}
        for i, n in ((0, "frames"), (1, "kappa"), (2, "w"), (4, "phi"), (5, "pi_att")):
            errs[n] = rel_err(r['av'][i], o['av'][i])
        gerrs = {k: rel_err(r['grads'][k], g) for k, g in o['grads'].items() if float(g.abs().max()) >= 1e-12}
        worst = max(gerrs, key=gerrs.get)
        print(f"{name} schedule {sched} hetero {hetero} narrow {narrow}: " + " ".join(f"{n}={e:.2e}" for n, e in errs.items()) +
              f" worst grad {gerrs[worst]:.2e} ({worst})")
        for n, e in errs.items():
            assert e <= 1e-4, f"{n}: relative error {e:.3e}"
        for k, e in gerrs.items():
            assert e <= 1e-3, f"grad {k}: rel err {e:.3e}"
        assert len(gerrs) >= 10
    _same_bits(res[1], res[0])


def test_training_step_narrow_equals_wide_bf16_fused_tick(dev, monkeypatch):
    """attention_cases.P2W with bf16 operands under PARROT_WK=2: schedule 7, the backward tick is wkb_kernel, which shares
    the row block.  Narrow on equals narrow off bit for bit; both meet the oracle at the bf16 bounds of
    tests/test_gpu_bf16.py (cost 5e-3, frames / kappa / w 2e-2, gradients 5e-2), which test_empty_support_bf16 uses."""
    o = NC.model_oracle("OUT_WKB")
    env = dict(PARROT_WK=2, PARROT_SCHEDULE=7)
    res = {}
    for narrow in (1, 0):
        res[narrow], got_sched = _train_step(dev, monkeypatch, "OUT_WKB", env, narrow, dtype='bf16')
        assert got_sched == 7
        r = res[narrow]
        assert abs(float(r['cost']) - float(o['cost'])) <= 5e-3 * abs(float(o['cost']))
        for i, n in ((0, "predicted frames"), (1, "kappa"), (2, "w")):
            assert_close(r['av'][i], o['av'][i], 2e-2, n)
        n = 0
        for k, g in o['grads'].items():
            if float(g.abs().max()) >= 1e-12:
                e = rel_err(r['grads'][k], g)
                assert e <= 5e-2, f"grad {k}: rel err {e:.3e}"
                n += 1
        assert n >= 10
        assert int((r['av'][4].abs().amax(-1) == 0).sum()) >= 10
    _same_bits(res[1], res[0])

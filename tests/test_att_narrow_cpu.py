"""Premises of tests/test_gpu_att_narrow.py, from the fp64 oracle and the library's host-side route query alone: every
row of every one-step case has the support it claims (so the width it claims), and takes the path it states; the model
cases keep their windows inside the text ("IN") or lose them ("OUT", "OUT_WKB") with every support narrow."""
import pytest
import torch

from tests import att_narrow_cases as NC
from tests import attention_cases as AC


@pytest.fixture()
def ops(monkeypatch):
    from parrot_amd import build, ops
    build.build(verbose=False)
    monkeypatch.delenv("PARROT_ATT_BWD_NARROW", raising=False)
    return ops


def test_route_query_states_the_rule(ops, monkeypatch):
    """parrot_att_bwd_route is att_bwd_route, the function the row block itself branches on: the bounds of the rule."""
    q = ops.att_bwd_route
    assert (ops.ATT_BWD_WIDE, ops.ATT_BWD_NARROW, ops.ATT_BWD_CAP) == (NC.WIDE, NC.NARROW, NC.CAP)
    assert q(200, 256, (0, 0)) == NC.NARROW and q(200, 256, (199, 199)) == NC.NARROW
    assert q(200, 256, (10, 10 + NC.CAP - 1)) == NC.NARROW and q(200, 256, (10, 10 + NC.CAP)) == NC.WIDE
    assert q(256, 256, (0, 63)) == NC.NARROW and q(257, 256, (0, 63)) == NC.WIDE and q(256, 257, (0, 63)) == NC.WIDE
    assert q(200, 256, (200, -1)) == NC.WIDE          # the empty support
    assert q(200, 256, (5, 4)) == NC.WIDE and q(200, 256, (-1, 3)) == NC.WIDE and q(200, 256, (190, 200)) == NC.WIDE
    assert q(200, 256, None) == NC.WIDE               # no support handed in
    assert q(1, 1, (0, 0)) == NC.NARROW
    monkeypatch.setenv("PARROT_ATT_BWD_NARROW", "0")
    assert q(200, 256, (0, 0)) == NC.WIDE and q(23, 32, (3, 19)) == NC.WIDE
    monkeypatch.setenv("PARROT_ATT_BWD_NARROW", "1")
    assert q(200, 256, (0, 0)) == NC.NARROW


@pytest.mark.parametrize("att_type", NC.ATT_TYPES)
@pytest.mark.parametrize("name", sorted(NC.STEP_CASES))
def test_step_cases_place_their_windows(ops, monkeypatch, name, att_type):
    (B, H, A, U, E), rows = NC.STEP_CASES[name]
    x, ref = NC.step_case(name, att_type)
    phi = ref['phi']
    assert phi.shape == (B, U) and len(rows) == B
    seen = set()
    for r, row in enumerate(rows):
        lo, hi = NC.claimed_support(row, U)
        if hi < lo:
            assert float(phi[r].max()) < NC.EMPTY, (r, float(phi[r].max()))
            width = 0
        else:
            assert float(phi[r, lo]) > NC.ALIVE and float(phi[r, hi]) > NC.ALIVE, (r, float(phi[r, lo]), float(phi[r, hi]))
            assert lo == 0 or float(phi[r, :lo].max()) < NC.DEAD, (r, float(phi[r, :lo].max()))
            assert hi == U - 1 or float(phi[r, hi + 1:].max()) < NC.DEAD, (r, float(phi[r, hi + 1:].max()))
            width = hi - lo + 1
        route = ops.att_bwd_route(U, E, (lo, hi))
        print(f"{name} {att_type} row {r}: support ({lo}, {hi}), {width} rows, route {route}")
        assert route == row[-1], (r, route)
        assert route == (NC.NARROW if 1 <= width <= NC.CAP and U <= 256 and E <= 256 else NC.WIDE)
        seen.add((width, route))
        monkeypatch.setenv("PARROT_ATT_BWD_NARROW", "0")
        assert ops.att_bwd_route(U, E, (lo, hi)) == NC.WIDE
        monkeypatch.delenv("PARROT_ATT_BWD_NARROW")
    assert ops.att_bwd_route(U, E, None) == NC.WIDE
    if name == "U200":
        assert {(1, NC.NARROW), (NC.CAP, NC.NARROW), (NC.CAP + 1, NC.WIDE), (0, NC.WIDE)} <= seen
    for g in ("dh1", "dkappa", "dp"):
        assert torch.isfinite(ref[g]).all()


@pytest.mark.parametrize("name", sorted(NC.MODEL_CASES))
def test_model_cases_keep_or_lose_their_windows(ops, name):
    o = NC.model_oracle(name)
    kw, T, B, U, _ = NC.MODEL_CASES[name]
    assert kw['num_layers'] == 2 and T <= 14 and B <= 5 and U <= NC.CAP
    phi = o['av'][4]
    E = o['av'][2].shape[-1]  # w [T, B, E]
    assert phi.shape == (T, B, U) and E <= 256
    sups = NC.oracle_supports(phi)
    empty = sum(s is None for s in sups)
    widths = [s[1] - s[0] + 1 for s in sups if s is not None]
    print(f"{name}: {empty} of {T * B} rows empty, support widths {min(widths)}..{max(widths)}")
    for s in sups:  # every support inside the text is narrow, whatever f32 makes of its last positions
        if s is not None:
            assert ops.att_bwd_route(U, E, s) == NC.NARROW
    assert ops.att_bwd_route(U, E, (U, -1)) == NC.WIDE
    if name == "IN":
        assert empty == 0 and float(AC.row_max(phi).min()) > 1e-3, "a window left the text"
    else:
        assert empty >= 10 and len(widths) >= 30
    for k, g in o['grads'].items():
        assert torch.isfinite(g).all(), k


@pytest.mark.parametrize("att_type", NC.ATT_TYPES)
@pytest.mark.parametrize("name", sorted(NC.STEP_CASES))
def test_step_cases_are_within_reach_of_float32(name, att_type):
    """The reference's own formulas in float32 (torch, CPU) against float64 stay below 0.6 of every bound the GPU test
    applies (ATT_TOL, PLACEMENT_TOL at U = 200; dp row by row as well): the placements are not so ill-conditioned that
    float32 arithmetic itself would miss them.  Measured worst fraction: 0.57 (U200 softmax, w)."""
    from tests.test_gpu_kernels import ATT_TOL, PLACEMENT_TOL, _att_reference
    from tests.util import rel_err
    U = NC.STEP_CASES[name][0][3]
    x, ref = NC.step_case(name, att_type)
    r32 = _att_reference(att_type, x, torch.float32)
    tol = {**ATT_TOL, **(PLACEMENT_TOL.get((att_type, U)) or {})}
    frac = {n: rel_err(r32[n], ref[n]) / tol[n] for n in ATT_TOL}
    frac['dp rows'] = max(rel_err(r32['dp'][r], ref['dp'][r]) for r in range(ref['dp'].shape[0])) / tol['dp']
    print(f"{name} {att_type}: " + " ".join(f"{n}={f:.2f}" for n, f in frac.items()))
    assert max(frac.values()) <= 0.6, frac

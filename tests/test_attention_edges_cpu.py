"""Premises of tests/test_gpu_attention_edges.py, recomputed from the fp64 oracle on the CPU: the cases of
tests/attention_cases.py really leave the text (P1-P4) or really stay inside it (W1, W2), every gradient is finite, and an
independent float32 evaluation of the oracle stays far inside the GPU tests' tolerances (the cases are not chaotic, so
1e-4 on the outputs and 1e-3 on the gradients are meaningful bounds for an f32 implementation)."""
import pytest
import torch

from tests import attention_cases as AC
from tests.util import rel_err


@pytest.mark.parametrize("name", AC.EDGE_CASES)
def test_edge_cases_leave_the_text(name):
    o = AC.oracle(name)
    T, B, U = AC.shape(name)
    rm = AC.row_max(o['av'][4])
    assert rm.shape == (T, B)
    empty, live = int((rm < AC.EMPTY_BELOW).sum()), int((rm > AC.LIVE_ABOVE).sum())
    print(f"{name}: {empty} of {T * B} rows empty, {live} live")
    assert empty >= 10 and live >= 30
    assert len(o['grads']) >= 10
    for k, g in o['grads'].items():
        assert torch.isfinite(g).all(), k


@pytest.mark.parametrize("name", AC.WIDE_CASES)
def test_wide_cases_keep_a_live_window(name):
    o = AC.oracle(name)
    T, B, U = AC.shape(name)
    rm = AC.row_max(o['av'][4])
    assert rm.shape == (T, B) and o['av'][4].shape[-1] == U
    assert float(rm.min()) > 1e-3, "a window left the text"
    for k, g in o['grads'].items():
        assert torch.isfinite(g).all(), k


@pytest.mark.parametrize("name", ["P1", "P2", "P3", "P4", "P2W", "W1", "W3"])
def test_float32_oracle_is_far_inside_the_tolerances(name):
    """The oracle's own formulas in float32 (torch, CPU) against float64.  Measured, worst output / worst gradient:
    P1 4.2e-7 / 2.2e-6, P2 2.4e-7 / 6.1e-7, P3 6.9e-7 / 1.5e-6, P4 3.0e-7 / 1.4e-6, P2W 3.0e-7 / 5.7e-7, W1 2.4e-6 /
    1.2e-5, W3 7.2e-6 / 2.4e-5.  The bounds asserted are a tenth of the GPU tests' 1e-4 / 1e-3: an implementation that
    rounds like float32 has an order of magnitude to spare on these cases."""
    from oracle import parrot_ref as R
    o = AC.oracle(name)
    cfg, p, batch = AC.build(name, dtype=torch.float32)
    for v in p.values():
        v.requires_grad_()
    cost, _, av, _ = R.compute_cost(p, cfg, *batch, 1)
    cost.backward()
    worst_out = rel_err(cost, o['cost'])
    for i in (0, 1, 2, 4, 5):
        worst_out = max(worst_out, rel_err(av[i], o['av'][i]))
    worst_grad = 0.0
    for k, g in o['grads'].items():
        assert torch.isfinite(p[k].grad).all(), k
        if float(g.abs().max()) >= 1e-12:
            worst_grad = max(worst_grad, rel_err(p[k].grad, g))
    print(f"{name}: float32 oracle vs float64: outputs {worst_out:.2e}, gradients {worst_grad:.2e}")
    assert AC.count_empty(av[4]) >= AC.count_empty(o['av'][4])  # what is empty in fp64 is exactly zero in f32
    assert worst_out <= 1e-5 and worst_grad <= 1e-4

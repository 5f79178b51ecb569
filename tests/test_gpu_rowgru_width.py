"""Width of the row-owning GRU scan blocks (rowgru.hip, PARROT_RG_WAVES): the 8-wave instantiation against the 4-wave one.

Every column tile's K sum stays in one wave, in chunk order, whatever the width, so the states, the saved activations
and the gradients must agree bit for bit -- torch.equal, no tolerance.  Shapes: H = 32 / 48 / 128 (48: fewer tiles than
waves in every phase, an odd chunk count, a partial last round of the backward's element-wise half), 5 rows (one partial
block) and 200 (13 blocks, the last of 8 rows), T = 1 / 3 / 64, forward + reverse chains and one chain alone, with and
without a step mask."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

NAMES = ("h", "z", "r", "rh", "c", "dC", "dG", "dh")


def _rand(shape, dev, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dev)


def _run(dev, monkeypatch, waves, T, B, H, reverse, mask, data):
    from parrot_amd import ops
    monkeypatch.setenv("PARROT_RG_WAVES", str(waves))
    n = len(reverse)
    run = ops.GruSeqRunner(T, B, H, n, reverse, dev, use_graph=False)
    for i in range(n):
        run.inputs[i].copy_(data["inp"][i])
        run.gate_inputs[i].copy_(data["gin"][i])
        run.h[i][0].copy_(data["h0"][i])
        for buf in (run.z[i], run.r[i], run.rh[i], run.c[i], run.dC[i], run.dG[i]):
            buf.fill_(float("nan"))  # (every element must be written by the kernels)
    run.bind(data["Wg"][:n], data["Wc"][:n], mask)
    # (a plan that fell back to the step launches would make the comparison of the two widths a tautology)
    assert run.route() == dict(rowwise=True, waves=waves, nch=H // 16, reason="rowwise")
    run.forward()
    for i in range(n):
        run.dh[i].copy_(data["dh"][i])
    run.backward()
    torch.cuda.synchronize()
    out = [{k: getattr(run, k)[i].clone() for k in NAMES} for i in range(n)]
    run.close()
    return out


@pytest.mark.parametrize("T", [1, 3, 64])
@pytest.mark.parametrize("B", [5, 200])
@pytest.mark.parametrize("H", [32, 48, 128])
def test_wide_blocks_bit_identical(dev, monkeypatch, H, B, T):
    data = dict(inp=[_rand((T, B, H), dev, 10 + i) for i in range(2)], gin=[_rand((T, B, 2 * H), dev, 20 + i) for i in range(2)],
                h0=[_rand((B, H), dev, 30 + i) for i in range(2)], dh=[_rand((T + 1, B, H), dev, 40 + i) for i in range(2)],
                Wc=[_rand((H, H), dev, 50 + i, 1 / math.sqrt(H)) for i in range(2)],
                Wg=[_rand((H, 2 * H), dev, 60 + i, 1 / math.sqrt(H)) for i in range(2)])
    step_mask = (torch.rand(T, B, generator=torch.Generator().manual_seed(6)) > 0.3).float().to(dev)
    for reverse in ([0, 1], [0], [1]):
        for mask in (None, step_mask):
            narrow = _run(dev, monkeypatch, 4, T, B, H, reverse, mask, data)
            wide = _run(dev, monkeypatch, 8, T, B, H, reverse, mask, data)
            for ch, (a, b) in enumerate(zip(narrow, wide)):
                for k in NAMES:
                    assert not torch.isnan(a[k]).any(), (k, "4 waves left elements unwritten")
                    assert torch.equal(a[k], b[k]), (
                        f"{k} chain {ch} reverse={reverse} mask={mask is not None}: "
                        f"max |diff| {float((a[k] - b[k]).abs().max()):.3e}")

"""Encoder through label tables (csrc/labeltables.hip, Parrot._encoder_forward_tables / _encoder_backward_tables) against
the products with the embedded text (PARROT_ENCODER_TABLES=0) and the float64 oracle (oracle/parrot_ref.py encoder_apply).

Gate: for ctx and every encoder gradient, the table path's error against float64 is at most twice the error of the product
path on the same inputs (max |x - ref| / max |ref|) -- the gate of the composed readout and the split GEMM.  Both paths
compute in f32; they differ in where they round (a table entry is one K = D dot product either way; the per-label sums
add their addends in a fixed tree where the products accumulate over K = Te Be inside the MFMAs).

The per-label sums accumulate in double and round once: with f32 tables one case ([7-20-32-4-17-False-same], forward
fork_gate_inputs.b, 1.543e-07 against 7.502e-08) missed the gate by the last bit of a 68-addend sum."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _case(dev, Q, D, ED, B, U, literal, pattern):
    from oracle import parrot_ref as R
    from parrot_amd.model import Parrot
    kw = dict(rnn_h_dim=16, readouts_dim=16, encoder_dim=ED, input_dim=D, num_layers=1, num_characters=Q,
              encoder_type='bidirectional', encoder_literal=literal)
    cfg = R.default_config(**kw)
    p = {k: v for k, v in R.init_params(cfg, seed=3, scale_by_fan_in=True).items()}
    m = Parrot(device=dev, use_graph=False, **kw).allocate()
    m.set_parameter_values(p)
    g = torch.Generator().manual_seed(B * 1000 + U)
    if pattern == 'same':  # every row the same label: one table row takes every addend, all other sums are zero
        labels = torch.full((B, U), Q // 2, dtype=torch.int64)
        mask = torch.ones(B, U, dtype=torch.float64)
    else:                  # label Q - 1 never occurs; labels_mask with zero tails of different lengths
        labels = torch.randint(0, Q - 1, (B, U), generator=g)
        lens = torch.randint(1, U + 1, (B,), generator=g)
        mask = (torch.arange(U)[None, :] < lens[:, None]).double()
    dctx = torch.randn(B, U, 2 * ED, generator=g, dtype=torch.float64)
    return cfg, p, m, labels, mask, dctx


def _reference(cfg, p, labels, mask, dctx):
    from oracle import parrot_ref as R
    enc = {k: v.clone().requires_grad_() for k, v in p.items() if '/encoder/' in k}
    ctx = R.encoder_apply(enc, cfg, labels) * mask[..., None]
    (ctx * dctx).sum().backward()
    return ctx.detach(), {k: v.grad for k, v in enc.items()}


def _run(m, dev, labels, mask, dctx):
    save = {}
    m.zero_grad()
    ctx = m._encoder_forward(labels.to(dev), mask.float().to(dev), save).clone()
    m._encoder_backward(dctx.float().to(dev), save)
    torch.cuda.synchronize()
    grads = {k: v.detach().clone() for k, v in m.get_gradient_dict().items() if '/encoder/' in k}
    return ctx, grads


def _err(x, ref):
    return float((x.double().cpu() - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


SHAPES = [(3, 5), (4, 17), (64, 200)]
CASES = [(Q, D, ED, B, U, lit, 'absent') for (Q, D) in ((43, 420), (7, 20)) for ED in (32, 128) for (B, U) in SHAPES
         for lit in (True, False)]
CASES += [(Q, D, ED, 4, 17, lit, 'same') for (Q, D) in ((43, 420), (7, 20)) for ED in (32, 128) for lit in (True, False)]


@pytest.mark.parametrize("Q,D,ED,B,U,literal,pattern", CASES)
def test_tables_vs_products_vs_float64(dev, monkeypatch, Q, D, ED, B, U, literal, pattern):
    cfg, p, m, labels, mask, dctx = _case(dev, Q, D, ED, B, U, literal, pattern)
    ref_ctx, ref_g = _reference(cfg, p, labels, mask, dctx)
    assert len(ref_g) == 15  # embed_label.W and, per direction, 2 x (W, b), 2 recurrent matrices, the initial state
    monkeypatch.setenv("PARROT_ENCODER_TABLES", "0")
    ctx0, g0 = _run(m, dev, labels, mask, dctx)
    assert m.encoder_path == 'products'
    monkeypatch.setenv("PARROT_ENCODER_TABLES", "1")
    ctx1, g1 = _run(m, dev, labels, mask, dctx)
    assert m.encoder_path == 'tables'
    assert set(g0) == set(g1) == set(ref_g)
    rows = [("ctx", _err(ctx1, ref_ctx), _err(ctx0, ref_ctx))] + [(k, _err(g1[k], ref_g[k]), _err(g0[k], ref_g[k])) for k in sorted(ref_g)]
    for name, e1, e0 in rows:
        print(f"{name}: tables {e1:.3e} products {e0:.3e}")
    bad = [(n, e1, e0) for n, e1, e0 in rows if not e1 <= 2 * e0]
    assert not bad, bad
    if pattern == 'same':  # rows of labels that never occur get no gradient at all
        ge = g1['/parrot/encoder/embed_label.W']
        keep = torch.ones(Q, dtype=torch.bool)
        keep[Q // 2] = False
        assert float(ge[keep.to(ge.device)].abs().max()) == 0.0


@pytest.mark.parametrize("N,Q,dims", [(15, 7, (32, 64, 32, 64)), (12800, 43, (128, 256, 128, 256)), (1031, 64, (4,)),
                                      (130, 3, (20, 8))])
def test_label_gather_and_segsum_kernels(dev, N, Q, dims):
    """The two kernels alone: gather == indexing, bit for bit; the segmented sum twice gives identical bits, matches a
    float64 index_add to f32 summation error, and a label that never occurs gives an exactly zero row.  N = 15 / 130 / 1031:
    partial slices and partial rounds of four rows; dims (20, 8): 64-column blocks that span two matrices and end early."""
    from parrot_amd import ops
    g = torch.Generator().manual_seed(N)
    labels = torch.randint(0, Q - 1, (N,), generator=g).to(torch.int32).to(dev)  # (label Q - 1 never occurs)
    tables = [torch.randn(Q, d, generator=g).to(dev) for d in dims]
    rows = [torch.full((N, d), float('nan'), device=dev) for d in dims]
    ops.label_gather(labels, tables, rows)
    for t, r in zip(tables, rows):
        assert torch.equal(r, t[labels.long()])
    dy = [torch.randn(N, d, generator=g).to(dev) for d in dims]
    out = []
    for _ in range(2):
        sums = [torch.full((Q, d), float('nan'), device=dev) for d in dims]
        ops.label_segsum(labels, dy, sums)
        out.append(sums)
    for a, b, y in zip(out[0], out[1], dy):
        assert torch.equal(a, b)
        ref = torch.zeros(Q, y.shape[1], dtype=torch.float64).index_add_(0, labels.long().cpu(), y.double().cpu())
        # f32 sums of at most N addends of magnitude <= max|y|: error <= N eps max|y| (far below it in practice)
        tol = N * 2.0 ** -24 * float(y.abs().max())
        assert float((a.double().cpu() - ref).abs().max()) <= tol
        assert float(a[Q - 1].abs().max()) == 0.0

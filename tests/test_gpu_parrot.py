"""Parity of the HIP decoder path (Parrot.compute_cost / sample_model through the C ABI) against
the fp64 oracle restatement of model.py on the same seeded inputs.

Tolerance: the north star asks for feature frames within 1e-4 relative in fp32; gradients are
compared norm-wise per parameter at 1e-3 (fp32 accumulation over T*B rows vs an fp64 oracle)."""
import pytest
import torch

from tests.util import assert_close, make_batch, rel_err

pytestmark = pytest.mark.gpu

SMALL = dict(rnn_h_dim=64, readouts_dim=48, encoder_dim=16, input_dim=24, speaker_dim=8, num_speakers=5)


def _build(dev, use_graph=False, param_overrides=None, **kw):
    """param_overrides: parameter name -> value the whole parameter is filled with (oracle and HIP model alike)."""
    from oracle import parrot_ref as R
    from parrot_amd.model import Parrot
    base = dict(SMALL)
    base.update(kw)
    cfg = R.default_config(**base)
    p = R.init_params(cfg, seed=7, scale_by_fan_in=True)
    for name, value in (param_overrides or {}).items():
        p[name].fill_(value)
    kw2 = {k: v for k, v in base.items()}
    m = Parrot(device=dev, use_graph=use_graph, **kw2).allocate()
    m.set_parameter_values(p)
    return cfg, p, m


def _check_cost_and_grads(dev, T, B, U, ragged=False, tol_out=1e-4, tol_grad=1e-3, expect_schedule=None,
                          param_overrides=None, **kw):
    from oracle import parrot_ref as R
    cfg, p, m = _build(dev, param_overrides=param_overrides, **kw)
    feat, fm, lab, lm, spk = make_batch(cfg, T, B, U, seed=3, ragged=ragged, speaker=cfg['use_speaker'])
    for v in p.values():
        v.requires_grad_()
    rc, rcarry, rav, rex = R.compute_cost(p, cfg, feat, fm, lab, lm, spk, 1)
    rc.backward()
    m.zero_grad()
    cost, updates, av, _ = m.compute_cost(feat.float().to(dev), fm.float().to(dev), lab.to(dev), lm.float().to(dev),
                                          None if spk is None else spk.to(dev), 1, B)
    cost.backward()
    assert_close(cost, rc, tol_out, "cost")
    if cfg['which_cost'] == 'MSE':
        assert_close(av[0], rav[0], tol_out, "predicted frames")
    assert_close(av[1], rav[1], tol_out, "kappa")
    assert_close(av[2], rav[2], tol_out, "w")
    assert_close(av[4], rav[4], tol_out, "phi")
    assert_close(av[5], rav[5], tol_out, "pi_att")
    grads = m.get_gradient_dict()
    worst = 0.0
    for name, ref in p.items():
        if ref.grad is None:
            continue
        e = rel_err(grads[name], ref.grad)
        scale = float(ref.grad.abs().max())
        if scale < 1e-12:
            assert float(grads[name].abs().max()) < 1e-6, name
            continue
        assert e <= tol_grad, f"grad {name}: rel err {e:.3e}"
        worst = max(worst, e)
    if expect_schedule is not None:  # the plan really ran the schedule under test (no silent fall-back)
        from parrot_amd import _lib
        ws = next(iter(m._train_ws.values()))
        assert int(_lib.load().parrot_decoder_schedule(ws['plan'])) == expect_schedule
    m.close()
    return worst


@pytest.mark.parametrize("L", [1, 2, 3])
def test_cost_and_grads_layers(dev, L):
    _check_cost_and_grads(dev, T=6, B=4, U=9, num_layers=L, encoder_type='bidirectional')


def test_cost_and_grads_feedback_speaker_ragged(dev):
    _check_cost_and_grads(dev, T=7, B=5, U=11, ragged=True, num_layers=3, encoder_type='bidirectional',
                          full_feedback=True, use_speaker=True)


def test_cost_and_grads_softmax_attention_nonliteral_encoder(dev):
    _check_cost_and_grads(dev, T=5, B=3, U=8, num_layers=2, encoder_type='bidirectional',
                          attention_type='softmax', encoder_literal=False, weak_feedback=True)


def test_cost_and_grads_gmm_head(dev):
    _check_cost_and_grads(dev, T=5, B=4, U=7, num_layers=2, encoder_type='bidirectional', which_cost='GMM',
                          k_gmm=3, tol_grad=2e-3)


def test_larger_batch_multi_chunk(dev):
    """B > 64 exercises the 64-row chunking of the step kernels; odd sizes exercise the masks."""
    _check_cost_and_grads(dev, T=4, B=70, U=13, num_layers=2, encoder_type='bidirectional', weak_feedback=True)


def test_graph_replay_equals_eager_and_tbptt_carry(dev):
    """hipGraph replay == eager launches (bitwise), and one long window == two windows with the
    carried state (start_flag=0; model.py:633-643, datasets.py:107-133)."""
    from oracle import parrot_ref as R
    T, B, U = 8, 4, 6
    outs = {}
    for use_graph in (False, True):
        cfg, p, m = _build(dev, use_graph=use_graph, num_layers=2, encoder_type='bidirectional', weak_feedback=True)
        feat, fm, lab, lm, _ = make_batch(cfg, T, B, U, seed=5)
        args = [t.to(dev) for t in (feat.float(), fm.float(), lab, lm.float())]
        for rep in range(2):  # second call replays the captured graph
            m.zero_grad()
            c, upd, av, _ = m.compute_cost(args[0], args[1], args[2], args[3], None, 1, B)
            c.backward()
        outs[use_graph] = (c.detach().clone(), av[0].clone(), m.flat_gradients.clone())
        if use_graph:
            c1, u1, av1, _ = m.compute_cost(args[0][:5], args[1][:5], args[2], args[3], None, 1, B)
            m.apply_updates(u1)
            c2, u2, av2, _ = m.compute_cost(args[0][4:], args[1][4:], args[2], args[3], None, 0, B)
            both = torch.cat([av1[0], av2[0]], 0)
            assert_close(both, av[0], 1e-5, "TBPTT carry")
        m.close()
    assert torch.equal(outs[False][0], outs[True][0])
    assert torch.equal(outs[False][1], outs[True][1])
    assert_close(outs[True][2], outs[False][2], 1e-6, "graph grads")


@pytest.mark.parametrize("kw", [dict(num_layers=3, full_feedback=True, use_speaker=True),
                                dict(num_layers=2, weak_feedback=True, sharpening_coeff=1.2, timing_coeff=0.9),
                                dict(num_layers=1)])
def test_sample_model_parity(dev, kw):
    from oracle import parrot_ref as R
    cfg, p, m = _build(dev, use_graph=True, encoder_type='bidirectional', **kw)
    N, U, S = 4, 9, 12
    _, _, lab, lm, spk = make_batch(cfg, 2, N, U, seed=9, speaker=cfg['use_speaker'])
    with torch.no_grad():
        ref = R.sample_model(p, cfg, lab, lm, spk, S)
    outs = m.sample_model(lab.numpy(), lm.float().numpy(), None, None if spk is None else spk.numpy(), N, S)
    for o, r, n in zip(outs, ref, ("sample_x", "k", "w", "pi", "phi", "pi_att")):
        assert o.shape == tuple(r.shape), n
        assert_close(torch.from_numpy(o), r, 1e-4, n)
    m.close()


def test_full_width_short_window(dev):
    """BASELINE cfg2 widths (H=1024, B=64, U=200, E=256) on a short window: parity on frames/cost."""
    from oracle import parrot_ref as R
    from parrot_amd.model import Parrot
    kw = dict(num_layers=2, encoder_type='bidirectional', rnn_h_dim=1024, readouts_dim=1024)
    cfg = R.default_config(**kw)
    p = R.init_params(cfg, seed=11, scale_by_fan_in=True, dtype=torch.float32)
    m = Parrot(device=dev, use_graph=True, **kw).allocate()
    m.set_parameter_values(p)
    T, B, U = 6, 64, 200
    feat, fm, lab, lm, _ = make_batch(cfg, T, B, U, seed=13, ragged=True, dtype=torch.float32)
    with torch.no_grad():
        rc, _, rav, _ = R.compute_cost(p, cfg, feat, fm, lab, lm, None, 1)
    cost, _, av, _ = m.compute_cost(feat.to(dev), fm.to(dev), lab.to(dev), lm.to(dev), None, 1, B)
    assert_close(cost, rc, 1e-4, "cost")
    assert_close(av[0], rav[0], 1e-4, "frames")
    cost.backward()
    g = m.flat_gradients
    assert torch.isfinite(g).all() and float(g.abs().max()) > 0
    m.close()


def test_sample_model_gmm_head_parity(dev):
    """GMM sampling head (model.py:1017-1033, sample_gmm :94-118) with explicit randomness."""
    from oracle import parrot_ref as R
    cfg, p, m = _build(dev, use_graph=True, encoder_type='bidirectional', num_layers=2, which_cost='GMM', k_gmm=4,
                       weak_feedback=True, use_speaker=True, sampling_bias=0.5)
    N, U, S = 3, 7, 9
    _, _, lab, lm, spk = make_batch(cfg, 2, N, U, seed=4, speaker=True)
    g = torch.Generator().manual_seed(11)
    unif = torch.rand(S, N, generator=g, dtype=torch.float64)
    noise = torch.randn(S, N, 63, generator=g, dtype=torch.float64)
    with torch.no_grad():
        ref = R.sample_model(p, cfg, lab, lm, spk, S, unif=unif, noise=noise)
    outs = m.sample_model_device(lab, lm.float(), spk, N, S, unif=unif.float(), noise=noise.float())
    for o, r, n in zip(outs, ref, ("sample_x", "k", "w", "pi", "phi", "pi_att")):
        assert tuple(o.shape) == tuple(r.shape), n
        assert_close(o, r, 2e-4, n)
    outs2 = m.sample_model(lab.numpy(), lm.float().numpy(), None, spk.numpy(), N, S)  # own seeded RNG
    assert outs2[0].shape == (S, N, 63)
    m.close()


def test_raw_output_head_trains_samplernn_on_predicted_frames(dev):
    """model.py:793-820: cost = 0*cost + 1*cost_raw, SampleRNN conditioned on the predicted frames."""
    from oracle import parrot_ref as R
    from oracle import samplernn_ref as S
    from parrot_amd.model import Parrot
    from parrot_amd.sampleRNN import lib
    from parrot_amd.sampleRNN.models.conditional import three_tier as tt
    lib.delete_all_params()
    lib.set_device(dev)
    tt.configure(DIM=32, EMB_SIZE=8)
    try:
        base = dict(SMALL, num_layers=2, encoder_type='bidirectional')
        cfg = R.default_config(**base)
        p = R.init_params(cfg, seed=7, scale_by_fan_in=True)
        c = S.config(DIM=32, EMB_SIZE=8)
        ps = S.init_params(c, seed=5, perturb=0.2)
        lib.set_params(ps)
        m = Parrot(device=dev, use_graph=False, raw_output=True, **base).allocate()
        m.set_parameter_values(p)
        T, B, U = 3, 2, 5
        feat, fm, lab, lm, _ = make_batch(cfg, T, B, U, seed=3)
        g = torch.Generator().manual_seed(8)
        raw = torch.randint(0, 256, (T + 1, B, 80), generator=g)
        for v in list(p.values()) + list(ps.values()):
            v.requires_grad_()
        _, _, rav, _ = R.compute_cost(p, cfg, feat, fm, lab, lm, None, 1)
        raw_mask = fm.repeat_interleave(80, dim=0).t()
        raw_seq = raw.permute(1, 0, 2).reshape(B, -1)
        z = torch.zeros(B, 1, 32, dtype=torch.float64)
        rc, rip, _, _ = S.compute_cost(ps, c, raw_seq, rav[0].transpose(0, 1), z, z, 1, raw_mask)
        rc.backward()
        m.zero_grad()
        cost, upd, av, cost_raw = m.compute_cost(feat.float().to(dev), fm.float().to(dev), lab.to(dev),
                                                 lm.float().to(dev), None, 1, B, raw_audio=raw.to(dev))
        cost.backward()
        assert_close(cost, rc, 1e-4, "cost == cost_raw")
        assert_close(cost_raw, rc, 1e-4, "cost_raw")
        grads = m.get_gradient_dict()
        for name in ('/parrot/readout_to_output.W', '/parrot/rnn1.state_to_gates', '/parrot/h1_to_readout.W'):
            assert rel_err(grads[name], p[name].grad) < 2e-3, name
        for name in ('SampleLevel.L2.W0', 'BigFrameLevel.rnn_inp_fusion.W1', 'FrameLevel.GRU1.Step.Recurrent_Gates.W0'):
            assert rel_err(lib.param(name).grad, ps[name].grad) < 2e-3, name
        assert len(upd) == 2 + 2 + 2  # h1, h2, k, w + SampleRNN h0 / big_h0
        m.close()
    finally:
        lib.delete_all_params()
        tt.configure(DIM=1024, EMB_SIZE=256)


# ----------------------------------------------------------------------------- LSTM decoder layers
@pytest.mark.parametrize("L", [1, 2, 3])
def test_lstm_decoder_cost_and_grads(dev, L):
    """cell_type='lstm' (BASELINE configs[3] generalisation): same scan with LSTM layers."""
    _check_cost_and_grads(dev, T=6, B=4, U=9, num_layers=L, encoder_type='bidirectional', cell_type='lstm')


def test_lstm_decoder_feedback_speaker_ragged(dev):
    _check_cost_and_grads(dev, T=7, B=5, U=11, ragged=True, num_layers=3, encoder_type='bidirectional',
                          full_feedback=True, use_speaker=True, cell_type='lstm')


def test_lstm_decoder_gmm_batch70(dev):
    _check_cost_and_grads(dev, T=4, B=70, U=8, num_layers=2, encoder_type='bidirectional', which_cost='GMM',
                          k_gmm=3, tol_grad=2e-3, cell_type='lstm', weak_feedback=True)


def test_lstm_decoder_graph_and_tbptt_carry(dev):
    from oracle import parrot_ref as R
    T, B, U = 8, 4, 6
    cfg, p, m = _build(dev, use_graph=True, num_layers=2, encoder_type='bidirectional', weak_feedback=True,
                       cell_type='lstm')
    feat, fm, lab, lm, _ = make_batch(cfg, T, B, U, seed=5)
    args = [t.to(dev) for t in (feat.float(), fm.float(), lab, lm.float())]
    for rep in range(2):
        m.zero_grad()
        c, upd, av, _ = m.compute_cost(args[0], args[1], args[2], args[3], None, 1, B)
        c.backward()
    full = av[0].clone()
    with torch.no_grad():
        rc1, carry, rav1, _ = R.compute_cost(p, cfg, feat[:5], fm[:5], lab, lm, None, 1)
        rc2, _, rav2, _ = R.compute_cost(p, cfg, feat[4:], fm[4:], lab, lm, None, 0, carry=carry)
    c1, u1, av1, _ = m.compute_cost(args[0][:5], args[1][:5], args[2], args[3], None, 1, B)
    m.apply_updates(u1)
    c2, u2, av2, _ = m.compute_cost(args[0][4:], args[1][4:], args[2], args[3], None, 0, B)
    assert_close(torch.cat([av1[0], av2[0]], 0), full, 1e-5, "TBPTT carry (cells included)")
    assert_close(c2, rc2, 1e-4, "second-window cost vs oracle")
    assert_close(av2[0], rav2[0], 1e-4, "second-window frames vs oracle")
    m.close()


@pytest.mark.parametrize("kw", [dict(num_layers=3, full_feedback=True, use_speaker=True),
                                dict(num_layers=2, weak_feedback=True, which_cost='GMM', k_gmm=3)])
def test_lstm_decoder_sample_model_parity(dev, kw):
    from oracle import parrot_ref as R
    cfg, p, m = _build(dev, use_graph=True, encoder_type='bidirectional', cell_type='lstm', **kw)
    N, U, S = 4, 9, 12
    _, _, lab, lm, spk = make_batch(cfg, 2, N, U, seed=9, speaker=cfg['use_speaker'])
    g = torch.Generator().manual_seed(11)
    unif = torch.rand(S, N, generator=g, dtype=torch.float64)
    noise = torch.randn(S, N, cfg['output_dim'], generator=g, dtype=torch.float64)
    with torch.no_grad():
        ref = R.sample_model(p, cfg, lab, lm, spk, S, unif=unif, noise=noise)
    outs = m.sample_model_device(lab, lm.float(), spk, N, S, unif=unif.float(), noise=noise.float())
    for o, r, n in zip(outs, ref, ("sample_x", "k", "w", "pi", "phi", "pi_att")):
        assert_close(o, r, 2e-4 if cfg['which_cost'] == 'GMM' else 1e-4, n)
    m.close()


# ----------------------------------------------------------------------------- scan schedules
@pytest.mark.parametrize("sched,chunk", [("0", "50"), ("3", "3"), ("3", "50"), ("5", "50")])
@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_scan_schedules_agree_with_oracle(dev, monkeypatch, sched, chunk, cell):
    """The merged-wavefront schedule (0), the chunk-skewed wavefront with hoisted projections (3: what layer_norm runs on;
    chunk 3 forces several chunks and a ragged last one) and the balanced wavefront (5) are orders of the same arithmetic:
    all must match the oracle, eager and graph.  (Schedules 1, 2 and 6 of rounds 1-3 -- measured losers -- were removed
    in round 5.)"""
    monkeypatch.setenv("PARROT_SCHEDULE", sched)
    monkeypatch.setenv("PARROT_CHUNK", chunk)
    for use_graph in (False, True):
        _check_cost_and_grads(dev, T=8, B=5, U=9, num_layers=3, encoder_type='bidirectional', full_feedback=True,
                              use_speaker=True, cell_type=cell, use_graph=use_graph)
    _check_cost_and_grads(dev, T=7, B=4, U=6, num_layers=2, encoder_type='bidirectional', cell_type=cell,
                          use_graph=True)


@pytest.mark.parametrize("wstep", ["1", "0"])
@pytest.mark.parametrize("sched", [5])
def test_balanced_wavefront_schedules(dev, monkeypatch, sched, wstep):
    """Schedule 5 (attention in one heterogeneous launch with the upper layers' input projections) on the shapes the
    other schedules are tested on, plus: one layer (falls back to 0), more rows than one row tile, the softmax window,
    ragged masks, a window of one step, eager and graph.  Both placements of the upper layers' w rows (round 6: in the
    layers' own step jobs; PARROT_S5_WSTEP=0: in the attention launch's projection jobs)."""
    monkeypatch.setenv("PARROT_SCHEDULE", str(sched))
    monkeypatch.setenv("PARROT_S5_WSTEP", wstep)
    for use_graph in (False, True):
        _check_cost_and_grads(dev, T=9, B=40, U=9, num_layers=2, encoder_type='bidirectional', use_graph=use_graph,
                              expect_schedule=sched)
    _check_cost_and_grads(dev, T=8, B=5, U=9, num_layers=3, encoder_type='bidirectional', full_feedback=True,
                          use_speaker=True, ragged=True, use_graph=True, expect_schedule=sched)
    _check_cost_and_grads(dev, T=6, B=4, U=9, num_layers=1, encoder_type='bidirectional', use_graph=True,
                          expect_schedule=0)
    _check_cost_and_grads(dev, T=5, B=3, U=8, num_layers=2, encoder_type='bidirectional', attention_type='softmax',
                          use_graph=True, expect_schedule=sched)
    _check_cost_and_grads(dev, T=1, B=4, U=6, num_layers=2, encoder_type='bidirectional', use_graph=True,
                          expect_schedule=sched)
    # LSTM layers: one fused product per layer-step, the input projections keep the gate-interleaved column order of
    # the tiled weight copies
    for use_graph in (False, True):
        _check_cost_and_grads(dev, T=8, B=5, U=9, num_layers=3, encoder_type='bidirectional', full_feedback=True,
                              use_speaker=True, cell_type='lstm', use_graph=use_graph, expect_schedule=5)
    _check_cost_and_grads(dev, T=7, B=20, U=6, num_layers=2, encoder_type='bidirectional', cell_type='lstm',
                          use_graph=True, ragged=True, expect_schedule=5)


def test_lstm_one_launch_per_tick_schedule(dev, monkeypatch):
    """Schedule 7 (LSTM layers: the attention of step q-1 inside the launch of tick q, layer 0's w rows behind the
    in-launch flag) forced onto f32 operands (ska_kernel + sk_body's flagged tail): oracle parity incl. every gradient
    for 1-3 layers, ragged masks, feedback + speaker, more than one row tile, eager and graph; and the forward pass
    agrees with schedule 0 to f32 summation order."""
    monkeypatch.setenv("PARROT_SCHEDULE", "7")
    for use_graph in (False, True):
        _check_cost_and_grads(dev, T=8, B=5, U=9, num_layers=3, encoder_type='bidirectional', full_feedback=True,
                              use_speaker=True, cell_type='lstm', use_graph=use_graph, ragged=True, expect_schedule=7)
    _check_cost_and_grads(dev, T=7, B=40, U=6, num_layers=2, encoder_type='bidirectional', cell_type='lstm',
                          use_graph=True, expect_schedule=7)
    _check_cost_and_grads(dev, T=6, B=4, U=9, num_layers=1, encoder_type='bidirectional', cell_type='lstm',
                          use_graph=True, expect_schedule=7)
    _check_cost_and_grads(dev, T=1, B=4, U=6, num_layers=2, encoder_type='bidirectional', cell_type='lstm',
                          use_graph=True, expect_schedule=7)
    # GRU layers are not covered: the plan runs the balanced wavefront instead
    _check_cost_and_grads(dev, T=5, B=4, U=6, num_layers=2, encoder_type='bidirectional', use_graph=True, expect_schedule=5)
    got = {}
    for sched in ("0", "7"):
        monkeypatch.setenv("PARROT_SCHEDULE", sched)
        cfg, p, m = _build(dev, use_graph=True, num_layers=3, encoder_type='bidirectional', cell_type='lstm')
        feat, fm, lab, lm, _ = make_batch(cfg, 9, 20, 7, seed=4, ragged=True)
        cost, _, av, _ = m.compute_cost(feat.float().to(dev), fm.float().to(dev), lab.to(dev), lm.float().to(dev), None, 1, 20)
        got[sched] = (cost.detach().clone(), av[0].detach().clone(), av[2].detach().clone())
        m.close()
    # (not bit for bit: the attention beside GEMM workgroups runs one block per batch row instead of column slices, and the
    # flagged tail deals its K chunks to the waves behind the main ring's -- same terms, other order)
    for a, b, n in zip(got["0"], got["7"], ("cost", "frames", "w")):
        assert_close(a, b.double().cpu(), 2e-6, f"schedule 7 vs 0: {n}")


# ----------------------------------------------------------------------------- layer_norm=True (model.py:24-34)
@pytest.mark.parametrize("kw", [
    dict(num_layers=3, full_feedback=True, use_speaker=True),
    dict(num_layers=2, weak_feedback=True, which_cost='GMM', k_gmm=3),
    dict(num_layers=1, weak_feedback=True),
    dict(num_layers=3, cell_type='lstm', weak_feedback=True, use_speaker=True),
])
def test_layer_norm_cost_and_grads(dev, monkeypatch, kw):
    """`_apply_norm` on every Fork output that the reference normalises (out_to_h*, speaker_to_h*, h{j}_to_h{l},
    h{l}_to_readout); chunk 3 makes the in-scan normalisations span several pipeline chunks."""
    monkeypatch.setenv("PARROT_CHUNK", "3")
    for use_graph in (False, True):
        _check_cost_and_grads(dev, T=8, B=5, U=9, ragged=True, encoder_type='bidirectional', layer_norm=True,
                              use_graph=use_graph, tol_grad=2e-3, **kw)


@pytest.mark.parametrize("kw", [dict(num_layers=3, full_feedback=True, use_speaker=True),
                                dict(num_layers=2, weak_feedback=True, cell_type='lstm'),
                                dict(num_layers=1, weak_feedback=True, use_speaker=True, which_cost='GMM', k_gmm=3)])
def test_layer_norm_sample_model_parity(dev, kw):
    from oracle import parrot_ref as R
    cfg, p, m = _build(dev, use_graph=True, encoder_type='bidirectional', layer_norm=True, **kw)
    N, U, S = 4, 9, 10
    _, _, lab, lm, spk = make_batch(cfg, 2, N, U, seed=9, speaker=cfg['use_speaker'])
    g = torch.Generator().manual_seed(11)
    unif = torch.rand(S, N, generator=g, dtype=torch.float64)
    noise = torch.randn(S, N, cfg['output_dim'], generator=g, dtype=torch.float64)
    with torch.no_grad():
        ref = R.sample_model(p, cfg, lab, lm, spk, S, unif=unif, noise=noise)
    outs = m.sample_model_device(lab, lm.float(), spk, N, S, unif=unif.float(), noise=noise.float())
    for o, r, n in zip(outs, ref, ("sample_x", "k", "w", "pi", "phi", "pi_att")):
        assert_close(o, r, 3e-4, n)
    m.close()


# ----------------------------------------------------------------------------- frozen vectors
def test_hip_path_matches_frozen_oracle_vectors(dev):
    """HIP path vs tests/golden/parrot_golden.npz (oracle-generated, see make_parrot_golden.py): cost, frames, window
    state, a handful of gradients and the decode loop for GRU / GMM / LSTM / layer_norm configurations."""
    import importlib.util
    import os
    import numpy as np
    from oracle import parrot_ref as R
    from parrot_amd.model import Parrot
    here = os.path.dirname(os.path.abspath(__file__))
    spec = importlib.util.spec_from_file_location("mk", os.path.join(here, "golden", "make_parrot_golden.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    gold = np.load(os.path.join(here, "golden", "parrot_golden.npz"))
    for name, kw in mk.CASES.items():
        full = dict(mk.SMALL, **kw)
        cfg = R.default_config(**full)
        p = R.init_params(cfg, seed=11, scale_by_fan_in=True)
        m = Parrot(device=dev, use_graph=True, **full).allocate()
        m.set_parameter_values(p)
        feat, fm, lab, lm, spk = make_batch(cfg, 6, 4, 9, seed=21, ragged=True, speaker=cfg['use_speaker'])
        m.zero_grad()
        cost, upd, av, _ = m.compute_cost(feat.float().to(dev), fm.float().to(dev), lab.to(dev), lm.float().to(dev),
                                          None if spk is None else spk.to(dev), 1, 4)
        cost.backward()
        g = lambda k: torch.from_numpy(gold[f"{name}|{k}"])
        assert_close(cost, g('cost'), 1e-4, f"{name} cost")
        if cfg['which_cost'] == 'MSE':
            assert_close(av[0], g('next_x'), 1e-4, f"{name} frames")
        assert_close(av[1], g('kappa'), 1e-4, f"{name} kappa")
        assert_close(av[2], g('w'), 1e-4, f"{name} w")
        assert_close(av[4], g('phi'), 1e-4, f"{name} phi")
        grads = m.get_gradient_dict()
        for k in mk.GRAD_KEYS:
            assert_close(grads[k], g('grad:' + k), 2e-3, f"{name} grad {k}")
        S = 5
        gen = torch.Generator().manual_seed(5)
        unif = torch.rand(S, 4, generator=gen, dtype=torch.float64)
        noise = torch.randn(S, 4, cfg['output_dim'], generator=gen, dtype=torch.float64)
        outs = m.sample_model_device(lab, lm.float(), spk, 4, S, unif=unif.float(), noise=noise.float())
        assert_close(outs[0], g('sample_x'), 3e-4, f"{name} sample_x")
        assert_close(outs[1], g('sample_k'), 3e-4, f"{name} sample_k")
        m.close()


# ----------------------------------------------------------------------------- full-size properties (BASELINE cfg2)
def test_full_size_cfg2_properties(dev, monkeypatch):
    """BASELINE configs[1] at its real sizes (L=2, H=1024, B=64, T_enc=200, T_dec=800), where the oracle is too slow:
    size-independent properties of the HIP path.
      * two runs give bitwise identical cost, frames, window state AND flat gradient;
      * reading only the window support == reading all context rows (bitwise: cost, frames, kappa; gradients to
        the summation-order noise of the split-K atomics);
      * one 800-frame window == two 400-frame windows with the carried state (frames);
      * the backward is linear in the upstream gradient."""
    from parrot_amd.model import Parrot
    kw = dict(num_layers=2, rnn_h_dim=1024, readouts_dim=1024, encoder_type='bidirectional')
    T, B, U = 800, 64, 200
    g = torch.Generator().manual_seed(1234)
    feat = torch.randn(T + 1, B, 63, generator=g).to(dev)
    fm = torch.ones(T + 1, B, device=dev)
    lab = torch.randint(0, 43, (B, U), generator=g).to(dev)
    lm = torch.ones(B, U, device=dev)

    def run(dense, upstream=None, windows=((0, T),)):
        monkeypatch.setenv("PARROT_ATT_DENSE", "1" if dense else "0")
        m = Parrot(device=dev, use_graph=True, seed=5, **kw).initialize()
        # spread kappa so that the window stays inside the context for a good part of the sequence
        with torch.no_grad():
            m.get_parameter_dict()['/parrot/h1_to_att/fork_kappa.b'].fill_(-1.5)
        outs = []
        m.zero_grad()
        for i, (a, b) in enumerate(windows):
            c, upd, av, _ = m.compute_cost(feat[a:b + 1], fm[a:b + 1], lab, lm, None, 1 if i == 0 else 0, B)
            if upstream is None:
                c.backward()
            else:
                c.backward(gradient=torch.tensor(upstream, device=dev))
            m.apply_updates(upd)
            outs.append((c.detach().clone(), av[0].clone(), av[1].clone()))
        grads = m.flat_gradients.clone()
        m.close()
        return outs, grads

    o1, g1 = run(False)
    o1b, g1b = run(False)
    # no float atomics anywhere on the path (split-K partials, column sums, the global norm and the lookup-table
    # gradients are all combined in a fixed order): a training step is reproducible bit for bit
    assert torch.equal(o1[0][0], o1b[0][0]) and torch.equal(o1[0][1], o1b[0][1]) and torch.equal(o1[0][2], o1b[0][2])
    assert torch.equal(g1b, g1), "run-to-run gradients"
    od, gd = run(True)
    assert torch.equal(o1[0][0], od[0][0]), "support vs dense: cost"
    assert torch.equal(o1[0][1], od[0][1]), "support vs dense: frames"
    assert torch.equal(o1[0][2], od[0][2]), "support vs dense: kappa"
    assert_close(gd, g1, 1e-6, "support vs dense: gradients")
    assert float(o1[0][2][-1].min()) > 50.0  # kappa moved through the context: the support test is not vacuous
    o2, _ = run(False, windows=((0, 400), (400, 800)))
    assert_close(torch.cat([o2[0][1], o2[1][1]], 0), o1[0][1], 1e-5, "TBPTT carry at full size")
    _, g3 = run(False, upstream=2.0)
    assert_close(g3, 2.0 * g1, 1e-6, "backward linearity")


# ----------------------------------------------------------------------------- profiled launch path
PROFILED_CASES = {
    # name: (model kwargs, compute dtype, T, B, U, environment, schedule the plan picks, plain launches expected)
    "gru_f32": (dict(num_layers=2, rnn_h_dim=64, readouts_dim=64, encoder_type='bidirectional', encoder_dim=32,
                     cell_type='gru'), 'float32', 4, 5, 7, {}, 5, True),
    "lstm_bf16_wide": (dict(num_layers=3, rnn_h_dim=128, readouts_dim=128, encoder_type='bidirectional', encoder_dim=64,
                            cell_type='lstm'), 'bf16', 5, 5, 9, {"PARROT_WK": "2"}, 7, False),
}


@pytest.mark.parametrize("case", sorted(PROFILED_CASES))
def test_profiled_launches_count_and_compute_the_same(dev, monkeypatch, case):
    """The per-dispatch timing of the step-kernel family (parrot_profile_begin / parrot_profile_end2: every launch goes out
    through hipExtLaunchKernelGGL between two events of its own and is recorded with its flops and bytes) on eager
    launches, as in bench.py's roofline leg: it counts launches, accounts work, and changes nothing that is computed --
    cost and every gradient are bit-equal to the same step without profiling.

    gru_f32: the plan picks schedule 5 (asserted) and, with all accumulators allocated, the K-balanced backward tick.  The
    step reaches sk_kernel (the gate / candidate launches of every tick, the backward tick's X and Y launches: the plain
    ones), ska_kernel (the attention beside the upper layer's input projections) and skb_kernel (the backward tick's row
    blocks beside the deferred downward products).
    lstm_bf16_wide: PARROT_WK=2 lets the wide kernel take these small launches, so the plan picks schedule 7 (asserted) with
    the fused backward tick.  The step reaches wka_kernel (every forward tick that carries an attention step), wk_kernel
    (the forward ticks without one: the first, and the two in which only upper layers are left) and wkb_kernel (every
    backward tick); the f32 encoder's step launches stay on sk_kernel.  The plain count is only bounded by the launch
    count here."""
    import ctypes as C
    from oracle import parrot_ref as R
    from parrot_amd import _lib
    from parrot_amd.model import Parrot
    kw, dtype, T, B, U, env, schedule, plain_expected = PROFILED_CASES[case]
    for name in ("PARROT_SCHEDULE", "PARROT_WK", "PARROT_BWD_HETERO", "PARROT_CHUNK", "PARROT_S5_WSTEP", "PARROT_GRU_ROWWISE"):
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    cfg = R.default_config(**kw)
    m = Parrot(device=dev, use_graph=False, compute_dtype=dtype, **kw).allocate()
    m.set_parameter_values(R.init_params(cfg, seed=17, scale_by_fan_in=True))
    feat, fm, lab, lm, _ = make_batch(cfg, T, B, U, seed=18, ragged=True)
    batch = (feat.float().to(dev), fm.float().to(dev), lab.to(dev), lm.float().to(dev))
    lib = _lib.load()

    def step():
        m.zero_grad()
        cost = m.compute_cost(*batch, None, 1, B)[0]
        cost.backward()
        torch.cuda.synchronize()
        return cost.detach().cpu().clone(), {k: v.detach().cpu().clone() for k, v in m.get_gradient_dict().items()}

    def end():
        us, fl, by, plain = C.c_double(), C.c_double(), C.c_double(), (C.c_double * 4)()
        n = lib.parrot_profile_end2(C.byref(us), C.byref(fl), C.byref(by), plain)
        return int(n), us.value, fl.value, by.value, [float(x) for x in plain]

    cost0, grads0 = step()
    lib.parrot_profile_begin()
    try:
        cost1, grads1 = step()
    finally:  # profiling is process-wide: a failing step must not leave it on for the tests that follow
        n, us, fl, by, plain = end()
    assert int(lib.parrot_decoder_schedule(next(iter(m._train_ws.values()))['plan'])) == schedule
    print(f"{case}: {n} launches ({plain[3]:.0f} plain), {us:.1f} us, {fl:.3e} flops, {by:.3e} bytes")
    assert n > 0
    assert 0 <= plain[3] <= n and plain[3] == int(plain[3])
    assert plain[3] < n  # both cases carry heterogeneous launches (ska / skb, wka / wkb): those are not counted as plain
    if plain_expected:
        assert plain[3] > 0 and plain[1] > 0 and plain[2] > 0
    assert fl > 0 and by > 0
    assert plain[1] <= fl and plain[2] <= by
    assert torch.equal(cost0, cost1)
    assert len(grads0) >= 10 and grads0.keys() == grads1.keys()
    for name, g0 in grads0.items():
        assert torch.equal(g0, grads1[name]), name
    lib.parrot_profile_begin()
    assert end()[0] == 0
    m.close()

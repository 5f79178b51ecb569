"""Model-level tests of the fused mixture-density head: Parrot.compute_cost / backward with PARROT_GMM_COST_FUSED at 1 (the
HIP kernels of csrc/gmmcost.hip) and at 0 (the torch element-wise path) against the fp64 oracle and against each other.

Bar: 2e-4 norm-wise, what the GMM parity tests of the decode path use."""
import pytest
import torch

from tests.util import assert_close, make_batch, rel_err

pytestmark = pytest.mark.gpu

BASE = dict(rnn_h_dim=32, readouts_dim=48, encoder_dim=16, input_dim=24, speaker_dim=8, num_speakers=5, output_dim=63,
            num_layers=2, weak_feedback=True, encoder_type='bidirectional', which_cost='GMM', k_gmm=20)
T, B, U = 6, 5, 7
TOL = 2e-4


def _setup(**kw):
    from oracle import parrot_ref as R
    base = dict(BASE, **kw)
    cfg = R.default_config(**base)
    p = R.init_params(cfg, seed=7, scale_by_fan_in=True)
    feat, fm, lab, lm, spk = make_batch(cfg, T, B, U, seed=3, ragged=True, speaker=cfg['use_speaker'])
    fm[:, 2] = 0  # one batch row masked out entirely
    return base, cfg, p, (feat, fm, lab, lm, spk)


def _carry_list(upd):
    return [v for _, v in upd]


def _oracle_carry(cfg, carry):
    hs = [x[0] if isinstance(x, tuple) else x for x in carry['h']]
    out = hs + [carry['k'], carry['w']]
    if cfg['cell_type'] == 'lstm':
        out += [x[1] for x in carry['h']]
    return out


def _run(dev, monkeypatch, switch, base, p, batch, scale=None):
    """One compute_cost + backward of a fresh model with PARROT_GMM_COST_FUSED = switch."""
    from parrot_amd.model import Parrot
    monkeypatch.setenv('PARROT_GMM_COST_FUSED', str(switch))
    feat, fm, lab, lm, spk = batch
    m = Parrot(device=dev, **base).allocate()
    m.set_parameter_values({k: v.detach() for k, v in p.items()})
    assert m.gmm_cost_path is None
    m.zero_grad()
    cost, upd, av, _ = m.compute_cost(feat.float().to(dev), fm.float().to(dev), lab.to(dev), lm.float().to(dev),
                                      None if spk is None else spk.to(dev), 1, B)
    (cost if scale is None else scale * cost).backward()
    torch.cuda.synchronize()
    res = dict(path=m.gmm_cost_path, cost=cost.detach().clone(), coeff=av[3].clone(), next_x=av[0].clone(),
               carry=[c.clone() for c in _carry_list(upd)], grads={k: v.clone() for k, v in m.get_gradient_dict().items()})
    m.close()
    return res


def _check_vs_oracle(res, cfg, p, batch, what):
    from oracle import parrot_ref as R
    for v in p.values():
        v.requires_grad_()
        v.grad = None
    rc, rcarry, rav, _ = R.compute_cost(p, cfg, *batch, 1)
    rc.backward()
    errs = dict(cost=assert_close(res['cost'], rc, TOL, what + " cost"),
                coeff=assert_close(res['coeff'], rav[3], TOL, what + " coeff"),
                mu=assert_close(res['next_x'], rav[0], TOL, what + " mu"))
    for i, (mine, ref) in enumerate(zip(res['carry'], _oracle_carry(cfg, rcarry))):
        errs[f'carry{i}'] = assert_close(mine, ref, TOL, what + f" carry {i}")
    for name, ref in p.items():
        if ref.grad is None:
            continue
        if float(ref.grad.abs().max()) < 1e-12:
            assert float(res['grads'][name].abs().max()) < 1e-6, name
            continue
        errs[name] = assert_close(res['grads'][name], ref.grad, TOL, what + " grad " + name)
    w = max(errs, key=errs.get)
    print(f"{what}: cost {errs['cost']:.2e} coeff {errs['coeff']:.2e} worst {w} {errs[w]:.2e}")


@pytest.mark.parametrize("kw", [dict(), dict(use_speaker=True), dict(cell_type='lstm'), dict(k_gmm=3)],
                         ids=['base', 'speaker', 'lstm', 'k3'])
def test_fused_and_torch_paths_vs_oracle(dev, monkeypatch, kw):
    """Ragged masks with one batch row masked out entirely, in every variant."""
    base, cfg, p, batch = _setup(**kw)
    fused = _run(dev, monkeypatch, 1, base, p, batch)
    torch_ = _run(dev, monkeypatch, 0, base, p, batch)
    assert fused['path'] == 'fused' and torch_['path'] == 'torch'
    _check_vs_oracle(fused, cfg, p, batch, "fused")
    assert_close(fused['cost'], torch_['cost'], TOL, "cost, fused vs torch")
    assert_close(fused['coeff'], torch_['coeff'], TOL, "coeff, fused vs torch")
    for name, g in torch_['grads'].items():
        if float(g.abs().max()) < 1e-12:
            assert float(fused['grads'][name].abs().max()) < 1e-6, name
            continue
        assert_close(fused['grads'][name], g, TOL, "fused vs torch grad " + name)


def test_upstream_gradient_scales_the_fused_gradients(dev, monkeypatch):
    """(3 * cost).backward(): the factor reaches the kernel through rowscale on the device."""
    base, cfg, p, batch = _setup()
    one = _run(dev, monkeypatch, 1, base, p, batch)
    three = _run(dev, monkeypatch, 1, base, p, batch, scale=3.0)
    assert three['path'] == 'fused'
    assert torch.equal(one['cost'], three['cost'])
    for name, g in one['grads'].items():
        if float(g.abs().max()) < 1e-12:
            continue
        assert rel_err(three['grads'][name], 3 * g) <= 1e-6, name


def test_second_tbptt_window(dev, monkeypatch):
    """A second window with start_flag = 0 starts from the carried state; the workspace of the first is reused."""
    from oracle import parrot_ref as R
    from parrot_amd.model import Parrot
    monkeypatch.setenv('PARROT_GMM_COST_FUSED', '1')
    base, cfg, p, _ = _setup()
    feat, fm, lab, lm, _ = make_batch(cfg, 2 * T - 1, B, U, seed=5)
    m = Parrot(device=dev, **base).allocate()
    m.set_parameter_values(p)
    a = [t.to(dev) for t in (feat.float(), fm.float(), lab, lm.float())]
    c1, u1, _, _ = m.compute_cost(a[0][:T + 1], a[1][:T + 1], a[2], a[3], None, 1, B)
    c1.backward()
    m.apply_updates(u1)
    m.zero_grad()
    c2, u2, av2, _ = m.compute_cost(a[0][T - 1:], a[1][T - 1:], a[2], a[3], None, 0, B)
    c2.backward()
    assert m.gmm_cost_path == 'fused'
    with torch.no_grad():
        _, carry, _, _ = R.compute_cost(p, cfg, feat[:T + 1], fm[:T + 1], lab, lm, None, 1)
    for v in p.values():
        v.requires_grad_()
    rc2, rcarry2, rav2, _ = R.compute_cost(p, cfg, feat[T - 1:], fm[T - 1:], lab, lm, None, 0, carry=carry)
    rc2.backward()
    assert_close(c2, rc2, TOL, "second-window cost")
    assert_close(av2[3], rav2[3], TOL, "second-window coeff")
    for i, (mine, ref) in enumerate(zip(_carry_list(u2), _oracle_carry(cfg, rcarry2))):
        assert_close(mine, ref, TOL, f"second-window carry {i}")
    grads = m.get_gradient_dict()
    for name in ('/parrot/readout_to_output/fork_gmm_mu.W', '/parrot/readout_to_output/fork_gmm_sigma.W',
                 '/parrot/readout_to_output/fork_gmm_coeff.b', '/parrot/rnn1.state_to_gates'):
        assert_close(grads[name], p[name].grad, TOL, "second-window grad " + name)
    m.close()


def test_raw_output_trains_through_the_torch_path(dev, monkeypatch):
    """A GMM head under raw_output (one component: the SampleRNN head is conditioned on 63-wide frames) keeps its torch
    graph through the leafs, whatever the switch says.  With one component dco_hat is 0 and O*K = O: this shows the
    dispatch and that the frames' gradient arrives, NOT that a multi-component head trains under raw_output (no such model
    can be built: the SampleRNN tiers take FEAT_DIM = 63 columns)."""
    from oracle import parrot_ref as R
    from oracle import samplernn_ref as S
    from parrot_amd.model import Parrot
    from parrot_amd.sampleRNN import lib
    from parrot_amd.sampleRNN.models.conditional import three_tier as tt
    monkeypatch.setenv('PARROT_GMM_COST_FUSED', '1')
    lib.delete_all_params()
    lib.set_device(dev)
    tt.configure(DIM=32, EMB_SIZE=8)
    try:
        base = dict(BASE, rnn_h_dim=64, readouts_dim=64, num_layers=1, weak_feedback=False, k_gmm=1)
        cfg = R.default_config(**base)
        p = R.init_params(cfg, seed=7, scale_by_fan_in=True)
        lib.set_params(S.init_params(S.config(DIM=32, EMB_SIZE=8), seed=5, perturb=0.2))
        m = Parrot(device=dev, use_graph=False, raw_output=True, **base).allocate()
        m.set_parameter_values(p)
        Tr, Br = 3, 2
        feat, fm, lab, lm, _ = make_batch(cfg, Tr, Br, 5, seed=3)
        raw = torch.randint(0, 256, (Tr + 1, Br, 80), generator=torch.Generator().manual_seed(8))
        m.zero_grad()
        cost, upd, av, cost_raw = m.compute_cost(feat.float().to(dev), fm.float().to(dev), lab.to(dev), lm.float().to(dev),
                                                 None, 1, Br, raw_audio=raw.to(dev))
        cost.backward()
        assert m.gmm_cost_path == 'torch'
        assert bool(torch.isfinite(cost)) and torch.equal(cost.detach(), cost_raw)
        g = m.get_gradient_dict()
        gmu = g['/parrot/readout_to_output/fork_gmm_mu.W']
        assert bool(torch.isfinite(gmu).all()) and float(gmu.abs().max()) > 0  # the raw-audio cost drives the frames
        assert float(g['/parrot/readout_to_output/fork_gmm_sigma.W'].abs().max()) == 0  # 0 * cost: nothing through the NLL
        m.close()
    finally:
        lib.delete_all_params()
        tt.configure(DIM=1024, EMB_SIZE=256)

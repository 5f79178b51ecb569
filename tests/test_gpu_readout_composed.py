"""Composed readout -> output products (parrot_amd/csrc/readout.hip; include/parrot_hip.h, ParrotReadoutComposedDesc).

Kernel level: forward, data backward, weight backward and the decomposition into the factors' gradients against float64
torch, with the error gate of test_split_gemm_error_gate_vs_f32_mfma: the element-wise error of every composed product
is at most 2 x the error of the same quantity from the uncomposed products (ops.gemm under PRECISION_F32) on the same
operands.  As in that test the operands are same-sign and wide-range: nothing cancels, so every element has a meaningful
relative error and the figure measures how rounding accumulates along the reductions.  (With signed operands the
element-wise figure of either path is set by whichever of a few hundred elements lands nearest zero -- with O = 1 a
result has 15 to 1000 elements -- and the ratio of two such maxima scatters by more than the gate's factor whatever the
kernels do.)  The bias gradients are sums, not products of the composition; they are held to the rounding bound of an f32
sum of their length.  Model level: Parrot with the switch PARROT_READOUT_COMPOSED at 1 and at 0 against the fp64 oracle."""
import ctypes as C

import pytest
import torch

from tests.util import assert_close, make_batch, rel_err_elem

pytestmark = pytest.mark.gpu

NAN = float('nan')


def _pos(gen, *shape, spread=0):
    """Same-sign values in [0.5, 1.5), times 2^k with k uniform in [-spread, spread]."""
    v = torch.rand(*shape, generator=gen) + 0.5
    if spread:
        v = v * torch.exp2(torch.randint(-spread, spread + 1, shape, generator=gen).float())
    return v


def _padded(rows, cols, ld, dev, gen, fill=NAN, spread=0):
    """A [rows, cols] view with leading dimension ld > cols; the pad columns hold `fill` (a NaN there poisons every
    result of a kernel that reads past a row's end)."""
    buf = torch.full((rows, ld), fill, dtype=torch.float32)
    buf[:, :cols] = _pos(gen, rows, cols, spread=spread)
    buf = buf.to(dev)
    return buf, buf[:, :cols]


class _Case:
    """Operands, descriptor and float64 references of one shape; built once per shape and shared by the tests."""

    def __init__(self, dev, M, segs, O, R, B=3, slice_rows=0, seed=11):
        from parrot_amd import _lib
        g = torch.Generator().manual_seed(seed + M + 7 * O + len(segs))
        self.dev, self.M, self.segs, self.O, self.R, self.B = dev, M, segs, O, R, B
        Kt = self.Kt = sum(segs)
        self.xb, self.x = zip(*[_padded(M, K, K + 8, dev, g, spread=4) for K in segs])
        self.Wrb, self.Wr = _padded(Kt, R, R + 4, dev, g, spread=4)
        self.Wr.mul_(1.0 / Kt)
        self.Wob, self.Wo = _padded(R, O, O + 1, dev, g, spread=4)
        self.Wo.mul_(1.0 / R)
        self.rb = [_pos(g, R).to(dev) for _ in segs]
        self.bo = _pos(g, O).to(dev)
        self.dpb, self.dp = _padded(M, O, O + 3, dev, g, spread=4)
        self.g0 = dict(gWr=torch.randn(Kt, R, generator=g).to(dev), gWo=torch.randn(R, O, generator=g).to(dev),
                       gbo=torch.randn(O, generator=g).to(dev), grb=[torch.randn(R, generator=g).to(dev) for _ in segs])
        d = self.d = _lib.ReadoutComposedDesc()
        d.M, d.nseg, d.R, d.O, d.zero_rows, d.slice_rows, d.nbias = M, len(segs), R, O, B, slice_rows, len(segs)
        for s, K in enumerate(segs):
            d.K[s], d.ldx[s], d.lddx[s] = K, K + 8, K + 4
            d.x[s], d.rb[s] = self.x[s].data_ptr(), self.rb[s].data_ptr()
        d.Wr, d.ldwr, d.Wo, d.ldwo, d.bo = self.Wr.data_ptr(), R + 4, self.Wo.data_ptr(), O + 1, self.bo.data_ptr()
        d.ldp, d.lddp, d.ldgwr, d.ldgwo = 66, O + 3, R, O
        d.dp = self.dp.data_ptr()
        n = int(_lib.load().parrot_readout_composed_ws_floats(C.byref(d)))
        assert n > 0
        d.ws_floats = n
        self.ws = torch.full((n,), NAN, device=dev)
        # float64 references
        X = torch.cat([x.double() for x in self.x], 1)
        Wr, Wo, dp = self.Wr.double(), self.Wo.double(), self.dp.double()
        rbs = sum(b.double() for b in self.rb)
        Wp = Wr @ Wo
        sdp = dp.sum(0)
        dWp = X.t() @ dp
        self.ref = dict(pred=X @ Wp + rbs @ Wo + self.bo.double(), dX=dp @ Wp.t(),
                        gWr=dWp @ Wo.t(), gWo=Wr.t() @ dWp + torch.outer(rbs, sdp), gbo=sdp, grb=Wo @ sdp)
        self.sum_abs = dict(gbo=dp.abs().sum(0), grb=Wo.abs() @ dp.abs().sum(0))

    def run(self):
        """One forward + backward call on fresh output buffers; returns the outputs (gradients without their start values
        are NOT subtracted: `gWr` etc. include g0)."""
        from parrot_amd import _lib, ops
        d, dev, M, O, B = self.d, self.dev, self.M, self.O, self.B
        pred = torch.full((M, 66), 7.0, device=dev)
        dxb = [torch.full((B + M, K + 4), 7.0, device=dev) for K in self.segs]
        out = dict(gWr=self.g0['gWr'].clone(), gWo=self.g0['gWo'].clone(), gbo=self.g0['gbo'].clone(),
                   grb=[t.clone() for t in self.g0['grb']])
        d.pred, d.gWr, d.gWo, d.gbo = pred.data_ptr(), out['gWr'].data_ptr(), out['gWo'].data_ptr(), out['gbo'].data_ptr()
        for s in range(len(self.segs)):
            d.dx[s], d.grb[s] = dxb[s].data_ptr(), out['grb'][s].data_ptr()
        _lib.call('parrot_readout_composed_fwd', C.byref(d), self.ws.data_ptr(), ops._stream())
        _lib.call('parrot_readout_composed_bwd', C.byref(d), self.ws.data_ptr(), ops._stream())
        torch.cuda.synchronize()
        out.update(pred=pred, dxb=dxb)
        return out

    def uncomposed(self):
        """The same quantities from the factors at full width, on the f32-input MFMA GEMM."""
        from parrot_amd import ops
        segs, x, Wr, Wo, dp = self.segs, self.x, self.Wr, self.Wo, self.dp
        with ops.gemm_precision(ops.PRECISION_F32):
            rbs = self.rb[0].clone()
            for b in self.rb[1:]:
                rbs.add_(b)
            k = 0
            ro = None
            for s, K in enumerate(segs):
                ro = ops.gemm(x[s], Wr[k:k + K], bias=rbs if s == 0 else None, out=ro, accumulate=s > 0)
                k += K
            pred = ops.gemm(ro, Wo, bias=self.bo)
            dread = ops.gemm(dp, Wo.t())
            dX, gWr, k = [], [], 0
            for s, K in enumerate(segs):
                dX.append(ops.gemm(dread, Wr[k:k + K].t()))
                gWr.append(ops.gemm(x[s].t(), dread))
                k += K
            gWo = ops.gemm(ro.t(), dp)
        torch.cuda.synchronize()
        return dict(pred=pred, dX=torch.cat(dX, 1), gWr=torch.cat(gWr, 0), gWo=gWo)


_cases = {}


def _case(dev, M, segs, O):
    key = (M, segs, O)
    if key not in _cases:
        R = 72 if segs == (32, 32, 16) else 256      # 72: the composition's reduction ends inside a 64-row block
        slice_rows = 64 if M == 130 else 0           # 130 rows in slices of 64: 3 slices; 1000 rows: 16 (automatic)
        c = _Case(dev, M, segs, O, R, slice_rows=slice_rows)
        c.out = c.run()
        _cases[key] = c
    return _cases[key]


SHAPES = [(M, segs, O) for M in (15, 130, 1000) for segs in ((32, 32, 16), (64, 96)) for O in (1, 63, 64)]
# K = 320: two workgroups along K in the weight backward (the second starts inside the first segment and crosses into the
# next), five 64-row blocks of W' through LDS in the forward and the data backward -- the index arithmetic of wide models
SHAPES.append((130, (256, 64), 63))


@pytest.mark.parametrize("M,segs,O", SHAPES)
def test_composed_products_vs_float64(dev, M, segs, O):
    c = _case(dev, M, segs, O)
    out, ref, B = c.out, c.ref, c.B
    # nothing outside the results is written, the rows of slot 0 are zero, no pad column leaks (a leak is a NaN or a 7)
    assert torch.equal(out['pred'][:, O:], torch.full_like(out['pred'][:, O:], 7.0))
    dX = []
    for s, K in enumerate(segs):
        b = out['dxb'][s]
        assert torch.equal(b[:, K:], torch.full_like(b[:, K:], 7.0)), "dX wrote past its row"
        assert torch.equal(b[:B, :K], torch.zeros_like(b[:B, :K])), "slot 0 of dX is not zero"
        dX.append(b[B:, :K])
    # the gate runs on a zero start: a product stored, as the uncomposed figures are (the run above accumulated onto
    # random g0, whose own rounding is not the products')
    z = _zero_start(c)
    got = dict(pred=out['pred'][:, :O], dX=torch.cat(dX, 1), gWr=z['gWr'], gWo=z['gWo'])
    for v in got.values():
        assert bool(torch.isfinite(v).all())
    unc = c.uncomposed()
    figures = {n: (rel_err_elem(got[n], ref[n]), rel_err_elem(unc[n], ref[n])) for n in ('pred', 'dX', 'gWr', 'gWo')}
    print(f"M={M} segs={segs} O={O}: element-wise error vs fp64 (composed, uncomposed):",
          {k: (f"{a:.2e}", f"{b:.2e}") for k, (a, b) in figures.items()})
    for n, (ec, eu) in figures.items():
        assert ec <= 2 * eu, (n, ec, eu)
    # bias gradients: f32 sums of M (+ O) terms, bound gamma_n * sum |terms|
    eps = 2.0 ** -24
    for n, length in (('gbo', M), ('grb', M + O)):
        bound = (length + 2) * eps * c.sum_abs[n] + 1e-30
        vals = [z[n]] if n == 'gbo' else z[n]
        for v in vals:
            err = (v.double() - ref[n]).abs()
            assert bool((err <= bound).all()), (n, float((err / bound).max()))
    # accumulation: the run on g0 added the same amounts
    for n in ('gWr', 'gWo'):
        assert_close(out[n], c.g0[n].double() + ref[n], 1e-5, n + " accumulated")
    assert_close(out['gbo'], c.g0['gbo'].double() + ref['gbo'], 1e-5, "gbo accumulated")
    for s in range(len(segs)):
        assert_close(out['grb'][s], c.g0['grb'][s].double() + ref['grb'], 1e-5, "grb accumulated")


def _zero_start(c):
    if not hasattr(c, 'zero_out'):
        g0 = c.g0
        c.g0 = dict(gWr=torch.zeros_like(g0['gWr']), gWo=torch.zeros_like(g0['gWo']), gbo=torch.zeros_like(g0['gbo']),
                    grb=[torch.zeros_like(t) for t in g0['grb']])
        c.zero_out = c.run()
        c.g0 = g0
    return c.zero_out


@pytest.mark.parametrize("M,segs,O", [(130, (32, 32, 16), 63), (1000, (64, 96), 64)])
def test_composed_runs_are_bit_identical(dev, M, segs, O):
    c = _case(dev, M, segs, O)
    a, b = c.out, c.run()
    for n in ('pred', 'gWr', 'gWo', 'gbo'):
        assert torch.equal(a[n], b[n]), n
    for s in range(len(segs)):
        assert torch.equal(a['dxb'][s], b['dxb'][s]) and torch.equal(a['grb'][s], b['grb'][s])


# ------------------------------------------------------------------------------------------------ model level
MODEL = dict(rnn_h_dim=64, readouts_dim=256, encoder_dim=16, input_dim=24, speaker_dim=8, num_speakers=5,
             encoder_type='bidirectional')


def _model_run(dev, monkeypatch, switch, **kw):
    """compute_cost + backward of a fresh model with PARROT_READOUT_COMPOSED = switch: the oracle's configuration,
    parameters and batch, and the run's path and results."""
    from oracle import parrot_ref as R
    from parrot_amd.model import Parrot
    monkeypatch.setenv('PARROT_READOUT_COMPOSED', str(switch))
    base = dict(MODEL)
    base.update(kw)
    cfg = R.default_config(**{k: v for k, v in base.items() if k != 'compute_dtype'})
    p = R.init_params(cfg, seed=7, scale_by_fan_in=True)
    m = Parrot(device=dev, **base).allocate()
    m.set_parameter_values(p)
    T, B, U = 7, 3, 9
    feat, fm, lab, lm, spk = make_batch(cfg, T, B, U, seed=3, ragged=True, speaker=cfg['use_speaker'])
    m.zero_grad()
    cost, _, av, _ = m.compute_cost(feat.float().to(dev), fm.float().to(dev), lab.to(dev), lm.float().to(dev),
                                    None if spk is None else spk.to(dev), 1, B)
    cost.backward()
    torch.cuda.synchronize()
    res = dict(path=m.readout_path, cost=cost.detach().clone(), frames=av[0].clone(), kappa=av[1].clone(),
               flat=m.flat_gradients.clone(), grads={k: v.clone() for k, v in m.get_gradient_dict().items()},
               ws_keys=set(next(iter(m._train_ws.values())).keys()))
    m.close()
    return cfg, p, (feat, fm, lab, lm, spk), res


_oracle = {}


def _oracle_run(cfg, p, batch, L):
    if L not in _oracle:
        from oracle import parrot_ref as R
        for v in p.values():
            v.requires_grad_()
        rc, _, rav, _ = R.compute_cost(p, cfg, *batch, 1)
        rc.backward()
        _oracle[L] = (rc.detach(), rav[0].detach(), rav[1].detach(), {k: v.grad for k, v in p.items() if v.grad is not None})
    return _oracle[L]


@pytest.mark.parametrize("L", [1, 2, 3])
def test_model_composed_and_factored_vs_oracle(dev, monkeypatch, L):
    worst = {}
    for switch in (1, 0):
        cfg, p, batch, res = _model_run(dev, monkeypatch, switch, num_layers=L)
        assert res['path'] == ('composed' if switch else 'factored')
        assert ('readouts' in res['ws_keys']) == (switch == 0)   # the composed path allocates no [T*B, R] buffer
        rc, rframes, rkappa, rgrads = _oracle_run(cfg, p, batch, L)
        errs = dict(cost=assert_close(res['cost'], rc, 1e-4, "cost"),
                    frames=assert_close(res['frames'], rframes, 1e-4, "frames"),
                    kappa=assert_close(res['kappa'], rkappa, 1e-4, "kappa"))
        for name, ref in rgrads.items():
            if float(ref.abs().max()) < 1e-12:
                assert float(res['grads'][name].abs().max()) < 1e-6, name
                continue
            errs[name] = assert_close(res['grads'][name], ref, 1e-3, "grad " + name)
        w = max(errs, key=errs.get)
        worst[switch] = errs[w]
        print(f"L={L} switch={switch}: cost {errs['cost']:.2e} frames {errs['frames']:.2e} kappa {errs['kappa']:.2e} "
              f"worst gradient/any {w} {errs[w]:.2e}")
    assert worst[1] <= 2 * worst[0], worst


@pytest.mark.parametrize("kw", [dict(which_cost='GMM', k_gmm=3), dict(layer_norm=True), dict(use_speaker=True),
                                dict(compute_dtype='bf16'), dict(readouts_dim=48)],
                         ids=['gmm', 'layer_norm', 'speaker', 'bf16', 'narrow_readout'])
def test_other_models_keep_the_factored_path(dev, monkeypatch, kw):
    runs = [_model_run(dev, monkeypatch, switch, num_layers=2, **kw)[3] for switch in (1, 0)]
    for r in runs:
        assert r['path'] == 'factored'
    for n in ('cost', 'frames', 'kappa', 'flat'):
        assert torch.equal(runs[0][n], runs[1][n]), n

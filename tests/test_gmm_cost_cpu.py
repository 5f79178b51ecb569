"""CPU tests of the fused mixture-density head (csrc/gmmcost.hip): argument checks of the two entry points (no launch
without a GPU), the dispatch predicate of Parrot.compute_cost, and the kernels' resource report (no scratch)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BADARG, UNSUPPORTED = 10001, 10002


@pytest.fixture(scope="module")
def lib():
    from parrot_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def _fwd_args(M=4, O=3, K=2, **kw):
    p = 0x1000  # never dereferenced: every call below is rejected before a launch
    a = dict(y=p, ldy=O, mu=p, ldmu=O * K, sig=p, ldsig=O * K, co=p, ldco=K, M=M, O=O, K=K, eps=1e-5, nll=p, pi=p, ldpi=K,
             logr=p, stream=None)
    a.update(kw)
    return [a[n] for n in ('y', 'ldy', 'mu', 'ldmu', 'sig', 'ldsig', 'co', 'ldco', 'M', 'O', 'K', 'eps', 'nll', 'pi', 'ldpi',
                           'logr', 'stream')]


def _bwd_args(M=4, O=3, K=2, **kw):
    p = 0x1000
    a = dict(y=p, ldy=O, mu=p, ldmu=O * K, sig=p + 64, ldsig=O * K, co=p, ldco=K, logr=p, rs=p, M=M, O=O, K=K, eps=1e-5,
             dmu=p + 0x1000, lddmu=O * K, dsig=p + 0x2000, lddsig=O * K, dco=p + 0x3000, lddco=K, stream=None)
    a.update(kw)
    return [a[n] for n in ('y', 'ldy', 'mu', 'ldmu', 'sig', 'ldsig', 'co', 'ldco', 'logr', 'rs', 'M', 'O', 'K', 'eps', 'dmu',
                           'lddmu', 'dsig', 'lddsig', 'dco', 'lddco', 'stream')]


@pytest.mark.parametrize("kw", [dict(y=None), dict(mu=None), dict(sig=None), dict(co=None), dict(nll=None), dict(logr=None),
                                dict(ldmu=5), dict(ldsig=5), dict(ldy=2), dict(ldco=1), dict(ldpi=1),
                                dict(M=0), dict(O=0), dict(K=0)],
                         ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_fwd_rejects_bad_arguments(lib, kw):
    assert lib.parrot_gmm_cost_fwd(*_fwd_args(**kw)) == BADARG


@pytest.mark.parametrize("kw", [dict(y=None), dict(mu=None), dict(sig=None), dict(co=None), dict(logr=None), dict(rs=None),
                                dict(dmu=None), dict(dsig=None), dict(dco=None),
                                dict(ldmu=5), dict(lddmu=5), dict(lddsig=5), dict(lddco=1), dict(M=0), dict(O=0), dict(K=0),
                                # the gradients' ranges may overlap neither an input's nor each other's:
                                dict(dmu=0x1000), dict(dsig=0x1000 + 64), dict(dco=0x1000), dict(dmu=0x1000 + 92),
                                dict(dsig=0x2000 - 4), dict(dco=0x2000), dict(dco=0x3000 - 28), dict(dmu=0x3000 + 8)],
                         ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_bwd_rejects_bad_arguments(lib, kw):
    assert lib.parrot_gmm_cost_bwd(*_bwd_args(**kw)) == BADARG


def test_more_than_64_components_are_unsupported(lib):
    assert lib.parrot_gmm_cost_fwd(*_fwd_args(K=65, ldmu=195, ldsig=195, ldco=65, ldpi=65)) == UNSUPPORTED
    assert lib.parrot_gmm_cost_bwd(*_bwd_args(K=65, ldmu=195, ldsig=195, ldco=65, lddmu=195, lddsig=195,
                                              lddco=65)) == UNSUPPORTED


def test_null_pi_out_is_not_a_bad_argument(lib):
    """pi_out may be NULL (then ldpi is not looked at): the call gets past the argument check -- K = 65 is what stops it."""
    assert lib.parrot_gmm_cost_fwd(*_fwd_args(K=65, ldmu=195, ldsig=195, ldco=65, pi=None, ldpi=0)) == UNSUPPORTED


SMALL = dict(rnn_h_dim=16, readouts_dim=12, encoder_dim=4, input_dim=6, num_layers=1, encoder_type='bidirectional')


def _predicate(**kw):
    from parrot_amd.model import Parrot
    m = Parrot(device='cpu', **dict(SMALL, **kw))
    assert m.gmm_cost_path is None  # no step has run
    return m._gmm_cost_fused()


def test_dispatch_predicate(monkeypatch):
    monkeypatch.delenv('PARROT_GMM_COST_FUSED', raising=False)
    assert _predicate(which_cost='GMM', k_gmm=20) is True
    assert _predicate(which_cost='GMM', k_gmm=64) is True
    assert _predicate(which_cost='GMM', k_gmm=65) is False
    assert _predicate(which_cost='MSE') is False
    monkeypatch.setenv('PARROT_GMM_COST_FUSED', '1')
    assert _predicate(which_cost='GMM', k_gmm=20) is True
    monkeypatch.setenv('PARROT_GMM_COST_FUSED', '0')
    assert _predicate(which_cost='GMM', k_gmm=20) is False


def test_dispatch_predicate_is_read_per_step(monkeypatch):
    from parrot_amd.model import Parrot
    m = Parrot(device='cpu', which_cost='GMM', k_gmm=3, **SMALL)
    monkeypatch.setenv('PARROT_GMM_COST_FUSED', '0')
    assert m._gmm_cost_fused() is False
    monkeypatch.setenv('PARROT_GMM_COST_FUSED', '1')
    assert m._gmm_cost_fused() is True


def test_raw_output_keeps_the_torch_path(monkeypatch):
    monkeypatch.setenv('PARROT_GMM_COST_FUSED', '1')
    from parrot_amd.model import Parrot
    m = Parrot(device='cpu', which_cost='GMM', k_gmm=3, **SMALL)
    m.raw_output = True  # (the predicate reads the attribute; building a SampleRNN head is not what is tested here)
    assert m._gmm_cost_fused() is False


def test_gmm_cost_kernels_use_no_scratch(tmp_path):
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")
    if not hipcc:
        pytest.skip("hipcc not available")
    src = os.path.join(ROOT, "parrot_amd", "csrc", "gmmcost.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", src, "-o", str(tmp_path / "g.o"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    name, scratch = None, {}
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            scratch[name] = int(m.group(1))
    assert any("gmm_cost_fwd_kernel" in n for n in scratch) and any("gmm_cost_bwd_kernel" in n for n in scratch), scratch
    assert all(v == 0 for v in scratch.values()), scratch

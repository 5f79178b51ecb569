"""CPU side of the encoder's label tables and of the scan block width: the dispatch predicate and its switch, the
agreement of header / ctypes bindings / INTEGRATION.md on the new symbols, the width switch's rounding, the compile-time
properties of the scan kernels (no scratch at either width), and the algebra the table path rests on, in float64."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("parrot_label_tables_supported", "parrot_label_gather", "parrot_label_segsum_ws_floats", "parrot_label_segsum")


@pytest.fixture(scope="module")
def lib():
    from parrot_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def _model(**kw):
    from parrot_amd.model import Parrot
    small = dict(rnn_h_dim=16, readouts_dim=12, encoder_dim=8, input_dim=6, num_layers=1)
    small.update(kw)
    return Parrot(device='cpu', **small).allocate()


def test_dispatch_predicate_and_switch(lib, monkeypatch):
    monkeypatch.delenv("PARROT_ENCODER_TABLES", raising=False)
    m = _model(encoder_type='bidirectional')
    assert m.encoder_path is None
    assert m._encoder_tables(4, 9)
    monkeypatch.setenv("PARROT_ENCODER_TABLES", "0")   # read per step
    assert not m._encoder_tables(4, 9)
    monkeypatch.setenv("PARROT_ENCODER_TABLES", "1")
    assert m._encoder_tables(4, 9)
    assert not _model(encoder_type='bidirectional', num_characters=65)._encoder_tables(4, 9)  # table too tall for the LDS sums
    assert _model(encoder_type='bidirectional', num_characters=64)._encoder_tables(4, 9)
    assert not _model(encoder_type='bidirectional', encoder_dim=6)._encoder_tables(4, 9)      # 16-byte column groups
    assert not _model(encoder_type=None)._encoder_tables(4, 9)


def test_supported_and_workspace_size(lib):
    assert lib.parrot_label_tables_supported(12800, 43) == 1
    assert lib.parrot_label_tables_supported(1, 64) == 1
    assert lib.parrot_label_tables_supported(1, 65) == 0
    assert lib.parrot_label_tables_supported(0, 43) == 0
    assert lib.parrot_label_segsum_ws_floats(12800, 43, 768) == 2 * 100 * 43 * 768  # slices of 128 rows, double partial sums
    assert lib.parrot_label_segsum_ws_floats(129, 7, 96) == 2 * 2 * 7 * 96


def test_bad_descriptors_are_rejected_without_gpu(lib):
    from parrot_amd import _lib
    d = _lib.LabelTablesDesc()
    assert lib.parrot_label_gather(C.byref(d), None) == 10001
    assert lib.parrot_label_segsum(C.byref(d), None, 0, None) == 10001
    d.N, d.Q, d.nseg, d.labels = 8, 65, 1, 16
    assert lib.parrot_label_gather(C.byref(d), None) == 10002
    d.Q, d.nseg = 7, 5
    assert lib.parrot_label_gather(C.byref(d), None) == 10001


def test_header_bindings_and_integration_agree(lib):
    from parrot_amd import _lib
    header = open(os.path.join(ROOT, "include", "parrot_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, header), s
        assert s in _lib.SIGNATURES and hasattr(lib, s), s
        assert s in doc, s
    assert "ParrotLabelTablesDesc" in header and "ParrotLabelTablesDesc" in doc
    src = '#include <stdio.h>\n#include "parrot_hip.h"\nint main(void){printf("%zu\\n", sizeof(ParrotLabelTablesDesc));return 0;}\n'
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "s.c")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", os.path.join(td, "s")])
        assert int(subprocess.check_output([os.path.join(td, "s")])) == C.sizeof(_lib.LabelTablesDesc)


def test_switches_are_documented():
    txt = open(os.path.join(ROOT, "parrot_amd", "csrc", "switches.h")).read()
    assert "PARROT_ENCODER_TABLES" in txt and "PARROT_RG_WAVES" in txt


def test_scan_kernels_use_no_scratch_at_either_width(tmp_path):
    """A spilled scan kernel is still correct; only the compiler's report shows it (see test_build_cpu.py)."""
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")
    if not hipcc:
        pytest.skip("hipcc not available")
    src = os.path.join(ROOT, "parrot_amd", "csrc", "rowgru.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", src, "-o", str(tmp_path / "rg.o"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    name, seen, bad = None, set(), []
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name and ("rg_fwd_kernel" in name or "rg_bwd_kernel" in name):
            seen.add(name)
            if int(m.group(1)) > 0:
                bad.append((name, int(m.group(1))))
    assert len(seen) == 32, seen  # H / 16 = 1..8, 4 and 8 waves, forward and backward
    assert not bad, bad


def test_table_algebra_float64():
    """x2^T dC == embed^T S_C, sum_q S == column sums, x2 W == (embed W)[labels], and d embed from both formulations."""
    g = torch.Generator().manual_seed(0)
    Q, D, ED, N = 7, 20, 8, 60
    embed = torch.randn(Q, D, generator=g, dtype=torch.float64)
    labels = torch.randint(0, Q - 1, (N,), generator=g)  # (label Q - 1 never occurs)
    W = torch.randn(D, ED, generator=g, dtype=torch.float64)
    b = torch.randn(ED, generator=g, dtype=torch.float64)
    dC = torch.randn(N, ED, generator=g, dtype=torch.float64)
    x2 = embed[labels]
    S = torch.zeros(Q, ED, dtype=torch.float64).index_add_(0, labels, dC)
    kw = dict(rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(x2 @ W + b, (embed @ W + b)[labels], **kw)
    torch.testing.assert_close(x2.t() @ dC, embed.t() @ S, **kw)
    torch.testing.assert_close(S.sum(0), dC.sum(0), **kw)
    dx = dC @ W.t()
    demb_scatter = torch.zeros(Q, D, dtype=torch.float64).index_add_(0, labels, dx)
    torch.testing.assert_close(S @ W.t(), demb_scatter, **kw)
    assert float(S[Q - 1].abs().max()) == 0.0

"""Which job descriptor a step-kernel workgroup picks and which epilogue fields it sees, in every launch mode the host
chooses (tests/step_launch_cases.py has the table): z-mode launches with grid.z = 1 and grid.z > 1, prefix-mode launches
from 2 jobs up to the most a plan makes, the heterogeneous launches beside the attention and state row blocks, the
generic one-tile path and the flagged last segment -- through the C ABI and the decoder entry points.

Every buffer a case writes is compared twice: against float64 with the tolerance the neighbouring test file uses for the
same kernel, and bit for bit against what the parent of the commit that introduced this file wrote at the same shapes
(tests/golden/step_launch_modes.json: SHA-256 per buffer; step_launch_modes_b5.npz: the arrays of the small runs).  The
kernels are atomic-free and deterministic: a change of the scalar path around the K loop, of the job lookup or of the
launch modes must leave every bit where it was.  A whole-buffer comparison covers the workgroups on both sides of every
boundary of the prefix table (every 16-column tile of every job is compared); tests/test_step_launch_modes_cpu.py checks
where those boundaries lie."""
import pytest
import torch

from tests import step_launch_cases as S
from tests.util import assert_close, rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return S.load_golden()


@pytest.mark.parametrize("B", S.BS)
@pytest.mark.parametrize("family", S.FAMILIES)
def test_step_launch_modes(dev, golden, family, B):
    written, refs, found, required = S.run(family, B, dev)
    cid = S.case_id(family, B)
    if required is not None:  # the plan really made the launches this case is about
        for kernel, zmode, njobs in required:
            assert any(k == kernel and z == zmode and (njobs is None or n == njobs) for k, z, n in found), \
                "%s: no %s launch (z-mode %s, %s jobs) among %s" % (cid, kernel, zmode, njobs, sorted(found))
    for name, t in written.items():
        assert t.dtype != torch.float32 or not bool(torch.isnan(t).any()), "%s: %s has elements nothing wrote" % (cid, name)
    assert set(refs) <= set(written)
    for name, (ref, tol) in refs.items():
        print("%s %s: rel err %.3e (bound %.0e)" % (cid, name, rel_err(written[name], ref), tol))
    for name, (ref, tol) in refs.items():
        assert_close(written[name], ref, tol, "%s: %s" % (cid, name))
    bad = S.check_golden(cid, written, golden)
    assert not bad, "%s differs from the recorded build:\n  %s" % (cid, "\n  ".join(bad))


"""The tail of the step kernels in the compiler's listing: between the last MFMA of the K loop's exit path and the first store of
the epilogue (the LDS meeting point lies in between) no scalar load is issued -- the descriptor fields the epilogue reads have
sat in scalar registers since the batch at the kernel's entry (sk_body, SK_TAIL_FIELDS), so the waves that reach the meeting
point last, whose time is the launch's, wait there for LDS only.  Counted by tools/isa_tail_region.py on the gate and candidate
instantiations of the three kernels that share sk_body.  hipcc cross-compiles without a GPU."""
import importlib.util
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KERNELS = [
    "_Z9sk_kernelILi2ELi2ELb1EEv8SkLaunch", "_Z9sk_kernelILi2ELi2ELb0EEv8SkLaunch",
    "_Z9sk_kernelILi2ELi1ELb1EEv8SkLaunch", "_Z9sk_kernelILi2ELi1ELb0EEv8SkLaunch",
    "_Z10ska_kernelILi2ELi2EEv8SkLaunch10AttFwdArgsii",
    "_Z10skb_kernelILi2ELi2EEv8SkLaunch10AttBwdArgs15GruStateBwdArgsiiiii",
]


def _tool():
    spec = importlib.util.spec_from_file_location("isa_tail_region", os.path.join(ROOT, "tools", "isa_tail_region.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")
    if not hipcc:
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "parrot_amd", "csrc")
    out = tmp_path_factory.mktemp("sk_isa") / "skinny.s"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-S",
                        os.path.join(csrc, "skinny.hip"), "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(out).read().split("\n")


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scalar_load_between_the_last_mfma_and_the_first_epilogue_store(listing, kernel):
    _, _, regs = _tool().regions(listing, kernel)
    # the step-GEMM body's meeting points: the reduction tails with MFMAs and no other barrier in front (the attention blocks
    # of the heterogeneous kernels reduce through LDS too, without MFMAs); sk_kernel<2,1> has two, the second the generic path's
    body = [r for r in regs if "v_mfma" in r["head"][0] and not any("s_barrier" in l for l in r["head"])]
    assert body, "no split-K meeting point found in %s" % kernel
    for r in body:
        print("%s: barrier at +%d, first store at +%d: %d s_load in front, %d behind; waits in front: %s"
              % (kernel, r["barrier"], r["store"], r["head_s_load"], r["tail_s_load"], r["head_waits"]))
        assert r["head_s_load"] == 0, "scalar loads between the K loop's last MFMA and the meeting point"
        assert r["tail_s_load"] == 0, "scalar loads between the meeting point and the first epilogue store"

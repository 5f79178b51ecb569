"""The step kernels' register budget: the heterogeneous launches put two workgroups of eight waves on a CU (ska_kernel runs
the upper layers' projections beside the attention blocks), i.e. four waves per SIMD, which the hardware grants only to
kernels of at most 128 VGPRs.  The resource report of skinny.hip must show that budget kept WITHOUT scratch for the tile
shapes the plans launch -- sk_kernel<1|2, 1|2, *>, ska_kernel<2,2>, skb_kernel<2,2>.  (A kernel squeezed into a budget by
its launch bounds reports the budget's VGPRs and a scratch size instead; tests/test_build_cpu.py holds every step kernel
to no scratch, this file adds the registers.)  hipcc cross-compiles without a GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WANTED = [r"sk_kernelILi%dELi%dELb%d" % (mb, nb, z) for mb in (1, 2) for nb in (1, 2) for z in (0, 1)] + \
         [r"ska_kernelILi2ELi2E", r"skb_kernelILi2ELi2E"]


def test_step_kernels_fit_four_waves_per_simd(tmp_path):
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")
    if not hipcc:
        pytest.skip("hipcc not available")
    src = os.path.join(ROOT, "parrot_amd", "csrc", "skinny.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", src, "-o", str(tmp_path / "sk.o"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    name, report = None, {}
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            report[name] = {}
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                report[name][key] = int(m.group(1))
    bad = []
    for want in WANTED:
        hits = [n for n in report if want in n]
        assert len(hits) == 1, (want, hits)
        v = report[hits[0]]
        print(hits[0], v)
        if v["vgprs"] > 128 or v["scratch"] != 0 or v["occupancy"] < 4:
            bad.append((hits[0], v))
    assert not bad, bad

"""Records what the step kernels write in the cases of tests/step_launch_cases.py: tests/golden/step_launch_modes.json (SHA-256,
shape and dtype of every written buffer) and tests/golden/step_launch_modes_b5.npz (the arrays of the B = 5 runs of the
C-ABI families).  tests/test_gpu_step_launch_modes.py holds later builds to these bits, so record from the build whose
results are the standard (a library of the same ABI built from that commit's kernels, through PARROT_HIP_LIB):

    PARROT_HIP_LIB=parrot_amd/libparrot_hip_parent.so python tools/record_step_launch_golden.py [OUTDIR]

Runs every case twice and refuses to write if the two runs differ (the premise of a bit-for-bit standard)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from tests import step_launch_cases as S  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else S.GOLDEN_DIR
    os.makedirs(out, exist_ok=True)
    dev = torch.device("cuda:0")
    digests, arrays = {}, {}
    for family in S.FAMILIES:
        for B in S.BS:
            cid = S.case_id(family, B)
            first = S.run(family, B, dev)[0]
            again = S.run(family, B, dev)[0]
            one = {k: S.digest(v) for k, v in first.items()}
            assert one == {k: S.digest(v) for k, v in again.items()}, cid + ": two runs of one build differ"
            digests[cid] = one
            if B == 5 and family in S.ARRAY_FAMILIES:
                for k, v in first.items():
                    arrays[cid + "/" + k] = np.ascontiguousarray(v.numpy())
            print(cid, len(one), "buffers")
    with open(os.path.join(out, os.path.basename(S.GOLDEN_JSON)), "w") as f:
        json.dump(digests, f, indent=0, sort_keys=False)
        f.write("\n")
    np.savez(os.path.join(out, os.path.basename(S.GOLDEN_NPZ)), **arrays)
    print("recorded", len(digests), "cases,", len(arrays), "arrays ->", out)


if __name__ == "__main__":
    main()

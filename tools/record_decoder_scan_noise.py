#!/usr/bin/env python
"""Records tests/golden/decoder_scan_noise.json: for every data set of tests/decoder_scan_cases.py and every buffer, the
error of the scan reference evaluated in float32 on the CPU against the same reference in float64 (tests.util.rel_err;
phi, a, b, kappa also element-wise).  The decoder scan edge tests widen a buffer's tolerance to 4 x this floor where the
floor exceeds a quarter of the project's scan tolerance.  Needs no GPU and no built library.

    python tools/record_decoder_scan_noise.py
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from tests import decoder_scan_cases as D  # noqa: E402


def main():
    torch.set_num_threads(1)  # one summation order, whatever the machine
    table = {}
    for case in D.CASES.values():
        name = D.noise_name(case)
        if name not in table:
            table[name] = {k: float("%.3e" % v) for k, v in sorted(D.noise_row(case).items())}
    with open(D.NOISE_FILE, "w") as f:
        json.dump(table, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d data sets -> %s" % (len(table), D.NOISE_FILE))


if __name__ == "__main__":
    main()

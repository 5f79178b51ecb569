"""Records what the decode planners make of the cases of tests/decode_plan_cases.py: tests/golden/decode_plan_digests.json
(return code, info16 and the digest of the placed program, one line per case).  tests/test_decode_plan_digests_cpu.py holds
later builds to it, so record from the build whose programs are the standard -- before a change to the planners, never
after one to make it pass.  Needs no GPU:

    python tools/record_decode_plan_digests.py [OUTFILE]

Plans every case twice and refuses to write if the two differ (the premise of a digest over raw bytes)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import decode_plan_cases as P  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else P.GOLDEN_JSON
    lines = []
    for name in P.CASES:
        rc, info, dig = P.plan(name)
        assert (rc, info, dig) == P.plan(name), name + ": two plans of one descriptor differ"
        assert (rc == 0) == P.CASES[name]["ok"], (name, rc, info)
        assert rc == 0 or int(dig, 16) == 0, (name, dig)
        lines.append("%s: %s" % (json.dumps(name), json.dumps({"rc": rc, "info16": info, "digest": dig})))
    with open(out, "w") as f:
        f.write("{\n" + ",\n".join(lines) + "\n}\n")
    print("recorded", len(lines), "cases ->", out)


if __name__ == "__main__":
    main()

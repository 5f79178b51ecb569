"""Records the decode-workspace fingerprints of the cases of tests/decode_workspace_cases.py:
tests/golden/decode_workspace_fingerprints.json, whose first entry names the commit it was recorded at.
tests/test_decode_workspace_cpu.py holds later builds to it, so record from the commit whose workspaces are the standard --
before a change to Parrot._sample_workspace, never after one to make it pass.  Needs no GPU:

    python tools/record_decode_workspace_fingerprints.py [OUTFILE]

Builds every case twice and refuses to write if the two differ (the premise: no address enters a fingerprint)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import decode_workspace_cases as W  # noqa: E402


def _fingerprint(name):
    with pytest.MonkeyPatch.context() as mp:
        return W.case_fingerprint(name, mp)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else W.GOLDEN_JSON
    assert not subprocess.check_output(["git", "status", "--porcelain", "parrot_amd"], cwd=ROOT), "parrot_amd/ has local changes"
    head = subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=ROOT).decode().strip()
    lines = ['"recorded_at_commit": %s' % json.dumps(head)]
    for name in W.CASES:
        fp = _fingerprint(name)
        assert fp == _fingerprint(name), name + ": two builds of one workspace differ"
        lines.append("%s: %s" % (json.dumps(name), json.dumps(fp, sort_keys=True)))
    with open(out, "w") as f:
        f.write("{\n" + ",\n".join(lines) + "\n}\n")
    print("recorded", len(lines) - 1, "cases at", head, "->", out)


if __name__ == "__main__":
    main()

"""Every decode program, byte for byte: the cases of tests/decode_plan_cases.py planned dry and held to the return code,
info16 and program digest recorded in tests/golden/decode_plan_digests.json (tools/record_decode_plan_digests.py).  The digest
covers the placed unit table and the program's records, so a planner change that moves a unit, a destination, an init or a
workspace address fails here; needs no GPU."""
import pytest

from tests import decode_plan_cases as P


@pytest.fixture(scope="module")
def golden():
    return P.golden()


def test_golden_file_and_case_table_name_the_same_cases(golden):
    assert sorted(golden) == sorted(P.CASES)


def test_digest_entry_rejects_bad_arguments():
    import ctypes as C
    from parrot_amd import _lib
    lib, d, dig = _lib.load(), P.desc(), C.c_ulonglong(7)
    assert lib.parrot_sample_plan_digest_dry(None, 256, C.byref(dig)) == P.BADARG
    assert lib.parrot_sample_plan_digest_dry(C.byref(d), 256, None) == P.BADARG
    assert lib.parrot_sample_plan_digest_dry(C.byref(d), 0, C.byref(dig)) == P.BADARG
    assert dig.value == 7


@pytest.mark.parametrize("name", list(P.CASES))
def test_plan_is_the_recorded_one(name, golden, monkeypatch):
    rc, info, dig = P.plan(name, monkeypatch)
    assert (rc == 0) == P.CASES[name]["ok"], (rc, info)
    if rc != 0:
        assert int(dig, 16) == 0 and info[2] == 0, (dig, info)   # refused for what it is, not by the replay
    else:
        assert info[2] == 0 and int(dig, 16) != 0
    want = golden[name]
    assert rc == want["rc"]
    assert info == want["info16"]
    assert dig == want["digest"]
    assert P.plan(name, monkeypatch) == (rc, info, dig)          # planning again gives the same program

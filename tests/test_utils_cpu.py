"""Decode post-processing that needs no GPU."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def test_end_of_utterance_matches_the_reference_loop():
    """tests/golden/eou_golden.npz: the lengths the reference's own loop (sample.py:145-163, executed from the reference
    script by make_eou_golden.py) assigned to six seeded attention histories -- windows that pass the end of the text,
    one that is too slow, one that never moves."""
    from parrot_amd.utils import end_of_utterance
    gold = np.load(os.path.join(HERE, "golden", "eou_golden.npz"))
    phi, mask, num_steps = gold['phi'], gold['labels_mask'], int(gold['num_steps'])
    got = [end_of_utterance(phi[n], int(mask[n].sum()), num_steps) for n in range(phi.shape[0])]
    assert got == gold['features_lengths'].tolist()
    assert [int(mask[n].sum()) for n in range(phi.shape[0])] == gold['labels_lengths'].tolist()


def test_env_int_parses_like_the_library(monkeypatch):
    """parrot_amd.utils.env_int reads a switch the way csrc/switches.h env_int does (C's atoi, the default when unset):
    the Python checks that decide which optional buffers to allocate agree with the library for every spelling."""
    import ctypes
    import ctypes.util

    from parrot_amd.utils import env_int
    atoi = ctypes.CDLL(ctypes.util.find_library("c")).atoi
    atoi.argtypes, atoi.restype = [ctypes.c_char_p], ctypes.c_int
    monkeypatch.delenv("PARROT_TEST_SWITCH", raising=False)
    assert env_int("PARROT_TEST_SWITCH", 7) == 7
    for v in ("0", "1", "2", "4", "-1", "+3", "00", "04", " 4", "\t\n1", "4x", "x4", "", " ", "on", "off", "1.5", "-",
              "+", "- 1", "0x10", "12345"):
        monkeypatch.setenv("PARROT_TEST_SWITCH", v)
        assert env_int("PARROT_TEST_SWITCH", 7) == atoi(v.encode()), repr(v)

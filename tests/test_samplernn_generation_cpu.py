"""The generation package beside three_tier.py (parrot_amd/sampleRNN/generation: inputs, device, serving) as a package:
both import orders give the same objects under both names, the host-side module needs neither torch nor the library, the
moved code reads the run configuration when it is called, and the one start-row rule is the rule of its three users."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "parrot_amd.sampleRNN.generation"
REEXPORTED = {
    "inputs": ["DRAW_K1", "DRAW_K2", "DRAW_MODES", "_M64", "_per_utterance", "_seed_image", "_splitmix64",
               "build_packed_draws", "build_packed_inputs", "draw_mode_code", "pack_utterances", "schedule_segment",
               "unpack_samples", "utterance_draw_u01", "utterance_seed"],
    "device": ["DeviceGenerator"],
    "serving": ["StreamingGenerator", "generate_packed", "generate_stream"],
}
SAME_OBJECTS = """
import importlib
tt = importlib.import_module("parrot_amd.sampleRNN.models.conditional.three_tier")
for module, names in %r.items():
    m = importlib.import_module("%s." + module)
    for name in names:
        assert getattr(tt, name) is getattr(m, name), (module, name)
print("same objects")
""" % (REEXPORTED, PKG)


def _children(*codes):
    """Runs each piece of code in a fresh interpreter of its own, all at once; returns their outputs."""
    procs = [subprocess.Popen([sys.executable, "-c", code], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                              text=True) for code in codes]
    outs = [p.communicate()[0] for p in procs]
    for p, out in zip(procs, outs):
        assert p.returncode == 0, out
    return outs


def test_both_import_orders_give_the_same_objects():
    three_tier_first = "import parrot_amd.sampleRNN.models.conditional.three_tier\n"
    package_first = "".join("import %s.%s\n" % (PKG, m) for m in REEXPORTED)
    for out in _children(three_tier_first + SAME_OBJECTS, package_first + SAME_OBJECTS):
        assert out.strip().endswith("same objects"), out


def test_host_side_module_needs_no_torch():
    out, = _children("import sys\nimport %s.inputs as m\nassert 'torch' not in sys.modules, 'torch was imported'\n"
                     "assert not any(n.endswith('parrot_amd._lib') for n in sys.modules)\n"
                     "print(m.pack_utterances([2, 1], 1), m.utterance_seed(1, 0) == m.utterance_seed(1, 0))" % PKG)
    assert out.strip() == "([0, 0], [0, 2], 3) True"


def test_configuration_is_read_when_called():
    from parrot_amd.sampleRNN.generation import inputs
    from parrot_amd.sampleRNN.models.conditional import three_tier as tt
    tt.configure(BIG_FRAME_SIZE=20, Q_LEVELS=16)
    try:
        pieces = inputs.unpack_samples(np.arange(40, dtype=np.int32).reshape(1, 40), [1], [0], [1])
    finally:
        tt.configure(BIG_FRAME_SIZE=80, Q_LEVELS=256)
    assert len(pieces) == 1 and pieces[0].shape == (20,) and (pieces[0] == 8).all()
    assert (tt.BIG_FRAME_SIZE, tt.Q_LEVELS, int(tt.Q_ZERO), tt.OVERLAP) == (80, 256, 128, 80)


class _Zeros:
    """A segment runner that returns zeros and keeps what it was called with."""

    def __init__(self):
        self.calls = []

    def __call__(self, features, starts, resume, seeds, temperatures):
        self.calls.append((starts.copy(), seeds.copy(), temperatures.copy()))
        return np.zeros((starts.shape[1], 80 * starts.shape[0]), dtype=np.int32)


@pytest.mark.parametrize("T", [2, 3])
def test_start_row_is_the_rule_of_its_three_users(T):
    """An utterance of min(2, T - s) frames whose prefix is slot s, for every s in 0 .. T-1: its start flag, seed and
    temperature are on row start_row(s, T) of the packed arrays and of the ring a StreamingGenerator.step runs (whose rows
    1 .. n the runner is handed), and nowhere when start_row says None."""
    from parrot_amd.sampleRNN.generation import inputs, serving
    SEED, TEMP, S = 0xFEDCBA9876543210, 0.75, T - 1
    for s in range(T):
        row = inputs.start_row(s, T)
        assert row == (s + 1 if s + 1 < T else None)
        n = min(2, T - s)
        _, starts = inputs.build_packed_inputs([np.ones((n, 63), np.float32)], [0], [s], T, 1)
        useed, utemp = inputs.build_packed_draws([SEED], [TEMP], [0], [s], T, 1)
        want = np.zeros((T, 1), dtype=bool)
        if row is not None:
            want[row, 0] = True
        assert np.array_equal(starts != 0, want)
        assert np.array_equal(useed, np.where(want, np.uint64(SEED), np.uint64(0)))
        assert np.array_equal(utemp, np.where(want, np.float32(TEMP), np.float32(0)))
        # the same slot of a ring of T slots: one-frame utterances fill slots 1 .. prefix - 1 of one stream, the two-frame
        # utterance follows; s = 0 is the prefix in the last slot (S) of the segment before, seen from the next step
        run = _Zeros()
        sg = serving.StreamingGenerator(1, S, run_segment=run, utterance_draws=True)
        prefix = s if s else S
        for _ in range(prefix - 1):
            sg.submit(np.ones((1, 63), np.float32), seed=1, temperature=2.0)
        sg.submit(np.ones((2, 63), np.float32), seed=SEED, temperature=TEMP)
        for _ in range(1 if s else 2):
            sg.step()
        flags, seeds, temps = run.calls[-1]
        rows = flags.shape[0]                       # the ring's rows 1 .. rows
        want = np.zeros((rows, 1), dtype=bool)
        if row is not None:
            assert 1 <= row <= rows
            want[row - 1, 0] = True
        assert np.array_equal(flags != 0, want)
        assert np.array_equal(seeds, np.where(want, np.uint64(SEED), np.uint64(0)))
        assert np.array_equal(temps, np.where(want, np.float32(TEMP), np.float32(0)))

"""The wave-parallel seeded draw (draw_mode 'scan') as far as it can be checked without a GPU: the float32 restatement of
its definition against the float64 oracle at the derived tolerance, the absorption pattern that tells the two modes apart,
the descriptor's layout, the command-line flag and the refusal of an unknown mode.  Cases:
tests/samplernn_draw_scan_cases.py."""
import ctypes as C

import numpy as np
import pytest

from tests import samplernn_draw_scan_cases as DC
from tests import samplernn_sampling_cases as SC


@pytest.fixture(scope="module")
def tt():
    from parrot_amd.sampleRNN.models.conditional import three_tier
    return three_tier


# ---- 1. the restated definition against the oracle ------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", DC.PATTERNS)
def test_restatement_follows_oracle(pattern):
    """All patterns x temperatures x seeds at B = 32, T = 3: a pick differs from the float64 oracle only within DELTA_SCAN
    of the boundary between the two picks, in at most 0.5 % of a case's draws."""
    B, T = 32, 3
    b4 = SC.b4_pattern(pattern)
    for temperature in DC.TEMPERATURES:
        for seed in DC.SEEDS:
            u = SC.u01_table(seed, T, B)
            picks = DC.emulate_picks_scan_f32(b4, temperature, u)
            draws, excused, worst = SC.judge_draws(picks, b4, temperature, u, delta=DC.DELTA_SCAN)
            print(f"SCAN-CPU {pattern} T={temperature} seed={seed}: draws {draws}, excused {excused} (worst {worst:.2e})")
            assert draws == BFS_DRAWS(B, T)


def BFS_DRAWS(B, T):
    return DC.BFS * (T - 1) * B


def test_scan_sums_are_the_definition_on_integers():
    """All terms 1: every tree sum is an exact integer, s_l = 4 (l + 1)."""
    s = DC.scan_sums_f32(np.ones(DC.Q, dtype=np.float32))
    assert s.dtype == np.float32 and np.array_equal(s, 4.0 * np.arange(1, 65))
    u = SC.u01_table(SC.EDGE_SEEDS[0], 3, 8)
    got = DC.emulate_picks_scan_f32(np.full(DC.Q, SC.EDGE_LOGIT, dtype=np.float32), 1.0, u)
    assert np.array_equal(got, np.minimum(np.floor(u * DC.Q), DC.Q - 1).astype(np.int32))
    for b, j, m in SC.edge_hits(SC.EDGE_SEEDS[0], 3, 8):
        assert got[b, j] == m


def test_scan_order_is_not_the_sequential_order():
    """A lane without a source adds nothing; rows are chained, not scanned: s_l is the prefix sum in exact arithmetic and
    differs from the sequential float32 sum in rounding on ordinary terms."""
    e = np.exp(SC.b4_pattern("randn") - SC.b4_pattern("randn").max()).astype(np.float32)
    s = DC.scan_sums_f32(e)
    exact = np.cumsum(e.astype(np.float64))[3::4]
    assert np.abs(s / exact - 1).max() < (DC.SCAN_ADDS + 1) * 2.0 ** -24
    seq = np.cumsum(e, dtype=np.float32)[3::4]
    assert not np.array_equal(s, seq)


# ---- 2. absorption ----------------------------------------------------------------------------------------------------------
def test_absorption_pattern_tells_the_modes_apart():
    b4 = DC.absorb_pattern()
    e = np.exp(b4 - b4.max()).astype(np.float32)
    assert e[0] == 1.0 and 0 < e[1] < 2.0 ** -24 and abs(e[1] / 5.6e-8 - 1) < 0.02
    assert np.cumsum(e, dtype=np.float32)[-1] == 1.0          # the sequential sum absorbs every other term
    c = SC.cdf64(b4, 1.0)
    assert abs((1 - c[0]) / 1.4e-5 - 1) < 0.05                 # the oracle gives them 1.4e-5 of the mass
    assert DC.scan_sums_f32(e)[-1] > 1.0                       # the tree keeps them
    B, T = 8, 3
    for seed in DC.ABSORB_SEEDS:
        u = SC.u01_table(seed, T, B)
        # (u01 == 1.0 would pick Q - 1 in every mode; none of these seeds has one)
        assert u.max() < 1.0
        assert (SC.emulate_picks_f32(b4, 1.0, u) == 0).all(), "the sequential mode picks code 0 for every u01"
        hits = DC.absorb_hits(seed, T, B)
        assert hits == [DC.ABSORB_HITS[seed]], (seed, hits)
        (b, j, want), = hits
        got = DC.emulate_picks_scan_f32(b4, 1.0, u)
        print(f"SCAN-CPU absorption seed {seed}: stream {b} column {j}: oracle {want}, restatement {got[b, j]}, "
              f"distance {SC.boundary_distance(c, u[b, j], got[b, j], want):.2e}")
        # (u01 itself carries 2^-25 = 3e-8 of rounding, half a code's mass here: the restated pick is a few codes off the
        # oracle's, far inside DELTA_SCAN, and it is not code 0)
        assert got[b, j] != 0 and abs(int(got[b, j]) - want) <= 4
        assert np.count_nonzero(got) == 1
        SC.judge_draws(got, b4, 1.0, u, delta=DC.DELTA_SCAN)


# ---- 3. the descriptor, the flag, the refusal -------------------------------------------------------------------------------
def test_descriptor_layout_is_unchanged():
    from parrot_amd._lib import SampleRnnGenDesc as D
    assert C.sizeof(D) == 936
    assert (D.temperature.offset, D.draw_mode.offset, D.seed.offset, D.big_Win_frames.offset) == (32, 36, 40, 48)
    assert D.draw_mode.size == 4 and not hasattr(D, "reserved")
    assert D().draw_mode == 0                                  # a zeroed descriptor is the sequential mode


def test_parser_has_the_flag():
    from parrot_amd.utils import sample_parse
    assert sample_parse([]).draw_mode == 'sequential'
    assert sample_parse(['--draw_mode', 'scan']).draw_mode == 'scan'
    with pytest.raises(SystemExit):
        sample_parse(['--draw_mode', 'tree'])


def test_unknown_mode_is_refused_before_any_device_call(tt, monkeypatch):
    from parrot_amd import _lib
    from parrot_amd.sampleRNN import lib

    def no_device(*a, **k):
        raise AssertionError("a device call in front of the mode check")
    monkeypatch.setattr(_lib, "call", no_device)
    monkeypatch.setattr(_lib, "load", no_device)
    monkeypatch.setattr(lib, "device", no_device)
    assert tt.draw_mode_code('sequential') == 0 and tt.draw_mode_code('scan') == 1
    feats = np.zeros((3, 2, 63), dtype=np.float32)
    for bad in ('tree', 'Scan', 1, None):
        with pytest.raises(ValueError):
            tt.DeviceGenerator(2, 3, draw_mode=bad)
        with pytest.raises(ValueError):
            tt.generate_packed([feats[:, 0]], n_streams=2, draw_mode=bad)
        with pytest.raises(ValueError):
            next(tt.generate_stream(feats, 2, draw_mode=bad))
        with pytest.raises(ValueError):
            tt.StreamingGenerator(2, 2, draw_mode=bad)
        with pytest.raises(ValueError):
            tt.generate_and_save_samples("t", features=feats, draw_mode=bad)
    with pytest.raises(ValueError):                             # the literal three-function loop has one way to draw
        tt.generate_and_save_samples("t", features=feats, use_device_loop=False, draw_mode='scan')


def test_sample_raw_refuses_an_unknown_mode(tt):
    from parrot_amd.model import SampleRnn
    m = object.__new__(SampleRnn)      # (no parameters, no device: the check comes first)
    m.three_tier = tt
    with pytest.raises(ValueError):
        m.sample_raw(None, None, "t", None, draw_mode='tree')

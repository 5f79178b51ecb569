"""Per-utterance seeds and temperatures of the SampleRNN generator (samplernn_generate_set_utterance_draws), as far as they
can be checked without a GPU: the draw key's two identities, the seed derivation, the refusals that need no plan, the
admission plumbing of StreamingGenerator against a host emulator of the plan's entry semantics, the premise of the GPU
oracle test, and the scratch use of the persistent sample kernel.  Cases: tests/samplernn_utt_draw_cases.py."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from oracle import samplernn_ref as S
from tests import samplernn_sampling_cases as SC
from tests import samplernn_utt_draw_cases as UC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tt():
    from parrot_amd.sampleRNN.models.conditional import three_tier
    return three_tier


# ---- 1. / 2. the key's identities -------------------------------------------------------------------------------------------
def test_key_identity_with_todays_key(tt):
    ts = (0, 1, 79, 80, 81, 159, 160, 799, 12345, 2 ** 31 - 2, 2 ** 31 + 7, 2 ** 40 + 1)
    for s in UC.SEEDS:
        for b in range(37):
            for t in ts:
                assert tt.utterance_draw_u01(UC.old_key_seed(s, b), t) == S.draw_u01(s, t, b), (s, b, t)


def test_key_identity_with_the_oracle(tt):
    for sigma in UC.SEEDS + tuple(UC.ORACLE_SEEDS):
        for n in (80, 81, 159, 400, 2 ** 33 + 5):
            assert tt.utterance_draw_u01(sigma, n) == S.draw_u01(sigma ^ UC.K2, n, 0), (sigma, n)
    us = [tt.utterance_draw_u01(234, n) for n in range(80, 2080)]
    assert 0.0 < min(us) and max(us) <= 1.0 and len(set(us)) > 1990 and 0.45 < np.mean(us) < 0.55


# ---- 3. utterance_seed --------------------------------------------------------------------------------------------------------
def test_utterance_seed(tt):
    a = [tt.utterance_seed(234, i) for i in range(1000)]
    assert a == [tt.utterance_seed(234, i) for i in range(1000)]
    assert all(isinstance(x, int) and 0 <= x < 2 ** 64 for x in a) and len(set(a)) == 1000
    assert max(a) >= 2 ** 63, "no seed with the top bit set among 1000: not a 64-bit derivation"
    assert set(a).isdisjoint(tt.utterance_seed(235, i) for i in range(1000))
    assert tt.utterance_seed(2 ** 64 + 234, 3) == tt.utterance_seed(234, 3)   # masked to 64 bits
    # written out once: seed + K1 (index + 1) through the splitmix64 finaliser
    x = (234 + UC.K1 * 4) & UC.M64
    x ^= x >> 30; x = (x * 0xBF58476D1CE4E5B9) & UC.M64; x ^= x >> 27; x = (x * 0x94D049BB133111EB) & UC.M64; x ^= x >> 31
    assert tt.utterance_seed(234, 3) == x


def test_seed_image_survives(tt):
    img = tt._seed_image([0, 1, 2 ** 63 - 1, 2 ** 63 + 5, 2 ** 64 - 1])
    assert img.dtype == np.int64 and img.tolist() == [0, 1, 2 ** 63 - 1, -2 ** 63 + 5, -1]
    assert img.view(np.uint64).tolist() == [0, 1, 2 ** 63 - 1, 2 ** 63 + 5, 2 ** 64 - 1]
    assert tt._seed_image(np.array([[2 ** 63 + 5, 7]], dtype=np.uint64)).shape == (1, 2)
    seeds, temps = tt.build_packed_draws([2 ** 63 + 5, 9, 11], [0.5, 1.0, 2.0], [1, 0, 1], [0, 0, 2], 3, 2)
    assert seeds.dtype == np.uint64 and seeds.tolist() == [[0, 0], [9, 2 ** 63 + 5], [0, 0]]   # (slot 2 + 1 = T: no row)
    assert temps.dtype == np.float32 and temps.tolist() == [[0, 0], [1.0, 0.5], [0, 0]]


# ---- 4. refusals that need no plan ----------------------------------------------------------------------------------------
def test_refusals_without_a_plan(tt):
    utts = [np.zeros((3, 63), dtype=np.float32)] * 3
    with pytest.raises(ValueError):
        tt.generate_packed(utts, n_streams=2, seeds=[1, 2])
    with pytest.raises(ValueError):
        tt.generate_packed(utts, n_streams=2, seeds=[1, 2, 3], temperatures=[1.0, 1.0])
    with pytest.raises(ValueError):
        tt.generate_packed(utts, n_streams=2, temperatures=[1.0, 1.0, 1.0])
    fake = lambda features, starts, resume, **kw: np.zeros((2, 80 * features.shape[0]), dtype=np.int32)
    off = tt.StreamingGenerator(2, 2, run_segment=fake)
    with pytest.raises(ValueError):
        off.submit(utts[0], seed=5)
    with pytest.raises(ValueError):
        off.submit(utts[0], temperature=0.5)
    on = tt.StreamingGenerator(2, 2, run_segment=fake, utterance_draws=True)
    with pytest.raises(ValueError):
        on.submit(utts[0])
    assert on.submit(utts[0], seed=2 ** 64 - 1) == 0


def test_c_entry_refuses_null_arguments():
    from parrot_amd import _lib
    fn = _lib.load().samplernn_generate_set_utterance_draws
    buf = (C.c_ulonglong * 4)()
    fbuf = (C.c_float * 4)()
    assert fn(None, C.addressof(buf), C.addressof(fbuf)) == 10001    # PARROT_ERR_BADARG
    # (a plan is only looked at after the pointers: any non-null value will do here)
    assert fn(C.addressof(buf), None, C.addressof(fbuf)) == 10001
    assert fn(C.addressof(buf), C.addressof(buf), None) == 10001


def test_three_argument_runners_keep_working(tt):
    calls = []

    def runner(features, starts, resume):
        calls.append(features.shape[0])
        return np.zeros((2, 80 * features.shape[0]), dtype=np.int32)

    sg = tt.StreamingGenerator(2, 2, run_segment=runner)
    sg.submit(np.zeros((3, 63), dtype=np.float32))
    assert len(sg.drain()) >= 1 and calls


# ---- 5. admission plumbing against the emulator -----------------------------------------------------------------------------
def _stream_inputs():
    r = np.random.RandomState(7)
    utts = [r.randn(n, 63).astype(np.float32) for n in UC.STREAM_LENGTHS]
    return utts, UC.utt_seeds(len(utts)), UC.utt_temperatures(len(utts))


@pytest.mark.parametrize("S_", UC.STREAM_SEGMENTS)
def test_admission_plumbing(tt, S_):
    utts, seeds, temps = _stream_inputs()
    B = UC.STREAM_B
    alone = [UC.emulate_standalone(tt.utterance_draw_u01, u, s, t) for u, s, t in zip(utts, seeds, temps)]
    sessions = []
    for order in (None, UC.STREAM_ORDER_2):
        emu = UC.PlanEmulator(tt.utterance_draw_u01, B, S_ + 1)
        sg = tt.StreamingGenerator(B, S_, run_segment=emu.run_segment, utterance_draws=True)
        got, stream, slot = UC.drain(sg, utts, seeds, temps, order)
        for i, want in enumerate(alone):
            assert got[i].shape == want.shape and np.array_equal(got[i], want), (S_, order, i, stream[i], slot[i])
        sessions.append((got, stream, slot))
    (a, sa, la), (b, sb, lb) = sessions
    same = [i for i in sa if sa[i] == sb[i]]
    moved = [i for i in same if la[i] != lb[i]]
    # the second order moves utterances to other slots of the same stream: the GPU test's second session is not void
    assert moved, (sa, sb, la, lb)
    for i in same:
        assert np.array_equal(a[i], b[i])
    # the draws are really in the samples: another seed gives another utterance, a neighbour's seed changes nothing
    drawn = [i for i, t in enumerate(temps) if t > 0 and utts[i].shape[0] > 1]
    i = drawn[0]
    other = UC.emulate_standalone(tt.utterance_draw_u01, utts[i], seeds[i] + 1, temps[i])
    assert not np.array_equal(other, alone[i])


def test_a_prefix_in_a_segments_last_slot(tt):
    """With segment_frames = 5 some utterance has its prefix in the last slot of a segment: its start flag, seed and
    temperature are on row 1 of the next segment (and the emulator run of test_admission_plumbing covers it)."""
    utts, seeds, temps = _stream_inputs()
    S_, B = 5, UC.STREAM_B
    seen = []

    def runner(features, starts, resume, seeds=None, temperatures=None):
        seen.append((starts.copy(), np.array(seeds), np.array(temperatures)))
        return np.zeros((B, 80 * features.shape[0]), dtype=np.int32)

    sg = tt.StreamingGenerator(B, S_, run_segment=runner, utterance_draws=True)
    _, stream, slot = UC.drain(sg, utts, seeds, temps)
    late = [i for i in slot if slot[i] % S_ == 0 and utts[i].shape[0] > 1]
    assert late, slot
    for i in late:
        seg = slot[i] // S_          # the segment whose slot 1 is the utterance's frame 1
        starts, sd, tp = seen[seg]
        assert starts[0, stream[i]] == 1 and int(sd[0, stream[i]]) == seeds[i] and tp[0, stream[i]] == np.float32(temps[i])
    for starts, sd, tp in seen:      # seeds and temperatures sit on start flags only
        assert sd.dtype == np.uint64 and tp.dtype == np.float32
        assert ((sd != 0) <= (starts != 0)).all()


# ---- 6. the premise of the GPU oracle test ----------------------------------------------------------------------------------
def test_float32_oracle_keeps_the_cap():
    """The oracle's own float32 run of every utterance of the GPU oracle test, judged by the GPU test's rule against its
    float64 run: at most SC.traj_slack_rows(n) of the n pieces leave."""
    from tests.test_gpu_samplernn import _greedy_follows_oracle
    n = len(UC.ORACLE_CASE.lengths)
    assert set(UC.ORACLE_TEMPERATURES) == set(UC.TEAM_TEMPERATURES)
    assert len(set(UC.ORACLE_SEEDS)) == n and max(UC.ORACLE_SEEDS) >= 2 ** 63
    left = 0
    for i in range(n):
        ref, ref_logits, oseed = UC.oracle_piece(i)
        out, _, _ = UC.oracle_piece(i, torch.float32)
        temp = UC.ORACLE_TEMPERATURES[i]
        assert ref.shape == (80 * UC.ORACLE_CASE.lengths[i],) and (ref[:80] == 128).all()
        if temp > 0:
            exact, _ = SC.draws_follow_oracle(out[None], ref[None], ref_logits[None], temp, oseed, 1)
        else:
            exact = _greedy_follows_oracle(out[None], ref[None], ref_logits[None], 1, slack_rows=1)
        left += 1 - len(exact)
    print(f"UTT-CPU float32 oracle: {n - left} of {n} utterances identical to float64")
    assert left <= SC.traj_slack_rows(n), f"{left} of {n} utterances leave the float64 trajectory in float32"
    # the draws shape the trajectories: a drawn utterance is not its greedy run
    p, feats, gref, _ = UC.GC.gru_reference()
    drawn = [i for i in range(n) if UC.ORACLE_TEMPERATURES[i] > 0]
    assert all(not np.array_equal(UC.oracle_piece(i)[0], gref[i, :80 * UC.ORACLE_CASE.lengths[i]]) for i in drawn)


# ---- 7. build property ----------------------------------------------------------------------------------------------------------
# ScratchSize [bytes/lane] of the six instantiations before the per-utterance entries existed (VGPRs then: 164 / 191 / 182 /
# 212 / 236 / 256): the entries live in the workgroup's shared block, not in registers across the sample steps.
PARENT_SCRATCH = {(256, 0): 0, (256, 1): 0, (512, 0): 0, (512, 1): 0, (1024, 0): 0, (1024, 1): 16}


def test_sample_kernel_scratch(tmp_path):
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")
    if not hipcc:
        pytest.skip("hipcc not available")
    src = os.path.join(ROOT, "parrot_amd", "csrc", "sr_persist.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", src, "-o", str(tmp_path / "srp.o"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    name, seen = None, {}
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            k = re.search(r"srp_kernelILi(\d+)ELb([01])E", name)
            if k:
                seen[(int(k.group(1)), int(k.group(2)))] = int(m.group(1))
    print("UTT-CPU srp_kernel scratch bytes per lane:", seen)
    assert set(seen) == set(PARENT_SCRATCH), seen
    bad = {k: v for k, v in seen.items() if v > PARENT_SCRATCH[k]}
    assert not bad, bad

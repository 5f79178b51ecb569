"""Row groups of the SampleRNN persistent sample kernel (`srp_kernel<D, true>`, sr_persist.hip): with
PARROT_SR_PERSIST_GROUPS = G a batch of up to 32 G streams runs the ten sample steps of a frame in ONE launch, as
ceil(B / 32) groups of 32 streams with exchange slots and a carry of their own.  Against the float64 oracle (greedy
indices and last-step logits), graph replay against eager launches and fresh plans, the eight-period chunk graph,
seeded draws in both groups, stacked LSTM tiers, and the default (switch unset, or a batch of one group) untouched.
Cases and references: tests/samplernn_groups_cases.py (premises checked by tests/test_samplernn_groups_cpu.py)."""
import contextlib

import numpy as np
import pytest

from oracle import samplernn_ref as S
from tests import samplernn_groups_cases as GC
from tests import samplernn_sampling_cases as SC
from tests.test_gpu_samplernn import _greedy_follows_oracle
from tests.util import assert_close

pytestmark = pytest.mark.gpu

SWITCH = "PARROT_SR_PERSIST_GROUPS"


@contextlib.contextmanager
def _model(dev, p, **cfg):
    """The generator's module at DIM 256 / EMB 32 (or the width and frame size cfg names) with the parameters p
    registered; defaults restored afterwards."""
    from parrot_amd.sampleRNN import lib
    from parrot_amd.sampleRNN.models.conditional import three_tier as tt
    lib.delete_all_params()
    lib.set_device(dev)
    tt.configure(**dict(dict(DIM=GC.DIM, EMB_SIZE=GC.EMB, RNN_TYPE='GRU', N_RNN=1), **cfg))
    try:
        lib.set_params(p)
        yield tt
    finally:
        lib.delete_all_params()
        tt.configure(DIM=1024, EMB_SIZE=256, RNN_TYPE='GRU', N_RNN=1, FRAME_SIZE=10)


@contextlib.contextmanager
def _plan(tt, B, T, groups, **kw):
    """A plan that must run on the persistent kernel in `groups` row groups (0: on launches)."""
    gen = tt.DeviceGenerator(B, T, **kw)
    try:
        assert gen.persistent == (groups > 0), "the persistent sample kernel %s" % (
            "did not engage" if groups else "engaged where it must not")
        assert gen.persist_groups == groups, (gen.persist_groups, groups)
        yield gen
    finally:
        gen.close()


def _generate(gen, feats):
    out = gen.generate(np.asarray(feats, dtype=np.float32)).cpu().numpy().copy()
    return out, gen.ws['logits'].detach().cpu().double()


def _follows_oracle(out, last, ref, ref_logits, B, what):
    """Greedy indices against the float64 oracle (a stream may leave it at a near-tie of the oracle's top two logits,
    one stream per started 16) and the last step's logits of the streams that stay, at 1e-4."""
    assert out.shape == ref.shape and out.dtype == np.int32 and (out[:, :80] == 128).all()
    assert out.min() >= 0 and out.max() <= 255
    exact = _greedy_follows_oracle(out, ref, ref_logits, B, slack_rows=GC.slack_rows(B))
    print(f"GROUPS-GPU {what}: rows identical {len(exact)} of {B}")
    assert_close(last[exact], ref_logits[exact, -1], 1e-4, "last-step logits")
    return exact


# ---- 1. the switch engages the kernel past 32 streams -------------------------------------------------------------------
def test_engages(dev, monkeypatch):
    p, _, _, _ = GC.gru_case(GC.GREEDY_CASES["B33"])
    with _model(dev, p) as tt:
        monkeypatch.delenv(SWITCH, raising=False)
        with _plan(tt, 33, 3, 0) as gen:
            assert 'persist_ws' not in gen.ws
        monkeypatch.setenv(SWITCH, "2")
        with _plan(tt, 33, 3, 2) as gen:
            assert gen.persistent and gen.persist_groups == 2
            two = gen.ws['persist_ws'].numel()
        with _plan(tt, 32, 3, 1) as gen:      # the plan takes ceil(B / 32) groups, not the maximum
            one = gen.ws['persist_ws'].numel()
        with _plan(tt, 65, 3, 0):             # three groups under a maximum of two: launches
            pass
        monkeypatch.setenv(SWITCH, "1")
        with _plan(tt, 33, 3, 0):
            pass
        # workspace = sync words + per group 8 exchange blocks ([2 D + Q] x 4 streams) and 8 carries
        per_group = 8 * ((2 * GC.DIM + 256) * 4 + 16 + 4 * 32 + 32 * 4 * 32)
        assert (one, two) == (1024 + per_group, 1024 + 2 * per_group)


# ---- 2. greedy parity ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(GC.GREEDY_CASES))
def test_greedy_parity(dev, name, monkeypatch):
    """Two calls on one plan: the second one meets the carry and the last-step logits every group left behind."""
    s = GC.GREEDY_CASES[name]
    p, feats, ref, ref_logits = GC.gru_case(s)
    monkeypatch.setenv(SWITCH, str(s.switch))
    with _model(dev, p) as tt:
        with _plan(tt, s.B, s.T, s.groups, temperature=0.0) as gen:
            for call in range(2):
                out, last = _generate(gen, feats)
                _follows_oracle(out, last, ref, ref_logits, s.B, f"{name} call {call}")


# ---- 3. graph == eager, replay == fresh plans ---------------------------------------------------------------------------
def test_graph_equals_eager_and_replay_equals_fresh(dev, monkeypatch):
    s = GC.GREEDY_CASES["B37"]
    p, feats, ref, ref_logits = GC.gru_case(s)
    feats2 = SC.features(s.T, s.B, GC.FEAT_SEED_2).numpy()
    monkeypatch.setenv(SWITCH, str(s.switch))
    with _model(dev, p) as tt:
        outs = {}
        for use_graph in (True, False):
            with _plan(tt, s.B, s.T, s.groups, temperature=0.0, use_graph=use_graph) as gen:
                first, last = _generate(gen, feats)
                _follows_oracle(first, last, ref, ref_logits, s.B, f"B37 graph={int(use_graph)}")
                second, _ = _generate(gen, feats2)     # another utterance on the plan: every group's carry is stale
                third, _ = _generate(gen, feats)
                outs[use_graph] = (first, second, third)
            assert np.array_equal(third, first), f"{(third != first).sum()} samples differ on the plan's third call"
        for a, b in zip(outs[True], outs[False]):
            assert np.array_equal(a, b), f"{(a != b).sum()} samples differ between graph replay and eager launches"
        assert not np.array_equal(outs[True][0], outs[True][1])
        for f, want in ((feats, outs[True][0]), (feats2, outs[True][1])):
            with _plan(tt, s.B, s.T, s.groups, temperature=0.0) as gen:
                fresh, _ = _generate(gen, f)
            assert np.array_equal(fresh, want), f"{(fresh != want).sum()} samples differ from a fresh plan's"


# ---- 4. the chunk graph -------------------------------------------------------------------------------------------------
def test_chunk_graph(dev, monkeypatch):
    s = GC.CHUNK_CASE
    p, feats, ref, ref_logits = GC.gru_case(s)
    monkeypatch.setenv(SWITCH, str(s.switch))
    with _model(dev, p) as tt:
        with _plan(tt, s.B, s.T, s.groups, temperature=0.0, use_graph=True) as gen:
            for call in range(2):
                out, last = _generate(gen, feats)
                _follows_oracle(out, last, ref, ref_logits, s.B, f"chunk call {call}")


# ---- 5. seeded draws ----------------------------------------------------------------------------------------------------
def test_seeded_draws(dev, monkeypatch):
    B, T = 37, 3
    c = S.config(DIM=GC.DIM, EMB_SIZE=GC.EMB)
    p = S.init_params(c, seed=GC.DRAW_PARAM_SEED, perturb=0.25)
    feats = SC.features(T, B, GC.DRAW_FEAT_SEED).numpy()
    monkeypatch.setenv(SWITCH, "2")
    with _model(dev, p) as tt:
        outs = []
        for seed in (GC.DRAW_SEEDS[0], GC.DRAW_SEEDS[0], GC.DRAW_SEEDS[1]):
            with _plan(tt, B, T, 2, temperature=1.0, seed=seed) as gen:
                outs.append(_generate(gen, feats)[0])
    assert np.array_equal(outs[0], outs[1]) and not np.array_equal(outs[0], outs[2])
    assert outs[0].min() >= 0 and outs[0].max() <= 255 and (outs[0][:, :80] == 128).all()
    # both groups really draw, every stream with its own b in the hash
    assert len(np.unique(outs[0][:32, 80:])) > 20 and len(np.unique(outs[0][32:, 80:])) > 20
    assert len({outs[0][b].tobytes() for b in range(B)}) == B
    assert not np.array_equal(outs[0][32:], outs[2][32:])


# ---- 6. stacked tiers ---------------------------------------------------------------------------------------------------
def test_stacked_lstm_tiers(dev, monkeypatch):
    s = GC.STACKED_CASE
    p, feats, ref, ref_logits = GC.stacked_reference()
    monkeypatch.setenv(SWITCH, str(s.switch))
    with _model(dev, p, RNN_TYPE='LSTM', N_RNN=2) as tt:
        with _plan(tt, s.B, s.T, s.groups, temperature=0.0, use_graph=True) as gen:
            for call in range(2):
                out, last = _generate(gen, feats)
                _follows_oracle(out, last, ref, ref_logits, s.B, f"stacked call {call}")


# ---- 7. the default is untouched ----------------------------------------------------------------------------------------
def test_one_group_is_the_default_kernel(dev, monkeypatch):
    p, feats, _, _ = GC.gru_case(GC.Case(5, 3, 1, 4))
    with _model(dev, p) as tt:
        monkeypatch.delenv(SWITCH, raising=False)
        with _plan(tt, 5, 3, 1, temperature=0.0) as gen:
            unset, last_unset = _generate(gen, feats)
            n_unset = gen.ws['persist_ws'].numel()
        monkeypatch.setenv(SWITCH, "4")
        with _plan(tt, 5, 3, 1, temperature=0.0) as gen:
            assert gen.persist_groups == 1
            switched, last_switched = _generate(gen, feats)
            assert gen.ws['persist_ws'].numel() == n_unset
    assert np.array_equal(switched, unset)
    assert np.array_equal(last_switched.numpy(), last_unset.numpy())

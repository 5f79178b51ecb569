"""Skip-connection stacks (--skip_conn True: Graves' stacks, ops.py:650-695, 861-880) on the device-resident SampleRNN
generator, behind PARROT_SR_SKIP_STACKS=1 (samplernn_generate_set_skip_stacks): every sample step's log-probability under
full forcing against the float64 oracle, free greedy runs on launches and on the persistent sample kernel,
generate_and_save_samples on the device loop, packing, segments, the setter's refusals, and plans of models without skip
connections untouched by the switch."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import samplernn_ref as S
from tests import samplernn_forced_cases as FC
from tests import samplernn_sampling_cases as SC
from tests.test_gpu_samplernn import _greedy_follows_oracle
from tests.test_gpu_samplernn_groups import _model, _plan
from tests.util import assert_close

pytestmark = pytest.mark.gpu

SWITCH = "PARROT_SR_SKIP_STACKS"
BADARG, UNSUPPORTED = 10001, 10002


@contextlib.contextmanager
def _skip_model(dev, p, **cfg):
    """_model, with SKIP_CONN put back afterwards (its own clean-up does not know the name)."""
    with _model(dev, p, **cfg) as tt:
        try:
            yield tt
        finally:
            tt.configure(SKIP_CONN=False)


def _env(monkeypatch, on=True, launches=False):
    if on:
        monkeypatch.setenv(SWITCH, "1")
    else:
        monkeypatch.delenv(SWITCH, raising=False)
    monkeypatch.delenv("PARROT_SR_PERSIST_GROUPS", raising=False)
    if launches:
        monkeypatch.setenv("PARROT_SR_PERSIST", "0")
    else:
        monkeypatch.delenv("PARROT_SR_PERSIST", raising=False)


def _params(rnn_type, n_rnn, dim=FC.DIM, emb=FC.EMB, seed=95, skip=True):
    c = S.config(DIM=dim, EMB_SIZE=emb, RNN_TYPE=rnn_type, N_RNN=n_rnn, SKIP_CONN=skip)
    return c, S.init_params(c, seed=seed, perturb=0.25)


def _cfg(rnn_type, n_rnn, skip=True, **kw):
    return dict(RNN_TYPE=rnn_type, N_RNN=n_rnn, SKIP_CONN=skip, **kw)


def _samples(gen, feats, **kw):
    return gen.generate(np.asarray(feats, dtype=np.float32), **kw).cpu().numpy().copy()


# ---- 1. every step against the oracle -----------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["persistent", "launches"])
@pytest.mark.parametrize("rnn_type,n_rnn", [("GRU", 2), ("GRU", 3), ("LSTM", 2), ("LSTM", 3)])
def test_full_forcing_follows_the_oracle(dev, rnn_type, n_rnn, path, monkeypatch):
    _env(monkeypatch, launches=path == "launches")
    B, T = 5, 3
    c, p = _params(rnn_type, n_rnn)
    feats = SC.features(T, B, FC.FEAT_SEED)
    forced = FC.codes(B, T)
    want = FC.log_probs({k: v.double() for k, v in p.items()}, c, forced, feats.double()).numpy()
    with _skip_model(dev, p, **_cfg(rnn_type, n_rnn)) as tt:
        with _plan(tt, B, T, 1 if path == "persistent" else 0, temperature=0.0, forcing=True, log_probs=True) as gen:
            assert gen.skip
            for call in range(2):
                samples, logp = gen.generate(feats.float().numpy(), forced=forced)
                samples, logp = samples.cpu().numpy().copy(), logp.cpu().numpy().copy()
                assert np.array_equal(samples[:, 80:], forced[:, 80:]) and (samples[:, :80] == 128).all()
                print(f"SKIP-GPU {rnn_type}{n_rnn} {path} call {call}: largest difference "
                      f"{np.abs(logp[:, 80:] - want).max():.3e}")
                assert_close(torch.from_numpy(logp[:, 80:]).double(), torch.from_numpy(want), FC.PARITY_TOL,
                             f"log-probabilities, {rnn_type} x {n_rnn} {path}")


# ---- 2. free greedy runs ------------------------------------------------------------------------------------------------
def _greedy(tt, p, c, B, T, persistent, feat_seed=8):
    feats = torch.randn(T, B, 63, generator=torch.Generator().manual_seed(feat_seed), dtype=torch.float64)
    with torch.no_grad():
        ref, ref_logits = S.generate(p, c, feats, return_logits=True)
    ref = ref.numpy()
    gen = tt.DeviceGenerator(B, T, temperature=0.0)
    try:
        assert gen.persistent == persistent
        for rep in range(2):
            out = _samples(gen, feats.float().numpy())
            exact = _greedy_follows_oracle(out, ref, ref_logits, B, slack_rows=1)
            last = gen.ws['logits'].detach().cpu().double()
            assert_close(last[exact], ref_logits[exact, -1], 1e-4, "last-step logits")
    finally:
        gen.close()


@pytest.mark.parametrize("rnn_type,n_rnn", [("GRU", 3), ("LSTM", 2)])
def test_greedy_on_launches(dev, rnn_type, n_rnn, monkeypatch):
    _env(monkeypatch)
    c, p = _params(rnn_type, n_rnn, dim=32, emb=8)
    with _skip_model(dev, p, **_cfg(rnn_type, n_rnn, DIM=32, EMB_SIZE=8)) as tt:
        _greedy(tt, p, c, 2, 3, persistent=False)


@pytest.mark.parametrize("rnn_type,n_rnn", [("GRU", 3), ("LSTM", 2)])
def test_greedy_on_the_persistent_kernel(dev, rnn_type, n_rnn, monkeypatch):
    _env(monkeypatch)
    c, p = _params(rnn_type, n_rnn)
    with _skip_model(dev, p, **_cfg(rnn_type, n_rnn)) as tt:
        _greedy(tt, p, c, 5, 3, persistent=True)


# ---- 3. generate_and_save_samples ---------------------------------------------------------------------------------------
def test_generate_and_save_samples_takes_the_device_loop(dev, monkeypatch):
    _env(monkeypatch)
    c, p = _params("GRU", 2, dim=32, emb=8)
    B, T = 2, 3
    feats = torch.randn(T, B, 63, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    with torch.no_grad():
        ref, ref_logits = S.generate(p, c, feats, return_logits=True)
    with _skip_model(dev, p, **_cfg("GRU", 2, DIM=32, EMB_SIZE=8)) as tt:
        # no generation functions: only the device loop can have produced this
        out = tt.generate_and_save_samples("t", None, feats.float().numpy(), None, 0., temperature=0.0)
        assert out.shape == (B, 80 * T) and out.dtype == np.int32
        _greedy_follows_oracle(out, ref.numpy(), ref_logits, B, slack_rows=1)
        drawn = tt.generate_and_save_samples("t", None, feats.float().numpy(), None, 0., temperature=1.0, top_k=8)
        assert drawn.shape == (B, 80 * T) and drawn.min() >= 0 and drawn.max() <= 255 and (drawn[:, :80] == 128).all()
        _env(monkeypatch, on=False)                     # and without the switch: the refusal of every earlier version
        with pytest.raises(ValueError):
            tt.generate_and_save_samples("t", None, feats.float().numpy(), None, 0., temperature=1.0, top_k=8)
        with pytest.raises(NotImplementedError):
            tt.DeviceGenerator(B, T)


# ---- 4. packing ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lengths", [(2, 1, 2), (3, 2, 3)], ids=["slots-2-1-2", "generated-2-1-2"])
def test_packed_utterance_equals_the_utterance_alone(dev, lengths, monkeypatch):
    """Three utterances on two streams; the one that starts second in its stream against the same utterance carried
    first in that stream of a plain plan of the same batch, bit for bit.  Both readings of 'utterances of 2, 1 and 2
    frames': counted with the prefix slot (the second utterance is then its prefix alone, in the plan's last slot) and
    counted in generated frames (it then generates one frame behind a restart inside the loop)."""
    _env(monkeypatch)
    c, p = _params("GRU", 2)
    B = 2
    feats = SC.features(max(lengths), len(lengths), 96).float().numpy()
    utts = [feats[:n, i].copy() for i, n in enumerate(lengths)]
    stream, first, T = None, None, None
    with _skip_model(dev, p, **_cfg("GRU", 2)) as tt:
        stream, first, T = tt.pack_utterances(lengths, B)
        second = [i for i in range(len(lengths)) if first[i] > 0]
        assert len(second) == 1 and lengths[second[0]] == min(lengths)
        pieces = tt.generate_packed(utts, n_streams=B, temperature=0.0)
        for i, n in enumerate(lengths):
            rect = np.zeros((max(2, n), B, 63), dtype=np.float32)
            rect[:n, stream[i]] = utts[i]
            with _plan(tt, B, max(2, n), 1, temperature=0.0) as gen:
                alone = _samples(gen, rect)[stream[i], :80 * n]
            assert pieces[i].shape == alone.shape and np.array_equal(pieces[i], alone), \
                f"utterance {i} (slot {first[i]} of stream {stream[i]}): {(pieces[i] != alone).sum()} samples differ"


# ---- 5. segments --------------------------------------------------------------------------------------------------------
def test_segments_equal_the_run_in_one_piece(dev, monkeypatch):
    _env(monkeypatch)
    c, p = _params("LSTM", 2)
    B, T = 5, 4
    feats = SC.features(T, B, 97).float().numpy()
    kw = dict(temperature=1.0, seed=79)
    with _skip_model(dev, p, **_cfg("LSTM", 2)) as tt:
        with _plan(tt, B, T, 1, **kw) as gen:
            whole = _samples(gen, feats)
        with _plan(tt, B, T, 1, **kw) as gen:
            a = _samples(gen, feats[:2], n_frames=1)
            b = _samples(gen, feats[2:], resume=True, n_frames=2)
    assert a.shape == (B, 160) and b.shape == (B, 160)
    assert np.array_equal(np.concatenate([a, b], axis=1), whole)
    assert len(np.unique(whole[:, 80:])) > 20          # draws, not a constant


# ---- 6. the setter's refusals -------------------------------------------------------------------------------------------
def test_setter_refusals_leave_the_plan_alone(dev, monkeypatch):
    from parrot_amd import _lib
    _env(monkeypatch)
    setter = _lib.load().samplernn_generate_set_skip_stacks
    B, T = 5, 3
    feats = SC.features(T, B, 98).float().numpy()
    c, p = _params("GRU", 2)
    with _skip_model(dev, p, **_cfg("GRU", 2)) as tt:
        with _plan(tt, B, T, 1, temperature=0.0) as gen:
            good = gen.skip_struct()
            before = _samples(gen, feats)
            assert setter(gen.plan, C.byref(good)) == BADARG               # after the first run
            with pytest.raises(_lib.HipCallError):
                gen.set_skip_stacks()
            assert np.array_equal(_samples(gen, feats), before)
        with _plan(tt, B, T, 1, temperature=0.0) as gen:                   # a null S_k, before the first run
            for tag, k in (("frm_S", 1), ("big_S", 0)):
                bad = gen.skip_struct()
                getattr(bad, tag)[k] = None
                assert setter(gen.plan, C.byref(bad)) == BADARG
            for name in ("big_bS", "frm_sum"):
                bad = gen.skip_struct()
                setattr(bad, name, None)
                assert setter(gen.plan, C.byref(bad)) == BADARG
            assert setter(gen.plan, None) == BADARG
            assert np.array_equal(_samples(gen, feats), before)
    c1, p1 = _params("GRU", 1, skip=False)
    with _skip_model(dev, p1, **_cfg("GRU", 1, skip=False)) as tt:        # the single-GRU plan: n_rnn = 0
        with _plan(tt, B, T, 1, temperature=0.0) as gen:
            assert not gen.skip
            fresh = _samples(gen, feats)
        with _plan(tt, B, T, 1, temperature=0.0) as gen:
            assert setter(gen.plan, C.byref(good)) == UNSUPPORTED          # (checked before any pointer is read)
            assert np.array_equal(_samples(gen, feats), fresh)


# ---- 7. off is off --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("temperature", [0.0, 1.0])
@pytest.mark.parametrize("rnn_type,n_rnn", [("GRU", 1), ("GRU", 2), ("LSTM", 2)])
def test_plans_without_skip_connections_do_not_see_the_switch(dev, rnn_type, n_rnn, temperature, monkeypatch):
    B, T = 5, 3
    feats = SC.features(T, B, 99).float().numpy()
    c, p = _params(rnn_type, n_rnn, skip=False)
    outs = []
    with _skip_model(dev, p, **_cfg(rnn_type, n_rnn, skip=False)) as tt:
        for on in (False, True):
            _env(monkeypatch, on=on)
            with _plan(tt, B, T, 1, temperature=temperature, seed=80) as gen:
                assert not gen.skip and 'big_skip_sum' not in gen.ws
                outs.append(_samples(gen, feats))
    assert np.array_equal(outs[0], outs[1])
    assert temperature == 0.0 or len(np.unique(outs[0][:, 80:])) > 20

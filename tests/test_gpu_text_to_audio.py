"""Text to audio in one stream on the GPU: the staging entry (samplernn_generate_stage_features, sr_stage.hip) against
torch.index_select, DeviceGenerator.generate(gather=) against generate(features) on every generation path,
StreamingGenerator(open_utterances=True) fed in pieces from device tensors against the standalone run in the recorded stream,
StreamingDecoder.run_segments() against run(), TextToAudio end to end, and sample.py --stream_audio 1 against the run
without the flag.  Every equality is bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import samplernn_ref as S
from tests import decode_forced_cases as FC
from tests import samplernn_groups_cases as GC
from tests import samplernn_packed_cases as PC
from tests import samplernn_sampling_cases as SC
from tests.test_gpu_decode_forced import OFF
from tests.test_gpu_decode_row_controls import ROOT, _env, _model as _decoder
from tests.test_gpu_decode_segments import STREAM
from tests.test_gpu_samplernn_groups import _model, _plan
from tests.test_gpu_samplernn_packed import _equal_pieces, _standalone
from tests.test_gpu_samplernn_utt_draws import _standalone as _standalone_drawn

pytestmark = pytest.mark.gpu

SWITCH = "PARROT_SR_PERSIST_GROUPS"
BADARG = 10001   # PARROT_ERR_BADARG
SENTINEL = -7.5


def _vocoder_params():
    return S.init_params(S.config(DIM=GC.DIM, EMB_SIZE=GC.EMB), seed=GC.GRU_SEEDS[0], perturb=0.25)


# ---- 1. the staging entry ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 5, 33])
def test_stage_features_against_index_select(dev, B, monkeypatch):
    from parrot_amd import _lib
    from parrot_amd import ops as hip
    stage = _lib.load().samplernn_generate_stage_features
    T, R = 5, 11
    monkeypatch.delenv(SWITCH, raising=False)
    g = torch.Generator().manual_seed(3 + B)
    with _model(dev, _vocoder_params()) as tt:
        gen = tt.DeviceGenerator(B, T, temperature=0.0)
        try:
            feats = gen.ws['features']
            for ld in (63, 64):
                src = torch.randn(R, ld, generator=g).to(dev)
                pad = torch.cat([src[:, :63], torch.zeros(1, 63, device=dev)])       # row R: what an idle slot reads
                for first, rows in ((0, 1), (1, 1), (0, T - 1), (1, T - 1)):
                    idx = torch.randint(0, R, (rows, B), generator=g, dtype=torch.int32)
                    flat = idx.view(-1)
                    flat[0::4], flat[1::7], flat[2::5] = -1, R, R + 7                 # idle, one past the end, far past
                    flat[-1] = R - 1
                    if B == 1 and rows == 1:
                        flat[0] = -1
                    want = torch.full((T, B, 63), SENTINEL, device=dev)
                    sel = torch.where((idx >= 0) & (idx < R), idx, torch.full_like(idx, R)).long().to(dev)
                    want[first:first + rows] = pad.index_select(0, sel.view(-1)).view(rows, B, 63)
                    feats.fill_(SENTINEL)
                    d_idx = idx.to(dev)
                    assert stage(gen.plan, src.data_ptr(), R, ld, d_idx.data_ptr(), first, rows, hip._stream()) == 0
                    torch.cuda.synchronize()
                    assert torch.equal(feats, want), f"B {B} ld {ld} first {first} rows {rows}"
            # a decoder's frame rows: a [R, 63] view of rows 64 floats apart, and R = 1
            wide = torch.randn(R, 64, generator=g).to(dev)
            idx = torch.zeros(T, B, dtype=torch.int32, device=dev)
            assert stage(gen.plan, wide[R - 1:, :63].data_ptr(), 1, 64, idx.data_ptr(), 0, T, hip._stream()) == 0
            torch.cuda.synchronize()
            assert torch.equal(feats, wide[R - 1, :63].expand(T, B, 63))
            feats.fill_(SENTINEL)
            src, ok = wide.data_ptr(), idx.data_ptr()
            for args in ((None, src, R, 64, ok, 0, 1), (gen.plan, None, R, 64, ok, 0, 1), (gen.plan, src, R, 64, None, 0, 1),
                         (gen.plan, src, R, 64, ok, -1, 1), (gen.plan, src, R, 64, ok, 0, 0), (gen.plan, src, R, 64, ok, 0, -1),
                         (gen.plan, src, R, 64, ok, 1, T), (gen.plan, src, R, 64, ok, T, 1), (gen.plan, src, R, 62, ok, 0, 1),
                         (gen.plan, src, 0, 64, ok, 0, 1), (gen.plan, src, -3, 64, ok, 0, 1)):
                assert stage(*args, hip._stream()) == BADARG, args
            torch.cuda.synchronize()
            assert bool((feats == SENTINEL).all()), "a refused call wrote"
        finally:
            gen.close()


# ---- 2. generate(gather=) == generate(features) ---------------------------------------------------------------------------------
def _gathered(feats, dev, ld, seed):
    """(src [R, ld] on the device, index [N, B]) that spell feats [N, B, 63]: its rows shuffled into a wider store, streams
    past the utterances' ends idle (-1 where the row is all zero would be as good: here every row is indexed)."""
    N, B = feats.shape[:2]
    perm = np.random.RandomState(seed).permutation(N * B + 3)[:N * B]
    src = torch.full((N * B + 3, ld), 9.0)
    src[torch.from_numpy(perm), :63] = torch.from_numpy(feats.reshape(N * B, 63))
    return src.to(dev), perm.reshape(N, B).astype(np.int32)


def _both_ways(tt, feats, dev, groups, lens, ld):
    """((samples, logits) from features, the same from gather) of the run of feats in one piece (lens None) or in segments."""
    N, B = feats.shape[:2]
    src, index = _gathered(feats, dev, ld, N + B)
    out = []
    for use_gather in (False, True):
        give = (lambda lo, hi: dict(gather=(src, index[lo:hi]))) if use_gather else (lambda lo, hi: dict(features=feats[lo:hi]))
        with _plan(tt, B, N if lens is None else max(lens) + 1, groups, temperature=0.0) as gen:
            if lens is None:
                parts = [gen.generate(**give(0, N)).cpu().numpy().copy()]
            else:
                parts = [gen.generate(n_frames=lens[0], **give(0, lens[0] + 1)).cpu().numpy()]
                done = lens[0] + 1
                for k in lens[1:]:
                    parts.append(gen.generate(resume=True, n_frames=k, **give(done, done + k)).cpu().numpy())
                    done += k
            out.append((np.concatenate(parts, axis=1), gen.ws['logits'].detach().cpu().numpy().copy()))
    return out


@pytest.mark.parametrize("case", ["persistent", "segments", "row_groups", "launches"])
def test_generate_gather_equals_features(dev, case, monkeypatch):
    p, feats, _, _ = GC.gru_reference()
    feats = np.asarray(feats, dtype=np.float32)
    monkeypatch.delenv(SWITCH, raising=False)
    B, N, groups, lens, cfg, ld = 5, 10, 1, None, {}, 64
    if case == "segments":
        lens, ld = [3, 3, 3], 63
    if case == "row_groups":
        monkeypatch.setenv(SWITCH, "2")
        B, groups = 37, 2
    if case == "launches":
        p = S.init_params(S.config(DIM=32, EMB_SIZE=8), seed=GC.GRU_SEEDS[0], perturb=0.25)
        B, N, groups, cfg, ld = 3, 4, 0, dict(DIM=32, EMB_SIZE=8), 63
    with _model(dev, p, **cfg) as tt:
        a, b = _both_ways(tt, np.ascontiguousarray(feats[:N, :B]), dev, groups, lens, ld)
    assert a[0].shape == (B, 80 * N) and (a[0][:, :80] == 128).all() and len(np.unique(a[0])) > 4
    assert np.array_equal(a[0], b[0]), f"{case}: {(a[0] != b[0]).sum()} samples differ"
    assert np.array_equal(a[1], b[1]), f"{case}: the last step's logits differ"


# ---- 3. open utterances fed from device tensors ---------------------------------------------------------------------------------
LENGTHS = [5, 12, 3, 7, 9, 4, 6]     # 7 utterances of 3 .. 12 frames on 5 streams, segments of 4


def _feed_in_pieces(sg, utts, dev, per_step, **draws):
    """Opens everything, then before every step feeds each unfinished utterance its next per_step[i] frames as a device
    tensor (row stride 64 for even i, 63 for odd i); returns (pieces, starved steps)."""
    n = len(utts)
    wide = [torch.cat([torch.from_numpy(u), torch.full((u.shape[0], 1), 3.0)], dim=1).to(dev) for u in utts]
    dense = [torch.from_numpy(u).to(dev) for u in utts]
    for i in range(n):
        assert sg.open(**{k: v[i] for k, v in draws.items()}) == i
    fed, chunks, done, starved, steps = [0] * n, [[] for _ in utts], [], 0, 0
    while not sg.idle():
        for i in range(n):
            k = min(per_step[i], utts[i].shape[0] - fed[i])
            if k and (steps % 3 != 2 or i % 2):            # every third step the even utterances get nothing
                frames = (wide[i][:, :63] if i % 2 == 0 else dense[i])[fed[i]:fed[i] + k]
                assert frames.stride(0) == (64 if i % 2 == 0 else 63)
                fed[i] += k
                sg.feed(i, frames, last=fed[i] == utts[i].shape[0])
        out = sg.step()
        starved += sg.starved is not None
        for i, chunk, d in out:
            assert i not in done and chunk.dtype == np.int32
            chunks[i].append(chunk)
            if d:
                done.append(i)
        steps += 1
        assert steps < 200
    assert sorted(done) == list(range(n))
    return [np.concatenate(c) for c in chunks], starved


@pytest.mark.parametrize("drawn", [False, True], ids=["greedy", "drawn"])
def test_open_utterances_equal_standalone(dev, drawn, monkeypatch):
    B, Sv = 5, 4
    p = _vocoder_params()
    feats = SC.features(max(LENGTHS), len(LENGTHS), GC.GRU_SEEDS[1]).numpy().astype(np.float32)
    utts = [feats[:n, i].copy() for i, n in enumerate(LENGTHS)]
    seeds, temps = [1000 + 17 * i for i in range(len(utts))], [1.0] * len(utts)
    monkeypatch.delenv(SWITCH, raising=False)
    with _model(dev, p) as tt:
        sg = tt.StreamingGenerator(B, Sv, temperature=1.0 if drawn else 0.0, utterance_draws=drawn, open_utterances=True,
                                   max_frames=16, store_utterances=len(utts))
        try:
            assert sg.gen.persistent
            pieces, starved = _feed_in_pieces(sg, utts, dev, [2, 3, 1, 2, 3, 4, 2], **(dict(seed=seeds) if drawn else {}))
            record = dict(sg.record)
        finally:
            sg.close()
        assert starved >= 1, "no step was starved: the rule is not exercised"
        stream, slot = [record[i][0] for i in range(len(utts))], [record[i][1] for i in range(len(utts))]
        assert any(s > 1 for s in slot), "no utterance was admitted into a freed stream"
        if drawn:
            items = list(enumerate(stream))
            want = _standalone_drawn(tt, B, 1, items, utts, seeds, temps, max(LENGTHS))
            want = [want[i] for i in range(len(utts))]
        else:
            own = PC.Packing(LENGTHS, tuple(stream), tuple(slot), max(s + n for s, n in zip(slot, LENGTHS)), B, min(LENGTHS),
                             max(LENGTHS))
            want = _standalone(tt, own, utts, 1)
    for piece, u in zip(pieces, utts):
        assert piece.shape == (80 * u.shape[0],) and (piece[:80] == 128).all()
    _equal_pieces(pieces, want, "open utterances, " + ("drawn" if drawn else "greedy"))
    if drawn:
        assert len(np.unique(np.concatenate(pieces))) > 20


# ---- 4. StreamingDecoder.run_segments() == run() --------------------------------------------------------------------------------
def _stream_model(dev, cost='MSE'):
    from oracle import parrot_ref as R
    full = dict(FC.SMALL, cell_type='gru', num_layers=2, weak_feedback=True, which_cost=cost)
    cfg = R.default_config(**full)
    p = R.init_params(cfg, seed=7, scale_by_fan_in=True)
    p['/parrot/h1_to_att/fork_kappa.b'].fill_(STREAM['kappa_bias'])
    m = _decoder(dev, dict(full=full, p=p), encoder_literal=False)
    g = torch.Generator().manual_seed(11)
    texts = [torch.randint(0, cfg['num_characters'], (n,), generator=g) for n in STREAM['texts']]
    return m, cfg, texts


@pytest.mark.parametrize("env, path", [({}, 'machine'), (OFF, 'launches')], ids=["gru2-machine", "gru2-launches"])
def test_run_segments_equal_run(dev, monkeypatch, env, path):
    from parrot_amd.decode import StreamingDecoder
    _env(monkeypatch, env)
    q = STREAM
    m, cfg, texts = _stream_model(dev)
    sd = StreamingDecoder(m, q['slots'], q['F'], q['U'], q['T'], extra=q['extra'])
    ids = [sd.submit(t) for t in texts]
    whole = {uid: (fr.clone(), ph.clone()) for uid, fr, ph in sd.run()}
    assert sorted(whole) == ids and m.decode_path == path
    sd2 = StreamingDecoder(m, q['slots'], q['F'], q['U'], q['T'], extra=q['extra'])
    assert [sd2.submit(t) for t in texts] == ids
    parts, finished = {}, []
    for uid, t0, frames, phi, done in sd2.run_segments(with_phi=True):
        assert uid not in finished and t0 == sum(f.shape[0] for f, _ in parts.get(uid, []))
        assert frames.shape[0] == phi.shape[0] and (done or frames.shape[0] == q['F'])
        parts.setdefault(uid, []).append((frames.clone(), phi.clone()))
        if done:
            finished.append(uid)
    assert sorted(finished) == ids and sd2.placements == sd.placements
    for uid in ids:
        fr, ph = torch.cat([f for f, _ in parts[uid]]), torch.cat([p_ for _, p_ in parts[uid]])
        assert torch.equal(fr, whole[uid][0]) and torch.equal(ph, whole[uid][1]), f"utterance {uid}"
    sd3 = StreamingDecoder(m, q['slots'], q['F'], q['U'], q['T'], extra=q['extra'])
    sd3.submit(texts[0])
    assert [len(item) for item in sd3.run_segments()][0] == 4
    assert min(w[0].shape[0] for w in whole.values()) < q['T'], "no utterance ends before the cap"
    m.close()


# ---- 5. TextToAudio end to end -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("drawn", [False, True], ids=["greedy", "drawn"])
def test_text_to_audio(dev, drawn, monkeypatch):
    """7 texts through 5 decoder slots (segments of 4) and 4 vocoder streams (segments of 2): every utterance's samples are
    the standalone vocoder run, in vocoder.record's stream, of the frames decode_segments gives it in decoder.placements'
    slot; the first audio is out while the decoder still has utterances in flight."""
    from parrot_amd.decode import TextToAudio
    _env(monkeypatch, {})
    monkeypatch.delenv(SWITCH, raising=False)
    q = STREAM
    N, U, T, Fq, extra, Bv = q['slots'], q['U'], q['T'], q['F'], q['extra'], 4
    m, cfg, texts = _stream_model(dev)
    assert cfg['output_dim'] == 63 and cfg['rnn_h_dim'] == 64
    seeds, temps = [500 + 3 * i for i in range(len(texts))], [1.0] * len(texts)
    with _model(dev, _vocoder_params()) as tt:
        tta = TextToAudio(m, N, Fq, U, T, Bv, 2, extra=extra, temperature=1.0 if drawn else 0.0, utterance_draws=drawn)
        try:
            assert tta.vocoder.gen.persistent and tta.vocoder.free_rows == N + Bv
            ids = [tta.submit(t, **(dict(seed=seeds[i]) if drawn else {})) for i, t in enumerate(texts)]
            assert ids == list(range(len(texts)))
            chunks, finished, in_flight_at_first_audio = {}, [], None
            for uid, chunk, done in tta.run():
                assert uid not in finished and chunk.dtype == np.int32 and chunk.size % 80 == 0
                if in_flight_at_first_audio is None and tta.first_audio_s is not None:
                    in_flight_at_first_audio = tta.decoder.busy
                chunks.setdefault(uid, []).append(chunk)
                if done:
                    finished.append(uid)
            assert sorted(finished) == ids and tta.first_audio_s > 0
            assert in_flight_at_first_audio, "the first audio came only after the decoder had finished its last utterance"
            placements, record = dict(tta.decoder.placements), {i: tta.vocoder.record[tta.tickets[i]] for i in ids}
            assert tta.vocoder.free_rows == N + Bv and not tta.decoder.busy and tta.vocoder.idle()
        finally:
            tta.close()
        assert any(seg > 0 for _, seg in placements.values()), "no text was admitted into a freed decoder slot"
        assert any(slot > 1 for _, slot in record.values()), "no utterance was admitted into a freed vocoder stream"
        # the frames decode_segments gives every utterance alone in its slot, cut by the end-of-utterance rule
        utts = []
        for i, text in enumerate(texts):
            slot, _ = placements[i]
            lab, lm = torch.zeros(N, U, dtype=torch.long), torch.zeros(N, U)
            lm[:, 0] = 1.
            lab[slot, :len(text)], lm[slot, :len(text)] = text, 1.
            run = m.decode_segments(lab, lm, None, N, T, Fq, forced_frames=torch.zeros(1, N, 63), n_forced=[0] * N, extra=extra)
            frames = torch.cat([o[0] for _, o in run])[:, slot]
            utts.append(frames[:int(run.lengths[slot])].cpu().numpy().copy())
        pieces = [np.concatenate(chunks[i]) for i in ids]
        for piece, u in zip(pieces, utts):
            assert piece.shape == (80 * u.shape[0],) and (piece[:80] == 128).all()
        stream = [record[i][0] for i in ids]
        if drawn:
            want = _standalone_drawn(tt, Bv, 1, list(enumerate(stream)), utts, seeds, temps, max(u.shape[0] for u in utts))
            want = [want[i] for i in ids]
        else:
            lengths = [u.shape[0] for u in utts]
            slot = [record[i][1] for i in ids]
            own = PC.Packing(lengths, tuple(stream), tuple(slot), max(s + n for s, n in zip(slot, lengths)), Bv, min(lengths),
                             max(lengths))
            want = _standalone(tt, own, utts, 1)
    assert min(u.shape[0] for u in utts) < T, "no utterance ends before the cap"
    _equal_pieces(pieces, want, "text to audio, " + ("drawn" if drawn else "greedy"))
    m.close()


# ---- 6. sample.py --stream_audio 1 ----------------------------------------------------------------------------------------------
def test_sample_py_stream_audio(dev, tmp_path, monkeypatch):
    """The wav files and the feature files of the run without the flag, byte for byte (--utterance_seed: an utterance's draws
    do not depend on where it ran); an experiment without --raw_output is refused."""
    monkeypatch.setenv("RESULTS_DIR", str(tmp_path))
    _env(monkeypatch, {})
    sys.path.insert(0, ROOT)
    import importlib
    from parrot_amd.sampleRNN import lib
    from parrot_amd.sampleRNN.models.conditional import three_tier as tt
    train = importlib.import_module("train")
    sample = importlib.import_module("sample")
    lib.delete_all_params()
    lib.set_device(dev)
    tt.configure(DIM=32, EMB_SIZE=8)
    try:
        for name, raw in (("raw", ["--raw_output", "1"]), ("plain", [])):
            train.main(["--experiment_name", name, "--rnn_h_dim", "64", "--readouts_dim", "64", "--batch_size", "2",
                        "--seq_size", "20", "--num_layers", "1", "--labels_type", "text", "--synthetic_examples", "4",
                        "--save_every", "3", "--max_steps", "3", "--save_dir", str(tmp_path), "--lr_schedule", "1"] + raw)
        N = 3
        base = ["--experiment_name", "raw", "--num_samples", str(N), "--num_steps", "12", "--save_dir", str(tmp_path),
                "--segment_frames", "4", "--stream_frames", "2", "--pack_streams", "2", "--utterance_seed", "5",
                "--timing_coeffs", "1,1.25,0.8"]
        out = os.path.join(str(tmp_path), "vctk", "samples")
        names = ["new_raw/sample_best_sample_%d.wav" % i for i in range(N)] + ["best_sample_%d.npy" % i for i in range(N)]
        read = lambda: [open(os.path.join(out, n), "rb").read() for n in names]
        gen_x, lengths = sample.main(base)
        want = read()
        for n in names:
            os.remove(os.path.join(out, n))
        got_x, got_lengths = sample.main(base + ["--stream_audio", "1"])
        assert got_lengths == lengths and np.array_equal(got_x, gen_x)
        for n, a, b in zip(names, read(), want):
            assert a == b, n + " differs"
        with pytest.raises(SystemExit, match="raw_output"):
            sample.main(["--experiment_name", "plain", "--num_samples", "2", "--num_steps", "12", "--save_dir", str(tmp_path),
                         "--segment_frames", "4", "--stream_frames", "2", "--stream_audio", "1"])
    finally:
        lib.delete_all_params()
        tt.configure(DIM=1024, EMB_SIZE=256)

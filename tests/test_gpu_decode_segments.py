"""Resumable decoding on the GPU (Parrot.sample_model*(state=, return_state=), decode_segments, StreamingDecoder;
parrot_sample_save_state / _load_state, decode_state.hip): the one-piece carry call and its state against the fp64 carry
oracle on every decode program and on the launches; segments chained over both cuttings bit-identical to the one-piece
call; the carry call bit-identical to the plain call wherever the program is the same; state round trip, row independence,
a prompt across a cut, replay without stale state, continuous admission, sample.py --segment_frames.  The cases and their
premise: tests/decode_segment_cases.py, tests/test_decode_segments_cpu.py."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import decode_forced_cases as FC
from tests import decode_segment_cases as SC
from tests.test_gpu_decode_forced import GMM_ON, IDS, OFF, RUNS
from tests.test_gpu_decode_row_controls import TOL, _abort_word, _env, _experiment, _model
from tests.util import assert_close, rel_err

pytestmark = pytest.mark.gpu

BF16 = ('lstm2_mse_n5', {'decode_dtype': 'bf16'}, 'machine')   # (model keyword, not a switch: see _case_model)
runs = pytest.mark.parametrize("name, env, path", RUNS, ids=IDS)
runs_bf16 = pytest.mark.parametrize("name, env, path", RUNS + [BF16], ids=IDS + ['lstm2_mse_n5-bf16-machine'])
S, CUTS, F = SC.S, SC.CUTS, SC.SEGMENT


def _case_model(dev, monkeypatch, name, env, params=None):
    bf16 = env.get('decode_dtype') == 'bf16'
    _env(monkeypatch, {} if bf16 else env)
    c = dict(FC.case(name))
    if bf16:  # (f32-representable: model and rounded oracle round the same weights)
        c['p'] = {k: v.float().double() for k, v in c['p'].items()}
    if params is not None:
        c['p'] = params
    return c, _model(dev, c, **({'decode_dtype': 'bf16'} if bf16 else {}))


def _args(c, t0, t1, forced, pad=0):
    """Keywords of the call that decodes frames t0 .. t1 - 1 (pad: further frames on zeros, the segments' overshoot)."""
    z = lambda a: torch.cat([a[t0:t1].float(), torch.zeros((pad,) + tuple(a.shape[1:]))]) if pad else a[t0:t1].float()
    kw = dict(unif=z(c['unif']), noise=z(c['noise']))
    if forced:
        kw.update(forced_frames=c['forced'][t0:t1].float(), n_forced=[min(max(n - t0, 0), t1 - t0) for n in c['n']])
    return kw


def _call(m, c, t0, t1, forced, state=None, pad=0, **kw):
    outs, st = m.sample_model_device(c['lab'], c['lm'].float(), c['spk'], c['N'], t1 - t0 + pad, state=state, return_state=True,
                                     **dict(_args(c, t0, t1, forced, pad), **kw))
    assert len(outs) == (7 if forced else 6)
    return [o.clone() for o in outs], st


def _healthy(m, path):
    from parrot_amd import _lib
    assert m.decode_path == path
    for key, ws in m._sample_ws.items():
        assert (_lib.load().parrot_sample_is_persistent(ws['plan']) != 0) == (path == 'machine'), key
        if path == 'machine':
            assert _abort_word(ws) == 0, "a spin timed out inside the machine"
        assert _lib.load().parrot_sample_status(ws['plan']) == 0


def _same(a, b, tag):
    assert len(a) == len(b), tag
    for x, y, n in zip(a, b, SC.NAMES):
        assert x.shape == y.shape and torch.equal(x, y), f"{tag}: {n} differs"


_ONE = {}  # (case, switches, forced) -> (outputs, state tensor, frames_done) of the one-piece carry call, on the CPU


def _one_piece(dev, monkeypatch, name, env, path, forced):
    key = (name, tuple(sorted(env.items())), forced)
    if key not in _ONE:
        c, m = _case_model(dev, monkeypatch, name, env)
        outs, st = _call(m, c, 0, S, forced)
        _healthy(m, path)
        assert list(m._sample_ws) == [('carry',) + (('forced',) if forced else ()) + (S, c['N'], c['U'])]
        m.close()
        _ONE[key] = ([o.cpu() for o in outs], st.tensor.cpu(), st.frames_done.tolist())
    return _ONE[key]


# ------------------------------------------------------------------------------------------------ 1. oracle parity
@runs_bf16
def test_one_piece_carry_call_matches_the_oracle(dev, monkeypatch, name, env, path):
    """The six (forced: seven) outputs and the returned state within 2e-4 of the float64 carry oracle and its packed carry.
    bf16 operands: free run only (no kernels with forcing), against the oracle with rounded operands at the 2e-3 that
    tests/test_gpu_decode_bf16.py holds its trajectories to."""
    c = FC.case(name)
    if env.get('decode_dtype') == 'bf16':
        from tests.test_gpu_decode_bf16 import rounded_oracle
        p = {k: v.float().double() for k, v in c['p'].items()}
        with torch.no_grad(), rounded_oracle():
            ref, carry = SC.carry_loop(p, c['cfg'], c['lab'], c['lm'], c['spk'], S, unif=c['unif'], noise=c['noise'])
        todo = [(False, ref, SC.pack(carry, c['cfg']), 2e-3)]
    else:
        todo = [(forced,) + tuple(SC.one_piece(name, forced)[i] for i in (0, 2)) + (TOL,) for forced in (False, True)]
    for forced, ref, packed, tol in todo:
        outs, state, done = _one_piece(dev, monkeypatch, name, env, path, forced)
        tag = f"{name} {env} {path} {'forced' if forced else 'free'}"
        for o, r, n in zip(outs, ref, SC.NAMES):
            print(f"{tag}: {n} {rel_err(o, r):.3e}")
        print(f"{tag}: state {rel_err(state, packed):.3e}")
        for o, r, n in zip(outs, ref, SC.NAMES):
            assert_close(o, r, tol, f"{tag}: {n}")
        assert state.shape == packed.shape and done == [S] * c['N']
        assert_close(state, packed, tol, f"{tag}: state")
        assert torch.equal(state[:, :c['cfg']['output_dim']], outs[0][-1]), "the state's x is the last fed-back frame"
        assert torch.equal(state[:, 64:64 + outs[1].shape[2]], outs[1][-1]), "the state's kappa is the last step's"


# ------------------------------------------------------------------------------------------------ 2. cuts
@runs_bf16
def test_chained_calls_are_the_one_piece_call(dev, monkeypatch, name, env, path):
    """sample_model_device chained through its state over [1, 4, 10] -- a one-frame call, an odd and an even one, so the
    launches end on either ping-pong slot: every output and the final state bit-identical to the one-piece carry call."""
    for forced in ((False,) if env.get('decode_dtype') == 'bf16' else (False, True)):
        ref, ref_state, _ = _one_piece(dev, monkeypatch, name, env, path, forced)
        c, m = _case_model(dev, monkeypatch, name, env)
        st, parts, t0 = None, [], 0
        for t1 in CUTS:
            outs, st = _call(m, c, t0, t1, forced, state=st)
            parts.append(outs)
            t0 = t1
        _healthy(m, path)
        m.close()
        _same([torch.cat(v).cpu() for v in zip(*parts)], ref, f"cuts {CUTS} forced={forced}")
        assert torch.equal(st.tensor.cpu(), ref_state) and st.frames_done.tolist() == [S] * c['N']


@runs_bf16
def test_decode_segments_is_the_one_piece_call(dev, monkeypatch, name, env, path):
    """decode_segments with 4 frames per segment: 4, 4 and a last segment that runs whole and is cut to 2.  Every output
    bit-identical to the one-piece carry call; the state is the one after the 12 frames run: bit-identical to a one-piece
    call of 12 frames whose last two run on zeros, whose first 10 frames are the 10-frame call's again."""
    for forced in ((False,) if env.get('decode_dtype') == 'bf16' else (False, True)):
        ref, _, _ = _one_piece(dev, monkeypatch, name, env, path, forced)
        c, m = _case_model(dev, monkeypatch, name, env)
        kw = _args(c, 0, S, forced)
        run = m.decode_segments(c['lab'], c['lm'].float(), c['spk'], c['N'], S, F, **kw)
        got = list(run)
        assert [t0 for t0, _ in got] == [0, 4, 8] and [o[0].shape[0] for _, o in got] == [4, 4, 2]
        assert list(m._sample_ws) == [('carry',) + (('forced',) if forced else ()) + (F, c['N'], c['U'])]
        _healthy(m, path)
        _same([torch.cat(v).cpu() for v in zip(*[o for _, o in got])], ref, f"segments of {F} forced={forced}")
        assert run.state.frames_done.tolist() == [12] * c['N'] and run.frames == S
        long, st12 = _call(m, c, 0, S, forced, pad=2)
        _same([o[:S].cpu() for o in long], ref, "the first 10 of 12 frames")
        assert torch.equal(run.state.tensor, st12.tensor), "the state after the overshoot"
        m.close()


# ------------------------------------------------------------------------------------------------ 3. the plain call
@runs_bf16
def test_carry_call_is_the_plain_call_where_the_program_is_the_same(dev, monkeypatch, name, env, path):
    """The one-piece carry call against sample_model_device without state arguments: bit-identical wherever the plain call's
    program keeps the fed-back frame on the chain (LSTM, GMM, launches, whole-K, one layer).  Where it composes the feedback
    (parrot_sample_is_persistent = 3: GRU stacks of two or three layers with an MSE head, cut along K) the carry call is
    bit-identical to the plain call under PARROT_PM_FBC=0, and within 2e-4 of -- not equal to -- the default plain call."""
    from parrot_amd import _lib
    ref, _, _ = _one_piece(dev, monkeypatch, name, env, path, False)

    def plain(switches):
        c, m = _case_model(dev, monkeypatch, name, switches)
        outs = m.sample_model_device(c['lab'], c['lm'].float(), c['spk'], c['N'], S, **_args(c, 0, S, False))
        outs = [o.clone().cpu() for o in outs]
        assert list(m._sample_ws) == [(S, c['N'], c['U'])]
        _healthy(m, path)
        program = _lib.load().parrot_sample_is_persistent(m._sample_ws[(S, c['N'], c['U'])]['plan'])
        m.close()
        return outs, program

    default, program = plain(env)
    if name == 'gru2_mse_n5' and not env:
        assert program == 3, "the default program of the two-layer GRU composes the feedback: else this test shows nothing"
    if program != 3:
        _same(default, ref, "plain call vs carry call")
        return
    assert not torch.equal(default[0], ref[0])
    for o, r, n in zip(default, ref, SC.NAMES):
        assert_close(o, r, TOL, f"default plain call vs carry call: {n}")
    on_chain, program = plain(dict(env, PARROT_PM_FBC="0"))
    assert program == 2
    _same(on_chain, ref, "plain call under PARROT_PM_FBC=0 vs carry call")


# ------------------------------------------------------------------------------------------------ 4. round trip
@runs_bf16
def test_save_load_save_returns_the_same_bits(dev, monkeypatch, name, env, path):
    """A state loaded into a fresh plan and saved again, no run between: the same bits -- gather and scatter agree on every
    piece's place.  A plan that has neither run nor been loaded has no state (BADARG); NULL arguments are refused."""
    from parrot_amd import _lib, ops
    lib = _lib.load()
    _, ref_state, _ = _one_piece(dev, monkeypatch, name, env, path, False)
    c, m = _case_model(dev, monkeypatch, name, env)
    ws = m._sample_workspace(S, c['N'], c['U'], carry=True)
    state = ref_state.to(dev)
    back = torch.full_like(state, float('nan'))
    assert lib.parrot_sample_save_state(ws['plan'], back.data_ptr(), ops._stream()) == 10001
    assert lib.parrot_sample_load_state(ws['plan'], None, ops._stream()) == 10001
    assert lib.parrot_sample_save_state(ws['plan'], None, ops._stream()) == 10001
    assert lib.parrot_sample_load_state(ws['plan'], state.data_ptr(), ops._stream()) == 0
    assert lib.parrot_sample_save_state(ws['plan'], back.data_ptr(), ops._stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(back, state)
    assert lib.parrot_sample_state_floats(C.byref(ws['desc'].base if hasattr(ws['desc'], 'base') else ws['desc'])) == state.shape[1]
    m.close()


def test_save_state_refuses_a_plan_that_stops_early(dev, monkeypatch):
    from parrot_amd import _lib, ops
    c, m = _case_model(dev, monkeypatch, 'gru2_mse_n5', {})
    m.sample_until_end_device(c['lab'], c['lm'].float(), c['spk'], c['N'], S, extra=8)
    ws = m._sample_ws[('stop', S, c['N'], c['U'], 8)]
    buf = torch.zeros(c['N'], m.decode_state_floats(), device=dev)
    assert _lib.load().parrot_sample_save_state(ws['plan'], buf.data_ptr(), ops._stream()) == 10002
    m.close()


# ------------------------------------------------------------------------------------------------ 5. rows are independent
@runs_bf16
def test_perturbing_one_row_of_a_state_changes_that_row_only(dev, monkeypatch, name, env, path):
    """Ten more frames from the one-piece call's state, and from the same state with row 2's first layer moved by 0.01:
    every other row of every output and of the new state bit-identical, row 2 not."""
    from parrot_amd.decode import DecodeState
    _, ref_state, done = _one_piece(dev, monkeypatch, name, env, path, False)
    c, m = _case_model(dev, monkeypatch, name, env)
    base = DecodeState(m, ref_state.to(dev), done)
    moved = base.clone()
    moved.h[0][2] += 0.01
    a, sa = _call(m, c, 0, S, False, state=base)
    b, sb = _call(m, c, 0, S, False, state=moved)
    _healthy(m, path)
    m.close()
    assert sa.frames_done.tolist() == [2 * S] * c['N']
    others = [i for i in range(c['N']) if i != 2]
    for x, y, n in zip(a + [sa.tensor.unsqueeze(0)], b + [sb.tensor.unsqueeze(0)], SC.NAMES[:6] + ("state",)):
        assert torch.equal(x[:, others], y[:, others]), f"{n}: another row changed"
        assert not torch.equal(x[:, 2], y[:, 2]), f"{n}: the perturbed row did not change"


# ------------------------------------------------------------------------------------------------ 6. a prompt across a cut
@runs
def test_a_prompt_across_a_cut(dev, monkeypatch, name, env, path):
    """Every row primed with 4 frames, the call cut at 3: the second call gets the fourth frame as its first (n_forced - 3
    = 1).  Bit-identical to the one-piece forced carry call, own_x and the state included."""
    c, m = _case_model(dev, monkeypatch, name, env)
    c['n'] = [4] * c['N']
    ref, ref_state = _call(m, c, 0, S, True)
    first, st = _call(m, c, 0, 3, True)
    second, st = _call(m, c, 3, S, True, state=st)
    _healthy(m, path)
    m.close()
    _same([torch.cat(v) for v in zip(first, second)], ref, "cut at 3")
    assert torch.equal(st.tensor, ref_state.tensor)
    assert torch.equal(ref[0][:4], c['forced'][:4].float().to(dev)) and not torch.equal(ref[0][4], c['forced'][4].float().to(dev))


# ------------------------------------------------------------------------------------------------ 7. replay
@runs
def test_replay_carries_no_stale_state(dev, monkeypatch, name, env, path):
    """Two different runs on one workspace -- set A from the initial state, then set B entering through the state A left --
    and the second alone on a fresh model: bit-identical, outputs and state."""
    from parrot_amd.decode import DecodeState
    cB = FC.case(name, 'B')
    c, m = _case_model(dev, monkeypatch, name, env)
    _, stA = _call(m, c, 0, S, True)
    entering = stA.clone()
    second, st2 = _call(m, dict(c, forced=cB['forced'], n=cB['n']), 0, S, True, state=stA)
    assert len(m._sample_ws) == 1 and torch.equal(stA.tensor, entering.tensor), "a call must not write the state it enters through"
    _healthy(m, path)
    m.close()
    c, m = _case_model(dev, monkeypatch, name, env)
    alone, st = _call(m, dict(c, forced=cB['forced'], n=cB['n']), 0, S, True, state=DecodeState(m, entering.tensor.clone(), entering.frames_done))
    m.close()
    _same(second, alone, "second run vs itself on a fresh model")
    assert torch.equal(st2.tensor, st.tensor) and not torch.equal(st2.tensor, entering.tensor)


# ------------------------------------------------------------------------------------------------ 8. continuous admission
STREAM = dict(slots=5, U=9, T=48, F=4, extra=8, kappa_bias=-1.0, texts=[7, 5, 8, 3, 6, 7, 4])


@pytest.mark.parametrize("cell, cost, env, path", [('gru', 'MSE', {}, 'machine'), ('lstm', 'GMM', GMM_ON, 'machine'),
                                                   ('gru', 'MSE', OFF, 'launches')], ids=["gru2-machine", "lstm2-k3-machine", "gru2-launches"])
def test_streaming_decoder(dev, monkeypatch, cell, cost, env, path):
    """7 utterances of unequal text length through 5 slots, 4 frames per segment: every utterance's frames and phi equal,
    bit for bit, a decode_segments run with the utterance alone in the same slot of a batch of the same shape, cut at the
    length utils.end_of_utterance gives for that run's full phi; the weights are tiled once."""
    from oracle import parrot_ref as R
    from parrot_amd.decode import StreamingDecoder
    from parrot_amd.utils import end_of_utterance
    _env(monkeypatch, env)
    q = STREAM
    N, U, T, Fq, extra = q['slots'], q['U'], q['T'], q['F'], q['extra']
    full = dict(FC.SMALL, cell_type=cell, num_layers=2, weak_feedback=True, which_cost=cost, **({'k_gmm': 3} if cost == 'GMM' else {}))
    cfg = R.default_config(**full)
    p = R.init_params(cfg, seed=7, scale_by_fan_in=True)
    p['/parrot/h1_to_att/fork_kappa.b'].fill_(q['kappa_bias'])
    m = _model(dev, dict(full=full, p=p), encoder_literal=False)   # (rows that do not see one another: StreamingDecoder insists)
    g = torch.Generator().manual_seed(11)
    texts = [torch.randint(0, cfg['num_characters'], (n,), generator=g) for n in q['texts']]
    rnd = [FC.G.randomness(1, cfg['output_dim'], 20 + i, steps=T) for i in range(len(texts))]
    sd = StreamingDecoder(m, N, Fq, U, T, extra=extra)
    ids = [sd.submit(t, **(dict(unif=rnd[i][0][:, 0], noise=rnd[i][1][:, 0]) if cost == 'GMM' else {})) for i, t in enumerate(texts)]
    done = {uid: (fr.clone(), ph.clone()) for uid, fr, ph in sd.run()}
    assert sorted(done) == ids == list(range(7)) and m.decode_path == path
    assert sd.tilings_run == 1 and sd.setups_run >= 2, "the weights are tiled once; admissions set the batch up again"
    assert any(seg > 0 for _, seg in sd.placements.values()), "no utterance was admitted into a freed slot"
    lengths, checks = {}, []
    for i, text in enumerate(texts):
        slot, _ = sd.placements[i]
        lab, lm = torch.zeros(N, U, dtype=torch.long), torch.zeros(N, U)
        lm[:, 0] = 1.   # the other slots: the one-character dummy
        lab[slot, :len(text)], lm[slot, :len(text)] = text, 1.
        kw = dict(forced_frames=torch.zeros(1, N, cfg['output_dim']), n_forced=[0] * N)
        if cost == 'GMM':
            unif, noise = torch.zeros(T, N), torch.zeros(T, N, cfg['output_dim'])
            unif[:, slot], noise[:, slot] = rnd[i][0][:, 0].float(), rnd[i][1][:, 0].float()
            kw.update(unif=unif, noise=noise)
        segs = [o for _, o in m.decode_segments(lab, lm, None, N, T, Fq, **kw)]
        sx, phi = torch.cat([o[0] for o in segs])[:, slot], torch.cat([o[4] for o in segs])[:, slot]
        lengths[i] = end_of_utterance(phi.cpu().numpy(), min(len(text), U - 1), T, extra)
        fr, ph = done[i]
        k = min(fr.shape[0], lengths[i])
        print(f"utterance {i} slot {slot}: length {fr.shape[0]}, host rule {lengths[i]}; frames equal over the first {k}: "
              f"{torch.equal(fr[:k], sx[:k])}, phi: {torch.equal(ph[:k], phi[:k])}, first 4 frames: {torch.equal(fr[:4], sx[:4])}")
        checks.append((i, slot, fr, ph, sx, phi))
    print(f"lengths {lengths}  placements {sd.placements}")
    for i, slot, fr, ph, sx, phi in checks:
        assert fr.shape[0] == ph.shape[0] == lengths[i], f"utterance {i}: length {fr.shape[0]}, the host rule gives {lengths[i]}"
        assert torch.equal(fr, sx[:lengths[i]]) and torch.equal(ph, phi[:lengths[i]]), f"utterance {i} in slot {slot}"
    assert min(lengths.values()) < T, "no utterance ends before the cap: the rule is not exercised"
    m.close()


# ------------------------------------------------------------------------------------------------ 9. sample.py
def test_sample_py_segment_frames(dev, tmp_path, monkeypatch):
    """--segment_frames 4, with and without --stop_at_end 1, writes the feature files the flagless run writes."""
    _env(monkeypatch, {})
    sample = _experiment(tmp_path, monkeypatch, "segs", [])
    N, Sq = 3, 24
    base = ["--experiment_name", "segs", "--num_samples", str(N), "--num_steps", str(Sq), "--save_dir", str(tmp_path)]
    files = lambda: [np.load(os.path.join(str(tmp_path), 'vctk', 'samples', f'best_sample_{i}.npy')) for i in range(N)]
    plain, plain_len = sample.main(base)
    want = files()
    for extra in ([], ["--stop_at_end", "1"]):
        got, lengths = sample.main(base + ["--segment_frames", "4"] + extra)
        assert lengths == plain_len and got.shape[0] == N and got.shape[1] <= Sq
        assert np.array_equal(got, plain[:, :got.shape[1]])
        for a, b in zip(files(), want):
            assert a.shape == b.shape and np.array_equal(a, b)

"""Continuous admission on one SampleRNN generation plan (three_tier.schedule_segment, StreamingGenerator), as far as it
can be checked without a GPU: the schedule's rules over the packings' length lists and hand-made queues, the chunks a
StreamingGenerator hands out when a fake runs its segments, the argument checks, and the new symbol in header and _lib."""
import os
import re

import numpy as np
import pytest

from tests import samplernn_packed_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tt():
    from parrot_amd.sampleRNN.models.conditional import three_tier as tt
    return tt


def _simulate(lengths, B, S, arrivals=None):
    """Runs schedule_segment until everything is placed.  arrivals[k] = how many utterances have been submitted before
    segment k (default: all of them up front).  Returns per utterance (stream, [absolute slots], absolute start-flag
    slot or None) and the list of segment lengths; checks the per-segment rules on the way."""
    tt = _tt()
    running, queue = [None] * B, []
    submitted, base, seg = 0, 0, 0
    where = {i: (None, [], None) for i in range(len(lengths))}
    seg_lens, order = [], []
    while submitted < len(lengths) or queue or any(r is not None for r in running):
        upto = len(lengths) if arrivals is None else (arrivals[seg] if seg < len(arrivals) else len(lengths))
        queue = queue + [(i, lengths[i]) for i in range(submitted, upto)]
        submitted = max(submitted, upto)
        before = (list(running), list(queue))
        out = tt.schedule_segment(running, queue, B, S)
        assert (list(running), list(queue)) == before, "the arguments were changed"
        assert out == tt.schedule_segment(running, queue, B, S), "not deterministic"
        placements, starts, n, running2, queue2 = out
        used = set()
        busiest = 0
        for ticket, b, slot, frame, count in placements:
            assert 0 <= b < B and 1 <= slot and slot + count - 1 <= S and count >= 1
            for s in range(slot, slot + count):
                assert (b, s) not in used, "two utterances share slot %d of stream %d" % (s, b)
                used.add((b, s))
            busiest = max(busiest, slot + count - 1)
            st, slots, flag = where[ticket]
            assert st in (None, b), "an utterance changed its stream"
            assert frame == len(slots), "frames out of order"
            if frame == 0:
                order.append((base + slot, b, ticket))
            where[ticket] = (b, slots + [base + s for s in range(slot, slot + count)], flag)
        assert n == busiest <= S, "a segment is as long as its busiest stream"
        for b in range(B):        # no hole inside a stream's segment: a stream is used from slot 1 on
            mine = sorted(s for bb, s in used if bb == b)
            assert mine == list(range(1, len(mine) + 1))
        for slot, b in starts:
            assert 1 <= slot <= n
            owner = [t for t, bb, s0, f0, c in placements if bb == b and s0 <= slot < s0 + c]
            assert len(owner) == 1
            st, slots, flag = where[owner[0]]
            assert flag is None
            where[owner[0]] = (st, slots, base + slot)
        for b, r in enumerate(running2):
            if r is not None:     # an unfinished utterance has reached the segment's last slot
                assert (b, n) in used and n == S and 1 <= r[1] < r[2]
        if n == 0:
            assert not placements and not queue2 and all(r is None for r in running2)
            assert arrivals is not None and submitted < len(lengths), "an empty segment with nothing left to come"
        running, queue = running2, queue2
        seg_lens.append(n)
        base += n
        seg += 1
        assert seg < 10000
    # admission is FIFO: by (the slot they begin at, stream) the tickets are in submission order
    assert [t for _, _, t in sorted(order)] == list(range(len(lengths)))
    for i, n in enumerate(lengths):
        b, slots, flag = where[i]
        assert len(slots) == n and slots == list(range(slots[0], slots[0] + n)), "slots are not consecutive"
        assert flag == (slots[1] if n >= 2 else None), "the start flag is on the slot after the first"
    return where, seg_lens


@pytest.mark.parametrize("S", [1, 2, 4, 7])
@pytest.mark.parametrize("case", ["GRU_PACKING", "GROUPS_PACKING", "STACKED_PACKING"])
def test_schedule_over_the_packings(case, S):
    c = getattr(PC, case)
    where, seg_lens = _simulate(list(c.lengths), c.B, S)
    assert sum(seg_lens) >= -(-sum(c.lengths) // c.B)
    n = len(c.lengths)
    _simulate(list(c.lengths), c.B, S, arrivals=[n // 2, n // 2, n])


def test_fifo_within_a_segment():
    """Streams are served in index order, the queue oldest first: with two streams free at once the older utterance takes
    the lower stream; a stream that frees up inside the segment takes the next one."""
    tt = _tt()
    placements, starts, n, running, queue = tt.schedule_segment([None, None], [(0, 2), (1, 5), (2, 3), (3, 1)], 2, 4)
    assert placements == [(0, 0, 1, 0, 2), (2, 0, 3, 0, 2), (1, 1, 1, 0, 4)]
    assert starts == [(2, 0), (4, 0), (2, 1)]
    assert n == 4 and running == [(2, 2, 3), (1, 4, 5)] and queue == [(3, 1)]
    placements, starts, n, running, queue = tt.schedule_segment(running, queue, 2, 4)
    assert placements == [(2, 0, 1, 2, 1), (3, 0, 2, 0, 1), (1, 1, 1, 4, 1)]
    assert starts == [] and n == 2 and running == [None, None] and queue == []


def test_hand_made_queues():
    tt = _tt()
    # empty queue, nothing running: nothing to run
    assert tt.schedule_segment([None] * 3, [], 3, 4) == ([], [], 0, [None] * 3, [])
    # more streams than utterances: the segment is as long as the longest, not S
    placements, starts, n, running, queue = tt.schedule_segment([None] * 4, [(0, 2), (1, 3)], 4, 8)
    assert n == 3 and running == [None] * 4 and starts == [(2, 0), (2, 1)]
    # an utterance longer than several segments
    where, seg_lens = _simulate([11], 2, 3)
    assert seg_lens == [3, 3, 3, 2] and where[0][1] == list(range(1, 12)) and where[0][2] == 2
    # an utterance that ends on the last slot of a segment; the next one's prefix is slot 1 of the next segment
    where, seg_lens = _simulate([4, 3], 1, 4)
    assert seg_lens == [4, 3] and where[1][1] == [5, 6, 7] and where[1][2] == 6
    # a prefix on the last slot of a segment: its start flag is slot 1 of the next one
    placements, starts, n, running, queue = tt.schedule_segment([None], [(0, 3), (1, 3)], 1, 4)
    assert placements == [(0, 0, 1, 0, 3), (1, 0, 4, 0, 1)] and starts == [(2, 0)] and running == [(1, 1, 3)]
    placements, starts, n, running, queue = tt.schedule_segment(running, queue, 1, 4)
    assert placements == [(1, 0, 1, 1, 2)] and starts == [(1, 0)] and n == 2 and running == [None]
    # one-frame utterances one after the other
    _simulate([1, 1, 1, 2, 1], 2, 2)
    rng = np.random.RandomState(4)
    for _ in range(20):
        lengths = [int(x) for x in rng.randint(1, 12, size=rng.randint(1, 30))]
        _simulate(lengths, int(rng.randint(1, 6)), int(rng.randint(1, 6)),
                  arrivals=sorted(int(x) for x in rng.randint(0, len(lengths) + 1, size=4)))


class _Fake:
    """A segment runner whose "samples" say where they were made: stream * 100000 + absolute slot in every sample of a
    slot (absolute = counted over all segments run so far, from 1)."""

    def __init__(self, B):
        self.B, self.base, self.calls = B, 0, []

    def __call__(self, features, starts, resume):
        n = features.shape[0]
        assert features.shape == (n, self.B, 63) and starts.shape == (n, self.B)
        assert resume == (len(self.calls) > 0)
        self.calls.append((features.copy(), starts.copy()))
        out = np.zeros((self.B, 80 * n), dtype=np.int32)
        for b in range(self.B):
            for s in range(n):
                out[b, 80 * s:80 * (s + 1)] = b * 100000 + self.base + s + 1
        self.base += n
        return out


def test_chunks_of_a_fake_runner():
    tt = _tt()
    lengths = list(PC.GRU_PACKING.lengths) + [1, 9]
    rng = np.random.RandomState(7)
    utts = [rng.randn(n, 63).astype(np.float32) for n in lengths]
    fake = _Fake(3)
    sg = tt.StreamingGenerator(3, 4, run_segment=fake)
    assert sg.gen is None and sg.idle() and sg.step() == [] and sg.drain() == []
    got = []
    assert [sg.submit(u) for u in utts[:6]] == list(range(6))
    got += sg.step() + sg.step()
    assert [sg.submit(u) for u in utts[6:]] == list(range(6, len(utts)))
    got += sg.drain()
    sg.close()
    assert sg.idle()
    chunks, done_at = {}, {}
    for k, (ticket, chunk, done) in enumerate(got):
        assert chunk.dtype == np.int32 and ticket not in done_at
        chunks.setdefault(ticket, []).append(chunk)
        if done:
            done_at[ticket] = k
    assert sorted(done_at) == list(range(len(utts)))
    for i, n in enumerate(lengths):
        piece = np.concatenate(chunks[i])
        b, first = sg.record[i]
        assert piece.shape == (80 * n,) and (piece[:80] == 128).all()                     # the prefix is Q/2
        want = np.repeat(b * 100000 + first + np.arange(n), 80)
        assert np.array_equal(piece[80:], want[80:]), "utterance %d got other slots than its own" % i
    # what the runner saw: every utterance's frames at its slots, a start flag on the slot of its frame 1 and nowhere else
    feats = np.concatenate([f for f, _ in fake.calls])
    flags = np.concatenate([s for _, s in fake.calls])
    want_f, want_s = np.zeros_like(feats), np.zeros_like(flags)
    for i, n in enumerate(lengths):
        b, first = sg.record[i]
        want_f[first - 1:first - 1 + n, b] = utts[i]
        if n >= 2:
            want_s[first, b] = 1
    assert np.array_equal(feats, want_f) and np.array_equal(flags, want_s)
    assert all(f.shape[0] <= 4 for f, _ in fake.calls)


def test_argument_checks():
    tt = _tt()
    fake = _Fake(2)
    for bad in (dict(n_streams=0, segment_frames=4), dict(n_streams=2, segment_frames=0), dict(n_streams=-1, segment_frames=1)):
        with pytest.raises(ValueError):
            tt.StreamingGenerator(run_segment=fake, **bad)
    sg = tt.StreamingGenerator(2, 3, run_segment=fake)
    for bad in (np.zeros((0, 63), np.float32), np.zeros((3, 62), np.float32), np.zeros((63,), np.float32)):
        with pytest.raises(ValueError):
            sg.submit(bad)
    assert sg.idle()
    with pytest.raises(ValueError):
        tt.schedule_segment([None], [(0, 0)], 1, 2)
    with pytest.raises(ValueError):
        tt.schedule_segment([None], [], 2, 2)       # one entry per stream
    with pytest.raises(ValueError):
        next(tt.generate_stream(np.zeros((4, 2, 63), np.float32), 0))
    tt.configure(SKIP_CONN=True)
    try:
        with pytest.raises(NotImplementedError):
            tt.StreamingGenerator(2, 3, run_segment=fake)
        with pytest.raises(NotImplementedError):
            next(tt.generate_stream(np.zeros((4, 2, 63), np.float32), 2))
    finally:
        tt.configure(SKIP_CONN=False)


def test_header_and_lib_agree_on_the_new_symbol():
    from parrot_amd import _lib
    import ctypes as C
    res, args = _lib.SIGNATURES["samplernn_generate_run_segment"]
    assert res is C.c_int and args == [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    txt = open(os.path.join(ROOT, "include", "parrot_hip.h")).read()
    assert re.search(r"int samplernn_generate_run_segment\(void\* plan, int n_periods, int resume, void\* stream\);", txt)

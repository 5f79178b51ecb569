"""LSTM stacks on the decode machine (plans_decode.hip, build_persist_lstm): planned and replayed symbolically on the
CPU -- no device memory is touched (parrot_sample_plan_pieces_dry).  A step is L + 2 phases: layer 0, attention, layers
1 .. L-1, composed output; a layer has H / 4 units (16 gate-interleaved columns each)."""
import ctypes as C

import pytest

from parrot_amd import _lib

NWG = 256


def _desc(L=2, H=1024, E=512, B=16, S=1000, R=1024, fb=(0,), speaker=False):
    d = _lib.SampleDesc()
    d.S, d.B, d.H, d.E, d.A, d.U, d.L, d.O, d.R, d.ldx = S, B, H, E, 10, 100, L, 63, R, 64
    d.cell = 1
    fake = 0x7000_0000_0000  # never dereferenced by the dry run
    for l in range(L):
        d.Wg_t[l], d.bg[l] = fake, fake   # Wc_t stays null: an LSTM layer has one product
        if l in fb:
            d.Wfg[l] = fake
        if speaker:
            d.seq_g[l] = fake
    d.Wro_t, d.ro_const, d.x = fake, fake, fake
    return d


def _plan(d, nwg=NWG):
    info = (C.c_int * 16)()
    rc = _lib.load().parrot_sample_plan_pieces_dry(C.byref(d), nwg, info)
    return rc, list(info)


CASES = {
    "configs2_lstm": dict(L=2, H=1024, E=512, R=1024, B=16, S=1000, fb=(0,)),
    "configs2_lstm_b64": dict(L=2, H=1024, E=512, R=1024, B=64, S=1000, fb=(0,)),
    "cfg4_3x1536": dict(L=3, H=1536, E=256, R=1536, B=16, S=1000, fb=(0,)),
    "one_layer_no_feedback": dict(L=1, H=256, E=128, R=256, B=5, S=50, fb=()),
    "full_feedback_speaker": dict(L=3, H=256, E=128, R=256, B=16, S=50, fb=(0, 1, 2), speaker=True),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_lstm_plan_is_legal(name):
    kw = CASES[name]
    L, H, B = kw["L"], kw["H"], kw["B"]
    rc, info = _plan(_desc(**kw))
    assert rc == 0, (rc, info)
    assert info[2] == 0, info                 # symbolic replay: reads satisfied, nothing written twice, every x[t] produced
    n = info[0]
    assert n == L + 2                         # phases per step: L layers, attention, composed output
    assert sum(info[4:4 + n]) == info[3]
    maxu = info[13]                           # units per workgroup and phase the plan was placed with
    assert 1 <= maxu <= 2 and n * maxu <= 12
    assert all(0 < c <= NWG * maxu for c in info[4:4 + n]), info
    # layer phases hold H / 4 tiles, the attention phase one unit per batch row, the output phase four tiles
    assert info[4] == H // 4 and info[5] == B and info[4 + n - 1] == 4
    assert all(c == H // 4 for c in info[6:4 + n - 1])


def test_cfg4_width_needs_two_units_per_workgroup_and_streams():
    rc, info = _plan(_desc(**CASES["cfg4_3x1536"]))
    assert rc == 0 and info[13] == 2          # 384 tiles per layer on 256 workgroups
    assert info[14] > 0                       # weight slabs beyond the LDS budget are streamed
    rc, info = _plan(_desc(**CASES["configs2_lstm"]))
    assert rc == 0 and info[13] == 1          # 256 tiles: one unit per workgroup


def test_persist_floats_is_zero_for_gmm_head_and_layer_norm():
    """(> 0 for the qualifying descriptors needs the device's workgroup count: tests/test_gpu_decode_lstm.py)"""
    lib = _lib.load()
    lib.parrot_sample_persist_floats.restype = C.c_longlong
    d = _desc()
    d.gmm_K = 3
    assert lib.parrot_sample_persist_floats(C.byref(d)) == 0
    d = _desc()
    d.layer_norm = 1
    assert lib.parrot_sample_persist_floats(C.byref(d)) == 0


def test_gmm_head_and_layer_norm_are_refused():
    for field in ("gmm_K", "layer_norm"):
        d = _desc()
        setattr(d, field, 1)
        rc, info = _plan(d)
        assert rc != 0 and info[2] == 0


def test_too_few_places_is_refused_not_misplanned():
    rc, info = _plan(_desc(**CASES["cfg4_3x1536"]), nwg=128)   # 384 tiles > 128 workgroups x 2 units
    assert rc != 0 and info[2] == 0

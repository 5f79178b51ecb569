"""GRU decoders with bf16 layer units on the decode machine (PARROT_PM_GRU_BF16=1; ParrotSampleDesc::bf16 with cell = 0 and
the appended Wc_t16; plans_decode.hip bf16_eligible / SamplePlan::tile): both GRU programs -- the step cut along K and the
whole-K phases -- planned dry and replayed symbolically on the CPU, no device memory is touched.  Every layer unit (gate,
candidate and every piece of either) becomes a PM_GEMM16 on the tile's bf16 slab; the fed-back-frame composition and the
attention fold are not taken, the output tiles stay f32 units; what the bf16 machine does not take gets no plan at all.
With the switch unset nothing moves: the golden digests of tests/decode_plan_cases.py hold with the switch set, too."""
import ctypes as C

import pytest

from parrot_amd import _lib
from tests import decode_plan_cases as P

SWITCH = "PARROT_PM_GRU_BF16"
SMALL = dict(H=64, E=32, R=48)
CFG2 = dict(L=2, H=1024, E=512, R=1024, S=1000, B=16)


@pytest.fixture
def env(monkeypatch):
    """Every planner switch unset, the GRU bf16 switch at 1."""
    for k in P.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv(SWITCH, "1")
    return monkeypatch


def _gru(bf16=True, **kw):
    d = P.desc(cell=0, bf16=bf16, **kw)
    if bf16:
        for l in range(d.L):
            d.Wc_t16[l] = P._addr(d, "Wc_t16", l)
    return d


def _plan(d, nwg=256):
    lib = _lib.load()
    info = (C.c_int * 16)()
    rc = lib.parrot_sample_plan_pieces_dry(C.byref(d), nwg, info)
    dig = C.c_ulonglong(0)
    rc2 = lib.parrot_sample_plan_digest_dry(C.byref(d), nwg, C.byref(dig))
    assert rc2 == rc, (rc, rc2)
    return rc, list(info), dig.value


def _planned(kw, nwg=256):
    """The bf16 plan of a shape: planned, replayed clean, and not the f32 plan of the same descriptor."""
    rc, info, dig = _plan(_gru(**kw), nwg)
    assert rc == 0 and info[2] == 0 and dig != 0, (rc, info, dig)
    rc32, info32, dig32 = _plan(_gru(bf16=False, **kw), nwg)
    assert rc32 == 0 and info32[2] == 0
    assert dig != dig32
    return info, info32


def test_the_appended_field_is_the_last_one():
    """(tests/decode_plan_cases.py derives its made-up addresses from field indices: an insertion would move every digest)"""
    assert _lib.SampleDesc._fields_[-1][0] == "Wc_t16"


@pytest.mark.parametrize("B", [5, 16, 37, 64])
@pytest.mark.parametrize("L", [1, 2, 3])
def test_step_cut_along_k_plans_with_bf16_layer_units(env, L, B):
    """2L + 2 phases, every piece boundary on a 32-row boundary (H = 64, E = 32, 64 fed-back rows).  The f32 plan of the same
    descriptor has the same phases and units: only kinds, weight pointers and residency differ."""
    info, info32 = _planned(dict(L=L, B=B, speaker=B == 37, **SMALL))
    assert info[0] == 2 * L + 2 and info[15] == 0
    assert info[:14] == info32[:14]


@pytest.mark.parametrize("B", [5, 16, 37, 64])
@pytest.mark.parametrize("L", [1, 2, 3])
def test_whole_k_phases_plan_with_bf16_layer_units(env, L, B):
    env.setenv("PARROT_PM_PIECES", "0")
    info, info32 = _planned(dict(L=L, B=B, whole=True, speaker=B == 16, **SMALL))
    assert info[0] == 2 * L + 3 and info[1] == 0
    assert info[:14] == info32[:14]


def test_whole_k_is_the_fallback_without_the_composed_output_matrix(env):
    info, _ = _planned(dict(L=2, B=16, whole=True, composed=False, **SMALL))
    assert info[0] == 7


@pytest.mark.parametrize("whole", [False, True])
def test_plans_on_64_workgroups(env, whole):
    if whole:
        env.setenv("PARROT_PM_PIECES", "0")
    info, _ = _planned(dict(L=2, B=16, whole=whole, **SMALL), nwg=64)
    assert info[0] == (7 if whole else 6)


@pytest.mark.parametrize("whole", [False, True])
def test_configs2_width(env, whole):
    """2 x GRU-1024, E = 512, R = 1024, S = 1000: both programs plan; bf16 slabs take half the LDS, so no more units stream
    their weights than in the f32 plan of the same program without fold and composition."""
    if whole:
        env.setenv("PARROT_PM_PIECES", "0")
    info, info32 = _planned(dict(whole=whole, **CFG2))
    print("streamed units, bf16 / f32:", info[14], info32[14])
    assert info[0] == (7 if whole else 6)


@pytest.mark.parametrize("kw", [dict(L=2, B=16, **SMALL), dict(L=3, B=5, **SMALL), CFG2])
def test_composed_feedback_rows_and_attention_fold_are_given_but_not_taken(env, kw):
    """Wgx_t / Wcx_t / Watt_t in the descriptor change nothing under bf16: 2L + 2 phases, info16[15] == 0, and the program is the
    one planned without them, digest for digest.  The f32 plan of the same descriptor takes both."""
    rc, info, dig = _plan(_gru(fbc=True, attfold=True, **kw))
    assert rc == 0 and info[2] == 0 and info[15] == 0 and info[0] == 2 * kw["L"] + 2, (rc, info)
    assert (rc, info, dig) == _plan(_gru(**kw))
    rc32, info32, _ = _plan(_gru(bf16=False, fbc=True, attfold=True, **kw))
    assert rc32 == 0 and info32[15] != 0


OK = dict(L=2, B=16, S=10, **SMALL)


@pytest.mark.parametrize("value", [None, "0"])
def test_refused_without_the_switch(env, value):
    if value is None:
        env.delenv(SWITCH)
    else:
        env.setenv(SWITCH, value)
    rc, info, dig = _plan(_gru(**OK))
    assert rc != 0 and dig == 0 and info[2] == 0
    env.setenv(SWITCH, "1")
    assert _plan(_gru(**OK))[0] == 0


@pytest.mark.parametrize("name,kw,unset,gmm_switch", [
    ("H48", dict(H=48), (), False),
    ("E48", dict(E=48), (), False),
    ("no_Wc_t16_1", {}, (("Wc_t16", 1),), False),
    ("no_Wg_t16_0", {}, (("Wg_t16", 0),), False),
    ("gmm", dict(gmm_K=3), (), False),
    ("gmm_with_switch", dict(gmm_K=3), (), True),
    ("layer_norm", dict(layer_norm=1), (), False),
    ("B65", dict(B=65), (), False),
])
def test_what_the_bf16_gru_machine_does_not_take_is_refused(env, name, kw, unset, gmm_switch):
    if gmm_switch:
        env.setenv("PARROT_PM_GMM", "1")
    d = _gru(**dict(OK, **kw))
    for f, l in unset:
        getattr(d, f)[l] = None
    rc, info, dig = _plan(d)
    assert rc != 0 and dig == 0 and info[2] == 0, (name, rc, info)
    env.setenv("PARROT_PM_PIECES", "0")
    d = _gru(whole=True, **dict(OK, **kw))
    for f, l in unset:
        getattr(d, f)[l] = None
    assert _plan(d)[0] != 0, name


@pytest.fixture(scope="module")
def golden():
    return P.golden()


@pytest.mark.parametrize("name", list(P.CASES))
def test_golden_digests_hold_with_the_switch_set(name, golden, monkeypatch):
    """The appended field and the switch move nothing: every case of the golden file -- the pinned refusal of a bf16 GRU
    descriptor without Wc_t16 among them -- plans to its recorded return code, info16 and digest with PARROT_PM_GRU_BF16=1."""
    monkeypatch.setenv(SWITCH, "1")
    rc, info, dig = P.plan(name, monkeypatch)
    want = golden[name]
    assert (rc, info, dig) == (want["rc"], want["info16"], want["digest"])


def test_python_refusals(monkeypatch):
    from parrot_amd.model import Parrot
    kw = dict(readouts_dim=48, encoder_dim=16, input_dim=24, num_layers=2, encoder_type='bidirectional', device='cpu',
              decode_dtype='bf16', cell_type='gru')
    monkeypatch.delenv(SWITCH, raising=False)
    why = Parrot(rnn_h_dim=64, **kw)._decode_bf16_refusal(16)
    assert 'lstm' in why and SWITCH in why
    monkeypatch.setenv(SWITCH, "0")
    assert 'lstm' in Parrot(rnn_h_dim=64, **kw)._decode_bf16_refusal(16)
    monkeypatch.setenv(SWITCH, "1")
    assert Parrot(rnn_h_dim=64, **kw)._decode_bf16_refusal(16) == ''
    assert 'GMM' in Parrot(rnn_h_dim=64, which_cost='GMM', **kw)._decode_bf16_refusal(16)
    monkeypatch.setenv("PARROT_PM_GMM", "1")
    assert 'GMM' in Parrot(rnn_h_dim=64, which_cost='GMM', **kw)._decode_bf16_refusal(16)
    monkeypatch.delenv("PARROT_PM_GMM")
    assert 'layer_norm' in Parrot(rnn_h_dim=64, layer_norm=True, **kw)._decode_bf16_refusal(16)
    assert '32' in Parrot(rnn_h_dim=48, **kw)._decode_bf16_refusal(16)
    assert '64' in Parrot(rnn_h_dim=64, **kw)._decode_bf16_refusal(65)
    monkeypatch.setenv('PARROT_SAMPLE_PERSIST', '0')
    assert 'PARROT_SAMPLE_PERSIST' in Parrot(rnn_h_dim=64, **kw)._decode_bf16_refusal(16)

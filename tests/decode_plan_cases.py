"""The case table of the decode planners (plans_decode.hip): one descriptor, its switches and its workgroup count per
case, for every program SamplePlan::plan_persist can pick -- the GRU step cut along K (with the fed-back frame in or out
of the chain, the attention projection folded or not), the whole-K GRU phases with an MSE or a GMM head, LSTM stacks in
f32 and bf16 -- and every refusal the CPU plan tests know.

A case is planned dry (no device memory is touched, the descriptor's pointers are made-up addresses that are only used
for address arithmetic).  tests/golden/decode_plan_digests.json records per case the return code, info16
(parrot_sample_plan_pieces_dry) and the digest of the placed program (parrot_sample_plan_digest_dry: unit table, program
records, tick counts); tests/test_decode_plan_digests_cpu.py holds every later build to them, so a change to the planners
that moves one unit, one destination or one workspace address shows.  tools/record_decode_plan_digests.py writes the
file; record it only from a build whose programs are the standard."""
import ctypes as C
import json
import os

from parrot_amd import _lib

GOLDEN_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode_plan_digests.json")
SWITCHES = ("PARROT_PM_PIECES", "PARROT_PM_FBC", "PARROT_PM_ATTFOLD", "PARROT_PM_GMM", "PARROT_PM_DATAFLOW")
FB_PATTERNS = ((), (0,), (0, 1), (0, 1, 2))
BADARG = 10001

# Made-up addresses, one per field so that a swapped pointer changes the digest; never dereferenced by a dry run.
_BASE = 0x7000_0000_0000


def _addr(d, field, l=None):
    names = [f[0] for f in d._fields_]
    return _BASE + (names.index(field) * 4 + (l or 0)) * 0x100_0000


def _set(d, *fields):
    for f in fields:
        setattr(d, f, _addr(d, f))


def _set_layer(d, l, *fields):
    for f in fields:
        getattr(d, f)[l] = _addr(d, f, l)


def desc(cell=0, L=2, H=256, E=128, B=16, S=7, R=256, fb=(0,), speaker=False, composed=True, whole=False, fbc=False,
         attfold=False, bf16=False, gmm_K=0, unset=(), **fields):
    """cell 0 GRU, 1 LSTM.  composed: Wro_t / ro_const (the step cut along K, the LSTM output phase); whole: Wr_t / Wo_t /
    bo_pad (the whole-K GRU phases); fbc: Wgx_t / Wcx_t; attfold: Watt_t; gmm_K: the composed head and its randomness.
    unset: pointer fields cleared again; fields: plain values set last."""
    d = _lib.SampleDesc()
    d.S, d.B, d.H, d.E, d.A, d.U, d.L, d.O, d.R, d.ldx = S, B, H, E, 10, 100, L, 63, R, 64
    d.cell = cell
    _set(d, "x", "w", "kappa", "a", "phi", "ctx", "WattT", "batt")
    for l in range(L):
        _set_layer(d, l, "Wg_t", "bg", "h")
        if cell == 0:
            _set_layer(d, l, "Wc_t", "bc")
        if l in fb:
            _set_layer(d, l, "Wfg", *(("Wfc",) if cell == 0 else ()))
        if speaker:
            _set_layer(d, l, "seq_g", *(("seq_c",) if cell == 0 else ()))
        if bf16:
            _set_layer(d, l, "Wg_t16")
    d.bf16 = 1 if bf16 else 0
    if composed:
        _set(d, "Wro_t", "ro_const")
    if whole:
        _set(d, "Wr_t", "Wo_t", "bo_pad", "br")
        if speaker:
            _set(d, "radd", "oadd", "oadd_pad")
    if fbc:
        _set_layer(d, 0, "Wgx_t", "Wcx_t")
    if attfold:
        _set(d, "Watt_t")
    if gmm_K:
        d.gmm_K = gmm_K
        d.rh_cols = (2 * d.O * gmm_K + gmm_K + 15) // 16 * 16
        _set(d, "Wrh_t", "rh_const", "unif", "noise", "pi_out")
    for f in unset:
        if isinstance(f, tuple):
            getattr(d, f[0])[f[1]] = None
        else:
            setattr(d, f, None)
    for k, v in fields.items():
        setattr(d, k, v)
    return d


CASES = {}   # name -> dict(kw = desc() keywords, nwg, env = switches set for the case (every other switch is unset), ok)


def _case(name, nwg=256, env=None, ok=True, **kw):
    assert name not in CASES, name
    CASES[name] = dict(kw=kw, nwg=nwg, env=dict(env or {}), ok=ok)


def _fbname(fb):
    return "fb" + ("".join(str(l) for l in fb) or "none")


# ---- GRU, the step cut along K.  Every stack and feedback pattern at every batch size (speaker terms on every other case),
for L in (1, 2, 3):
    for fb in FB_PATTERNS:
        if fb and fb[-1] >= L:
            continue
        for i, B in enumerate((5, 16, 37, 64)):
            sp = (i + L + len(fb)) % 2 == 1
            _case(f"pieces_L{L}_B{B}_{_fbname(fb)}{'_spk' if sp else ''}", L=L, B=B, fb=fb, speaker=sp)
# ... the fed-back frame out of the chain and the attention fold, each alone and together, speaker on and off,
for L in (2, 3):
    for B in (5, 16, 37):
        for fbc, af in ((True, False), (False, True), (True, True)):
            for sp in (False, True):
                _case(f"pieces_L{L}_B{B}_fb0{'_fbc' if fbc else ''}{'_attfold' if af else ''}{'_spk' if sp else ''}",
                      L=L, B=B, fb=(0,), fbc=fbc, attfold=af, speaker=sp)
_case("pieces_L1_B16_fb0_attfold", L=1, fb=(0,), attfold=True)
_case("pieces_L2_B16_fb01_fbc_given_not_taken", L=2, fb=(0, 1), fbc=True)   # not the pattern the composition covers
# ... on 64 workgroups (L 3: pieces are joined until every phase fits, info16[1] is smaller than on 256),
for L in (1, 2, 3):
    for fbc in (False, True):
        _case(f"pieces_L{L}_B16_fb0{'_fbc' if fbc else ''}_nwg64", nwg=64, L=L, fb=(0,), fbc=fbc, attfold=True)
_case("pieces_L3_B16_fb012_spk_nwg64_joined", nwg=64, L=3, fb=(0, 1, 2), speaker=True)   # 12 partial sums, 19 on 256
_case("refused_pieces_L3_B64_fb012_spk_nwg64", nwg=64, ok=False, L=3, B=64, fb=(0, 1, 2), speaker=True)  # no join makes it fit
# ... the switches, and the configs[2] width.
_case("pieces_L2_B16_fb0_fbc_attfold_FBC0", env={"PARROT_PM_FBC": "0"}, fbc=True, attfold=True)
_case("pieces_L2_B16_fb0_fbc_attfold_ATTFOLD0", env={"PARROT_PM_ATTFOLD": "0"}, fbc=True, attfold=True)
_case("pieces_L2_B16_fb0_fbc_attfold_DATAFLOW0", env={"PARROT_PM_DATAFLOW": "0"}, fbc=True, attfold=True)
_case("pieces_configs2", L=2, H=1024, E=512, R=1024, S=1000, fbc=True, attfold=True)
_case("pieces_configs2_plain", L=2, H=1024, E=512, R=1024, S=1000)

# ---- GRU, whole-K phases: PARROT_PM_PIECES=0, or a descriptor without the composed output matrix.
_WHOLE = {"PARROT_PM_PIECES": "0"}
for L in (1, 2, 3):
    for fb in FB_PATTERNS:
        if fb and fb[-1] >= L:
            continue
        for i, B in enumerate((5, 16, 37, 64)):
            sp = (i + L + len(fb)) % 2 == 0
            _case(f"whole_L{L}_B{B}_{_fbname(fb)}{'_spk' if sp else ''}", env=_WHOLE, whole=True, L=L, B=B, fb=fb, speaker=sp)
_case("whole_L2_B16_fb0_no_composed_matrix", whole=True, composed=False)
_case("whole_L2_B16_fb0_nwg64", nwg=64, env=_WHOLE, whole=True)
_case("whole_L2_B16_fb0_DATAFLOW1", env=dict(_WHOLE, PARROT_PM_DATAFLOW="1"), whole=True)
_case("whole_configs2", env=_WHOLE, whole=True, L=2, H=1024, E=512, R=1024, S=1000)

# ---- GRU, whole-K phases with a GMM head (PARROT_PM_GMM=1)
_GMM = {"PARROT_PM_GMM": "1"}
for K in (1, 3, 20):
    for L in (1, 2, 3):
        B = (5, 16, 37)[(L + K) % 3]
        fb = FB_PATTERNS[1 + (L + K) % L] if L > 1 else (0,)
        _case(f"whole_gmm_K{K}_L{L}_B{B}_{_fbname(fb)}", env=_GMM, composed=False, gmm_K=K, L=L, B=B, fb=fb, speaker=K == 3)
_case("whole_gmm_K3_L2_B16_nwg64", nwg=64, env=_GMM, composed=False, gmm_K=3)
_case("whole_gmm_K20_L2_B16_nwg64_refused", nwg=64, env=_GMM, ok=False, composed=False, gmm_K=20)

# ---- LSTM stacks: the cases of tests/test_decode_lstm_plan_cpu.py in f32 and bf16, GMM heads, the 3 x 1536 width
LSTM = {
    "configs2_lstm": dict(L=2, H=1024, E=512, R=1024, B=16, S=1000, fb=(0,)),
    "configs2_lstm_b64": dict(L=2, H=1024, E=512, R=1024, B=64, S=1000, fb=(0,)),
    "cfg4_3x1536": dict(L=3, H=1536, E=256, R=1536, B=16, S=1000, fb=(0,)),
    "one_layer_no_feedback": dict(L=1, H=256, E=128, R=256, B=5, S=50, fb=()),
    "full_feedback_speaker": dict(L=3, H=256, E=128, R=256, B=16, S=50, fb=(0, 1, 2), speaker=True),
}
for name, kw in LSTM.items():
    _case("lstm_" + name, cell=1, **kw)
    _case("lstm_bf16_" + name, cell=1, bf16=True, **kw)
for K in (3, 20):
    _case(f"lstm_gmm_K{K}_L2_B16", env=_GMM, cell=1, composed=False, gmm_K=K)
    _case(f"lstm_gmm_K{K}_L3_B37_fb012", env=_GMM, cell=1, composed=False, gmm_K=K, L=3, B=37, fb=(0, 1, 2), speaker=True)
_case("lstm_gmm_K20_cfg4_3x1536", env=_GMM, cell=1, composed=False, gmm_K=20, **LSTM["cfg4_3x1536"])
_case("lstm_gmm_K8_L2_B16_nwg64", nwg=64, env=_GMM, cell=1, composed=False, gmm_K=8, S=50)
_case("lstm_bf16_padding_rows", cell=1, bf16=True, L=3, H=64, E=32, R=48, B=5, S=14, fb=(0, 1, 2), speaker=True)

# ---- refusals: every one of the CPU plan tests (test_decode_plan_cpu, _lstm_plan_cpu, _bf16_plan_cpu, _gmm_cpu)
_case("refused_pieces_configs2_nwg100", nwg=100, ok=False, L=2, H=1024, E=512, R=1024, S=1000)
_case("refused_pieces_switched_off_no_whole_k_matrices", env=_WHOLE, ok=False, L=2, H=1024, E=512, R=1024, S=1000)
_case("refused_lstm_gmm_without_switch", ok=False, cell=1, **dict(LSTM["configs2_lstm"], gmm_K=1))
_case("refused_lstm_gmm_plain_fields_without_switch", ok=False, cell=1, gmm_K=3, composed=False)
_case("refused_lstm_gmm_switch_0", env={"PARROT_PM_GMM": "0"}, ok=False, cell=1, gmm_K=3, composed=False)
_case("refused_lstm_layer_norm", ok=False, cell=1, layer_norm=1, **LSTM["configs2_lstm"])
_case("refused_lstm_cfg4_nwg128", nwg=128, ok=False, cell=1, **LSTM["cfg4_3x1536"])
_BF = dict(cell=1, bf16=True, L=2, H=64, E=32, R=48, B=16, S=10, fb=(0,))
_case("lstm_bf16_small", **_BF)
_case("refused_bf16_H48", ok=False, **dict(_BF, H=48))
_case("refused_bf16_E48", ok=False, **dict(_BF, E=48))
_case("refused_bf16_gru", ok=False, **dict(_BF, cell=0))
_case("refused_bf16_gmm", ok=False, **dict(_BF, gmm_K=3))
_case("refused_bf16_gmm_with_switch", env=_GMM, ok=False, **dict(_BF, gmm_K=3))
_case("refused_bf16_layer_norm", ok=False, layer_norm=1, **_BF)
_case("refused_bf16_B65", ok=False, **dict(_BF, B=65))
_case("refused_bf16_layer_without_copy", ok=False, unset=(("Wg_t16", 1),), **_BF)
_LG = dict(cell=1, composed=False, L=2, B=16, S=50, gmm_K=3)
_case("refused_lstm_gmm_K20_nwg64", nwg=64, env=_GMM, ok=False, **dict(_LG, gmm_K=20))
_case("refused_lstm_gmm_K9_nwg64", nwg=64, env=_GMM, ok=False, **dict(_LG, gmm_K=9))
_case("refused_lstm_gmm_K65", env=_GMM, ok=False, **dict(_LG, gmm_K=65))
_case("refused_lstm_gmm_layer_norm", env=_GMM, ok=False, layer_norm=1, **_LG)
for f in ("Wrh_t", "rh_const", "unif", "noise", "pi_out"):
    _case("refused_lstm_gmm_without_" + f, env=_GMM, ok=False, unset=(f,), **_LG)
_case("refused_lstm_gmm_rh_cols_392", env=_GMM, ok=False, rh_cols=392, **_LG)
_case("refused_lstm_gmm_rh_cols_368", env=_GMM, ok=False, rh_cols=368, **_LG)


def plan(name, monkeypatch=None):
    """(rc, info16, digest) of a case, planned under the case's switches -- set through `monkeypatch`, or in os.environ and
    restored (the recorder)."""
    c = CASES[name]
    saved = {k: os.environ.get(k) for k in SWITCHES}
    for k in SWITCHES:
        v = c["env"].get(k)
        if monkeypatch is not None:
            monkeypatch.setenv(k, v) if v is not None else monkeypatch.delenv(k, raising=False)
        elif v is not None:
            os.environ[k] = v
        else:
            os.environ.pop(k, None)
    try:
        lib = _lib.load()
        d = desc(**c["kw"])
        info = (C.c_int * 16)()
        rc = lib.parrot_sample_plan_pieces_dry(C.byref(d), c["nwg"], info)
        dig = C.c_ulonglong(0)
        rc2 = lib.parrot_sample_plan_digest_dry(C.byref(d), c["nwg"], C.byref(dig))
        assert rc2 == rc, (name, rc, rc2)
        return rc, list(info), "%016x" % dig.value
    finally:
        if monkeypatch is None:
            for k, v in saved.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v


def golden():
    with open(GOLDEN_JSON) as f:
        return json.load(f)

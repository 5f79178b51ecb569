"""Cases and fingerprint of the decode workspace (Parrot._sample_workspace), shared by tests/test_decode_workspace_cpu.py
and tools/record_decode_workspace_fingerprints.py.

A workspace is built on the CPU device with the library's plan entries replaced by recording stubs, so no HIP call is
made.  parrot_sample_persist_floats[_forced] is stubbed with them: it sizes the machine's workspace for the device's
compute units (0 without a device), so its own answer would differ between a machine with a GPU and one without; the
stub answers PERSIST_FLOATS wherever the Python side asks and records how many pointer slots of the descriptor were set when it was asked.  The fingerprint holds what the
library would have been handed and nothing that differs from run to run: every scalar field of the descriptor; for every
pointer field and array slot None or the NAME of the workspace tensor or stored parameter that starts at that address;
shape, dtype and zero-fill of every tensor of ws and ws['pm'] (torch.empty is patched to fill with NaN, so a tensor that
reads all zero was asked for as zeros); the cache key; the stubbed calls in order.  Addresses never enter it.

tests/golden/decode_workspace_fingerprints.json records the fingerprints of the commit named in its header; the test
holds every later build to them key for key, so a workspace refactor that drops a buffer, turns a padded `zeros` into an
`empty`, or hands the library another tensor shows without a device.

Shapes are the smallest that reach each branch: H = 64, E = 32, A = 10, R = 64, O = 63, U = 5, S = 3, N = 3."""
import ctypes as C
import json
import os

import torch

from parrot_amd import _lib

GOLDEN_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode_workspace_fingerprints.json")
SWITCHES = ("PARROT_PM_GRU_BF16", "PARROT_PM_GMM", "PARROT_SAMPLE_PERSIST", "PARROT_PM_ATTFOLD", "PARROT_PM_FBC",
            "PARROT_PM_PIECES", "PARROT_PM_DATAFLOW")
STUBBED = ("parrot_sample_create", "parrot_sample_create_forced", "parrot_sample_set_row_controls", "parrot_sample_is_bf16",
           "parrot_sample_stops_early", "parrot_sample_destroy", "parrot_sample_persist_floats",
           "parrot_sample_persist_floats_forced")
PERSIST_FLOATS = 4096
BASE = dict(rnn_h_dim=64, readouts_dim=64, input_dim=32, encoder_type=None, attention_size=10, output_dim=63,
            speaker_dim=8, num_speakers=5, k_gmm=3)
S, N, U = 3, 3, 5
_GRU2 = dict(num_layers=2, weak_feedback=True)
_LSTM = dict(cell_type='lstm', num_layers=2, weak_feedback=True)

CASES = {}   # name -> dict(kw = Parrot keywords over BASE, N, stop_extra, forced, env = the case's switches, all others unset)


def _case(name, env=None, N=N, stop_extra=0, forced=False, **kw):
    assert name not in CASES, name
    CASES[name] = dict(kw=kw, N=N, stop_extra=stop_extra, forced=forced, env=dict(env or {}))


_case("gru1", num_layers=1)
_case("gru2_composed_feedback", **_GRU2)                      # _fb_layers == [1]: Wgx_t / Wcx_t
_case("gru2_forced", forced=True, **_GRU2)                    # ... which a forced plan does not get
_case("gru2_n17", N=17, **_GRU2)                              # no attention fold above 16 rows
_case("gru2_attfold0", env={"PARROT_PM_ATTFOLD": "0"}, **_GRU2)
_case("gru2_fbc0", env={"PARROT_PM_FBC": "0"}, **_GRU2)
_case("gru3_full_feedback", num_layers=3, full_feedback=True)
_case("lstm", **_LSTM)
_case("lstm_bf16", decode_dtype='bf16', **_LSTM)
_case("gru_bf16", env={"PARROT_PM_GRU_BF16": "1"}, decode_dtype='bf16', **_GRU2)
_case("gmm", which_cost='GMM', **_GRU2)
_case("gmm_machine", env={"PARROT_PM_GMM": "1"}, which_cost='GMM', **_GRU2)
_case("speaker_mse", use_speaker=True, **_GRU2)
_case("speaker_gmm", use_speaker=True, which_cost='GMM', **_GRU2)
_case("speaker_gmm_machine", env={"PARROT_PM_GMM": "1"}, use_speaker=True, which_cost='GMM', **_GRU2)
_case("layer_norm", layer_norm=True, **_GRU2)                 # no pm, ln_scratch
_case("stop8", stop_extra=8, **_GRU2)
_case("forced_stop8", stop_extra=8, forced=True, **_GRU2)
_case("lstm_forced_stop8", stop_extra=8, forced=True, **_LSTM)
_case("h72_machine_refuses", rnn_h_dim=72, **_GRU2)
_case("persist_off", env={"PARROT_SAMPLE_PERSIST": "0"}, **_GRU2)


def set_switches(monkeypatch, env):
    for k in SWITCHES:
        if k in env:
            monkeypatch.setenv(k, env[k])
        else:
            monkeypatch.delenv(k, raising=False)


def model(name):
    from parrot_amd.model import Parrot
    return Parrot(device=torch.device('cpu'), **dict(BASE, **CASES[name]["kw"])).allocate()


def _pointer_slots_set(d):
    n = 0
    for field, ctype in d._fields_:
        v = getattr(d, field)
        if isinstance(v, C.Structure):
            n += _pointer_slots_set(v)
        elif ctype is C.c_void_p:
            n += v is not None
        elif isinstance(v, C.Array):
            n += sum(x is not None for x in v)
    return n


def install_stubs(monkeypatch, is_bf16=1, stops_early=1, row_controls_rc=0, persist_floats=PERSIST_FLOATS):
    """Replaces the STUBBED entries of the loaded library with stubs and torch.empty with one that fills with NaN.
    Returns the record: a list of (entry name, arguments) in call order."""
    lib, calls = _lib.load(), []

    def create(name):
        def stub(desc_ref, plan_ref):
            plan_ref._obj.value = 0x1000 + len(calls)
            calls.append((name, (desc_ref._obj,)))
            return 0
        return stub

    def floats(name):
        def stub(desc_ref):
            calls.append((name, (_pointer_slots_set(desc_ref._obj),)))
            return persist_floats
        return stub

    def answer(name, value):
        def stub(*args):
            calls.append((name, args))
            return value
        return stub

    monkeypatch.setattr(lib, "parrot_sample_create", create("parrot_sample_create"))
    monkeypatch.setattr(lib, "parrot_sample_create_forced", create("parrot_sample_create_forced"))
    monkeypatch.setattr(lib, "parrot_sample_set_row_controls", answer("parrot_sample_set_row_controls", row_controls_rc))
    monkeypatch.setattr(lib, "parrot_sample_is_bf16", answer("parrot_sample_is_bf16", is_bf16))
    monkeypatch.setattr(lib, "parrot_sample_stops_early", answer("parrot_sample_stops_early", stops_early))
    monkeypatch.setattr(lib, "parrot_sample_destroy", answer("parrot_sample_destroy", 0))
    monkeypatch.setattr(lib, "parrot_sample_persist_floats", floats("parrot_sample_persist_floats"))
    monkeypatch.setattr(lib, "parrot_sample_persist_floats_forced", floats("parrot_sample_persist_floats_forced"))
    empty = torch.empty

    def nan_empty(*a, **kw):
        t = empty(*a, **kw)
        return t.fill_(float('nan')) if t.is_floating_point() else t

    monkeypatch.setattr(torch, "empty", nan_empty)
    return calls


def _tensors(ws):
    """name -> tensor or None, for every tensor slot of ws and ws['pm'] (lists by index, the machine's tables by key)."""
    out = {}

    def put(name, v):
        if v is None or torch.is_tensor(v):
            out[name] = v
        elif isinstance(v, list):
            for i, x in enumerate(v):
                put(f"{name}[{i}]", x)
        elif isinstance(v, dict):
            for k, x in v.items():
                put(f"{name}.{k}" if isinstance(k, str) else f"{name}[{','.join(str(i) for i in k)}]", x)
    for k, v in ws.items():
        if k not in ("plan", "desc", "ldx"):
            put(k, v)
    return out


def _describe(d, names, scalars, pointers, prefix=""):
    for field, ctype in d._fields_:
        v = getattr(d, field)
        if isinstance(v, C.Structure):
            _describe(v, names, scalars, pointers)
        elif ctype is C.c_void_p:
            pointers[prefix + field] = names(v)
        elif isinstance(v, C.Array):
            pointers[prefix + field] = [names(x) for x in v]
        else:
            scalars[prefix + field] = v


def fingerprint(m, S, N, U, stop_extra=0, forced=False, calls=None):
    """The fingerprint of m._sample_workspace(S, N, U, stop_extra=, forced=), built under install_stubs (`calls`: its record)."""
    before = set(m._sample_ws)
    ws = m._sample_workspace(S, N, U, stop_extra=stop_extra, forced=forced)
    new = [k for k in m._sample_ws if k not in before]
    assert len(new) == 1 and m._sample_ws[new[0]] is ws
    tensors = _tensors(ws)
    by_addr = {}
    for name, t in list(m.store.storage.items()) + list(tensors.items()):
        if t is not None:
            assert t.data_ptr() not in by_addr, (name, by_addr[t.data_ptr()])
            by_addr[t.data_ptr()] = name

    def names(addr):
        return None if not addr else by_addr.get(addr, "?")
    scalars, pointers = {}, {}
    _describe(ws["desc"], names, scalars, pointers)
    fp = dict(key=list(new[0]), ldx=ws["ldx"], forced_descriptor=isinstance(ws["desc"], _lib.SampleForcedDesc),
              scalars=scalars, pointers=pointers,
              tensors={n: None if t is None else [list(t.shape), str(t.dtype), bool((t == 0).all())]
                       for n, t in tensors.items()})
    if calls is not None:
        fp["calls"] = [[name] + ([names(a) for a in args[1:]] if name == "parrot_sample_set_row_controls" else
                                 list(args) if "persist_floats" in name else []) for name, args in calls]
    return json.loads(json.dumps(fp))


def case_fingerprint(name, monkeypatch):
    """The fingerprint of a case: its switches, the stubs, a fresh model."""
    c = CASES[name]
    set_switches(monkeypatch, c["env"])
    m = model(name)
    calls = install_stubs(monkeypatch)
    return fingerprint(m, S, c["N"], U, c["stop_extra"], c["forced"], calls)


def golden():
    with open(GOLDEN_JSON) as f:
        return json.load(f)

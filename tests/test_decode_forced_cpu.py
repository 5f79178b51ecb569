"""The premise of tests/test_gpu_decode_forced.py, and everything of the forced frames that needs no device: the forced
loop of tests/decode_forced_cases.py IS the oracle's sample_model when nothing is forced and reproduces a run from its own
frames, every case can tell a decode that ignores the forcing, the GMM seeds keep their margins; a forced descriptor plans
dry without the composition while every unforced one keeps its digest; the ctypes struct is the header's; the Python entry
points refuse bad arguments before anything is allocated; sample.py's flag."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import decode_forced_cases as FC
from tests import decode_plan_cases as P
from tests.util import rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------- the forced oracle
@pytest.mark.parametrize("name", ["gru2_mse_n5", "lstm2_k3_n5", "layer_norm"])
def test_nothing_forced_is_sample_model(name):
    """All n = 0 (and no frames at all): the loop's six outputs equal oracle.parrot_ref.sample_model exactly, own_x = sample_x."""
    c = FC.case(name)
    kw = dict(unif=c['unif'], noise=c['noise'])
    with torch.no_grad():
        zero = FC.forced_loop(c['p'], c['cfg'], c['lab'], c['lm'], c['spk'], c['S'], c['forced'], [0] * c['N'], **kw)
        none = FC.forced_loop(c['p'], c['cfg'], c['lab'], c['lm'], c['spk'], c['S'], **kw)
    for run in (zero, none):
        for a, b, n in zip(run, c['free'], FC.NAMES):
            assert torch.equal(a, b), n
        assert torch.equal(run[6], run[0])


@pytest.mark.parametrize("name", ["gru2_mse_n5", "lstm2_k3_n5"])
def test_forcing_a_run_with_its_own_frames_reproduces_it(name):
    """forced = the free run's own_x, n = S everywhere: every output of the free run, bit for bit."""
    c = FC.case(name)
    with torch.no_grad():
        own = FC.forced_loop(c['p'], c['cfg'], c['lab'], c['lm'], c['spk'], c['S'], unif=c['unif'], noise=c['noise'])
        again = FC.forced_loop(c['p'], c['cfg'], c['lab'], c['lm'], c['spk'], c['S'], own[6], [c['S']] * c['N'], unif=c['unif'],
                               noise=c['noise'])
    for a, b, n in zip(again, own, FC.NAMES):
        assert torch.equal(a, b), n


@pytest.mark.parametrize("name", sorted(FC.CASES))
@pytest.mark.parametrize("which", ["A", "B"])
def test_case_premise(name, which):
    """Every case and both sets: the forced region of sample_x holds the given frames; behind the prompt the forced run is
    more than 0.05 away from the free run (a decode that ignored the forcing could not pass); the forced oracle's float32
    twin stays within F32_MARGIN; GMM cases keep PICK_MARGIN on every draw of every run the GPU tests compare with."""
    c = FC.case(name, which)
    free = FC.free_region(c)
    assert c['n'] == FC.prompt_lengths(c['N'], which) and len(c['n']) == c['N']
    assert torch.equal(c['ref'][0][~free], c['forced'][~free])
    assert not torch.equal(c['ref'][6][~free], c['forced'][~free])
    assert torch.equal(c['ref'][0][free], c['ref'][6][free])
    e = rel_err(c['ref'][0][free], c['free'][0][free])
    e32 = FC.f32_error(c)
    print(f"{name} {which}: forced vs free behind the prompt {e:.2e}, float32 error {e32:.2e}")
    assert e > 0.05
    assert e32 <= FC.F32_MARGIN
    if c['gmm']:
        m = FC.pick_margin(c, c['ref'])
        print(f"{name} {which}: pick margin {m:.2e}")
        assert m >= FC.PICK_MARGIN
        if which == 'A':
            assert FC.pick_margin(c, c['free']) >= FC.PICK_MARGIN and FC.f32_error(c, forced=False) <= FC.F32_MARGIN


def test_prompt_lengths_cover_the_edges():
    S = FC.S
    assert FC.prompt_lengths(5) == [0, 4, 1, S, S - 1]
    assert FC.prompt_lengths(17)[15:] == [0, 4] and len(FC.prompt_lengths(17)) == 17
    assert FC.prompt_lengths(5, 'B') != FC.prompt_lengths(5) and sorted(FC.prompt_lengths(5, 'B'))[0] == 0
    assert FC.prompt_lengths(5, 'A', steps=48) == [0, 4, 1, 48, 47]
    with torch.no_grad():
        c = FC.case_with_controls('gru2_mse_n5')
    assert rel_err(c['ref'][0], FC.case('gru2_mse_n5')['ref'][0]) > 0.05, "the controls must change the forced run"
    assert FC.f32_error(c) <= FC.F32_MARGIN


# ---------------------------------------------------------------------------------------------------- dry plans
def _forced_desc(kw):
    """ParrotSampleForcedDesc: the case's descriptor with made-up addresses in the three fields behind it."""
    from parrot_amd import _lib
    fd = _lib.SampleForcedDesc()
    fd.base = P.desc(**kw)
    for i, f in enumerate(("forced", "n_forced", "own_x")):
        setattr(fd, f, P._BASE + (len(_lib.SampleDesc._fields_) * 4 + i) * 0x100_0000)
    return fd


def _plan(d, nwg=256):
    """(rc, info16, digest) of a dry plan: a SampleForcedDesc through the _forced entries, a SampleDesc through the plain ones."""
    from parrot_amd import _lib
    lib = _lib.load()
    sfx = "_forced" if isinstance(d, _lib.SampleForcedDesc) else ""
    info, dig = (C.c_int * 16)(), C.c_ulonglong(0)
    rc = getattr(lib, "parrot_sample_plan_pieces_dry" + sfx)(C.byref(d), nwg, info)
    assert getattr(lib, "parrot_sample_plan_digest_dry" + sfx)(C.byref(d), nwg, C.byref(dig)) == rc
    return rc, list(info), dig.value


FORCED_PLANS = ["pieces_L2_B16_fb0_fbc_attfold", "pieces_L3_B5_fb0_fbc", "pieces_L1_B16_fb0_attfold", "pieces_configs2",
                "whole_L2_B16_fb0_spk", "whole_gmm_K3_L2_B16_nwg64", "lstm_configs2_lstm", "lstm_gmm_K3_L2_B16"]


@pytest.mark.parametrize("name", FORCED_PLANS)
def test_a_forced_descriptor_plans_without_the_composition(name, monkeypatch):
    """The case's descriptor with the three forced fields: it plans, the replay's verdict is 0, info16[15] shows no
    composition (bit 0) and keeps the fold (bit 1) where the unforced plan has it.  Where the unforced plan composes, the
    forced plan is the one PARROT_PM_FBC=0 gives: same phases, partial sums and units per phase."""
    assert name in P.CASES
    rc0, info0, dig0 = P.plan(name, monkeypatch)   # (sets the case's switches)
    assert rc0 == 0
    d = _forced_desc(P.CASES[name]["kw"])
    rc, info, dig = _plan(d, P.CASES[name]["nwg"])
    assert rc == 0 and info[2] == 0 and dig != 0
    assert info[15] & 1 == 0 and info[15] & 2 == info0[15] & 2
    if d.gmm_K == 0:  # (a GMM head's sampling rows need no mark: their kernel argument alone tells them)
        assert dig != int(dig0, 16), "the frame's units carry the mark of a forced plan"
    assert _plan(d, P.CASES[name]["nwg"]) == (rc, info, dig)
    free = _forced_desc(P.CASES[name]["kw"])
    free.forced = free.n_forced = free.own_x = None   # the forced entries with nothing forced: the recorded plan
    assert _plan(free, P.CASES[name]["nwg"]) == (rc0, info0, int(dig0, 16))
    if info0[15] & 1:
        monkeypatch.setenv("PARROT_PM_FBC", "0")
        rc1, info1, _ = _plan(P.desc(**P.CASES[name]["kw"]), P.CASES[name]["nwg"])
        assert rc1 == 0 and info1 == info
        assert info[0] == info0[0] + 1
    else:
        assert info == info0


def test_unforced_descriptors_keep_their_digests(monkeypatch):
    """A sample of the recorded cases (tests/test_decode_plan_digests_cpu.py holds all of them): the appended fields, left
    NULL, change no program."""
    golden = P.golden()
    for name in FORCED_PLANS + ["lstm_bf16_small", "whole_configs2"]:
        rc, info, dig = P.plan(name, monkeypatch)
        assert (rc, info, dig) == (golden[name]["rc"], golden[name]["info16"], golden[name]["digest"]), name


def test_bf16_with_forcing_has_no_plan(monkeypatch):
    rc0, _, _ = P.plan("lstm_bf16_small", monkeypatch)
    assert rc0 == 0
    rc, info, dig = _plan(_forced_desc(P.CASES["lstm_bf16_small"]["kw"]))
    assert rc != 0 and dig == 0


def test_struct_sizes_and_offsets_match_the_header(tmp_path):
    """ParrotSampleForcedDesc is the decode descriptor, unchanged in size, and three pointers behind it."""
    from parrot_amd import _lib
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "parrot_hip.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(ParrotSampleDesc), sizeof(ParrotSampleForcedDesc), '
                   'offsetof(ParrotSampleForcedDesc, base), offsetof(ParrotSampleForcedDesc, forced), '
                   'offsetof(ParrotSampleForcedDesc, n_forced), offsetof(ParrotSampleForcedDesc, own_x));return 0;}\n')
    exe = tmp_path / "s"
    subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    D, F = _lib.SampleDesc, _lib.SampleForcedDesc
    want = [C.sizeof(D), C.sizeof(F), F.base.offset, F.forced.offset, F.n_forced.offset, F.own_x.offset]
    assert [int(v) for v in subprocess.check_output([str(exe)]).split()] == want
    assert F.base.offset == 0 and F.forced.offset == C.sizeof(D) and C.sizeof(F) == C.sizeof(D) + 3 * C.sizeof(C.c_void_p)
    assert not any(f[0] in ("forced", "n_forced", "own_x") for f in D._fields_), "the decode descriptor itself did not grow"
    fd = F()
    fd.S, fd.Wc_t16[1] = 7, 0x1234   # the base's fields read and write as the object's own
    assert fd.base.S == 7 and fd.base.Wc_t16[1] == 0x1234


def test_forced_entries_reject_bad_arguments():
    from parrot_amd import _lib
    lib, fd, dig, info = _lib.load(), _forced_desc({}), C.c_ulonglong(7), (C.c_int * 16)()
    assert lib.parrot_sample_plan_digest_dry_forced(None, 256, C.byref(dig)) == P.BADARG
    assert lib.parrot_sample_plan_digest_dry_forced(C.byref(fd), 0, C.byref(dig)) == P.BADARG
    assert lib.parrot_sample_plan_pieces_dry_forced(None, 256, info) == P.BADARG
    assert lib.parrot_sample_create_forced(None, None) == P.BADARG and lib.parrot_sample_persist_floats_forced(None) == 0
    assert dig.value == 7
    fd.n_forced = None   # two of three
    plan = C.c_void_p()
    assert lib.parrot_sample_create_forced(C.byref(fd), C.byref(plan)) == P.BADARG and not plan.value


# ---------------------------------------------------------------------------------------------------- argument validation
def _never_allocated(**kw):
    from parrot_amd.model import Parrot
    return Parrot(device=torch.device('cpu'), **dict(dict(FC.SMALL, cell_type='lstm', num_layers=1, which_cost='MSE'), **kw))


O = 63  # output_dim of the small model


@pytest.mark.parametrize("kw, match", [
    (dict(forced_frames=np.zeros((4, 3, O))), "go together"),
    (dict(n_forced=[0, 1, 2]), "go together"),
    (dict(forced_frames=np.zeros((4, 3, O - 1)), n_forced=[0, 1, 2]), "shape"),
    (dict(forced_frames=np.zeros((4, 2, O)), n_forced=[0, 1, 2]), "shape"),
    (dict(forced_frames=np.zeros((3, O)), n_forced=[0, 1, 2]), "shape"),
    (dict(forced_frames=np.zeros((7, 3, O)), n_forced=[0, 1, 2]), "P <= 6"),
    (dict(forced_frames=np.zeros((4, 3, O)), n_forced=[0, 1]), "n_forced needs 3 values"),
    (dict(forced_frames=np.zeros((4, 3, O)), n_forced=[0, 5, 2]), r"0 \.\. 4"),
    (dict(forced_frames=np.zeros((4, 3, O)), n_forced=[0, -1, 2]), r"0 \.\. 4"),
    (dict(forced_frames=np.zeros((4, 3, O)), n_forced=[0, 1.5, 2]), "whole numbers"),
    (dict(forced_frames=np.full((4, 3, O), np.nan), n_forced=[0, 1, 2]), "finite"),
    (dict(forced_frames=np.full((4, 3, O), np.inf), n_forced=[0, 0, 0]), "finite"),
])
def test_bad_arguments_are_refused_before_anything_is_allocated(kw, match):
    m = _never_allocated()
    lab, lm = np.zeros((3, 4), dtype='int64'), np.ones((3, 4), dtype='float32')
    for call in (lambda: m.sample_model_device(lab, lm, None, 3, 6, **kw),
                 lambda: m.sample_model(lab, lm, None, None, 3, 6, **kw),
                 lambda: m.sample_until_end_device(lab, lm, None, 3, 6, **kw),
                 lambda: m.sample_until_end(lab, lm, None, None, 3, 6, **kw)):
        with pytest.raises(ValueError, match=match):
            call()
    assert not m._sample_ws and m.decode_path is None


def test_bf16_decode_refuses_forcing():
    m = _never_allocated(num_layers=2, weak_feedback=True, decode_dtype='bf16')
    lab, lm = np.zeros((3, 4), dtype='int64'), np.ones((3, 4), dtype='float32')
    for call in (m.sample_model_device, m.sample_until_end_device):
        with pytest.raises(ValueError, match="bf16"):
            call(lab, lm, None, 3, 6, forced_frames=np.zeros((4, 3, O)), n_forced=[0, 1, 2])
    assert m._decode_forced_refusal() and not _never_allocated()._decode_forced_refusal()
    assert not m._sample_ws


def test_check_forced_returns_what_the_call_writes():
    m = _never_allocated()
    assert m._check_forced(3, 6) is None
    fr, n = m._check_forced(3, 6, torch.ones(4, 3, O, dtype=torch.float64), torch.tensor([0, 4, 2]))
    assert fr.dtype == np.float32 and fr.shape == (4, 3, O) and n.dtype == np.int32 and n.tolist() == [0, 4, 2]
    fr, n = m._check_forced(3, 6, np.zeros((6, 3, O)), (6, 0, 3.0))
    assert fr.shape == (6, 3, O) and n.tolist() == [6, 0, 3]


# ---------------------------------------------------------------------------------------------------- sample.py's flag
def test_prime_frames_flag():
    from parrot_amd.utils import prime_frames, sample_parse
    assert sample_parse([]).prime_frames == 0 and sample_parse(["--prime_frames", "3"]).prime_frames == 3
    with pytest.raises(SystemExit, match="--phrase"):
        sample_parse(["--prime_frames", "3", "--phrase", "hello"])
    with pytest.raises(SystemExit, match="negative"):
        sample_parse(["--prime_frames", "-1"])
    feats = np.arange(5 * 2 * 3, dtype=np.float64).reshape(5, 2, 3)
    mask = np.array([[1, 1], [1, 1], [1, 0], [1, 0], [0, 0]], dtype=np.float32)
    fr, n = prime_frames(feats, mask, 3, 100)
    assert fr.dtype == np.float32 and np.array_equal(fr, feats[:3]) and n.dtype == np.int32 and n.tolist() == [3, 2]
    fr, n = prime_frames(feats, mask, 9, 100)
    assert fr.shape == (5, 2, 3) and n.tolist() == [4, 2]
    fr, n = prime_frames(feats, mask, 9, 2)
    assert fr.shape == (2, 2, 3) and n.tolist() == [2, 2]

"""The host's half of tests/test_gpu_step_launch_modes.py, checked WITHOUT a GPU: which launches get the z-grid (grid.z =
job: the kernel instantiation that never reads the launch header) and which the prefix table along x
(parrot_step_launch_mode = sk_make_launch + sk_prepare, no HIP call), and that the decoder plans of the GPU cases make the
launch kinds those cases are about (dry-run plans, parrot_decoder_trace_jobs)."""
import ctypes as C
import os

import pytest

from tests import step_launch_cases as S

H = S.H


def _lib():
    from parrot_amd import _lib as L
    try:
        return L, L.load()
    except L.HipLibraryMissing:
        pytest.skip("libparrot_hip.so not built")


MODE_CASES = {
    # name: (jobs (M, N, K[, lstm_H]), z-mode, grid.z)
    "one job": ([(5, H, 64)], True, 1),
    "one generic job": ([(33, H, 63)], True, 1),
    "two chains of one width": ([(33, 2 * H, H)] * 2, True, 2),
    "four chains of one width": ([(64, H, H)] * 4, True, 4),
    "gates of different K, same width": ([(64, 2 * H, H + S.E), (64, 2 * H, H)], True, 2),
    "gates and candidates": ([(33, 2 * H, H), (33, H, H)], False, 1),
    "lstm cell beside a linear job of its width": ([(20, 4 * H, H, H), (20, 4 * H, H)], True, 2),
    "lstm cell beside its hidden width": ([(20, 4 * H, H, H), (20, H, H)], False, 1),
    "a narrow job between wide ones": ([(64, H, H), (64, 16, H), (64, H, H)], False, 1),
    "nine jobs": ([(64, H, H), (64, H, H), (64, H, H), (64, H, H), (64, 16, H), (64, 16, H), (64, H, H), (64, H, H),
                   (64, 16, H)], False, 1),
    "nine jobs of one width": ([(64, H, H)] * 9, True, 9),
    "one generic job keeps every job on one tile": ([(64, 2 * H, H), (64, H, 63)], False, 1),
    # the headline step's launches (h = 1024, B = 64): gates 64 x 2 x 2, candidates, the backward's X launch 32 x 2 x 4
    "cfg2 gates": ([(64, 2048, 1280), (64, 2048, 1024)], True, 2),
    "cfg2 candidates": ([(64, 1024, 1280), (64, 1024, 1024)], True, 2),
    "cfg2 backward X": ([(64, 1024, 1024)] * 4, True, 4),
}


@pytest.mark.parametrize("name", sorted(MODE_CASES))
def test_zmode_or_prefix(name):
    _lib()
    jobs, zmode, gz = MODE_CASES[name]
    got = S.launch_mode(jobs)
    assert got == S.expected_mode(jobs), name
    assert got["zmode"] == zmode and got["grid"][2] == gz, (name, got)
    ends = got["ends"]
    assert all(b > a for a, b in zip([0] + ends, ends)), (name, ends)  # every job owns at least one workgroup
    if zmode:
        assert got["grid"][0] == ends[0] and ends == [ends[0] * (q + 1) for q in range(len(jobs))]
    else:
        assert got["grid"][0] == ends[-1]
    if any(j[2] % 16 for j in jobs):
        assert got["nb"] == 1, (name, got)
    if name == "cfg2 gates":
        assert (got["mb"], got["nb"], got["grid"]) == (2, 2, (64, 2, 2))
    if name == "cfg2 backward X":
        assert (got["mb"], got["nb"], got["grid"]) == (2, 2, (32, 2, 4))


def test_query_rejects_bad_job_lists():
    L, lib = _lib()
    one = (C.c_int * 10)(*([16] * 10))
    info = (C.c_int * 16)()
    for n in (0, 10, -1):
        assert lib.parrot_step_launch_mode(n, one, one, one, None, info) == 10001
    assert lib.parrot_step_launch_mode(1, None, one, one, None, info) == 10001
    zero = (C.c_int * 1)(0)
    assert lib.parrot_step_launch_mode(1, zero, one, one, None, info) == 10001
    lstm = (C.c_int * 1)(5)  # N = 16 is not 4 * 5
    assert lib.parrot_step_launch_mode(1, one, one, one, lstm, info) == 10001
    assert lib.parrot_step_launch_mode(1, one, one, one, None, info) == 0 and info[0] == 1 and info[4] == 1


@pytest.mark.parametrize("B", S.BS)
@pytest.mark.parametrize("family", sorted(S.DECODER_PLANS))
def test_decoder_plans_make_the_launch_kinds(monkeypatch, family, B):
    """Dry-run plans of the GPU cases' descriptors: the schedule, and every launch kind the GPU case requires of its plan.
    dec_gru3: the K-balanced backward tick fills all nine slots of the table, in a plain and in a heterogeneous launch."""
    from tests.test_schedule_cpu import _make_plan
    L, lib = _lib()
    cell, nl, sched, accum, seq_init = S.DECODER_PLANS[family]
    for k in S.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    plan, _, _ = _make_plan(L, lib, sched, cell, nl, seq_init, monkeypatch, S.T, B, S.H, S.E, S.A, S.U, hetero=accum)
    try:
        assert int(lib.parrot_decoder_schedule(plan)) == S.DECODERS[family][2]
        found = S.plan_modes(plan)
        for kernel, zmode, njobs in S.DECODERS[family][3]:
            assert (kernel, zmode, njobs) in found, (family, B, (kernel, zmode, njobs), sorted(found))
        if family == "dec_gru3":
            assert int(lib.parrot_decoder_backward_tick(plan)) == 8
            assert max(n for _, _, n in found) == 9
        # both sides of every boundary of a prefix table hold workgroups of the launch: no job of a plan is empty
        for which in (0, 1):
            for jobs in S.plan_launches(plan, which).values():
                gemm = [(M, N, K, N // 4 if e == 4 else 0) for M, N, K, e in jobs if e >= 0]
                if gemm:
                    ends = S.launch_mode(gemm)["ends"]
                    assert all(b > a for a, b in zip([0] + ends, ends)), (family, gemm, ends)
    finally:
        lib.parrot_decoder_destroy(plan)

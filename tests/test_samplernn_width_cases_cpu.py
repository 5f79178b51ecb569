"""The premises of tests/test_gpu_samplernn_widths.py, checked without a GPU: the case table reaches all twelve
instantiations of the persistent sample kernel, its group counts are the library's, its (width, frame size) pairs are ones
srp_eligible takes, and its seeds condition the comparisons (the float32 oracle stays an order of magnitude under the
project's bar on the forced log-probabilities, and follows the float64 greedy run on all but one stream in 16)."""
import itertools

import numpy as np
import pytest
import torch

from tests import samplernn_forced_cases as FC
from tests import samplernn_groups_cases as GC
from tests import samplernn_width_cases as WC
from tests.test_gpu_samplernn import _greedy_follows_oracle


def _dry(B, max_groups):
    from parrot_amd import _lib
    return int(_lib.load().samplernn_persist_groups_dry(B, max_groups))


def test_cases_cover_all_twelve_instantiations():
    table = set(itertools.product(("plain", "fx"), (256, 512, 1024), (False, True)))
    assert len(table) == 12
    here = {WC.instantiation(c) for c in WC.CASES}
    assert here | set(WC.CREDITED) == table and here <= table
    # the eight at 512 and 1024 each have a case in this module; only D = 256 at FS = 10 is credited to the other modules
    assert {i for i in table if i[1] != 256} <= here
    assert all(i[1] == 256 for i in WC.CREDITED)
    for body, D, mg in sorted(table):
        n = sum(WC.instantiation(c) == (body, D, mg) for c in WC.CASES)
        print(f"WIDTHS-CPU srp{'_fx' if body == 'fx' else ''}_kernel<{D}, {str(mg).lower()}>: {n} cases here"
              + (f"; credited to {WC.CREDITED[body, D, mg][0]}" if (body, D, mg) in WC.CREDITED else ""))
    # every instantiation at 512 and 1024 meets a partial team and a full complement of teams
    for body, D in itertools.product(("plain", "fx"), (512, 1024)):
        assert {c.B for c in WC.CASES if (c.body, c.DIM) == (body, D)} == {5, 32, 33, 37}
    assert len(set(WC.CASES)) == len(WC.CASES) and len({WC.case_id(c) for c in WC.CASES}) == len(WC.CASES)


def test_case_shapes_are_the_edges():
    assert WC.WIDTHS == {256: 32, 512: 64, 1024: 256}
    assert WC.BATCHES == (5, 32, 33, 37) and WC.REF_B == max(WC.BATCHES) and WC.REF_T == 3
    assert 5 % 4 == 1 and 32 == GC.ROWS_PER_GROUP and 33 == GC.ROWS_PER_GROUP + 1
    assert 37 % 4 == 1 and 37 > GC.ROWS_PER_GROUP + 4          # a partial team behind a full one in group 1
    fs = {c.FS for c in WC.CASES if c.DIM == 256}
    assert fs == {2, 16} and all(c.body == "fx" and c.B in (5, 33) for c in WC.CASES if c.DIM == 256)
    assert 16 - 1 > 12 and 2 - 2 == 0                          # the loop gather (SRP_GMAX = 12); the clamp of a single early row
    for D, B, groups in WC.DRAW_SHAPES:
        assert (D, B, groups) in WC.shapes()
    assert {(s.DIM, s.groups) for s in WC.DRAW_SHAPES} == {(512, 1), (1024, 2)}


@pytest.mark.parametrize("case", WC.CASES, ids=WC.case_id)
def test_group_arithmetic(case):
    assert _dry(case.B, WC.MAX_GROUPS) == case.groups == GC.groups_for(case.B, WC.MAX_GROUPS)
    assert case.groups == (1 if case.B <= 32 else 2)
    assert _dry(case.B, 1) == (1 if case.B <= 32 else 0)       # without the switch a batch above 32 runs on launches


def test_every_case_is_eligible():
    for c in WC.CASES:
        assert WC.eligible(c.DIM, c.FS), c
        assert c.DIM in (256, 512, 1024) and 2 * c.FS <= 64 and 80 % c.FS == 0
        nsteps = c.FS                                          # one launch covers the FS steps between two frame-tier steps
        assert c.FS + nsteps <= 64                             # SRP_MAXHIST: srp_launch's own bound
    assert not WC.eligible(256, 3) and not WC.eligible(256, 40) and not WC.eligible(128, 10) and not WC.eligible(256, 0)


@pytest.mark.parametrize("DIM,FS", sorted({(c.DIM, c.FS) for c in WC.CASES}))
def test_forced_reference_is_conditioned(DIM, FS):
    """A condition on the inputs, not a measurement of the kernel: on these parameters, features and codes a float32
    evaluation of the oracle's own expression stays a factor ten under the bar the kernels are held to."""
    p, feats, forced, lp, lp32 = WC.forced_reference(DIM, FS)
    assert feats.shape == (WC.REF_T, WC.REF_B, 63) and forced.shape == (WC.REF_B, 80 * WC.REF_T)
    assert lp.shape == lp32.shape == (WC.REF_B, 80 * (WC.REF_T - 1)) and lp.dtype == np.float64 and lp32.dtype == np.float32
    assert p['FrameLevel.h0'].shape[-1] == DIM
    assert np.isfinite(lp).all() and (lp < 0).all()
    for c in WC.CASES:
        if (c.DIM, c.FS) != (DIM, FS) or c.body != "fx":
            continue
        e = WC.f32_oracle_error(c)
        print(f"WIDTHS-CPU forced {WC.case_id(c)}: float32 oracle against float64 {e:.3e}")
        assert 0 < e <= FC.PARITY_TOL / 10, (c, e)
        _, f, codes, want = WC.forced_case(c)
        assert f.shape == (WC.REF_T, c.B, 63) and codes.shape == (c.B, 240) and want.shape == (c.B, 160)


@pytest.mark.parametrize("DIM", [512, 1024])
def test_greedy_seeds_condition_the_gpu_cases(DIM):
    """The rule of tests/test_samplernn_groups_cpu.py::test_seeds_condition_the_gpu_cases: float32 throughout follows the
    float64 greedy run on all but at most one stream in 16 of every case, so the GPU test's allowance of one per started 16
    is not used up by the choice of seeds.  (How GREEDY_SEEDS were found: the first pairs tried that pass.)"""
    for c in WC.cases(body="plain", widths=(DIM,)):
        _, feats, ref, logits = WC.greedy_case(c)
        _, _, ref32, logits32 = WC.greedy_case(c, torch.float32)
        assert feats.shape == (3, c.B, 63) and ref.shape == (c.B, 240) and logits.shape == (c.B, 160, 256)
        exact = _greedy_follows_oracle(ref32, ref, logits, c.B, slack_rows=GC.f32_slack_rows(c.B))
        print(f"WIDTHS-CPU greedy {WC.case_id(c)}: float32 oracle rows identical {len(exact)} of {c.B}")
        assert float((logits32[exact, -1] - logits[exact, -1]).abs().max()) <= 1e-4 * float(logits[exact, -1].abs().max())
        assert len({ref[b].tobytes() for b in range(c.B)}) == c.B      # streams differ
    assert len(np.unique(WC.greedy_reference(DIM)[2][:, 80:])) > 20


def test_one_reference_serves_every_case():
    """Streams never meet: the forced pass over five streams of the middle is the slice (to the last bits of a float64:
    the host's products block the two batches differently)."""
    from oracle import samplernn_ref as S
    p, feats, forced, lp, _ = WC.forced_reference(512)
    c = S.config(DIM=512, EMB_SIZE=WC.WIDTHS[512])
    part = FC.log_probs({k: v.double() for k, v in p.items()}, c, forced[30:35], torch.from_numpy(feats[:, 30:35]).double())
    assert float(np.abs(part.numpy() - lp[30:35]).max()) <= 1e-12 * float(np.abs(lp).max())

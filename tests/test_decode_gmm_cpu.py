"""GMM-head decode on the persistent machine (PARROT_PM_GMM=1; plans_decode.hip gmm_eligible, persist.hip PM_SAMPLE), the
parts that need no GPU: the premise of the parity cases, and the LSTM program planned and replayed symbolically
(parrot_sample_plan_pieces_dry)."""
import ctypes as C

import pytest

from parrot_amd import _lib
from tests import decode_gmm_cases as G


@pytest.mark.parametrize("name", sorted(G.CASES))
def test_the_oracles_pick_is_no_coin_flip(name):
    """Conditions on the INPUTS of tests/test_gpu_decode_gmm.py, not tolerances on the decode: on the fp64 oracle's run no
    cumulative mixture weight lies within PICK_MARGIN = 1e-3 of the uniform number it is compared with, and the oracle's
    own float32 run stays within F32_MARGIN = 2e-5 of it (decode_gmm_cases: why the first alone is not enough).  The seeds
    in decode_gmm_cases.SEEDS are the first from 0 up (1000 up for the replay's second randomness) for which both hold; a
    case whose seed fails gets another seed."""
    c = G.case(name)
    K = c['cfg']['k_gmm']
    assert tuple(c['ref'][3].shape) == (G.S, c['N'], K)
    assert float(c['unif'].max()) < 1.0
    margin = G.pick_margin(c)
    err32 = G.f32_error(c)
    print(f"{name}: seed {G.SEEDS[name]}, margin {margin:.3e}, oracle float32 against float64 {err32:.3e}")
    assert margin >= G.PICK_MARGIN
    assert err32 <= G.F32_MARGIN


def _desc(L, K, B, H=256, E=128, R=256, S=50, O=63):
    d = _lib.SampleDesc()
    d.S, d.B, d.H, d.E, d.A, d.U, d.L, d.O, d.R, d.ldx = S, B, H, E, 10, 100, L, O, R, 64
    d.cell = 1
    fake = 0x7000_0000_0000  # never dereferenced by the dry run
    for l in range(L):
        d.Wg_t[l], d.bg[l] = fake, fake
    d.Wfg[0] = fake
    d.gmm_K = K
    d.rh_cols = (2 * O * K + K + 15) // 16 * 16
    d.Wrh_t, d.rh_const, d.x, d.unif, d.noise, d.pi_out = (fake,) * 6
    return d


def _plan(d, nwg):
    info = (C.c_int * 16)()
    rc = _lib.load().parrot_sample_plan_pieces_dry(C.byref(d), nwg, info)
    return rc, list(info)


def _places(d, nwg):
    return nwg * (1 if max(d.H // 4, d.B) <= nwg else 2)


@pytest.mark.parametrize("nwg", [256, 64])
@pytest.mark.parametrize("B", [5, 17, 64])
@pytest.mark.parametrize("K", [1, 3, 20])
@pytest.mark.parametrize("L", [1, 2, 3])
def test_lstm_gmm_plan_is_legal(monkeypatch, L, K, B, nwg):
    """L + 3 phases: layer 0, attention, layers 1 .. L-1, composed head (NH16 / 16 column tiles), sampling (one unit per
    batch row); the symbolic replay finds every read written in an earlier phase and nothing written twice.  A head with
    more tiles than places (workgroups x units per workgroup and phase) is not planned: K = 20 (159 tiles) on 64
    workgroups.  Without the switch nothing of this is planned."""
    d = _desc(L, K, B)
    tiles = d.rh_cols // 16
    monkeypatch.delenv("PARROT_PM_GMM", raising=False)
    rc, info = _plan(d, nwg)
    assert rc != 0 and info[2] == 0
    monkeypatch.setenv("PARROT_PM_GMM", "0")
    assert _plan(d, nwg)[0] != 0
    monkeypatch.setenv("PARROT_PM_GMM", "1")
    rc, info = _plan(d, nwg)
    if tiles > _places(d, nwg):
        assert (K, nwg) == (20, 64)
        assert rc != 0 and info[2] == 0
        return
    assert rc == 0, (rc, info)
    n = info[0]
    assert n == L + 3 and info[2] == 0
    assert sum(info[4:4 + n]) == info[3]
    assert info[4] == d.H // 4 and info[5] == B
    assert all(c == d.H // 4 for c in info[6:4 + n - 2])
    assert info[4 + n - 2] == tiles and info[4 + n - 1] == B


def test_head_tiles_beyond_the_places_are_not_planned(monkeypatch):
    """O = 63 on 64 workgroups with one unit per workgroup and phase: K = 8 is 64 tiles, K = 9 is 72."""
    monkeypatch.setenv("PARROT_PM_GMM", "1")
    rc, info = _plan(_desc(2, 8, 16), 64)
    assert rc == 0 and info[13] == 1 and info[4 + 3] == 64
    rc, info = _plan(_desc(2, 9, 16), 64)
    assert rc != 0 and info[2] == 0
    rc, info = _plan(_desc(2, 9, 16), 256)
    assert rc == 0 and info[4 + 3] == 72


def test_what_the_gmm_machine_does_not_take(monkeypatch):
    """More than 64 components, bf16 operands, layer_norm, a missing composed head or randomness: no plan."""
    monkeypatch.setenv("PARROT_PM_GMM", "1")
    for field, value in (("gmm_K", 65), ("bf16", 1), ("layer_norm", 1), ("Wrh_t", None), ("rh_const", None), ("unif", None),
                         ("noise", None), ("pi_out", None), ("rh_cols", 384 + 8), ("rh_cols", 368)):
        d = _desc(2, 3, 16)
        setattr(d, field, value)
        rc, info = _plan(d, 256)
        assert rc != 0 and info[2] == 0, field
    assert _plan(_desc(2, 3, 16), 256)[0] == 0


def test_three_layers_with_two_units_per_workgroup_fit_the_unit_table(monkeypatch):
    """L = 3 at a width with more layer tiles than workgroups: 6 phases x 2 units = the 12 entries of the table."""
    monkeypatch.setenv("PARROT_PM_GMM", "1")
    rc, info = _plan(_desc(3, 20, 16, H=1536, E=256, R=1536), 256)
    assert rc == 0 and info[0] == 6 and info[13] == 2 and info[2] == 0

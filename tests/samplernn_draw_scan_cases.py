"""Cases, tolerance and float32 restatement of the wave-parallel seeded draw (SampleRnnGenDesc::draw_mode = 1;
`srp_scan_draw` of sr_common.h as used by `sr_pick_kernel` in samplernn.hip and by the pick of `srp_kernel` in
sr_persist.hip; three_tier.DeviceGenerator(draw_mode='scan')).

The draw: terms e_q = expf((lg_q - max) / temperature); lane l of one 64-lane wave owns the n = Q / 64 contiguous codes
n l + j and sums them left to right (p_l); an inclusive Hillis-Steele scan with offsets 1, 2, 4, 8 inside each row of 16
lanes (w_l); the three row totals chained R_0 = T_0, R_1 = R_0 + T_1, R_2 = R_1 + T_2 and added to the rows behind them
(s_l); tot = s_63, u = u01 tot; l* = lowest lane with u < s_l (none: Q - 1); inside l* the terms are added one at a time
to s_{l*-1} (0 for lane 0) and the first code with u < c is the pick (none: the lane's last code).

The constructions (bias-only logits, patterns, uniforms, judging rules, shapes, seeds) are those of
tests/samplernn_sampling_cases.py.  This module imports no GPU code.  tests/test_samplernn_draw_scan_cpu.py checks its
premises; tests/test_gpu_samplernn_draw_scan.py runs the cases."""
import numpy as np

from tests import samplernn_sampling_cases as SC

Q, BFS, LANES = SC.Q, SC.BFS, 64

# The tolerance, by the argument at the top of samplernn_sampling_cases.py with the scan's depth in place of 256: a sum the
# draw compares u with has at most 10 + 4 float32 additions behind it -- 3 inside the lane, 4 of the row scan and 3 of the
# row chain for s_{l-1}, then up to 4 terms of the last lane -- so the ratio `u01 tot < c` tests is off by at most
# 2 (14 + 3) 2^-24 = 2.0e-6, and DELTA_SCAN is twice that, rounded up to a power of two: 2^-17 -- 8 times tighter than the
# sequential mode's DELTA.
SCAN_ADDS = 10 + 4
DELTA_SCAN = 2.0 ** -17
_bound = 2 * (SCAN_ADDS + 3) * 2.0 ** -24
assert abs(_bound / 2.0e-6 - 1) < 0.02
assert DELTA_SCAN / 2 < 2 * _bound <= DELTA_SCAN          # the smallest power of two that holds twice the bound
assert SC.DELTA == 8 * DELTA_SCAN

BIAS_SHAPES = SC.BIAS_SHAPES
TEMPERATURES, SEEDS, PATTERNS = SC.TEMPERATURES, SC.SEEDS, SC.PATTERNS


def scan_sums_f32(e):
    """s_l of the definition for terms e [Q] (float32): [64] float32.  Every addition is one rounded float32 addition."""
    e = np.asarray(e, dtype=np.float32)
    assert e.size % LANES == 0
    e = e.reshape(LANES, e.size // LANES)
    w = e[:, 0].copy()
    for j in range(1, e.shape[1]):
        w = (w + e[:, j]).astype(np.float32)
    lane = np.arange(LANES)
    for off in (1, 2, 4, 8):
        src = np.where(lane % 16 >= off, np.roll(w, off), np.float32(0))
        w = (w + src).astype(np.float32)
    r0 = w[15]
    r1 = np.float32(r0 + w[31])
    r2 = np.float32(r1 + w[47])
    s = w.copy()
    for k, r in ((1, r0), (2, r1), (3, r2)):
        s[16 * k:16 * k + 16] = (r + w[16 * k:16 * k + 16]).astype(np.float32)
    assert s.dtype == np.float32
    return s


def emulate_picks_scan_f32(logits, temperature, u):
    """The scan draw restated in numpy float32 for an array of uniforms against one logit vector.  (numpy's exp is not
    bit-equal to the device's expf, so this is a restatement, not a bit reference.)"""
    lg = np.asarray(logits, dtype=np.float32)
    e = np.exp((lg - lg.max()) / np.float32(temperature)).astype(np.float32)
    n = e.size // LANES
    s = scan_sums_f32(e)
    uu = (np.asarray(u).astype(np.float32) * s[-1]).astype(np.float32)
    out = np.empty(uu.shape, dtype=np.int32)
    for idx in np.ndindex(uu.shape):
        x = uu[idx]
        hit = np.nonzero(x < s)[0]
        if hit.size == 0:
            out[idx] = e.size - 1
            continue
        ls = int(hit[0])
        c = np.float32(0) if ls == 0 else s[ls - 1]
        pick = n * ls + n - 1
        for j in range(n):
            c = np.float32(c + e[n * ls + j])
            if x < c:
                pick = n * ls + j
                break
        out[idx] = pick
    return out


# ---- absorption: what the mode changes, and the proof that it reaches the kernel ---------------------------------------------
# Logit 0 at code 0, ABSORB_LOGIT everywhere else, temperature 1: every other term is e^-16.7 = 5.6e-8, below 2^-24, so the
# sequential walk's running sum 1 + 5.6e-8 rounds back to 1.0 at every step (tot = 1.0 exactly) and it picks code 0 for
# every u01 < 1; the tree adds the small terms to each other first and keeps them, as the float64 oracle does, which gives
# the other 255 codes 1.4e-5 of the mass.  The seeds were searched for: each holds one draw at B = 8, T = 3 whose oracle
# pick is not 0 (the CPU test checks that they still deliver).
ABSORB_LOGIT = -16.7
ABSORB_SHAPES = SC.EDGE_SHAPES           # launch-D32-B8, persist-D256-B8: B = 8, T = 3
ABSORB_SEEDS = (62, 63)
ABSORB_HITS = {62: (1, 78, 168), 63: (1, 57, 53)}   # seed: (stream, column, the oracle's pick)


def absorb_pattern():
    b = np.full(Q, ABSORB_LOGIT, dtype=np.float32)
    b[0] = 0.0
    return b


def absorb_hits(seed, T, B):
    """[(stream, column, oracle pick)] of the draws whose float64 pick is not code 0."""
    u = SC.u01_table(seed, T, B)
    want = SC.oracle_picks(absorb_pattern(), 1.0, u)
    return [(int(b), int(j), int(want[b, j])) for b, j in np.argwhere(want != 0)]

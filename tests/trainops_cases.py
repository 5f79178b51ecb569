"""The case tables of the edge tests of the SampleRNN training operators (parrot_amd/csrc/trainops.hip: gather-sum forward,
segmented-sum backward, softmax cross-entropy, ReLU gate, weight-norm fold and its backward) and of the audio quantisers
(parrot_amd/csrc/quantize.hip), their data, their float64 references and their error bounds.

A case is the smallest shape at which one branch of a kernel is live; its group names the branch.  Data is seeded from
the case's key.  The references are written from the contract in include/parrot_hip.h, take the float32-rounded operands
(what is measured is the kernel's arithmetic, not the rounding of its inputs) and compute in float64.

Gather-sum, segmented sum and the `wn-int` group hold small integers: any order of summation is exact in float32, so
the GPU result must be bit-equal to the reference.  For the float cases this module states, per kernel, the longest chain
of dependent roundings behind one result; the bound is 2 * chain * u (u = 2^-24), scaled as the functions below say.  The
factor 2 covers expf, logf, the division and sqrtf, which may be off by more than half an ulp on the device.

This module imports no GPU code.  tests/test_trainops_cases_cpu.py checks the premises of the tables;
tests/test_gpu_trainops_edges.py runs the cases."""
import zlib
from collections import namedtuple

import numpy as np
import torch

U = 2.0 ** -24
MAX_FLOATS = 400_000      # floats in one buffer of a case (the three quantiser clamp cases excepted)
GS_CH = 128               # sorted positions per block of the segmented sum's first pass
WN_KS, WN_RC = 16, 64     # row slices of the weight-norm column sums; rows per block of the scaling pass
Q_MINMAX_CLAMP = 64 * 256 * 8      # floats of a row that row_minmax_kernel's 64 blocks cover in 8 rounds
Q_QUANT_CLAMP = 256 * 256 * 4      # ... quantize_kernel's 256 blocks in 4 rounds
MU2LIN_CLAMP = 4096 * 256          # ... mu2linear_kernel's 4096 blocks in one round


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _ints(g, shape, lim=8):
    return torch.randint(-lim, lim + 1, shape, generator=g).float()


# ---- gather-sum forward -------------------------------------------------------------------------------------------------
# y and add are padded rows of a wider matrix in every case (ldy = D + 8, ldadd = D + 4); every shape with and without add.
FwdCase = namedtuple("FwdCase", "id group N J Q D has_add ldadd ldy")
FWD = {}


def rows_per_block(D):
    """Rows a 256-thread block of gs_fwd_kernel covers: 256 / (16-byte column groups of a row, at most 256)."""
    return 256 // min(D // 4, 256)


def _fwd(group, N, J, Q, D):
    for has_add in (1, 0):
        name = "%s-N%d-J%d-Q%d-D%d-%s" % (group, N, J, Q, D, "add" if has_add else "noadd")
        assert name not in FWD, name
        FWD[name] = FwdCase(name, group, N, J, Q, D, has_add, D + 4, D + 8)


# D/4 = 1; 3, 5 and 255 do not divide 256 (the last threads of a block idle); 256 groups; 257: a second column pass for
# one lane.  Two blocks and one row.
for _D in (4, 12, 20, 1020, 1024, 1028):
    _fwd("fwd-cols", 2 * rows_per_block(_D) + 1, 3, 5, _D)
# the four-in-flight loop: never entered (1, 2), with no tail (4, 8), with a tail (5, 9); the narrowest row
for _J in (1, 2, 4, 5, 8, 9):
    _fwd("fwd-J", 70, _J, 7, 36)
for _J in (1, 4, 8):
    _fwd("fwd-J", 40, _J, 3, 4)
# N below, at and above a block's rows (32 rows per block at D = 32; one at D = 1024)
for _N in (1, 31, 32, 33, 65):
    _fwd("fwd-rows", _N, 3, 6, 32)
_fwd("fwd-rows", 2, 2, 4, 1024)
_fwd("fwd-Q1", 40, 3, 1, 8)


def fwd_data(c):
    """tbl [J, Q, D], idx [N, J] (row 0 picks table row 0 at every j, the last row picks Q - 1), add [N, D]: integers in
    [-8, 8]."""
    g = _gen("gs-fwd", c.N, c.J, c.Q, c.D)
    tbl = _ints(g, (c.J, c.Q, c.D))
    idx = torch.randint(0, c.Q, (c.N, c.J), generator=g)
    idx[0, :] = 0
    if c.N >= 2:
        idx[-1, :] = c.Q - 1
    else:
        idx[0, 1::2] = c.Q - 1
    return dict(tbl=tbl, idx=idx, add=_ints(g, (c.N, c.D)))


def gather_sum_reference(tbl, idx, add=None):
    """y[i] = add[i] + sum_j tbl[j][idx[i, j]], float64."""
    N, J = idx.shape
    y = torch.zeros(N, tbl.shape[2], dtype=torch.float64) if add is None else add.double().clone()
    for j in range(J):
        y += tbl[j].double()[idx[:, j]]
    return y


# ---- segmented-sum backward ---------------------------------------------------------------------------------------------
# A case is a list of run lengths per position j (runs[j][q] rows pick table row q; 0 = an empty bin).  dy is a padded
# matrix (lddy = D + 4); every histogram with accumulate 0 and 1.
BwdCase = namedtuple("BwdCase", "id group runs N J Q D lddy accumulate")
BWD = {}


def _bwd(group, tag, runs, D):
    runs = tuple(tuple(r) for r in runs)
    N, Q = sum(runs[0]), len(runs[0])
    assert all(sum(r) == N and len(r) == Q for r in runs)
    for acc in (0, 1):
        name = "%s-%s-N%d-J%d-Q%d-D%d-%s" % (group, tag, N, len(runs), Q, D, "acc" if acc else "set")
        assert name not in BWD, name
        BWD[name] = BwdCase(name, group, runs, N, len(runs), Q, D, D + 4, acc)


def _sparse(Q, filled):
    return [filled.get(q, 0) for q in range(Q)]


# bin edges on the edges of the 128-position chunks, one past them, one before them
_bwd("bwd-aligned", "a", [(128, 256, 128, 0, 128), (256, 128, 0, 128, 128)], 8)
_bwd("bwd-shifted", "a", [(129, 128, 256, 128), (129, 256, 128, 128)], 8)
_bwd("bwd-before", "a", [(127, 128, 256, 129), (127, 256, 128, 129)], 8)
# the eight-in-flight loop: not entered (1, 2, 7), no tail (8, 16, 24), a tail of one (9, 17, 25)
_bwd("bwd-runs", "a", [(7, 8, 9, 16, 17, 1, 24, 2, 25), (25, 2, 24, 1, 17, 16, 9, 8, 7)], 12)
# N = Q, one row per bin: 128 runs in every chunk
_bwd("bwd-one-per-bin", "a", [(1,) * 256, (1,) * 256], 4)
_bwd("bwd-one-per-bin", "b", [(1,) * 128], 8)
# few bins used, the first and the last empty
_bwd("bwd-sparse", "a", [_sparse(64, {5: 3, 9: 130, 40: 200, 62: 1}), _sparse(64, {1: 1, 33: 300, 34: 33})], 8)
# one run over four chunks between short neighbours
_bwd("bwd-long", "a", [(3, 400, 2, 1), (1, 2, 400, 3)], 8)
# D above 1024: a second column pass, for one lane (1028) and for all (2048)
_bwd("bwd-D", "a", [(5, 0, 9), (9, 5, 0)], 1028)
_bwd("bwd-D", "b", [(3, 2)], 2048)
_bwd("bwd-Q1", "a", [(130,)], 8)
_bwd("bwd-Q1", "b", [(0, 1, 0)], 4)


def histogram(runs, *key):
    """idx [N, J]: at position j, runs[j][q] rows hold q; which rows is a seeded permutation per j."""
    N = sum(runs[0])
    idx = torch.empty(N, len(runs), dtype=torch.int64)
    for j, r in enumerate(runs):
        col = torch.repeat_interleave(torch.arange(len(r)), torch.tensor(r))
        idx[torch.randperm(N, generator=_gen("hist", j, *key)), j] = col
    return idx


def sort_bins(idx, Q):
    """(perm [J, N], offs [J, Q + 1]) int32 by the recipe of parrot_amd.ops._EmbedSumFn.backward: rows sorted by (index,
    row) per position (a stable sort), the first sorted position of every bin."""
    vals, perm = torch.sort(idx.to(torch.int32).t().contiguous(), dim=1, stable=True)
    bins = torch.arange(Q + 1, dtype=torch.int32).unsqueeze(0).expand(idx.shape[1], -1).contiguous()
    offs = torch.searchsorted(vals, bins).to(torch.int32).contiguous()
    return perm.to(torch.int32).contiguous(), offs


def bwd_data(c):
    """idx [N, J], perm, offs, dy [N, D] and the old dtbl [J, Q, D]: integers in [-8, 8]."""
    g = _gen("gs-bwd", c.runs, c.D)
    idx = histogram(c.runs, c.runs, c.D)
    perm, offs = sort_bins(idx, c.Q)
    return dict(idx=idx, perm=perm, offs=offs, dy=_ints(g, (c.N, c.D)), old=_ints(g, (c.J, c.Q, c.D)))


def segmented_sum_reference(idx, dy, Q, old=None):
    """dtbl[j][q] = (old +) sum of dy[i] over the rows with idx[i, j] == q, float64."""
    N, J = idx.shape
    out = torch.zeros(J, Q, dy.shape[1], dtype=torch.float64) if old is None else old.double().clone()
    for j in range(J):
        out[j].index_add_(0, idx[:, j], dy.double())
    return out


# ---- softmax cross-entropy ----------------------------------------------------------------------------------------------
CeCase = namedtuple("CeCase", "id group rows Q ld ldd")
CE = {}


def _ce(group, rows, Q, ld=None, ldd=None):
    name = "%s-R%d-Q%d" % (group, rows, Q)
    assert name not in CE, name
    CE[name] = CeCase(name, group, rows, Q, Q + 3 if ld is None else ld, Q + 5 if ldd is None else ldd)


# a lane's share of a row: nothing for most lanes (1, 2), one short of a wave, a wave, one more, ... four and a bit
for _Q in (1, 2, 63, 64, 65, 127, 129, 257):
    _ce("ce-Q", 17, _Q)
# four rows per block: one to four waves of a single block at work, a second block with one
for _R in (1, 2, 3, 4, 5):
    _ce("ce-rows", _R, 65)
_ce("ce-dense", 9, 256, 256, 256)   # the model's call: rows without padding

CE_ROWSCALES = (0.0, 1e-3, 1.0, -2.0)


def ce_data(c):
    """logits [rows, Q] float32, target [rows], rowscale [rows].  By row i: i % 8 = 0 is shifted by +80, 1 by -80, 2 has
    every other class 250 lower (those underflow to exact zeros), 3 has -inf at a third of the classes other than the
    target; the target is class 0, Q - 1, the argmax, the argmin for i % 4 = 0..3; rowscale runs through 0, 1e-3, 1, -2
    with a period of its own, so neighbouring rows differ by up to three orders of magnitude."""
    g = _gen("ce", c.rows, c.Q)
    x = (torch.randn(c.rows, c.Q, generator=g) * 4).float()
    t = torch.zeros(c.rows, dtype=torch.int64)
    for i in range(c.rows):
        kind = i % 8
        if kind == 0:
            x[i] += 80.0
        elif kind == 1:
            x[i] -= 80.0
        elif kind == 2:
            x[i, 1::2] -= 250.0
        t[i] = (0, c.Q - 1, int(x[i].argmax()), int(x[i].argmin()))[i % 4]
        if kind == 3:
            q = torch.arange(c.Q)
            x[i, (q % 3 == 0) & (q != t[i])] = float("-inf")
    rs = torch.tensor([CE_ROWSCALES[(i + i // 4) % 4] for i in range(c.rows)], dtype=torch.float32)
    return dict(x=x, target=t, rowscale=rs)


def ce_reference(x, target, rowscale):
    """lse = log sum exp, ce = lse - picked, p = softmax, dlogits = rowscale * (p - onehot); float64."""
    x = x.double()
    lse = torch.logsumexp(x, 1)
    ce = lse - x.gather(1, target[:, None])[:, 0]
    p = torch.exp(x - lse[:, None])
    onehot = torch.zeros_like(x).scatter_(1, target[:, None], 1.0)
    return dict(lse=lse, ce=ce, p=p, onehot=onehot, dlogits=rowscale.double()[:, None] * (p - onehot))


def ce_chain_length(Q):
    """Dependent roundings behind lse / ce of one row: a lane's share of the Q terms of the sum, the six steps of the wave
    reduction, expf, logf, and the two additions (log s + max, lse - picked)."""
    return -(-Q // 64) + 6 + 1 + 1 + 2


def ce_bound(c, ref):
    """Per row, for lse and for ce: 2 * chain * u * (1 + |lse| + |ce|)."""
    return 2.0 * ce_chain_length(c.Q) * U * (1.0 + ref["lse"].abs() + ref["ce"].abs())


def dlogits_bound(c, x, rowscale, ref):
    """Per element: |rowscale| * (p * (err_lse + u |x - lse| + 3u) + u + [q == target] u |1 - p|).  exp(x - lse) inherits
    the error of lse and of the rounded difference, relative to p; 3u: expf and the product; the u that follows is
    absolute (times |rowscale|): what is left where p underflows.  A class at -inf has p = 0 and no first term.

    The last term is a correction of the first derivation, which allowed one rounding, u, for the whole of
    `rowscale * (p - onehot)`.  At the target class the result is rowscale * (p - 1) with p possibly tiny, and two
    roundings act on a value of magnitude |1 - p|: the subtraction and the product, each up to u relative to it, so
    2u |1 - p| <= u + u |1 - p| is what the formula `g * (expf(x - l) - 1)` can cost; p's own terms do not cover it when
    p is small.  (Measured with rowscale = 1e-3f: 1.34 x the first bound on the device, and the same 1.34 from this
    formula evaluated in float32 on the host; the kernel computes what the header states.)"""
    d = (x.double() - ref["lse"][:, None]).abs()
    d = torch.where(torch.isinf(x), torch.zeros_like(d), d)
    return rowscale.double().abs()[:, None] * (ref["p"] * (ce_bound(c, ref)[:, None] + U * d + 3 * U) + U
                                               + ref["onehot"] * U * (1.0 - ref["p"]).abs())


# ---- ReLU gate ----------------------------------------------------------------------------------------------------------
RELU_N = (0, 4, 1020, 1024, 1028)    # nothing; one thread; one short of a block, a block, a block and one thread
DENORM_MIN = np.array([1], dtype=np.int32).view(np.float32)[0]
# gates at the head of the buffer (n = 4 sees the first four) and again at its tail
RELU_GATES = (0.0, -0.0, DENORM_MIN, np.nan, np.inf, -np.inf, -DENORM_MIN, -1.0, 1.0)


def relu_data(n):
    """(dy, gate) float32 numpy arrays.  Where a special gate is closed, dy is NaN, +inf or -inf in turn."""
    rng = np.random.RandomState(zlib.crc32(repr(("relu", n)).encode()))
    dy, gate = rng.randn(n).astype(np.float32), rng.randn(n).astype(np.float32)
    k = min(n, len(RELU_GATES))
    for at in ((0, n - k) if n else ()):
        gate[at:at + k] = np.array(RELU_GATES[:k], dtype=np.float32)
        for i in range(k):
            if not gate[at + i] > 0:
                dy[at + i] = (np.nan, np.inf, -np.inf)[i % 3]
    return dy, gate


def relu_reference(dy, gate):
    """dy where gate > 0 (an IEEE comparison: the smallest denormal is open, NaN and -0.0 are closed), else +0.0."""
    with np.errstate(invalid="ignore"):
        return np.where(gate > 0, dy, np.float32(0.0)).astype(np.float32)


# ---- weight-norm fold ---------------------------------------------------------------------------------------------------
# Every leading dimension exceeds N (W: N + 3, W_eff: N + 5, dW_eff: N + 2, dW: N + 7).
WnCase = namedtuple("WnCase", "id group K N ld ldo ldd lddw kind")
WN = {}


def _wn(group, K, N, kind="float"):
    name = "%s-K%d-N%d" % (group, K, N)
    assert name not in WN, name
    WN[name] = WnCase(name, group, K, N, N + 3, N + 5, N + 2, N + 7, kind)


def wn_slice_rows(K):
    """Rows of one of the WN_KS slices of wn_colsum_kernel."""
    return -(-K // WN_KS)


def wn_unrolled_rounds(K):
    """Rounds of the 16-row unrolled loop that wave 0 runs on a full slice (`for (; k + 12 < k1; k += 16)`)."""
    return max(0, -(-(wn_slice_rows(K) - 12) // 16))


# K below, at and above 4 (one row per wave), 16 (one row per slice: K = 1 and 17 leave slices that start past K) and 64
# (a second block of the scaling pass); the unrolled loop with one round (208, 448) and several (529: slices of 34 rows,
# the last one of 19)
for _K in (1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 208, 448, 529):
    _wn("wn-K", _K, 65)
# one column; one short of a column block (with K short of a chunk); two blocks and two lanes
for _K, _N in ((70, 1), (63, 63), (70, 64), (70, 130)):
    _wn("wn-N", _K, _N)
for _K, _N in ((1, 5), (2, 65), (4, 65), (17, 63), (65, 130), (529, 65)):
    _wn("wn-int", _K, _N, "int")

WN_ACC_CASES = ("wn-K-K65-N65", "wn-int-K17-N63")   # run with the four combinations of accumulate_w and accumulate_g


def wn_is_square_column(N):
    """Columns of a `wn-int` case whose sum of squares is a perfect square."""
    return torch.arange(N) % 3 == 0


def wn_data(c):
    """W, dW_eff, old dW [K, N]; g, old dg [N].
    int: integers in [-8, 8]; every third column is zero except for the entries (2, 3, 6), (3, 4) or one value, whose
    squares sum to a perfect square; no column is zero; g has no zero.
    float: the column norms and |g| are 10^uniform(-3, 3) with both ends present in the same matrix (column 0 has norm
    1e-3 and g = 1e3, the last column the reverse), g of either sign."""
    g = _gen("wn", c.K, c.N, c.kind)
    K, N = c.K, c.N
    if c.kind == "int":
        W = _ints(g, (K, N))
        W[0, W.abs().sum(0) == 0] = 1.0
        pattern = (2.0, 3.0, 6.0) if K >= 3 else ((3.0, 4.0) if K == 2 else (5.0,))
        for n in torch.nonzero(wn_is_square_column(N))[:, 0].tolist():
            W[:, n] = 0.0
            at = torch.randperm(K, generator=g)[:len(pattern)]
            W[at, n] = torch.tensor(pattern) * (1.0 if n % 2 else -1.0)
        gg = _ints(g, (N,))
        gg[gg == 0] = 1.0
        return dict(W=W, g=gg, dWe=_ints(g, (K, N)), old_dW=_ints(g, (K, N)), old_dg=_ints(g, (N,)))
    norms = 10.0 ** (torch.rand(N, generator=g, dtype=torch.float64) * 6 - 3)
    gs = 10.0 ** (torch.rand(N, generator=g, dtype=torch.float64) * 6 - 3)
    gs = gs * (torch.randint(0, 2, (N,), generator=g) * 2 - 1)
    norms[0], gs[0] = 1e-3, 1e3
    if N > 1:
        norms[-1], gs[-1] = 1e3, -1e-3
    W = torch.randn(K, N, generator=g, dtype=torch.float64)
    W = W / W.norm(dim=0) * norms
    return dict(W=W.float(), g=gs.float(), dWe=torch.randn(K, N, generator=g), old_dW=torch.randn(K, N, generator=g),
                old_dg=torch.randn(N, generator=g))


def wn_reference(W, g, dWe):
    """The header's contract in float64: norm, W_eff, dot = sum_k dW_eff W, dg = dot / norm,
    dW = g / norm * (dW_eff - W dot / norm^2); absdot = sum_k |dW_eff W| (what the dot's error scales with)."""
    W, g, dWe = W.double(), g.double(), dWe.double()
    ss = (W * W).sum(0)
    norm = ss.sqrt()
    dot = (dWe * W).sum(0)
    return dict(ss=ss, norm=norm, W_eff=W * (g / norm), dot=dot, absdot=(dWe * W).abs().sum(0), dg=dot / norm,
                dW=(g / norm) * (dWe - W * (dot / (norm * norm))))


def wn_chain_length(K):
    """Dependent roundings behind one column sum (of squares, or of dW_eff W): a wave's share of a slice (one fused
    multiply-add per row), the two additions that join a wave's four accumulators, the two that join the four waves, and
    the WN_KS additions over the slices."""
    return -(-wn_slice_rows(K) // 4) + 2 + 2 + WN_KS


def wn_bounds(c, W, g, dWe, ref, old_dW=None, old_dg=None):
    """Bounds on |kernel - reference| with r = 2u per rounding:
      sum of squares  relative  e_ss = chain * r (all terms positive)
      norm            relative  e_n = e_ss / 2 + r                       (sqrtf)
      W_eff           relative  e_n + 2r                                 (g / norm, the product)
      dot             absolute  E_dot = chain * r * sum_k |dW_eff W|     (the terms cancel)
      dg              E_dot / norm + |dg| (e_n + r)                      (the kernel divides by its own norm)
      q = dot / norm^2:  E_q = E_dot / norm^2 + |q| (2 e_n + 2r)         (norm * norm, the division)
      t = dW_eff - W q:  E_t = |W| E_q + r |W q| + r |t|                 (the product, the subtraction)
      dW = g / norm * t: |g / norm| E_t + |dW| (e_n + 2r)                (g / norm, the product)
    and one more rounding of the result where a call accumulates."""
    r = 2.0 * U
    W, g, dWe = W.double(), g.double(), dWe.double()
    e_ss = wn_chain_length(c.K) * r
    e_n = e_ss / 2 + r
    norm = ref["norm"]
    E_dot = wn_chain_length(c.K) * r * ref["absdot"]
    q = ref["dot"] / (norm * norm)
    E_q = E_dot / (norm * norm) + q.abs() * (2 * e_n + 2 * r)
    t = dWe - W * q
    E_t = W.abs() * E_q + r * (W * q).abs() + r * t.abs()
    b = dict(norm=norm * e_n, W_eff=ref["W_eff"].abs() * (e_n + 2 * r), dg=E_dot / norm + ref["dg"].abs() * (e_n + r),
             dW=(g / norm).abs() * E_t + ref["dW"].abs() * (e_n + 2 * r))
    if old_dg is not None:
        b["dg"] = b["dg"] + r * (old_dg.double() + ref["dg"]).abs()
    if old_dW is not None:
        b["dW"] = b["dW"] + r * (old_dW.double() + ref["dW"]).abs()
    return b


# ---- quantisers ---------------------------------------------------------------------------------------------------------
# Rows of x and of the classes are padded (ld = n + 7, ldo = n + 3: an odd leading dimension of the int16 output where
# n is even).  In a clamp case the row minimum sits at n - 1 and the maximum at n - 2: in the tail that only the last
# round of the strided loops reads.
QuantCase = namedtuple("QuantCase", "id group rows n ld ldo")
QUANT = {}
QUANT_CLAMP_GROUPS = ("q-clamp-minmax", "q-clamp-quantize", "q-clamp-mu2linear")


def _quant(group, rows, n):
    name = "%s-R%d-n%d" % (group, rows, n)
    assert name not in QUANT, name
    QUANT[name] = QuantCase(name, group, rows, n, n + 7, n + 3)


_quant("q-rows", 5, 334)       # a plain row, an entirely negative one, a constant one, a positive one, a plain one
_quant("q-rows", 3, 2)         # rows of two samples
_quant("q-clamp-minmax", 2, Q_MINMAX_CLAMP + 300)
_quant("q-clamp-quantize", 1, Q_QUANT_CLAMP + 300)
_quant("q-clamp-mu2linear", 1, MU2LIN_CLAMP + 300)   # (its classes are what mu2linear expands)


def quant_constant_rows(c):
    return (2,) if c.rows >= 5 else ()


def quant_data(c):
    """x [rows, n] float32 numpy."""
    rng = np.random.RandomState(zlib.crc32(repr(("quant", c.rows, c.n)).encode()))
    if c.n == 2:
        return np.array([[0.25, -3.0], [7.0, 2.0], [-1.0, -5.0]], dtype=np.float32)
    x = (rng.randn(c.rows, c.n) * 0.3).astype(np.float32)
    if c.group == "q-rows":
        x[1] = -np.abs(x[1]) - 0.5
        x[2] = 0.375
        x[3] = np.abs(x[3]) + 0.5
    else:
        x[:, -1] = x.min(1) - 1.0
        x[:, -2] = x.max(1) + 1.0
    return x

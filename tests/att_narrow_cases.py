"""Cases of the attention backward row block's two paths (att_bwd_body.h): narrow -- the saved support is present, inside
the text and at most CAP = 64 rows wide, U <= 256, E <= 256: only the support's context rows are fetched and reduced --
and wide, everything else.

One-step cases (STEP_CASES): every batch row places its window exactly.  The recipe is the one of
test_attention_window_placements (tests/test_gpu_kernels.py, _place_windows), generalised from "only u = 0 survives" to
"the support is exactly [lo, hi]": exp(-x) is exactly 0.0f for x > 104, so a mixture of effective width b' whose centre
lies sqrt(110 / b') to the RIGHT of position lo - 1 is exactly zero on lo - 1 (x = 110) and everything left of it, and
alive on lo (x < 80 for b' > 2.4) and a dozen positions to its right; the first half of a row's mixtures is placed like
that at lo, the second half mirrored at hi.  The support the forward step saves is the first / last position of non-zero
phi: (lo, hi), whatever lies between.  Texts of U = 200 reach supports of CAP and CAP + 1 rows this way with the narrow
windows of the placement test (beta_hat + 3).

Every row states the route it expects; tests/test_att_narrow_cpu.py checks the placement from the fp64 oracle alone and
the route from the library's host-side query, tests/test_gpu_att_narrow.py runs the kernels.  The fp64 reference of a
case is computed once per process and shared, unchanged."""
import functools

import torch

from tests import attention_cases as AC
from tests.test_gpu_kernels import ATT_ALIGN, ATT_EPS, ATT_SHARP, ATT_TIMING, _att_inputs, _att_reference
from tests.util import make_batch

CAP = 64
WIDE, NARROW = 0, 1
ALIVE, DEAD, EMPTY = 1e-40, 5e-46, 1e-60  # fp64 phi: surely non-zero in f32 / surely 0.0f (as the placement test) / empty row

# name: ((B, H, A, U, E), rows); row = (lo, hi, route) for the support [lo, hi], ("past" | "before", route) for an empty one
STEP_CASES = {
    "U23": ((8, 64, 10, 23, 32), [
        (3, 19, NARROW),            # the middle of the text
        ("past", WIDE),             # empty support (U, -1): past the text
        ("before", WIDE),           # ... and before it
        (0, 0, NARROW),             # one position, u = 0
        (22, 22, NARROW),           # one position, u = U - 1
        (0, 22, NARROW),            # the whole text
        (0, 14, NARROW),            # touches u = 0
        (7, 22, NARROW),            # touches u = U - 1, U no multiple of 16: 16 rows, one per wave
    ]),
    "U200": ((8, 64, 10, 200, 256), [
        (90, 110, NARROW),          # the middle of the text
        ("past", WIDE),
        ("before", WIDE),
        (0, 0, NARROW),
        (199, 199, NARROW),
        # (the two widest rows start near u = 0: kappa - u loses log2(kappa) bits in f32 and b (kappa - u)^2 amplifies the
        # loss, so at (70, 133) the reference's own formulas in float32 already miss the forward bound on phi, 2.6e-5
        # against 2e-5; tests/test_att_narrow_cpu.py holds every case's float32 evaluation below 0.6 of each bound)
        (2, 2 + CAP - 1, NARROW),   # exactly CAP rows: four per wave
        (2, 2 + CAP, WIDE),         # CAP + 1 rows
        (170, 199, NARROW),         # touches u = U - 1, U no multiple of 16; a ragged last round of the waves
    ]),
    "U257": ((4, 64, 10, 257, 32), [(10, 30, WIDE), (0, 0, WIDE), (40, 60, WIDE), ("past", WIDE)]),   # no preload: U > 256
    "E260": ((4, 64, 10, 64, 260), [(0, 30, WIDE), (10, 40, WIDE), (0, 0, WIDE), ("past", WIDE)]),    # no preload: E > 256
    # narrow context rows, but H > 1024: no Watt column preload, dh1 through the fallback loop
    "H1100": ((4, 1100, 10, 40, 64), [(5, 30, NARROW), (0, 0, NARROW), (20, 39, NARROW), ("before", WIDE)]),
}
ATT_TYPES = ("graves", "softmax")


def claimed_support(row, U):
    """(u_lo, u_hi) the forward step must save for the row; the empty support is (U, -1)."""
    return (U, -1) if isinstance(row[0], str) else (row[0], row[1])


def place(att_type, x, U, rows):
    """kappa_prev [B, A] (float32) that puts every row's support where `rows` says (inputs only, fp64)."""
    B, A = x['kprev'].shape
    assert len(rows) == B
    p = x['h1'].double().cpu() @ x['Watt'].double().cpu() + x['batt'].double().cpu()
    step = ATT_ALIGN * torch.exp(p[:, 2 * A:]) / ATT_TIMING
    beff = (torch.exp(p[:, A:2 * A]) * ATT_SHARP + ATT_EPS) * (0.5 if att_type == "softmax" else 1.0)
    reach = torch.sqrt(110.0 / beff)
    k = torch.empty((B, A), dtype=torch.float64)
    h = A // 2
    for i, row in enumerate(rows):
        if row[0] == "past":
            kappa = torch.full((A,), U + 15.0, dtype=torch.float64)
        elif row[0] == "before":
            kappa = torch.full((A,), -15.0, dtype=torch.float64)
        else:
            lo, hi = row[0], row[1]
            assert 0 <= lo <= hi < U
            if lo == hi:
                assert lo in (0, U - 1), "a single position survives only at an edge of the text"
                kappa = (lo + 1) - reach[i] if lo == 0 else (hi - 1) + reach[i]
            else:
                kappa = torch.cat([(lo - 1) + reach[i, :h], (hi + 1) - reach[i, h:]])
        k[i] = kappa - step[i]
    return k.float()


@functools.lru_cache(maxsize=None)
def step_case(name, att_type):
    """(x, ref): CPU inputs of the case (float32, as _att_inputs with narrow windows and the placed kappa_prev) and the fp64
    reference of _att_reference.  Shared between tests: nothing in it may be modified."""
    (B, H, A, U, E), rows = STEP_CASES[name]
    x = _att_inputs("cpu", B, H, A, U, E)
    x['batt'] = x['batt'].clone()
    x['batt'][A:2 * A] += 3.0
    x['kprev'] = place(att_type, x, U, rows)
    return x, _att_reference(att_type, x)


# ---- whole training steps on the SMALL model: 2 layers, T <= 14, B <= 5 -----------------------------------------------
# name: (model kwargs, T, B, U, fork_kappa.b)
MODEL_CASES = {
    # kappa advances e^0.5 positions per frame: the windows stay inside the text, every support is a few rows of U = 40
    "IN": (dict(num_layers=2, weak_feedback=True), 12, 4, 40, 0.5),
    # attention_cases.P1: the windows start on the first positions of a short text and leave it within a few frames
    "OUT": AC.CASES["P1"],
    # attention_cases.P2W with bf16 operands under PARROT_WK=2: schedule 7, the backward tick is wkb_kernel
    "OUT_WKB": AC.CASES["P2W"],
}


def model_kwargs(name):
    return dict(AC.SMALL, **MODEL_CASES[name][0])


def model_overrides(name):
    return {AC.KAPPA_BIAS: MODEL_CASES[name][4]}


@functools.lru_cache(maxsize=None)
def model_oracle(name):
    """fp64 oracle of a model case, as attention_cases.oracle (which serves the two cases taken from there)."""
    if name == "OUT":
        return AC.oracle("P1")
    if name == "OUT_WKB":
        return AC.oracle("P2W")
    from oracle import parrot_ref as R
    kw, T, B, U, bias = MODEL_CASES[name]
    cfg = R.default_config(**dict(AC.SMALL, **kw))
    p = R.init_params(cfg, seed=7, scale_by_fan_in=True, dtype=torch.float64)
    p[AC.KAPPA_BIAS].fill_(bias)
    batch = make_batch(cfg, T, B, U, seed=3, ragged=True, dtype=torch.float64, speaker=cfg['use_speaker'])
    for v in p.values():
        v.requires_grad_()
    cost, _, av, _ = R.compute_cost(p, cfg, *batch, 1)
    cost.backward()
    grads = {k: v.grad.detach() for k, v in p.items() if v.grad is not None}
    return dict(cfg=cfg, params={k: v.detach() for k, v in p.items()}, batch=batch, cost=cost.detach(),
                av=[x.detach() for x in av], grads=grads)


def oracle_supports(phi):
    """Per (t, b) row of the oracle's phi [T, B, U]: (lo, hi) bounding every position that can be non-zero in f32 (fp64
    phi >= DEAD), or None for a row that is exactly zero in f32 (maximum below DEAD)."""
    phi = torch.as_tensor(phi).detach().double().cpu()
    out = []
    for row in phi.reshape(-1, phi.shape[-1]):
        if float(row.max()) < DEAD:
            out.append(None)
            continue
        idx = torch.nonzero(row >= DEAD).flatten()
        out.append((int(idx[0]), int(idx[-1])))
    return out

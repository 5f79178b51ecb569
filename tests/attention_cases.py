"""Model-level cases that drive the attention window to its edges and past the text.

`fork_kappa.b` is raised so that kappa advances e (bias 1.0) or e^1.5 (bias 1.5) positions per frame and more: on the
short ragged texts of P1-P4 the window leaves the context within a few frames, exp(-b (kappa - u)^2) underflows to
exactly 0.0f for every position, and the forward step saves the empty support (U, -1).  W1 / W2 keep the window inside a
long text (U = 260 / 520) and cross the thresholds on U of the forward kernels instead.

The fp64 oracle of each case (outputs and every gradient) is computed once per process and shared, unchanged, by
tests/test_attention_edges_cpu.py (the premises) and tests/test_gpu_attention_edges.py (the parity runs)."""
import functools

import torch

from tests.util import make_batch

SMALL = dict(rnn_h_dim=64, readouts_dim=48, encoder_dim=16, input_dim=24, speaker_dim=8, num_speakers=5,
             encoder_type='bidirectional')
KAPPA_BIAS = '/parrot/h1_to_att/fork_kappa.b'
EMPTY_BELOW = 1e-60  # fp64 phi maximum of a (t, b) row below which the f32 window is exactly zero everywhere
LIVE_ABOVE = 1e-30

CASES = {
    # name: (model kwargs, T, B, U, fork_kappa.b)
    "P1": (dict(num_layers=2, weak_feedback=True), 14, 5, 9, 1.0),
    "P2": (dict(num_layers=2, weak_feedback=True, cell_type='lstm'), 14, 5, 9, 1.0),
    "P3": (dict(num_layers=3, full_feedback=True, use_speaker=True), 12, 37, 11, 1.5),
    "P4": (dict(num_layers=2, weak_feedback=True, attention_type='softmax'), 14, 5, 9, 1.0),
    "W1": (dict(num_layers=1), 10, 3, 260, 1.0),
    "W2": (dict(num_layers=2), 6, 3, 520, 1.0),
    # W1 with a second layer: a one-layer decoder has no upper layers to carry the attention beside, so schedule 5
    # resolves to 0 for W1 and only this case runs U = 260 in the 512-thread block of ska_kernel
    "W3": (dict(num_layers=2), 10, 3, 260, 1.0),
    # P2 at the narrowest widths the wide bf16 step kernel takes (H and E multiples of 64): the only way to wkb_kernel,
    # the fused backward tick of schedule 7 with bf16 operands
    "P2W": (dict(num_layers=2, weak_feedback=True, cell_type='lstm', encoder_dim=32), 14, 5, 9, 1.0),
}
EDGE_CASES = ("P1", "P2", "P3", "P4", "P2W")
WIDE_CASES = ("W1", "W2", "W3")


def model_kwargs(name):
    return dict(SMALL, **CASES[name][0])


def overrides(name):
    """Parameter overrides of the case: name -> fill value."""
    return {KAPPA_BIAS: CASES[name][4]}


def shape(name):
    return CASES[name][1:4]


def build(name, dtype=torch.float64):
    """(cfg, params, batch) of a case: init_params(seed=7) with the override applied, make_batch(seed=3, ragged)."""
    from oracle import parrot_ref as R
    kw, T, B, U, _ = CASES[name]
    cfg = R.default_config(**dict(SMALL, **kw))
    p = R.init_params(cfg, seed=7, scale_by_fan_in=True, dtype=dtype)
    for k, v in overrides(name).items():
        p[k].fill_(v)
    batch = make_batch(cfg, T, B, U, seed=3, ragged=True, dtype=dtype, speaker=cfg['use_speaker'])
    return cfg, p, batch


def row_max(phi):
    """[T, B] maximum of phi over the context positions."""
    return torch.as_tensor(phi).detach().double().cpu().amax(-1)


def count_empty(phi):
    return int((row_max(phi) < EMPTY_BELOW).sum())


@functools.lru_cache(maxsize=None)
def oracle(name):
    """fp64 oracle of a case: dict(cfg, params, batch, cost, av = attention_vars, grads = name -> gradient).
    Shared between tests: nothing in it may be modified."""
    from oracle import parrot_ref as R
    cfg, p, batch = build(name)
    for v in p.values():
        v.requires_grad_()
    cost, _, av, _ = R.compute_cost(p, cfg, *batch, 1)
    cost.backward()
    grads = {k: v.grad.detach() for k, v in p.items() if v.grad is not None}
    return dict(cfg=cfg, params={k: v.detach() for k, v in p.items()}, batch=batch, cost=cost.detach(),
                av=[x.detach() for x in av], grads=grads)

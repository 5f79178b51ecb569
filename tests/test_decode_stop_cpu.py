"""The end-of-utterance stop of the decode machine, as far as it can be checked without a GPU: the per-row arguments built
from labels_mask plus the rule the kernel applies (emulated in numpy, operation for operation) give exactly what
end_of_utterance gives on the same phi; the CLI switch; the refusals and their reasons."""
import numpy
import pytest

from parrot_amd.utils import end_of_utterance, end_of_utterance_args, sample_parse

U, S, EXTRA = 9, 40, 8


def device_rule(phi, pos, ncmp, S, extra):
    """What pm_att_row + the host do for one row: first step t with phi[t, pos] > phi[t, j] for all j < ncmp (strict; a NaN
    compares false; no j: true), then min(S, first + extra); S if no step fires."""
    for t in range(phi.shape[0]):
        holds = True
        for j in range(ncmp):
            holds = holds and bool(phi[t, pos] > phi[t, j])
        if holds:
            return min(S, t + extra)
    return S


def _mask(ll):
    m = numpy.zeros((1, U), dtype=numpy.float32)
    m[0, :ll] = 1
    return m


@pytest.mark.parametrize("ll", [0, 1, 2, U - 1, U])
def test_argument_builder_follows_the_python_slices(ll):
    pos, ncmp = end_of_utterance_args(_mask(ll), U)
    assert pos.dtype == numpy.int32 and ncmp.dtype == numpy.int32
    assert int(pos[0]) == min(ll, U - 1)
    # phi[:, :pos - 1]: pos = 0 -> [:-1] = all but the last position; pos = 1 -> [:0] = nothing to beat
    assert int(ncmp[0]) == numpy.zeros((1, U))[:, :int(pos[0]) - 1].shape[1]


@pytest.mark.parametrize("ll", [0, 1, 2, U - 1, U])
@pytest.mark.parametrize("kind", ["random", "peaked", "never", "nan"])
def test_device_rule_equals_end_of_utterance(ll, kind):
    rng = numpy.random.RandomState(100 * ll + len(kind))
    phi = rng.rand(S, U).astype(numpy.float32)
    pos = min(ll, U - 1)
    if kind == "peaked":   # the weight moves onto `pos` from step 11 on
        phi[11:, pos] += 2.0
    elif kind == "never":  # position 0 always wins (pos = 0 compares with itself: strict, never)
        phi[:, 0] = 3.0
        phi[:, pos] = min(phi[:, pos].min(), 0.5) if pos else 3.0
    elif kind == "nan":    # NaNs at the steps that would have fired first, on either side of the comparison
        phi[11:, pos] += 2.0
        phi[11, pos] = numpy.nan
        phi[12, 0] = numpy.nan
    p, n = end_of_utterance_args(_mask(ll), U)
    got = device_rule(phi, int(p[0]), int(n[0]), S, EXTRA)
    assert got == end_of_utterance(phi, pos, S, EXTRA)
    if kind == "never" and ll != 1:
        assert got == S
    if ll == 1:  # nothing to beat: fires at step 0, NaN or not
        assert got == EXTRA
    if kind == "peaked" and ll not in (0, 1):
        assert got <= 11 + EXTRA
    if kind == "nan" and ll not in (0, 1):  # neither NaN step may be the one that fires
        assert got not in (11 + EXTRA, 12 + EXTRA)


def test_a_row_of_nans_never_fires():
    phi = numpy.full((S, U), numpy.nan, dtype=numpy.float32)
    p, n = end_of_utterance_args(_mask(5), U)
    assert device_rule(phi, int(p[0]), int(n[0]), S, EXTRA) == S == end_of_utterance(phi, 5, S, EXTRA)


def test_batch_of_masks():
    m = numpy.concatenate([_mask(ll) for ll in (0, 1, 2, U - 1, U)])
    pos, ncmp = end_of_utterance_args(m, U)
    assert pos.tolist() == [0, 1, 2, U - 1, U - 1]
    assert ncmp.tolist() == [U - 1, 0, 1, U - 2, U - 2]


def test_stop_at_end_parses_and_defaults_to_off():
    assert sample_parse([]).stop_at_end == 0
    assert sample_parse(['--stop_at_end', '1']).stop_at_end == 1


def test_refusals_name_their_reason_without_a_gpu(monkeypatch):
    from parrot_amd.model import Parrot
    kw = dict(rnn_h_dim=64, readouts_dim=48, encoder_dim=16, input_dim=24, num_layers=2, encoder_type='bidirectional',
              device='cpu')
    assert Parrot(**kw)._decode_stop_refusal(16, 8) == ''
    assert Parrot(cell_type='lstm', **kw)._decode_stop_refusal(64, 40) == ''
    cases = [(Parrot(which_cost='GMM', **kw), 16, 8, 'GMM'), (Parrot(layer_norm=True, **kw), 16, 8, 'layer_norm'),
             (Parrot(**kw), 16, 7, 'extra >= 8'), (Parrot(**kw), 16, 0, 'extra >= 8'), (Parrot(**kw), 65, 8, '64')]
    for m, N, extra, word in cases:
        assert word in m._decode_stop_refusal(N, extra)
        with pytest.raises(ValueError, match=word):  # raised before anything is allocated or the library is loaded
            m.sample_until_end_device(numpy.zeros((N, U), dtype=numpy.int64), numpy.ones((N, U), dtype=numpy.float32), None,
                                      N, 48, extra=extra)
        assert not m._sample_ws and not m._allocated
    monkeypatch.setenv('PARROT_SAMPLE_PERSIST', '0')
    assert 'PARROT_SAMPLE_PERSIST' in Parrot(**kw)._decode_stop_refusal(16, 8)

"""CPU: the float64 restatement of the ConvLSTM BPTT in the persistent kernel's form (tests/lstm_bptt_ref.py) against
float64 autograd, and the five mutation probes: each wrong version of the recurrence must move at least one of d_i .. d_o
by more than 1e-2 relative Frobenius -- the order of a bf16 plan's own distance to float64 -- so that the comparisons of
tests/test_lstm_bptt_gpu.py can see it."""
import numpy as np
import pytest

import lstm_bptt_ref as bref
import lstm_ref as ref
from recurrent_gaze_prediction_amd import synthetic as syn

SHAPES = [(2, 3), (2, 6)]
_CASE = {}


def case(B, T):
    """Inputs, saved state, dh_head, the clean d_i .. d_o and autograd's gradients: computed once, never modified."""
    if (B, T) not in _CASE:
        p = syn.lstm_params(41)
        x = syn.c3d_features(42 + T, B, T)
        gt, _ = syn.gaze_maps(43, B, T)
        gt = (gt / gt.sum((2, 3), keepdims=True)).astype(np.float32)
        saved, dh_head = bref.saved_and_head_grad(x, gt, p)
        _, _, auto = ref.loss_and_grads(x, gt, p)
        _CASE[(B, T)] = (p, saved, dh_head, bref.bptt(saved, dh_head, p), auto)
    return _CASE[(B, T)]


@pytest.mark.parametrize('B,T', SHAPES)
def test_kernel_form_matches_float64_autograd(B, T):
    p, saved, _, d, auto = case(B, T)
    got = bref.cell_grads(saved, d)
    assert set(got) == set(ref.CELL)
    assert got['ConvLSTM_Whc'] is None and auto['ConvLSTM_Whc'] is None
    for k in ref.CELL:
        if k == 'ConvLSTM_Whc':
            continue
        err = bref.fro(got[k], auto[k])
        print('%dx%d %s: %.3e' % (B, T, k, err))
        assert err < 1e-10, k


@pytest.mark.parametrize('mutation', bref.MUTATIONS)
@pytest.mark.parametrize('B,T', SHAPES)
def test_mutation_is_visible_in_the_pre_activation_gradients(B, T, mutation):
    p, saved, dh_head, d, _ = case(B, T)
    bad = bref.bptt(saved, dh_head, p, mutation)
    moved = {k: bref.fro(bad[k].numpy(), d[k].numpy()) for k in bref.GATES}
    print('%dx%d %s: %s' % (B, T, mutation, ', '.join('%s %.3e' % kv for kv in moved.items())))
    assert max(moved.values()) > 1e-2


def test_unknown_mutation_is_refused():
    p, saved, dh_head, _, _ = case(2, 3)
    with pytest.raises(AssertionError):
        bref.bptt(saved, dh_head, p, 'no_such_mutation')

"""CPU: tests/_lite_bound.py on a small case.  The float64 restatement of the lite engine's arithmetic with its operands
quantised as include/drp.h specifies (lite_model) must lie inside the bound on every component; the same restatement with a
deliberately wrong activation quantiser (8 significant bits toward zero: u_x = 2^-7 where the bound assumes 2^-10) must leave
it on at least one -- the condition that the bound can fail.

The case: the 8-particle one-step fixture and its lists with the seed-0 weights' MAGNITUDES.  A forward running error bound is a
worst case: it is approached where no cancellation helps, i.e. where every product has one sign and rounding toward zero errs
in one direction; there a quantiser eight times coarser than specified must show.  (On signed weights the errors of a 64-deep
sum largely cancel and any worst-case bound is far from them: such a case can only ever pass.)"""
import numpy as np
import pytest

import _f64_ref as R
import _lite_bound as LB


@pytest.fixture(scope='module')
def case(golden):
    g = golden.one_step
    W = {k: np.abs(v) for k, v in R.weights64(golden.weights_seed0).items()}
    inp = [g['n8/' + k] for k in ('attr', 's_cur', 's_delta', 'dens')]
    idx, cnt = g['n8/nbr_idx'], g['n8/nbr_cnt']
    taps = {}
    ref = R.forward64(W, *inp, idx, cnt, taps)
    return W, inp, idx, cnt, taps, ref


@pytest.mark.parametrize('shift', [0, 3, -2])
def test_the_specified_quantisation_is_inside_and_a_coarser_one_is_not(case, shift):
    W, inp, idx, cnt, taps, ref = case
    bound = LB.lite_bound(W, *inp, idx, cnt, taps, shift)
    assert bound.shape == ref.shape and np.isfinite(bound).all() and (bound > 0).all()
    err = np.abs(LB.lite_model(W, *inp, idx, cnt, shift) - ref)
    print('[lite bound] shift %d: specified quantiser %.3f of the bound at most' % (shift, (err / bound).max()))
    assert (err > 0).any() and (err <= bound).all()
    wrong = np.abs(LB.lite_model(W, *inp, idx, cnt, shift, x_bits=8) - ref)
    print('[lite bound] shift %d: u_x = 2^-7 quantiser %.3f of the bound at most, %d of %d components outside'
          % (shift, (wrong / bound).max(), int((wrong > bound).sum()), wrong.size))
    assert (wrong > bound).any()


@pytest.mark.parametrize('which,case_name', [('weights_seed0', 'n64'), ('weights_seed0', 'n8'), ('weights_trained', 'n50')])
def test_the_ceiling_on_signed_weights(golden, which, case_name):
    """the first-order ceiling on the fixtures' own (signed) weights: the specified quantisation stays under it, a u_x = 2^-5
    quantiser and a chain fed the weights' LOW halves (what a wrong operand does) leave it"""
    W = R.weights64(getattr(golden, which))
    g, p = (golden.one_step, case_name + '/') if which == 'weights_seed0' else (golden.trained, 'one_step/%s/' % case_name)
    inp = [g[p + k] for k in ('attr', 's_cur', 's_delta', 'dens')]
    idx, cnt = g[p + 'nbr_idx'], g[p + 'nbr_cnt']
    taps = {}
    ref = R.forward64(W, *inp, idx, cnt, taps)
    ceiling = LB.lite_ceiling(W, *inp, idx, cnt, taps)
    disp = np.abs(ref - inp[1]).max()
    err = np.abs(LB.lite_model(W, *inp, idx, cnt, 0) - ref)
    wrong = np.abs(LB.lite_model(W, *inp, idx, cnt, 0, x_bits=8) - ref)
    low = {k: (v - LB.round_nearest(v, 11, -14) if 'relation_encoder.model.2.weight' in k else v) for k, v in W.items()}
    wrong_operand = np.abs(LB.lite_model(low, *inp, idx, cnt, 0) - ref)
    print('[lite ceiling] %s %s: ceiling at most %.2e of the displacement; specified %.3f, u_x = 2^-7 %.3f, low halves %.1f of it'
          % (which, case_name, ceiling.max() / disp, (err / ceiling).max(), (wrong / ceiling).max(), (wrong_operand / ceiling).max()))
    assert ceiling.max() < 1e-2 * disp
    assert (err <= ceiling).all()
    # the margin of twelve standard deviations leaves room for a quantiser 8 x coarser (that one is the worst-case bound's test,
    # above); 32 x coarser (6 significant bits) and a wrong operand are outside
    coarse = np.abs(LB.lite_model(W, *inp, idx, cnt, 0, x_bits=6) - ref)
    assert (coarse > ceiling).any() and (wrong_operand > ceiling).any()


def test_the_quantisers():
    x = np.array([1.0, 1.0 + 2.0 ** -10, 1.0 + 2.0 ** -11, -1.9999, 3e-6, 65504.0, 0.0])
    h = LB.round_toward_zero(x)
    np.testing.assert_array_equal(h[:3], [1.0, 1.0 + 2.0 ** -10, 1.0])
    assert np.all(np.abs(h) <= np.abs(x)) and np.all(np.abs(x - h) <= np.maximum(LB.U_X * np.abs(x), 2.0 ** -24))
    np.testing.assert_array_equal(LB.round_nearest(x, 11, -14), x.astype(np.float16).astype(np.float64))
    f = np.float32(x)
    bf = ((f.view(np.uint32) + 0x7fff + ((f.view(np.uint32) >> 16) & 1)) & 0xffff0000).view(np.float32)
    np.testing.assert_array_equal(LB.round_nearest(f.astype(np.float64), 8), bf.astype(np.float64))


def test_the_terms_scale_as_derived(case):
    """the bound is monotone in each unit roundoff and its floor follows the shift"""
    W, inp, idx, cnt, taps, _ = case
    b = LB.lite_bound(W, *inp, idx, cnt, taps, 0)
    assert (LB.lite_bound(W, *inp, idx, cnt, taps, 0, u_x=2 * LB.U_X) > b).all()
    assert (LB.lite_bound(W, *inp, idx, cnt, taps, 0, u_node=2 * LB.U_NODE) > b).all()
    assert (LB.lite_bound(W, *inp, idx, cnt, taps, -6) > b).all()                 # a smaller shift: a larger floor
    assert (LB.lite_bound(W, *inp, idx, cnt, taps, 0, self_const=np.ones(inp[0].shape[0], bool)) <= b).all()

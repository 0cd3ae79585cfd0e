"""CPU: the numpy float64 restatement of the reference's forward (tests/_f64_ref.py) -- the host yardstick of the device's
float64 evaluation -- pinned to the reference's own fp32 outputs and intermediates (tests/golden/one_step.npz)."""
import numpy as np
import pytest

from oracle import propnet_sparse as osp

import _f64_ref as R

ONE_STEP = ['n8', 'n50', 'n64', 'n150', 'blob150', 'n300', 'n600', 'n1200']
MID = ['n8', 'n64']


def run(golden, case, taps=None):
    g = golden.one_step
    a, s, sd, d = [g[case + '/' + k] for k in ('attr', 's_cur', 's_delta', 'dens')]
    idx, cnt = osp.build_neighbours(s, sd)
    np.testing.assert_array_equal(cnt, g[case + '/nbr_cnt'].astype(np.int32))
    return R.forward64(R.weights64(golden.weights_seed0), a, s, sd, d, idx, cnt, taps), idx, cnt


@pytest.mark.parametrize('case', ONE_STEP)
def test_s_pred_agrees_with_the_reference(golden, case):
    """within 2e-6 absolute of the reference's fp32 output: the bound test_one_step holds the oracle to"""
    out, _, _ = run(golden, case)
    assert out.dtype == np.float64
    err = np.abs(out - golden.one_step[case + '/s_pred']).max()
    print('[f64 ref] %s: max |s_pred - reference fp32| = %.3e' % (case, err))
    assert err < 2e-6


@pytest.mark.parametrize('case', MID)
def test_taps_agree_with_the_reference(golden, case):
    """the intermediates against the reference's, at the absolute bounds tests/test_oracle_golden.py uses for the same
    tensors (2e-6 for the encodings and the prediction, 5e-6 for the propagated effects)"""
    g = golden.one_step
    taps = {}
    run(golden, case, taps)
    assert sorted(taps) == sorted(R.TAPS)
    np.testing.assert_allclose(taps['particle_encode'], g[case + '/particle_encode'], rtol=0, atol=2e-6)
    np.testing.assert_allclose(taps['particle_pred'], g[case + '/particle_pred'], rtol=0, atol=2e-6)
    for p in range(3):
        np.testing.assert_allclose(taps['effect_%d' % p], g[case + '/particle_effect_%d' % p], rtol=0, atol=5e-6)
    slot = g[case + '/edge_slot'].astype(np.int64)          # the reference's per-edge rows -> (receiver, slot)
    for b in range(slot.shape[0]):
        ok = slot[b, :, 0] >= 0
        i, k = slot[b, ok, 0], slot[b, ok, 1]
        np.testing.assert_allclose(taps['relation_encode'][b, i, k], g[case + '/relation_encode'][b, ok], rtol=0, atol=2e-6)
        for p in range(3):
            np.testing.assert_allclose(taps['effect_rel_%d' % p][b, i, k], g[case + '/effect_rel_%d' % p][b, ok], rtol=0, atol=5e-6)


def test_slots_past_the_count_do_not_count(golden):
    """whatever stands in a list past the receiver's count changes nothing, and an aggregate is its slots' sum"""
    taps = {}
    out, idx, cnt = run(golden, 'n8', taps)
    g = golden.one_step
    junk = np.where(np.arange(10)[None, None, :] < cnt[:, :, None], idx, 3)
    out2 = R.forward64(R.weights64(golden.weights_seed0), g['n8/attr'], g['n8/s_cur'], g['n8/s_delta'], g['n8/dens'], junk, cnt)
    np.testing.assert_array_equal(out, out2)
    assert np.abs(taps['agg_1'] - taps['effect_rel_1'].sum(2)).max() <= 1e-13 * np.abs(taps['agg_1']).max()
    assert np.all(taps['relation_encode'][np.arange(10)[None, None, :] >= cnt[:, :, None]] == 0)

"""Host: what the GPU tests of the matching losses' float64 yardstick lean on (tests/_match_f64_ref.py, tests/_match_ref.py), and the
option that carries the probe -- no device.

(a) every one-shot case of tests/test_gpu_match_f64.py has a uniqueness margin of at least R.MARGIN_MIN = 1e-9 in double (10^5
    times the solver's rounding): any exact solver returns the reference's partners, so NO case is excluded from the partner
    comparison on the device.  The seeds are chosen here.
(b) the duals certify the optimum: u_i + v_j <= C_ij to r 2^-52 max C, equality on the pairs, sum u + sum v = cost; and the
    certificate function finds a matching that is not optimal.
(c) the exact grid case: every cost is an exact multiple of 2^-14 and the margin is 0 -- there are ties, which only the tie rule
    decides.
(d) the trainer's cases of tests/test_gpu_train_f64_match.py: the uniqueness margin and, for the mix, the Chamfer arg-min margin
    of every (step, sample) on the float64 prediction are at least F.PROBE_MARGIN_MIN = 1e-7 = 2.5 x R.DRIFT, the fp32-vs-float64
    drift of a squared distance -- the condition under which the fp32 side's partners can be held to the float64 side's;
    train_match64(matches=sigma) has cost >= opt_cost for a valid sigma that is not the optimum, and equal costs for the optimum;
    the constructed flip batch has a margin BELOW the drift, as it is meant to.
(e) check_match_probe_option, the command line, and the three older options' pinned refusals restated for MATCH_LOSSES.
Every figure is printed before it is asserted."""
import numpy as np
import pytest

import _match_f64_ref as F
import _match_ref as R
import _untracked_ref as U
from dyn_res_pile_manip_amd import synthetic as syn
from dyn_res_pile_manip_amd import train_gnn_dyn as TG


# ---- (a), (b) ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B', F.BATCHES)
@pytest.mark.parametrize('shape', F.SHAPES)
def test_one_shot_cases_have_a_unique_optimum_and_certifying_duals(shape, B):
    p, q, n_p, n_q = F.wide_case(shape, B)
    ref = F.one_shot_reference(shape, B, want_margin=True)
    print('[match-f64] %s B=%d: uniqueness margins %s' % (shape, B, ref['margin']))
    assert (ref['margin'] >= R.MARGIN_MIN).all()
    for b in range(B):
        n, m = int(n_p[b]), int(n_q[b])
        c = F.certificate(p[b], q[b], n, m, ref['u'][b], ref['v'][b], ref['match_pq'][b], ref['cost'][b])
        bound = c['r'] * 2.0 ** -52
        print('[match-f64]     sample %d (%d x %d): slack %.2e tight %.2e sum %.2e of max C (bound %.2e)' % (b, n, m, c['slack'], c['tight'],
                                                                                                         c['sum'], bound))
        assert c['slack'] <= bound and c['tight'] <= bound and c['sum'] <= bound and c['cost'] <= bound
        # padding: no partner, no dual, no gradient
        assert (ref['match_pq'][b, n:] == -1).all() and (ref['u'][b, n:] == 0).all() and (ref['grad'][b, n:] == 0).all()


def test_the_certificate_refuses_a_matching_that_is_not_optimal():
    shape = (70, 130, 70, 130)
    p, q, n_p, n_q = F.wide_case(shape, 1)
    ref = F.one_shot_reference(shape, 1)
    pq = ref['match_pq'][0].copy()
    pq[[3, 4]] = pq[[4, 3]]
    on = np.arange(70)
    cost = float(R.cost64(p[0, :70], q[0, :130])[on, pq[:70]].sum())
    c = F.certificate(p[0], q[0], 70, 130, ref['u'][0], ref['v'][0], pq, cost)
    assert cost > ref['cost'][0] and c['tight'] > 1e-6 and c['sum'] > 1e-6
    with pytest.raises(AssertionError):
        pq[5] = pq[6]
        F.certificate(p[0], q[0], 70, 130, ref['u'][0], ref['v'][0], pq, cost)


# ---- (c) ---------------------------------------------------------------------------------------------------------------------------
def test_the_grid_case_is_exact_and_has_ties():
    p, q, n_p, n_q = F.grid_case()
    ref = R.match64(p, q, n_p, n_q, exact32=False)
    for b in range(2):
        C = R.cost64(p[b, :n_p[b]], q[b, :n_q[b]]) * 2.0 ** 14
        assert (C == np.round(C)).all() and C.max() < 2 ** 20
        assert ref['margin'][b] == 0.0                          # another matching at the same cost: the tie rule decides
        assert (ref['u'][b] * 2.0 ** 14 == np.round(ref['u'][b] * 2.0 ** 14)).all()
        assert (ref['v'][b] * 2.0 ** 14 == np.round(ref['v'][b] * 2.0 ** 14)).all()
    assert ref['cost'][0] == 0.0 and ref['cost'][1] > 0.0       # sample 0: every row of p has a copy in q


# ---- (d) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('impulses', ['data', 'actions'])
@pytest.mark.parametrize('name,wset', U.TRAIN_CASES)
def test_trainer_cases_keep_their_partners_under_the_fp32_drift(golden, name, wset, impulses):
    for targets in F.TARGETS:
        info = F.train_reference(golden, name, wset, impulses, targets, 'chamfer+match')[4]
        print('[match-f64] %s %s %s %s: uniqueness margin %.3e, Chamfer arg-min margin %.3e (r %d..%d)'
              % (name, wset, impulses, targets, info['margin'], info['chamfer_margin'], info['r'].min(), info['r'].max()))
        assert info['margin'] >= F.PROBE_MARGIN_MIN > 2 * R.DRIFT and info['chamfer_margin'] >= F.PROBE_MARGIN_MIN
        np.testing.assert_allclose(info['cost'], info['opt_cost'], rtol=1e-13)       # (two orders of one sum)
        if targets == 'dense':
            assert (info['r'] == np.asarray(golden.train[name + '/particle_nums'])[None, :]).all()


def test_degenerate_batches_have_margins_too(golden):
    for label, batch in (('tiny', U.tiny_batch()), ('single point', U.single_point_batch(golden))):
        info = F.reference(F.batch_kw(batch), golden.weights_seed0)[4]
        print('[match-f64] %s: uniqueness margin %.3e' % (label, info['margin']))
        assert info['margin'] >= F.PROBE_MARGIN_MIN


def test_a_given_matching_costs_no_less_than_the_optimum(golden):
    kw = F.train_kw(golden, 'b2_r5', 'data', 'dense')
    loss, terms, _, _, info = F.reference(kw, golden.weights_seed0)
    swapped = info['match'].copy()
    swapped[:, :, [0, 1]] = swapped[:, :, [1, 0]]               # rows 0 and 1 are real and matched in every problem (dense targets)
    assert (swapped[:, :, :2] >= 0).all()
    loss2, terms2, _, _, info2 = F.reference(kw, golden.weights_seed0, matches=swapped)
    np.testing.assert_array_equal(info2['opt_cost'], info['opt_cost'])
    assert (info2['cost'] > info2['opt_cost']).all() and (terms2 > terms).all() and loss2 > loss
    loss3, terms3, _, _, info3 = F.reference(kw, golden.weights_seed0, matches=info['match'])
    np.testing.assert_allclose(info3['cost'], info3['opt_cost'], rtol=1e-13)
    assert loss3 == loss


def test_the_flip_batch_has_a_margin_below_the_drift(golden):
    kw = F.flip_kw(golden)
    assert (np.abs(kw['targets'][:, :, 1] - kw['targets'][:, :, 0]).max(axis=-1) > 0).all()
    info = F.reference(kw, golden.weights_seed0)[4]
    print('[match-f64] flip batch: uniqueness margin %.3e against the drift %.1e' % (info['margin'], R.DRIFT))
    assert 0 < info['margin'] < R.DRIFT / 10


# ---- (e) ---------------------------------------------------------------------------------------------------------------------------
def test_the_option_and_the_pinned_refusals(tmp_path):
    config = syn.default_config()
    config['train'].update({'n_rollout': 2, 'n_history': 1, 'n_epoch': 1})
    empty = {'train': [], 'valid': []}
    run_dir = tmp_path / 'run'
    for loss in TG.MATCH_LOSSES:
        # the three older options keep refusing these losses ...
        for kw in ({'probe_every': 1}, {'grad_probe_every': 1}):
            with pytest.raises(ValueError, match='no float64 yardstick'):
                TG.check_probe_options(loss, kw.get('grad_probe_every', 0), kw.get('probe_every', 0))
            with pytest.raises(ValueError, match='no float64 yardstick'):
                TG.train(config, None, empty, loss=loss, **kw)
            with pytest.raises(ValueError, match='no float64 yardstick'):
                TG.main(config, data_root=str(tmp_path), train_dir=str(run_dir), loss=loss, **kw)
            # ... with their message first where the new option is given beside them
            with pytest.raises(ValueError, match='no float64 yardstick'):
                TG.train(config, None, empty, loss=loss, match_probe_every=1, **kw)
            with pytest.raises(ValueError, match='no float64 yardstick'):
                TG.main(config, data_root=str(tmp_path), train_dir=str(run_dir), loss=loss, match_probe_every=1, **kw)
        with pytest.raises(ValueError, match='no float64 yardstick'):
            TG.probe_batch(None, None, loss=loss)
        # the new option: accepted with the losses it is for
        TG.check_match_probe_option(loss, 0)
        TG.check_match_probe_option(loss, 3)
        for bad in (-1, 1.5):
            with pytest.raises(ValueError, match='match_probe_every'):
                TG.check_match_probe_option(loss, bad)
        # given alone
        for kw in ({'grad_probe_every': 1}, {'probe_every': 1}, {'sinkhorn_probe_every': 1}):
            with pytest.raises(ValueError, match='match_probe_every alone'):
                TG.check_match_probe_option(loss, 1, **kw)
        with pytest.raises(ValueError):
            TG.train(config, None, empty, loss=loss, match_probe_every=1, sinkhorn_probe_every=1)
    TG.check_match_probe_option('mse', 0)
    for other in ('mse', 'chamfer', 'transport', 'sinkhorn'):
        with pytest.raises(ValueError, match='match_probe_every needs a loss'):
            TG.check_match_probe_option(other, 1)
        with pytest.raises(ValueError, match='match_probe_every'):
            TG.train(config, None, empty, loss=other, match_probe_every=1)
        with pytest.raises(ValueError, match='match_probe_every'):
            TG.main(config, data_root=str(tmp_path), train_dir=str(run_dir), loss=other, match_probe_every=1)
    with pytest.raises(ValueError, match='match_weight'):
        TG.probe_batch_match(None, None, loss='chamfer+match', match_weight=1.0)
    with pytest.raises(ValueError, match='probe_batch_match needs a loss'):
        TG.probe_batch_match(None, None, loss='chamfer')
    with pytest.raises(ValueError, match='impulses'):
        TG.probe_batch_match(None, None, impulses='pushes')
    z = np.zeros
    batch = TG.PaddedBatch((z((1, 3, 4, 3), np.float32), None, z((1, 3, 4), np.float32), np.array([4], np.int32),
                            np.array([100.0], np.float32), None, z((1, 2, 5, 3), np.float32), np.array([[5, 5]], np.int32)))
    batch.actions = z((1, 2, 4), np.float32)
    batch.depth_only = True
    with pytest.raises(ValueError, match='depth-only'):
        TG.probe_batch_match(None, batch, impulses='data')
    assert not run_dir.exists()                                  # main() refuses before it touches the disk or a device
    # the command line
    for argv in (['--loss', 'mse', '--match-probe-every', '2'], ['--loss', 'match', '--match-probe-every', '2', '--probe-every', '2'],
                 ['--loss', 'chamfer+match', '--match-probe-every', '-1'],
                 ['--loss', 'match', '--match-probe-every', '2', '--sinkhorn-probe-every', '2'],
                 ['--data', 'depth', '--loss', 'sinkhorn', '--match-probe-every', '1']):
        with pytest.raises(ValueError):
            TG._cli(argv + ['--data-root', str(tmp_path), '--train-dir', str(run_dir)])
    assert not run_dir.exists()


def test_the_engine_refuses_a_loss_that_has_no_matching():
    """Engine.train_gradient_probe(loss=...) and Engine.train_grad_f64_match check their keywords before they touch the device"""
    from dyn_res_pile_manip_amd.engine import Engine
    e = Engine.__new__(Engine)                                   # no context: the checks come first
    x = np.zeros((1, 2, 3, 3), np.float32)
    for bad in ('chamfer', 'mse', 'sinkhorn'):
        with pytest.raises(ValueError, match='loss'):
            e.train_gradient_probe(x, x[:, :1], x[..., 0], [3], [1.0], targets=x[:, :1], target_nums=[[3]], loss=bad)
        with pytest.raises(ValueError, match='loss'):
            e.train_grad_f64_match(x, x[:, :1], x[..., 0], [3], [1.0], x[:, :1], [[3]], loss=bad)
    with pytest.raises(ValueError, match='loss'):
        e.train_gradient_probe(x, x[:, :1], x[..., 0], [3], [1.0], loss='match')                       # no targets

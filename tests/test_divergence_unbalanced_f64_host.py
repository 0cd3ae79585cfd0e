"""Host: the reference of the unbalanced Sinkhorn divergence's float64 yardstick (tests/_divergence_unbalanced_f64_ref.py), what a
drift of the predicted states does to the weight gradients through the relaxed plans, and the option that carries the probe -- no
device.

(a) train_sinkhorn64_unbalanced equals _divergence_unbalanced_ref.train_divergence64 fed the plans it formed itself -- loss, terms,
    every gradient and the state gradient bit for bit -- and at rho = inf, w = 1 it equals _divergence_f64_ref.train_sinkhorn64
    bit for bit.
(b) its state gradient equals central differences (h = 1e-5) of the loss it reports on test_divergence_f64_host.five_by_six() at
    K = 300, at rho / eps in {1, 4, 25} and masses 1 and 1.2: within 1e-6 of the largest gradient component, the balanced test's
    rule.  Measured: at most 6.0e-9 of it.
(c) test_divergence_f64_host.py (c) with the relaxed plans: on _transport_ref.train_batch() (K = 50, eps scale 1 and 0.25 at
    rho = 4 eps, both impulse sources, both masses, seed-0 and trained weights) the states the loss SEES are (1) rounded to fp32,
    (2) moved by 1e-4 of the step's largest displacement with the signs of default_rng(2024).  Asserted: the reference alone
    stays within GRAD_REL = 2e-4 under both -- the condition under which the device probe's bound can hold at all.  Measured
    (worst tensor over the eight cases of a weight set):
        rounded to fp32      seed-0 7.4e-8    trained 7.8e-8
        1e-4 displacement    seed-0 3.9e-6    trained 1.3e-4 (eps scale 0.25, unit masses) -- below GRAD_REL, but not by much
(d) the option plumbing of sinkhorn_reach_probe_every, that the pinned older refusals are still raised with their words, and that
    Engine.cloud_divergence_f64 refuses mass_q / want_transported without a reach before the library is touched.
Every figure is printed before it is asserted (DESIGN.md 2 records them)."""
import numpy as np
import pytest

import _divergence_f64_ref as R
import _divergence_unbalanced_f64_ref as RU
import _divergence_unbalanced_ref as UB
import _train_actions_ref as A
import _untracked_ref as U
from dyn_res_pile_manip_amd import synthetic as syn
from dyn_res_pile_manip_amd import train_gnn_dyn as TG
from test_divergence_f64_host import DRIFT_REL, five_by_six, tensor_shifts

GRAD_REL = A.GRAD_REL


# ---- the cases themselves ----------------------------------------------------------------------------------------------------------
def test_the_cases_carry_two_reaches_and_four_masses():
    kw = RU.train_case('data', 'count')
    assert kw['reach'].shape == (2,) and kw['reach'][0] != kw['reach'][1]
    np.testing.assert_array_equal(kw['mass_q'], np.array([[12.0 / 9, 5.0 / 6], [7.0 / 9, 10.0 / 6]]))
    assert len(set(kw['mass_q'].ravel())) == 4
    np.testing.assert_array_equal(RU.train_case('data', 'unit')['mass_q'], np.ones((2, 2)))
    assert (kw['reach'] >= 4.0 * kw['eps']).all()


# ---- (a) -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('impulses', ['data', 'actions'])
def test_it_is_train_divergence64_fed_its_own_plans(golden, impulses):
    kw = RU.train_case(impulses, 'count')
    loss, terms, grads, gs, info = RU.run(golden.weights_seed0, kw)
    l2, t2, g2, gs2 = UB.train_divergence64(golden.weights_seed0, kw['states'], kw['states_delta'], kw['attrs'], kw['particle_nums'],
                                            kw['particle_dens'], kw['targets'], kw['target_nums'], info['plans'],
                                            actions=kw.get('actions'))
    print('[divergence-unbalanced-f64] %s: loss %.15e against %.15e' % (impulses, loss, l2))
    assert loss == l2 and loss > 0
    np.testing.assert_array_equal(terms, t2)
    np.testing.assert_array_equal(gs, gs2)
    for k in grads:
        np.testing.assert_array_equal(grads[k], g2[k])
    assert info['col_err'].shape == (2, 2) and info['self_err'].shape == (2, 2, 2) and info['transported'].shape == (2, 2)
    # (a target heavier than the prediction can leave a share above 1: the smallest one is what the probe reports)
    assert (info['transported'] > 0).all() and info['transported'].min() < 1 and np.isfinite(info['transported']).all()


@pytest.mark.parametrize('impulses', ['data', 'actions'])
def test_the_infinite_reach_is_train_sinkhorn64(golden, impulses):
    kw = R.train_case(impulses)
    a = R.train_sinkhorn64(golden.weights_seed0, kw['states'], kw['states_delta'], kw['attrs'], kw['particle_nums'],
                           kw['particle_dens'], kw['targets'], kw['target_nums'], kw['eps'], kw['iters'], actions=kw.get('actions'))
    b = RU.run(golden.weights_seed0, dict(kw, reach=np.inf, mass_q=1.0))
    assert a[0] == b[0]
    np.testing.assert_array_equal(a[1], b[1])
    np.testing.assert_array_equal(a[3], b[3])
    for k in a[2]:
        np.testing.assert_array_equal(a[2][k], b[2][k])
    np.testing.assert_array_equal(a[4]['col_err'], b[4]['col_err'])
    np.testing.assert_array_equal(a[4]['self_err'], b[4]['self_err'])
    for t in range(2):
        for s in range(2):
            n = int(kw['particle_nums'][s])
            assert b[4]['transported'][t, s] == UB._sum_asc(np.full(n, 1.0 / n))


def test_the_padded_batch_is_pair64_on_the_double_prediction():
    p, q, _ = UB.half_seen_pile()
    rng = np.random.default_rng(3)
    p64 = p.astype(np.float64) + 1e-9 * rng.standard_normal(p.shape)
    P, Q = np.zeros((2, 80, 3)), np.zeros((2, 40, 3), np.float32)
    P[0, :72], P[1, :30], Q[0, :36], Q[1, :36] = p64, p64[:30], q, q
    eps, rho, w = np.array([4e-4, 2e-4]), np.array([16e-4, 50e-4]), np.array([0.5, 1.2])
    out = RU.divergence64_wide(P, Q, [72, 30], [36, 36], eps, rho, w, 20)
    for b, n in ((0, 72), (1, 30)):
        ref = UB.pair64(None, q, eps[b], rho[b], w[b], 20, p64=p64[:n])
        assert out['divergence'][b] == ref[0] and out['transported'][b] == ref[8]
        np.testing.assert_array_equal(out['grad'][b, :n], ref[1])
        assert (out['grad'][b, n:] == 0).all() and (out['f'][b, n:] == 0).all()


# ---- (b) -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ratio,mass', [(1.0, 1.0), (1.0, 1.2), (4.0, 1.0), (4.0, 1.2), (25.0, 1.0), (25.0, 1.2)])
def test_state_gradient_agrees_with_central_differences_of_the_reported_loss(golden, ratio, mass):
    kw = dict(five_by_six())
    kw['reach'], kw['mass_q'] = ratio * kw['eps'], mass
    loss, _, _, gs, _ = RU.run(golden.weights_seed0, kw)
    h = 1e-5
    worst = 0.0
    for i in range(5):
        for k in range(3):
            vals = []
            for sgn in (1.0, -1.0):
                def see(t, b, x, cur):
                    x[i, k] += sgn * h
                    return x
                vals.append(RU.run(golden.weights_seed0, kw, see)[0])
            worst = max(worst, abs((vals[0] - vals[1]) / (2 * h) - gs[0, 0, i, k]))
    gmax = float(np.abs(gs).max())
    print('[divergence-unbalanced-f64] 5 x 6, K = 300, rho = %g eps, mass %g: central differences of the reported loss within %.2e '
          'of the state gradient, largest component %.2e (%.2e of it)' % (ratio, mass, worst, gmax, worst / gmax))
    assert gmax > 0 and worst <= 1e-6 * gmax


# ---- (c) -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('wset', ['seed0', 'trained'])
def test_what_a_drift_of_the_predicted_states_does_to_the_weight_gradients(golden, wset):
    w = U.weights_of(golden, wset)
    worst = {'fp32': 0.0, 'drift': 0.0}
    for impulses in ('data', 'actions'):
        for scale in R.EPS_SCALES:
            for mass in RU.MASSES:
                kw = RU.train_case(impulses, mass, scale)
                base = RU.run(w, kw)[2]
                rng = np.random.default_rng(2024)

                def rounded(t, b, x, cur):
                    return x.astype(np.float32).astype(np.float64)

                def drifted(t, b, x, cur):
                    disp = float(np.sqrt(((x - cur) ** 2).sum(axis=1)).max())
                    return x + DRIFT_REL * disp * rng.choice([-1.0, 1.0], size=x.shape)
                got = {'fp32': tensor_shifts(RU.run(w, kw, rounded)[2], base), 'drift': tensor_shifts(RU.run(w, kw, drifted)[2], base)}
                print('[divergence-unbalanced-f64] %-7s %-7s eps scale %-4s %-5s masses: worst tensor shift %.2e (states rounded to '
                      'fp32), %.2e (moved by %.0e of the displacement)' % (wset, impulses, scale, mass, got['fp32'], got['drift'],
                                                                           DRIFT_REL))
                for k in worst:
                    worst[k] = max(worst[k], got[k])
    print('[divergence-unbalanced-f64] %s: worst %.2e (fp32), %.2e (drift), GRAD_REL %.0e' % (wset, worst['fp32'], worst['drift'],
                                                                                              GRAD_REL))
    assert worst['fp32'] <= GRAD_REL and worst['drift'] <= GRAD_REL


# ---- (d) -------------------------------------------------------------------------------------------------------------------------
def test_the_new_probe_option_and_the_pinned_refusals(tmp_path):
    config = syn.default_config()
    empty = {'train': [], 'valid': []}
    run_dir = tmp_path / 'run'
    loss = 'sinkhorn'
    where = {'data_root': str(tmp_path), 'train_dir': str(run_dir)}
    tail = ['--data-root', str(tmp_path), '--train-dir', str(run_dir)]
    # accepted with the loss and a reach
    TG.check_sinkhorn_reach_probe_option(loss, 0)
    TG.check_sinkhorn_reach_probe_option('mse', 0)
    TG.check_sinkhorn_reach_probe_option(loss, 3, 4.0)
    TG.check_sinkhorn_reach_probe_option(loss, 3, float('inf'))
    TG.check_sinkhorn_options(loss, 4.0, 'count', 0)           # (train() itself builds a device optimizer: the GPU test runs it)
    # refused without a reach, with a message that names the balanced option
    for call in (lambda **k: TG.train(config, None, empty, **k), lambda **k: TG.main(config, **dict(where, **k))):
        with pytest.raises(ValueError, match='sinkhorn_probe_every'):
            call(loss=loss, sinkhorn_reach_probe_every=2)
        # with any other loss
        for other in TG.LOSSES + TG.MATCH_LOSSES + TG.TRANSPORT_LOSSES:
            with pytest.raises(ValueError, match='sinkhorn_reach'):
                call(loss=other, sinkhorn_reach_probe_every=2, sinkhorn_reach_scale=4.0)
            with pytest.raises(ValueError, match='sinkhorn_reach_probe_every needs a loss'):
                TG.check_sinkhorn_reach_probe_option(other, 2, 4.0)
        # beside any of the four other probe options
        for kw in ({'probe_every': 1}, {'grad_probe_every': 1}, {'sinkhorn_probe_every': 1}, {'match_probe_every': 1}):
            with pytest.raises(ValueError):
                call(loss=loss, sinkhorn_reach_scale=4.0, sinkhorn_reach_probe_every=2, **kw)
            with pytest.raises(ValueError, match='sinkhorn_reach_probe_every alone'):
                TG.check_sinkhorn_reach_probe_option(loss, 2, 4.0, **kw)
        # for a bad count
        for bad in (-1, 1.5):
            with pytest.raises(ValueError, match='sinkhorn_reach_probe_every must be'):
                call(loss=loss, sinkhorn_reach_scale=4.0, sinkhorn_reach_probe_every=bad)
    for argv in (['--loss', loss, '--sinkhorn-reach-probe-every', '2'],
                 ['--loss', 'mse', '--sinkhorn-reach-probe-every', '2'],
                 ['--loss', 'transport', '--sinkhorn-reach-scale', '4', '--sinkhorn-reach-probe-every', '2'],
                 ['--loss', loss, '--sinkhorn-reach-scale', '4', '--sinkhorn-reach-probe-every', '-1'],
                 ['--loss', loss, '--sinkhorn-reach-scale', '4', '--sinkhorn-reach-probe-every', '2', '--probe-every', '2'],
                 ['--loss', loss, '--sinkhorn-reach-scale', '4', '--sinkhorn-reach-probe-every', '2', '--grad-probe-every', '2'],
                 ['--loss', loss, '--sinkhorn-reach-scale', '4', '--sinkhorn-reach-probe-every', '2', '--sinkhorn-probe-every', '2'],
                 ['--loss', loss, '--sinkhorn-reach-scale', '4', '--sinkhorn-reach-probe-every', '2', '--match-probe-every', '2']):
        with pytest.raises((ValueError, SystemExit)):
            TG._cli(argv + tail)
    assert not run_dir.exists()
    # the two pinned older refusals, with their words
    for call in (lambda **k: TG.train(config, None, empty, **k), lambda **k: TG.main(config, **dict(where, **k))):
        with pytest.raises(ValueError, match='no float64 yardstick for the unbalanced'):
            call(loss=loss, sinkhorn_reach_scale=4.0, sinkhorn_probe_every=2)
        for kw in ({'probe_every': 1}, {'grad_probe_every': 1}):
            with pytest.raises(ValueError, match='no float64 yardstick'):
                call(loss=loss, **kw)
    with pytest.raises(ValueError, match='no float64 yardstick'):
        TG.probe_batch(None, None, loss=loss)
    with pytest.raises(SystemExit):
        TG._cli(['--loss', loss, '--sinkhorn-reach-scale', '4', '--sinkhorn-probe-every', '2'] + tail)
    assert not run_dir.exists()
    # the probe call checks the reach options like run_batch
    with pytest.raises(ValueError, match='sinkhorn_mass'):
        TG.probe_batch_sinkhorn(None, None, sinkhorn_mass='count')
    with pytest.raises(ValueError, match='sinkhorn_reach_scale'):
        TG.probe_batch_sinkhorn(None, None, sinkhorn_reach_scale=0.0)

    z = np.zeros
    batch = TG.PaddedBatch((z((1, 3, 4, 3), np.float32), None, z((1, 3, 4), np.float32), np.array([4], np.int32),
                            np.array([100.0], np.float32), None, z((1, 2, 5, 3), np.float32), np.array([[5, 3]], np.int32)))
    batch.actions = z((1, 2, 4), np.float32)
    batch.depth_only = True

    class Recorder(object):                     # the engine call the hook makes on a depth-only batch through the push
        def train_gradient_probe(self, *a, **k):
            self.a, self.k = a, k
            return {'rel': 0.0}

    class Model(object):
        engine = Recorder()
    with pytest.raises(ValueError, match='depth-only'):
        TG.probe_batch_sinkhorn(Model, batch, impulses='data', sinkhorn_reach_scale=4.0)
    TG.probe_batch_sinkhorn(Model, batch, impulses='actions', transport_eps_scale=0.5, transport_iters=7, sinkhorn_reach_scale=4.0,
                            sinkhorn_mass='count')
    k = Model.engine.k
    assert Model.engine.a[1] is None and k['actions'] is not None and k['iters'] == 7
    np.testing.assert_array_equal(k['eps'], [0.5 / 100.0])
    np.testing.assert_array_equal(k['reach'], [4.0 / 100.0])
    assert k['reach'].shape == (1,) and k['mass_q'].shape == (2, 1)
    np.testing.assert_array_equal(k['mass_q'], [[5.0 / 4], [3.0 / 4]])
    TG.probe_batch_sinkhorn(Model, batch, impulses='actions', sinkhorn_reach_scale=4.0)
    np.testing.assert_array_equal(Model.engine.k['mass_q'], np.ones((2, 1)))
    TG.probe_batch_sinkhorn(Model, batch, impulses='actions')                       # without a reach: today's call
    assert 'reach' not in Model.engine.k and 'mass_q' not in Model.engine.k


def test_the_engine_refuses_the_reach_keywords_without_a_reach():
    from dyn_res_pile_manip_amd.engine import Engine
    eng = object.__new__(Engine)                # no library, no device: the refusals come before either is touched
    p, q = np.zeros((1, 4, 3)), np.zeros((1, 5, 3), np.float32)
    with pytest.raises(ValueError, match='give reach'):
        eng.cloud_divergence_f64(p, q, eps=1e-3, iters=5, mass_q=1.2)
    with pytest.raises(ValueError, match='give reach'):
        eng.cloud_divergence_f64(p, q, eps=1e-3, iters=5, want_transported=True)
    with pytest.raises(ValueError, match='give reach'):
        eng.train_grad_f64_divergence(None, None, None, None, None, None, None, 1e-3, 5, mass_q=1.2)
    with pytest.raises(ValueError, match='give reach'):
        eng.train_gradient_probe(None, None, None, None, None, targets=p, target_nums=p, eps=1e-3, iters=5, mass_q=1.2)
    with pytest.raises(ValueError, match='reach='):
        eng.train_gradient_probe(None, None, None, None, None, targets=p, target_nums=p, reach=4e-3)
    with pytest.raises(ValueError, match='reach='):
        eng.train_gradient_probe(None, None, None, None, None, targets=p, target_nums=p, loss='match', reach=4e-3)

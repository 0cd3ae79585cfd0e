"""Host: the reference of the Sinkhorn divergence's float64 yardstick (tests/_divergence_f64_ref.py), what a drift of the predicted
states does to the weight gradients through the plans, and the option that carries the probe -- no device.

(a) train_sinkhorn64 equals _divergence_ref.train_divergence64 fed the plans it formed itself: the same loop, the same surrogate
    -- loss, terms, every gradient and the state gradient bit for bit.
(b) its state gradient equals central differences of the loss it reports, on a 5 x 6 problem (one sample, one step) at K = 300
    (converged, so that the plans are constants of the derivative to rounding): within 1e-6 of the largest gradient component,
    the rule of tests/test_divergence_host.py (a).
(c) the plans are exp(. / eps) of the cost, so a drift d of a predicted state moves a plan entry by about 2 |p - q| d / eps
    relatively.  On _transport_ref.train_batch() (K = 50, eps scale 1 and 0.25, both impulse sources, seed-0 and trained weights)
    the states the loss SEES are (1) rounded to fp32, (2) moved by 1e-4 of the step's largest displacement -- the bound the
    engines are held to (load_weights(max_disp_rel=1e-4)) -- with a random sign per coordinate, a worst case; the reverse pass
    still starts at the unperturbed state.  The shift of every weight-gradient tensor is taken as a share of that tensor's
    largest gradient.  Asserted: the reference alone stays within GRAD_REL = 2e-4 under both -- the condition under which the
    device probe's bound can hold at all.  Measured (worst tensor over the four cases of a weight set):
        rounded to fp32      seed-0 2.4e-8    trained 2.2e-8
        1e-4 displacement    seed-0 1.3e-6    trained 1.1e-4 -- below GRAD_REL, but not by much (the signs are one seeded draw)
(d) the option plumbing of sinkhorn_probe_every, and that the three pinned refusals are still raised.
Every figure is printed before it is asserted (DESIGN.md 2 records them)."""
import numpy as np
import pytest

import _divergence_f64_ref as R
import _divergence_ref as D
import _train_actions_ref as A
import _transport_ref as T
import _untracked_ref as U
from dyn_res_pile_manip_amd import synthetic as syn
from dyn_res_pile_manip_amd import train_gnn_dyn as TG

GRAD_REL = A.GRAD_REL
DRIFT_REL = 1e-4                    # of the step's largest displacement


def run(w, kw, see=None, K=None):
    return R.train_sinkhorn64(w, kw['states'], kw['states_delta'], kw['attrs'], kw['particle_nums'], kw['particle_dens'],
                              kw['targets'], kw['target_nums'], kw['eps'], kw['iters'] if K is None else K, actions=kw.get('actions'),
                              see=see)


# ---- (a) -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('impulses', ['data', 'actions'])
def test_it_is_train_divergence64_fed_its_own_plans(golden, impulses):
    kw = R.train_case(impulses)
    loss, terms, grads, gs, info = run(golden.weights_seed0, kw)
    l2, t2, g2, gs2 = D.train_divergence64(golden.weights_seed0, kw['states'], kw['states_delta'], kw['attrs'], kw['particle_nums'],
                                           kw['particle_dens'], kw['targets'], kw['target_nums'], info['plans'],
                                           actions=kw.get('actions'))
    print('[divergence-f64] %s: loss %.15e against %.15e' % (impulses, loss, l2))
    assert loss == l2 and loss > 0
    np.testing.assert_array_equal(terms, t2)
    np.testing.assert_array_equal(gs, gs2)
    for k in grads:
        np.testing.assert_array_equal(grads[k], g2[k])
    assert info['col_err'].shape == (2, 2) and info['self_err'].shape == (2, 2, 2)
    assert (info['col_err'] > 0).all() and (info['col_err'] < T.COL_ERR_MAX * 10).all()


# ---- (b) -------------------------------------------------------------------------------------------------------------------------
def five_by_six():
    """one sample, one step, 5 particles against 6 target points drawn from its recorded next state"""
    st, ac, at, nums, dens = A.synthetic_batch([5], 1, 60, kinds=('blob',))
    rng = np.random.default_rng(5)
    sd = A._sd32(st[0, 0], ac[0, 0])[None, None]
    rows = st[0, 1][rng.integers(0, 5, 6)]
    tg = (rows + U.JITTER * rng.standard_normal((6, 3))).astype(np.float32)[None, None]
    return dict(states=st, states_delta=sd, attrs=at, particle_nums=nums, particle_dens=dens, targets=tg,
                target_nums=np.array([[6]], np.int32), eps=R.eps_of(dens), iters=300)


def test_state_gradient_agrees_with_central_differences_of_the_reported_loss(golden):
    kw = five_by_six()
    assert kw['states'].shape == (1, 2, 5, 3) and kw['targets'].shape == (1, 1, 6, 3)
    loss, _, _, gs, _ = run(golden.weights_seed0, kw)
    h = 1e-5
    worst = 0.0
    for i in range(5):
        for k in range(3):
            vals = []
            for sgn in (1.0, -1.0):
                def see(t, b, x, cur):
                    x[i, k] += sgn * h
                    return x
                vals.append(run(golden.weights_seed0, kw, see)[0])
            worst = max(worst, abs((vals[0] - vals[1]) / (2 * h) - gs[0, 0, i, k]))
    gmax = float(np.abs(gs).max())
    print('[divergence-f64] 5 x 6, K = 300: central differences of the reported loss within %.2e of the state gradient, largest '
          'component %.2e' % (worst, gmax))
    assert gmax > 0 and worst <= 1e-6 * gmax


# ---- (c) -------------------------------------------------------------------------------------------------------------------------
def tensor_shifts(g, base):
    """-> the largest shift of a tensor as a share of that tensor's largest gradient"""
    return max(float(np.abs(g[k] - base[k]).max() / np.abs(base[k]).max()) for k in base if np.abs(base[k]).max() > 0)


@pytest.mark.parametrize('wset', ['seed0', 'trained'])
def test_what_a_drift_of_the_predicted_states_does_to_the_weight_gradients(golden, wset):
    w = U.weights_of(golden, wset)
    worst = {'fp32': 0.0, 'drift': 0.0}
    for impulses in ('data', 'actions'):
        for scale in R.EPS_SCALES:
            kw = R.train_case(impulses, scale)
            base = run(w, kw)[2]
            rng = np.random.default_rng(2024)

            def rounded(t, b, x, cur):
                return x.astype(np.float32).astype(np.float64)

            def drifted(t, b, x, cur):
                disp = float(np.sqrt(((x - cur) ** 2).sum(axis=1)).max())
                return x + DRIFT_REL * disp * rng.choice([-1.0, 1.0], size=x.shape)
            got = {'fp32': tensor_shifts(run(w, kw, rounded)[2], base), 'drift': tensor_shifts(run(w, kw, drifted)[2], base)}
            print('[divergence-f64] %-7s %-7s eps scale %-4s: worst tensor shift %.2e (states rounded to fp32), %.2e (moved by %.0e '
                  'of the displacement)' % (wset, impulses, scale, got['fp32'], got['drift'], DRIFT_REL))
            for k in worst:
                worst[k] = max(worst[k], got[k])
    print('[divergence-f64] %s: worst %.2e (fp32), %.2e (drift), GRAD_REL %.0e' % (wset, worst['fp32'], worst['drift'], GRAD_REL))
    assert worst['fp32'] <= GRAD_REL and worst['drift'] <= GRAD_REL


# ---- (d) -------------------------------------------------------------------------------------------------------------------------
def test_the_new_probe_option_and_the_pinned_refusals(tmp_path):
    config = syn.default_config()
    empty = {'train': [], 'valid': []}
    run_dir = tmp_path / 'run'
    loss = 'sinkhorn'
    # the three pinned refusals, as tests/test_divergence_host.py has them
    for kw in ({'probe_every': 1}, {'grad_probe_every': 1}):
        with pytest.raises(ValueError, match='no float64 yardstick'):
            TG.train(config, None, empty, loss=loss, **kw)
        with pytest.raises(ValueError, match='no float64 yardstick'):
            TG.main(config, data_root=str(tmp_path), train_dir=str(run_dir), loss=loss, **kw)
    with pytest.raises(ValueError, match='no float64 yardstick'):
        TG.probe_batch(None, None, loss=loss)
    # the new option: accepted with the loss it is for ...
    TG.check_sinkhorn_probe_option(loss, 0)
    TG.check_sinkhorn_probe_option(loss, 3)
    TG.check_sinkhorn_probe_option('mse', 0, 2, 0)
    # ... refused with any other, together with either older option (which refuse the loss first), and for a bad count
    for other in TG.LOSSES + TG.MATCH_LOSSES + TG.TRANSPORT_LOSSES:
        with pytest.raises(ValueError, match='sinkhorn_probe_every'):
            TG.train(config, None, empty, loss=other, sinkhorn_probe_every=1)
        with pytest.raises(ValueError, match='sinkhorn_probe_every'):
            TG.main(config, data_root=str(tmp_path), train_dir=str(run_dir), loss=other, sinkhorn_probe_every=1)
    for kw in ({'probe_every': 1}, {'grad_probe_every': 1}):
        with pytest.raises(ValueError, match='no float64 yardstick'):
            TG.train(config, None, empty, loss=loss, sinkhorn_probe_every=1, **kw)
        with pytest.raises(ValueError, match='sinkhorn_probe_every alone'):
            TG.check_sinkhorn_probe_option(loss, 1, **{k: 1 for k in kw})
        with pytest.raises(ValueError, match='sinkhorn_probe_every'):
            TG.train(config, None, empty, loss='mse', sinkhorn_probe_every=1, **kw)
    for bad in (-1, 1.5):
        with pytest.raises(ValueError, match='sinkhorn_probe_every'):
            TG.train(config, None, empty, loss=loss, sinkhorn_probe_every=bad)
    # the command line carries it, and refuses the same combinations before the disk or a device is touched
    for argv in (['--loss', 'mse', '--sinkhorn-probe-every', '2'], ['--loss', loss, '--sinkhorn-probe-every', '2', '--probe-every', '2'],
                 ['--loss', loss, '--sinkhorn-probe-every', '-1']):
        with pytest.raises(ValueError):
            TG._cli(argv + ['--data-root', str(tmp_path), '--train-dir', str(run_dir)])
    assert not run_dir.exists()
    # the transport loss's two options are range-checked by the probe call too, and a depth-only batch needs the push
    with pytest.raises(ValueError, match='transport_iters'):
        TG.probe_batch_sinkhorn(None, None, transport_iters=0)
    with pytest.raises(ValueError, match='transport_eps_scale'):
        TG.probe_batch_sinkhorn(None, None, transport_eps_scale=0.0)
    with pytest.raises(ValueError, match='impulses'):
        TG.probe_batch_sinkhorn(None, None, impulses='pushes')
    z = np.zeros
    batch = TG.PaddedBatch((z((1, 3, 4, 3), np.float32), None, z((1, 3, 4), np.float32), np.array([4], np.int32),
                            np.array([100.0], np.float32), None, z((1, 2, 5, 3), np.float32), np.array([[5, 5]], np.int32)))
    batch.actions = z((1, 2, 4), np.float32)
    batch.depth_only = True
    with pytest.raises(ValueError, match='depth-only'):
        TG.probe_batch_sinkhorn(None, batch, impulses='data')

    class Recorder(object):                     # the engine call the hook makes on a depth-only batch through the push
        def train_gradient_probe(self, *a, **k):
            self.a, self.k = a, k
            return {'rel': 0.0}

    class Model(object):
        engine = Recorder()
    TG.probe_batch_sinkhorn(Model, batch, impulses='actions', transport_eps_scale=0.5, transport_iters=7)
    k = Model.engine.k
    assert Model.engine.a[1] is None and k['actions'] is not None and k['iters'] == 7
    np.testing.assert_array_equal(k['eps'], [0.5 / 100.0])
    assert k['targets'].shape == (1, 2, 5, 3) and k['target_nums'].dtype == np.int32
    assert 'pinned' in TG.probe_batch_sinkhorn.__doc__ and 'probe_every' in TG.probe_batch_sinkhorn.__doc__

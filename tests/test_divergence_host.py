"""Host: the reference of the Sinkhorn divergence (tests/_divergence_ref.py), the bias of the transport loss it removes, and
the options that carry the loss -- no device.

The clouds of (a)-(c) are the first n points of a square grid of spacing 0.02 in a plane, every coordinate moved by 0.002 x a
standard normal draw; eps = 0.02^2, the squared spacing (the trainer's default: transport_eps_scale 1 over the density).
(a) the gradient of pair64 equals central differences of its own value, at 9 x 12 displaced clouds and K = 300 (converged, so that
    the plans are constants of the derivative to rounding): within 1e-6 of the largest gradient component;
(b) at q = p, bit-equal clouds of 40 and 100 points, K = 50: |divergence| <= 1e-6 x the transport term and the largest gradient
    component <= 1e-2 x the transport gradient's on the same input -- a perfect prediction is left alone;
(c) 200 steps of gradient descent on p from p = q, 64 points, step n_p 3 / 8: the transport loss shrinks the radius of gyration by
    more than 2 %, the divergence changes it by less than 0.1 %;
(d) self_err <= 1e-9 at K = 50 on every case of _untracked_ref.chamfer_cases() at eps scale 1;
(e) the option plumbing of train_gnn_dyn: 'sinkhorn' is accepted everywhere, the probes refuse it, the transport loss's two options
    are range-checked with it, DIVERGENCE_LOSSES is there and the four older tuples are what they were.
Every figure is printed before it is asserted (DESIGN.md 9 records them)."""
import numpy as np
import pytest

import _divergence_ref as D
import _transport_ref as T
import _untracked_ref as U
from dyn_res_pile_manip_amd import synthetic as syn
from dyn_res_pile_manip_amd import train_gnn_dyn as TG

EPS = D.GRID_SPACING ** 2
K = 50


def gyration(x):
    return float(np.sqrt(((x - x.mean(axis=0)) ** 2).sum(axis=1).mean()))


# ---- (a) -------------------------------------------------------------------------------------------------------------------------
def test_gradient_agrees_with_central_differences_of_the_value():
    p64 = D.grid_cloud(9, 1).astype(np.float64)
    q = D.grid_cloud(12, 2, shift=(0.013, -0.007, 0.004)).astype(np.float64)
    grad = D.pair64(None, q, EPS, 300, p64=p64)[1]
    h = 1e-5                                                         # truncation ~ h^2 x third derivative, rounding ~ 1e-16 x value / h
    worst = 0.0
    for i in range(9):
        for k in range(3):
            vals = []
            for sgn in (1.0, -1.0):
                pp = p64.copy()
                pp[i, k] += sgn * h
                vals.append(D.pair64(None, q, EPS, 300, p64=pp)[0])
            worst = max(worst, abs((vals[0] - vals[1]) / (2 * h) - grad[i, k]))
    gmax = float(np.abs(grad).max())
    print('[divergence] 9 x 12, K = 300: central differences within %.2e of the gradient, largest component %.2e' % (worst, gmax))
    assert worst <= 1e-6 * gmax


# ---- (b) -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [40, 100])
def test_a_perfect_prediction_is_left_alone_where_transport_pushes_it(n):
    p = D.grid_cloud(n, 3)
    value, grad = D.pair64(p, p.copy(), EPS, K)[:2]
    term, tgrad = T.pair64(p, p.copy(), EPS, K)[:2]
    print('[divergence] q = p, %d points, K = %d: divergence %.2e against a transport term of %.2e; largest gradient component '
          '%.2e against transport\'s %.2e (ratio %.1e)' % (n, K, value, term, np.abs(grad).max(), np.abs(tgrad).max(),
                                                            np.abs(grad).max() / np.abs(tgrad).max()))
    assert abs(value) <= 1e-6 * term
    assert np.abs(grad).max() <= 1e-2 * np.abs(tgrad).max()


def test_transport_pushes_a_perfect_prediction():
    """the figures of the bias, printed for DESIGN.md 9: no bound but that the push is there"""
    p, q = D.grid_cloud(40, 3), D.grid_cloud(25, 4)
    same = np.abs(T.pair64(p, p.copy(), EPS, K)[1]).max()
    other = np.abs(T.pair64(p, q, EPS, K)[1]).max()
    print('[divergence] transport gradient, largest component: %.2e at q = p (40 x 40), %.2e for unrelated clouds (40 x 25)' % (same, other))
    assert same > 1e-2 * other


# ---- (c) -------------------------------------------------------------------------------------------------------------------------
def test_descent_shrinks_the_pile_under_transport_and_holds_it_under_the_divergence():
    q = D.grid_cloud(64, 5).astype(np.float64)
    n, steps = 64, 200
    lr = n * 3.0 / 8.0
    r0 = gyration(q)
    radius = {}
    for name, grad_of in (('transport', lambda x: T.pair64(None, q, EPS, K, p64=x)[1]),
                          ('divergence', lambda x: D.pair64(None, q, EPS, K, p64=x)[1])):
        x = q.copy()
        for _ in range(steps):
            x = x - lr * grad_of(x)
        radius[name] = gyration(x)
    shrink = {k: (r0 - v) / r0 for k, v in radius.items()}
    print('[divergence] %d steps of descent from p = q, 64 points: radius of gyration %.7f -> transport %.7f (%.2f %%), divergence '
          '%.7f (%.1e)' % (steps, r0, radius['transport'], 100 * shrink['transport'], radius['divergence'], shrink['divergence']))
    assert shrink['transport'] > 0.02
    assert abs(shrink['divergence']) < 1e-3


# ---- (d) -------------------------------------------------------------------------------------------------------------------------
def test_self_err_at_the_default_sweep_count():
    worst = 0.0
    for shape, B in U.chamfer_cases():
        p, q, n_p, n_q = U.chamfer_case(shape, B)
        ref = D.divergence64(p, q, n_p, n_q, T.case_eps(n_p, n_q), K)
        err = float(ref['self_err'].max())
        print('[divergence] %-22s B=%d K=%d: self_err %.2e, col_err %.2e, divergence %s' % (shape, B, K, err, ref['col_err'].max(),
                                                                                           ' '.join('%.3e' % v for v in ref['divergence'])))
        worst = max(worst, err)
        assert (ref['divergence'] > 0).all()                         # unrelated clouds: well above zero
    assert worst <= 1e-9


# ---- (e) -------------------------------------------------------------------------------------------------------------------------
def _depth_only_batch():
    z = np.zeros
    batch = TG.PaddedBatch((z((1, 3, 4, 3), np.float32), z((1, 2, 4, 3), np.float32), z((1, 3, 4), np.float32),
                            np.array([4], np.int32), np.array([100.0], np.float32), None, z((1, 2, 5, 3), np.float32),
                            np.array([[5, 5]], np.int32)))
    batch.actions = z((1, 2, 4), np.float32)
    batch.depth_only = True
    return batch


def test_the_new_loss_name_its_options_and_its_refusals(tmp_path):
    assert TG.LOSSES == ('mse', 'chamfer')                           # the four older tuples: unchanged
    assert TG.MATCH_LOSSES == ('match', 'chamfer+match')
    assert TG.TRANSPORT_LOSSES == ('transport',)
    assert TG.UNTRACKED_LOSSES == ('chamfer', 'match', 'chamfer+match', 'transport')
    assert TG.DIVERGENCE_LOSSES == ('sinkhorn',)
    config = syn.default_config()
    empty = {'train': [], 'valid': []}
    loss = 'sinkhorn'
    TG.check_loss(loss)
    TG.check_probe_options(loss, 0, 0)
    run = tmp_path / 'run'
    for kw in ({'probe_every': 1}, {'grad_probe_every': 1}):
        with pytest.raises(ValueError, match='no float64 yardstick'):
            TG.train(config, None, empty, loss=loss, **kw)
        with pytest.raises(ValueError, match='no float64 yardstick'):
            TG.main(config, data_root=str(tmp_path), train_dir=str(run), loss=loss, **kw)
    with pytest.raises(ValueError, match='no float64 yardstick'):
        TG.probe_batch(None, None, loss=loss)
    for argv in (['--probe-every', '2'], ['--grad-probe-every', '2']):
        with pytest.raises(ValueError, match='no float64 yardstick'):
            TG._cli(['--loss', loss] + argv + ['--data-root', str(tmp_path), '--train-dir', str(run)])
    assert TG.resolve_data_options('depth', 'sinkhorn', None) == ('sinkhorn', 'actions')
    assert TG.resolve_data_options('particles', loss, None) == (loss, 'data')
    assert TG.resolve_data_options('particles', loss, 'actions') == (loss, 'actions')
    with pytest.raises(ValueError, match='impulses'):
        TG.resolve_data_options('depth', loss, 'data')
    TG.check_depth_only(_depth_only_batch(), loss, 'actions')
    with pytest.raises(ValueError, match='depth-only'):
        TG.check_depth_only(_depth_only_batch(), loss, 'data')
    with pytest.raises(ValueError, match='depth-only'):
        TG.run_batch(None, None, _depth_only_batch(), loss=loss, impulses='data')
    # an unknown name: the message names the old tuples and the new one
    for call in (lambda: TG.train(config, None, empty, loss='emd'), lambda: TG.run_batch(None, None, None, loss='emd'),
                 lambda: TG.check_probe_options('emd', 0, 0)):
        with pytest.raises(ValueError, match='loss must be one of') as e:
            call()
        assert all(name in str(e.value) for name in ('mse', 'chamfer+match', 'transport', 'sinkhorn'))
    # the transport loss's two options apply: range-checked before anything is touched
    for bad in (0.0, -1.0, float('inf'), float('nan')):
        with pytest.raises(ValueError, match='transport_eps_scale'):
            TG.train(config, None, empty, loss=loss, transport_eps_scale=bad)
        with pytest.raises(ValueError, match='transport_eps_scale'):
            TG.run_batch(None, None, None, loss=loss, transport_eps_scale=bad)
        with pytest.raises(ValueError, match='transport_eps_scale'):
            TG.main(config, data_root=str(tmp_path), train_dir=str(run), loss=loss, transport_eps_scale=bad)
    for bad in (0, -3, TG.TRANSPORT_MAX_ITERS + 1, 2.5):
        with pytest.raises(ValueError, match='transport_iters'):
            TG.train(config, None, empty, loss=loss, transport_iters=bad)
        with pytest.raises(ValueError, match='transport_iters'):
            TG.run_batch(None, None, None, loss=loss, transport_iters=bad)
        with pytest.raises(ValueError, match='transport_iters'):
            TG.main(config, data_root=str(tmp_path), train_dir=str(run), loss=loss, transport_iters=bad)
    TG.check_loss(loss, 0.5, 0.25, 1)
    TG.check_loss(loss, 0.5, 4.0, TG.TRANSPORT_MAX_ITERS)
    assert not run.exists()                                          # main() refuses before it touches the disk or a device
    for argv in (['--loss', 'sinkhorn', '--transport-iters', '0'], ['--loss', 'sinkhorn', '--transport-eps-scale', '0'],
                 ['--data', 'depth', '--loss', 'sinkhorn', '--transport-iters', '1001'],
                 ['--data', 'depth', '--loss', 'sinkhorn', '--impulses', 'data']):
        with pytest.raises((SystemExit, ValueError)):
            TG._cli(argv + ['--data-root', str(tmp_path), '--train-dir', str(run)])
    assert not run.exists()

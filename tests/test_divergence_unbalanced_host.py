"""Host: the reference of the unbalanced Sinkhorn divergence (tests/_divergence_unbalanced_ref.py), what a finite reach does on a
pile seen partly, and the options that carry it -- no device.

Clouds and eps are tests/test_divergence_host.py's: a jittered grid of spacing 0.02, eps = 0.02^2.  rho = reach; w = the target's
total mass.
(a) the gradient of pair64 equals central differences of its own value at (rho / eps, w) in {(4, 1), (25, 1), (4, 0.6), (25, 12/9)},
    9 x 12 displaced clouds, K = 300.  MEASURED on this reference (worst of the four): 9.5e-10 of the largest gradient component
    (step 1e-6); the bound is 5 x that, below 1e-6;
(b) reach = inf, w = 1 returns _divergence_ref.pair64's bits;
(c) rho = 1e6 eps: the value is within 1e-5 (relative) of the balanced one (measured 2.7e-6);
(d) the half-seen pile (half_seen_pile: a correct 12 x 6 prediction whose columns 6..11 were not observed), rho = 4 eps,
    w = n_q / n_p, K = 50: the unseen columns 9..11 get at most 0.1 of the balanced mean gradient norm there, the seen columns
    0..3 at most 0.05 of the balanced mean over the unseen columns 6..11, col_err <= 1e-6;
(e) p == q, 40 and 100 points, rho = 4 eps: |value| and the largest gradient component at most 1e-10;
(f) K = 50, rho = 4 eps: col_err <= 1e-6 and self_err <= 1e-9 on every shape of tests/test_gpu_divergence.py's SHAPES for
    w in {1, n_q / n_p};
(g) every option, default and refusal of train_gnn_dyn and the reference's parameter ranges.
Every figure is printed before it is asserted (DESIGN.md 9 records them)."""
import inspect

import numpy as np
import pytest

import _divergence_ref as D
import _divergence_unbalanced_ref as R
import _untracked_ref as U
from dyn_res_pile_manip_amd import synthetic as syn
from dyn_res_pile_manip_amd import train_gnn_dyn as TG

EPS = D.GRID_SPACING ** 2
K = 50
# tests/test_gpu_divergence.py's SHAPES (that module needs the device library to import)
SHAPES = [(1, 1, 1, 1), (1, 7, 4, 9), (5, 3, 8, 8), (3, 5, 8, 8), (64, 64, 70, 66), (65, 63, 65, 64), (257, 300, 260, 300),
          (16, 17, 20, 20), (33, 32, 40, 40)]
FD_MEASURED = 9.5e-10                                                # (a): the module docstring's figure
FD_BOUND = 5 * FD_MEASURED
assert FD_BOUND < 1e-6


# ---- (a) -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ratio,w', [(4, 1.0), (25, 1.0), (4, 0.6), (25, 12 / 9)])
def test_gradient_agrees_with_central_differences_of_the_value(ratio, w):
    p64 = D.grid_cloud(9, 1).astype(np.float64)
    q = D.grid_cloud(12, 2, shift=(0.01, -0.005, 0.0))
    rho = ratio * EPS
    grad = R.pair64(None, q, EPS, rho, w, 300, p64=p64)[1]
    h = 1e-6
    worst = 0.0
    for i in range(9):
        for k in range(3):
            vals = []
            for sgn in (1.0, -1.0):
                pp = p64.copy()
                pp[i, k] += sgn * h
                vals.append(R.pair64(None, q, EPS, rho, w, 300, p64=pp)[0])
            worst = max(worst, abs((vals[0] - vals[1]) / (2 * h) - grad[i, k]))
    gmax = float(np.abs(grad).max())
    print('[unbalanced] 9 x 12, K = 300, rho = %g eps, w = %.3f: central differences within %.2e of the gradient\'s largest component %.2e'
          % (ratio, w, worst / gmax, gmax))
    assert worst <= FD_BOUND * gmax


# ---- (b), (c) --------------------------------------------------------------------------------------------------------------------
def test_an_infinite_reach_is_the_balanced_code_and_a_large_one_its_limit():
    p, q = D.grid_cloud(9, 1), D.grid_cloud(12, 2, shift=(0.01, -0.005, 0.0))
    for k in (1, K):
        got, want = R.pair64(p, q, EPS, np.inf, 1.0, k, want_plans=True), D.pair64(p, q, EPS, k, want_plans=True)
        assert len(got) == len(want) + 1
        for a, b in zip(got[:8] + got[9:], want):
            assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
        assert abs(got[8] - 1.0) <= 1e-15
    batch = R.divergence64(p[None], q[None], [9], [12], EPS, np.inf, 1.0, K)
    plain = D.divergence64(p[None], q[None], [9], [12], EPS, K)
    for key in plain:
        assert batch[key].tobytes() == plain[key].tobytes(), key
    balanced = D.pair64(p, q, EPS, 300)[0]
    large = R.pair64(p, q, EPS, 1e6 * EPS, 1.0, 300)[0]
    rel = abs(large - balanced) / abs(balanced)
    print('[unbalanced] 9 x 12, K = 300: rho = 1e6 eps gives %.9e, balanced %.9e, rel %.2e' % (large, balanced, rel))
    assert rel <= 1e-5


# ---- (d) -------------------------------------------------------------------------------------------------------------------------
def half_seen_thresholds(balanced_grad, grad, col, col_err, label):
    """the three thresholds of (d), shared with tests/test_gpu_divergence_unbalanced.py"""
    nb, nu = R.column_norms(balanced_grad, col), R.column_norms(grad, col)
    unseen, seen = nu[9:].mean() / nb[9:].mean(), nu[:4].mean() / nb[6:].mean()
    print('[unbalanced] %s half-seen pile, mean gradient norm per column\n  balanced   %s\n  unbalanced %s\n  columns 9-11: %.3f of the '
          'balanced; columns 0-3: %.4f of the balanced unseen mean; col_err %.2e'
          % (label, ' '.join('%.1e' % v for v in nb), ' '.join('%.1e' % v for v in nu), unseen, seen, col_err))
    assert unseen <= 0.1
    assert seen <= 0.05
    assert col_err <= 1e-6


def test_a_finite_reach_leaves_the_unseen_side_and_the_seen_interior_alone():
    p, q, col = R.half_seen_pile()
    assert p.shape == (72, 3) and q.shape == (36, 3)
    balanced = D.pair64(p, q, EPS, K)
    got = R.pair64(p, q, EPS, 4 * EPS, len(q) / len(p), K)
    unit = R.pair64(p, q, EPS, 4 * EPS, 1.0, K)
    print('[unbalanced] unit masses instead: %s; transported %.3f (count) %.3f (unit)'
          % (' '.join('%.1e' % v for v in R.column_norms(unit[1], col)), got[8], unit[8]))
    half_seen_thresholds(balanced[1], got[1], col, got[6], 'float64 reference:')
    assert 0.0 < got[8] <= 1.0


# ---- (e) -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [40, 100])
def test_equal_clouds_have_no_value_and_no_gradient(n):
    p = D.grid_cloud(n, 3)
    value, grad = R.pair64(p, p.copy(), EPS, 4 * EPS, 1.0, K)[:2]
    print('[unbalanced] q = p, %d points, rho = 4 eps: value %.2e, largest gradient component %.2e' % (n, value, np.abs(grad).max()))
    assert abs(value) <= 1e-10 and np.abs(grad).max() <= 1e-10


# ---- (f) -------------------------------------------------------------------------------------------------------------------------
def test_the_certificates_at_the_default_sweep_count():
    worst_col = worst_self = 0.0
    for shape in SHAPES:
        p, q, n_p, n_q = U.chamfer_case(shape, 1, seed=0)
        n, m = int(n_p[0]), int(n_q[0])
        for w in (1.0, m / n):
            out = R.pair64(p[0, :n], q[0, :m], EPS, 4 * EPS, w, K)
            worst_col, worst_self = max(worst_col, out[6]), max(worst_self, float(out[7].max()))
            assert out[6] <= 1e-6 and out[7].max() <= 1e-9, (shape, w, out[6], out[7])
            assert 0.0 < out[8] <= max(1.0, w) + 1e-12
    print('[unbalanced] K = %d, rho = 4 eps, every shape and both masses: worst col_err %.2e, worst self_err %.2e' % (K, worst_col, worst_self))


# ---- (g) -------------------------------------------------------------------------------------------------------------------------
def test_the_reference_refuses_what_the_entry_points_refuse():
    p, q = D.grid_cloud(5, 1), D.grid_cloud(3, 2)
    for rho, w in ((0.0, 1.0), (-EPS, 1.0), (EPS / 1025, 1.0), (np.nan, 1.0), (-np.inf, 1.0), (4 * EPS, 0.124), (4 * EPS, 8.01),
                   (4 * EPS, np.nan), (np.inf, 0.6)):
        with pytest.raises(ValueError):
            R.pair64(p, q, EPS, rho, w, 3)
    R.pair64(p, q, EPS, EPS / 1024, 0.125, 3)
    R.pair64(p, q, EPS, 4 * EPS, 8.0, 3)


def test_the_options_their_defaults_and_their_refusals(tmp_path):
    config = syn.default_config()
    empty = {'train': [], 'valid': []}
    run = tmp_path / 'run'
    for fn in (TG.run_batch, TG.train, TG.main):
        sig = inspect.signature(fn).parameters
        assert sig['sinkhorn_reach_scale'].default is None and sig['sinkhorn_mass'].default == 'unit'
    assert TG.SINKHORN_MASSES == ('unit', 'count')
    # accepted: balanced by default, a reach with either mass, an infinite reach with unit masses
    TG.check_sinkhorn_options('sinkhorn')
    TG.check_sinkhorn_options('mse')
    for mass in TG.SINKHORN_MASSES:
        TG.check_sinkhorn_options('sinkhorn', 4.0, mass)
    TG.check_sinkhorn_options('sinkhorn', float('inf'), 'unit')
    TG.check_sinkhorn_options('sinkhorn', 1.0 / 1024, 'unit')
    TG.check_sinkhorn_options('sinkhorn', None, 'unit', 3)           # the balanced loss keeps its probe
    # every way in refuses the same things, before it touches the disk or a device
    ways = (lambda **kw: TG.train(config, None, empty, **kw), lambda **kw: TG.run_batch(None, None, None, **kw),
            lambda **kw: TG.main(config, data_root=str(tmp_path), train_dir=str(run), **kw))
    for call in ways:
        for loss in ('mse', 'chamfer', 'match', 'chamfer+match', 'transport'):
            with pytest.raises(ValueError, match='sinkhorn_reach_scale'):
                call(loss=loss, sinkhorn_reach_scale=4.0)
            with pytest.raises(ValueError, match='sinkhorn_mass'):
                call(loss=loss, sinkhorn_mass='count')
        with pytest.raises(ValueError, match='needs sinkhorn_reach_scale'):
            call(loss='sinkhorn', sinkhorn_mass='count')
        with pytest.raises(ValueError, match='finite sinkhorn_reach_scale'):
            call(loss='sinkhorn', sinkhorn_reach_scale=float('inf'), sinkhorn_mass='count')
        with pytest.raises(ValueError, match='sinkhorn_mass must be one of'):
            call(loss='sinkhorn', sinkhorn_reach_scale=4.0, sinkhorn_mass='equal')
        for bad in (0.0, -4.0, float('nan'), 1.0 / 1025):
            with pytest.raises(ValueError, match='sinkhorn_reach_scale'):
                call(loss='sinkhorn', sinkhorn_reach_scale=bad)
    for call in ways[::2]:                                           # (run_batch has no probe schedule)
        with pytest.raises(ValueError, match='no float64 yardstick for the unbalanced'):
            call(loss='sinkhorn', sinkhorn_reach_scale=4.0, sinkhorn_probe_every=2)
    tail = ['--data-root', str(tmp_path), '--train-dir', str(run)]
    for argv in (['--loss', 'sinkhorn', '--sinkhorn-mass', 'count'], ['--loss', 'transport', '--sinkhorn-reach-scale', '4'],
                 ['--sinkhorn-reach-scale', '4'], ['--loss', 'sinkhorn', '--sinkhorn-reach-scale', '0'],
                 ['--loss', 'sinkhorn', '--sinkhorn-reach-scale', '4', '--sinkhorn-mass', 'equal'],
                 ['--loss', 'sinkhorn', '--sinkhorn-reach-scale', '4', '--sinkhorn-probe-every', '2'],
                 ['--data', 'depth', '--loss', 'sinkhorn', '--sinkhorn-reach-scale', 'inf', '--sinkhorn-mass', 'count']):
        with pytest.raises(SystemExit):
            TG._cli(argv + tail)
    assert not run.exists()
    # the two derived arrays
    dens = np.array([2500.0, 400.0], np.float32)
    np.testing.assert_array_equal(TG.sinkhorn_reach(dens, 4.0), 4.0 / dens.astype(np.float64))
    np.testing.assert_array_equal(TG.sinkhorn_reach(dens, 4.0), 4.0 * TG.transport_eps(dens, 1.0))
    nums, tnums = np.array([9, 6], np.int32), np.array([[12, 7], [5, 10]], np.int32)
    np.testing.assert_array_equal(TG.sinkhorn_mass_q('unit', nums, tnums), np.ones((2, 2)))
    np.testing.assert_array_equal(TG.sinkhorn_mass_q('count', nums, tnums), np.array([[12 / 9, 5 / 6], [7 / 9, 10 / 6]]))
    with pytest.raises(ValueError, match='1/8'):
        TG.sinkhorn_mass_q('count', np.array([90], np.int32), np.array([[10]], np.int32))


def test_the_engine_refuses_the_new_arguments_without_a_reach():
    """Engine.cloud_divergence / train_step_divergence: reach=None is the balanced call, which has neither a mass nor a
    transported share -- refused before the library is touched"""
    from dyn_res_pile_manip_amd.engine import Engine
    e = object.__new__(Engine)                                       # no context: the refusals come first
    p = D.grid_cloud(5, 1)[None]
    for kw in ({'mass_q': 0.6}, {'want_transported': True}):
        with pytest.raises(ValueError, match='give reach'):
            Engine.cloud_divergence(e, p, p, eps=EPS, iters=3, **kw)
    with pytest.raises(ValueError, match='give reach'):
        Engine.train_step_divergence(e, None, None, None, None, None, None, EPS, 3, states_delta=p, mass_q=0.6)
    sig = inspect.signature(Engine.cloud_divergence).parameters
    assert sig['reach'].default is None and sig['mass_q'].default is None and sig['want_transported'].default is False
    sig = inspect.signature(Engine.train_step_divergence).parameters
    assert sig['reach'].default is None and sig['mass_q'].default is None

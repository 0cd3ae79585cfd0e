"""Host: the reference of the entropy-regularised transport loss (tests/_transport_ref.py) and the options that carry the loss --
no device.

(a) the plan's row sums are a_i to 1e-14 (the last update is f's), on every case of _untracked_ref.chamfer_cases();
(b) col_err falls strictly with K on a 5 x 3 and a 64 x 64 case, over sweep counts that keep it above the double rounding floor;
(c) central differences of the term with the plan held fixed agree with the gradient: tests/test_match_host.py's step 2^-20 and
    bound 1e-5 of the largest entry;
(d) equal counts, a well-separated 8 x 8 case, eps = 1e-2, 1e-3, 1e-4 of the mean cost with col_err < 1e-9: the term approaches
    the matching term monotonically.  Both sides read the same fp32 cost matrix, so the limit is match64's `cost` / (3 r); its
    `match` (squared fp32 differences summed in double) is within the fp32 rounding of a cost, 2^-22.  "Monotonically" holds to
    the rounding of each eps: a plan entry is exp of an exponent of size max C / eps, rounded to 2^-52 of that size a few times;
(e) the default sweep count is the smallest of {10, 20, 50, 100, 200} whose col_err is at most 1 % of the total mass on every case
    of chamfer_cases() at eps scale 1 (the table is printed; DESIGN.md 9 records it);
(f) the option plumbing of train_gnn_dyn: the new name is accepted everywhere, the probes refuse it, the two new options are
    range-checked, TRANSPORT_LOSSES is there and LOSSES and MATCH_LOSSES are what they were."""
import numpy as np
import pytest

import _match_ref as R
import _transport_ref as T
import _untracked_ref as U
from dyn_res_pile_manip_amd import synthetic as syn
from dyn_res_pile_manip_amd import train_gnn_dyn as TG

FD_H = 2.0 ** -20           # tests/test_match_host.py
FD_BOUND = 1e-5


@pytest.fixture(scope='module')
def col_err_table():
    """col_err of every case of chamfer_cases() at every candidate sweep count, eps scale 1: computed once"""
    table = {}
    for shape, B in U.chamfer_cases():
        p, q, n_p, n_q = U.chamfer_case(shape, B)
        for K in T.ITERS_CANDIDATES:
            table[(shape, B, K)] = T.transport64(p, q, n_p, n_q, T.case_eps(n_p, n_q), K)
    return table


# ---- (a) -------------------------------------------------------------------------------------------------------------------------
def test_row_sums_are_the_row_masses(col_err_table):
    worst = max(float(r['row_err'].max()) for r in col_err_table.values())
    print('[transport] largest |n_p sum_j P_ij - 1| over %d solves: %.2e' % (len(col_err_table), worst))
    assert worst <= 1e-14


# ---- (b) -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,sweeps', [((5, 3, 8, 8), (1, 2, 3, 5, 8, 10)), ((64, 64, 64, 64), (1, 2, 5, 10, 20, 50))])
def test_col_err_falls_with_the_sweeps(shape, sweeps):
    p, q, n_p, n_q = U.chamfer_case(shape, 1)
    errs = [float(T.transport64(p, q, n_p, n_q, T.case_eps(n_p, n_q), K)['col_err'][0]) for K in sweeps]
    print('[transport] %s: col_err over K = %s: %s' % (shape, sweeps, ' '.join('%.2e' % e for e in errs)))
    assert all(a > b for a, b in zip(errs, errs[1:]))
    assert errs[-1] > 1e-13                                           # (still above the rounding floor: the comparison means something)


# ---- (c) -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(5, 3, 8, 8), (3, 5, 8, 8), (70, 130, 70, 130), (64, 64, 64, 64)])
def test_gradient_agrees_with_central_differences_of_the_term_with_the_plan_fixed(shape):
    p, q, n_p, n_q = U.chamfer_case(shape, 1)
    n, m = int(n_p[0]), int(n_q[0])
    p64, q64 = p[0, :n].astype(np.float64), q[0, :m].astype(np.float64)
    term, g, _, _, _, P = T.pair64(None, q64, float(T.case_eps(n_p, n_q)[0]), 20, p64=p64)

    def term_at(pp):
        d = pp[:, None, :] - q64[None, :, :]
        return float((P * (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])).sum() / 3.0)
    assert abs(term_at(p64) - term) <= 1e-15 * term
    assert (np.abs(g).max(axis=1) > 0).all()                          # every real row has a gradient, whichever cloud is larger
    worst = 0.0
    order = np.argsort(-np.abs(g).ravel())
    for flat in list(order[:3]) + [order[len(order) // 2]]:
        i, k = np.unravel_index(int(flat), g.shape)
        vals = []
        for sgn in (1.0, -1.0):
            pp = p64.copy()
            pp[i, k] += sgn * FD_H
            vals.append(term_at(pp))
        cd = (vals[0] - vals[1]) / (2 * FD_H)
        res = abs(cd - g[i, k]) / np.abs(g).max()
        worst = max(worst, res)
        assert res < FD_BOUND, (shape, i, k, cd, g[i, k])
    print('[transport] %s: central differences on 4 entries, worst residual %.3e' % (shape, worst))


# ---- (d) -------------------------------------------------------------------------------------------------------------------------
def separated_case():
    """8 points near the corners of a cube of side 0.05 and a shuffled copy moved by a fifth of that: one clear matching"""
    rng = np.random.default_rng(3)
    g = np.stack(np.meshgrid(*[np.arange(2)] * 3, indexing='ij'), -1).reshape(-1, 3)
    p = (0.2 + 0.05 * g + 0.004 * rng.standard_normal((8, 3))).astype(np.float32)
    q = (p[rng.permutation(8)] + 0.011 * rng.standard_normal((8, 3))).astype(np.float32)
    return p, q


def test_the_term_tends_to_the_matching_term_as_eps_falls():
    p, q = separated_case()
    C = R.cost32(p, q).astype(np.float64)
    ref = R.match64(p[None], q[None], [8], [8])
    limit = ref['cost'][0] / (3.0 * 8)
    d, tol = [], []
    for frac in (1e-2, 1e-3, 1e-4):
        eps = frac * C.mean()
        term, _, _, _, col_err, _ = T.pair64(p, q, eps, 50)
        assert col_err < 1e-9, (frac, col_err)
        d.append(abs(term - limit))
        tol.append(term * 2.0 ** -52 * (64 + 8 * C.max() / eps))
        print('[transport] eps = %g of the mean cost: col_err %.2e, term - matching %.3e (rounding bound %.1e), against match64\'s '
              'double sum %.2e rel' % (frac, col_err, term - limit, tol[-1], abs(term - ref['match'][0]) / term))
        assert abs(term - ref['match'][0]) <= 2.0 ** -22 * term
    assert d[0] > 100 * tol[0]                                       # the approach is visible above the rounding ...
    assert d[0] >= d[1] - tol[1] and d[1] >= d[2] - tol[2]           # ... monotone ...
    assert d[2] <= tol[2]                                            # ... and arrives


# ---- (e) -------------------------------------------------------------------------------------------------------------------------
def test_the_default_sweep_count_is_the_smallest_candidate_within_one_percent(col_err_table):
    worst = {K: 0.0 for K in T.ITERS_CANDIDATES}
    for shape, B in U.chamfer_cases():
        errs = [float(col_err_table[(shape, B, K)]['col_err'].max()) for K in T.ITERS_CANDIDATES]
        print('[transport] %-22s B=%d col_err at K = %s: %s' % (shape, B, T.ITERS_CANDIDATES, ' '.join('%.2e' % e for e in errs)))
        for K, e in zip(T.ITERS_CANDIDATES, errs):
            worst[K] = max(worst[K], e)
    print('[transport] worst over the cases: %s' % ' '.join('K=%d %.2e' % (K, worst[K]) for K in T.ITERS_CANDIDATES))
    enough = [K for K in T.ITERS_CANDIDATES if worst[K] <= T.COL_ERR_MAX]
    assert enough and TG.TRANSPORT_ITERS == enough[0]
    assert TG.TRANSPORT_EPS_SCALE == T.EPS_SCALE == 1.0


# ---- (f) -------------------------------------------------------------------------------------------------------------------------
def _depth_only_batch():
    z = np.zeros
    batch = TG.PaddedBatch((z((1, 3, 4, 3), np.float32), z((1, 2, 4, 3), np.float32), z((1, 3, 4), np.float32),
                            np.array([4], np.int32), np.array([100.0], np.float32), None, z((1, 2, 5, 3), np.float32),
                            np.array([[5, 5]], np.int32)))
    batch.actions = z((1, 2, 4), np.float32)
    batch.depth_only = True
    return batch


def test_the_new_loss_name_its_options_and_its_refusals(tmp_path):
    assert TG.LOSSES == ('mse', 'chamfer')                           # unchanged
    assert TG.MATCH_LOSSES == ('match', 'chamfer+match')             # unchanged
    assert TG.TRANSPORT_LOSSES == ('transport',)
    assert TG.UNTRACKED_LOSSES == ('chamfer', 'match', 'chamfer+match', 'transport')
    config = syn.default_config()
    empty = {'train': [], 'valid': []}
    loss = 'transport'
    TG.check_loss(loss)
    TG.check_probe_options(loss, 0, 0)
    for kw in ({'probe_every': 1}, {'grad_probe_every': 1}):
        with pytest.raises(ValueError, match='no float64 yardstick'):
            TG.train(config, None, empty, loss=loss, **kw)
        with pytest.raises(ValueError, match='no float64 yardstick'):
            TG.main(config, data_root=str(tmp_path), train_dir=str(tmp_path / 'run'), loss=loss, **kw)
    with pytest.raises(ValueError, match='no float64 yardstick'):
        TG.probe_batch(None, None, loss=loss)
    assert TG.resolve_data_options('depth', loss, None) == (loss, 'actions')
    assert TG.resolve_data_options('particles', loss, None) == (loss, 'data')
    assert TG.resolve_data_options('particles', loss, 'actions') == (loss, 'actions')
    TG.check_depth_only(_depth_only_batch(), loss, 'actions')
    with pytest.raises(ValueError, match='depth-only'):
        TG.check_depth_only(_depth_only_batch(), loss, 'data')
    with pytest.raises(ValueError, match='depth-only'):
        TG.run_batch(None, None, _depth_only_batch(), loss=loss, impulses='data')
    # 'emd' is still no name, and the message still lists the two old tuples
    for call in (lambda: TG.train(config, None, empty, loss='emd'), lambda: TG.run_batch(None, None, None, loss='emd'),
                 lambda: TG.check_probe_options('emd', 0, 0)):
        with pytest.raises(ValueError, match='loss must be one of') as e:
            call()
        assert 'chamfer+match' in str(e.value) and 'mse' in str(e.value) and 'transport' in str(e.value)
    # the two new options: read by the transport loss only, range-checked before anything is touched
    for bad in (0.0, -1.0, float('inf'), float('nan')):
        with pytest.raises(ValueError, match='transport_eps_scale'):
            TG.train(config, None, empty, loss=loss, transport_eps_scale=bad)
        with pytest.raises(ValueError, match='transport_eps_scale'):
            TG.run_batch(None, None, None, loss=loss, transport_eps_scale=bad)
        with pytest.raises(ValueError, match='transport_eps_scale'):
            TG.main(config, data_root=str(tmp_path), train_dir=str(tmp_path / 'run'), loss=loss, transport_eps_scale=bad)
        TG.check_loss('match', 0.5, bad)
    for bad in (0, -3, TG.TRANSPORT_MAX_ITERS + 1, 2.5):
        with pytest.raises(ValueError, match='transport_iters'):
            TG.train(config, None, empty, loss=loss, transport_iters=bad)
        with pytest.raises(ValueError, match='transport_iters'):
            TG.run_batch(None, None, None, loss=loss, transport_iters=bad)
        with pytest.raises(ValueError, match='transport_iters'):
            TG.main(config, data_root=str(tmp_path), train_dir=str(tmp_path / 'run'), loss=loss, transport_iters=bad)
        TG.check_loss('chamfer', 0.5, 1.0, bad)
    TG.check_loss(loss, 0.5, 0.25, 1)
    TG.check_loss(loss, 0.5, 4.0, TG.TRANSPORT_MAX_ITERS)
    assert not (tmp_path / 'run').exists()                           # main() refuses before it touches the disk or a device
    for argv in (['--loss', 'emd'], ['--loss', 'transport', '--transport-iters', '0'],
                 ['--loss', 'transport', '--transport-eps-scale', '0'], ['--loss', 'transport', '--probe-every', '2'],
                 ['--data', 'depth', '--loss', 'transport', '--transport-iters', '1001']):
        with pytest.raises((SystemExit, ValueError)):
            TG._cli(argv + ['--data-root', str(tmp_path), '--train-dir', str(tmp_path / 'run')])
    assert not (tmp_path / 'run').exists()


def test_eps_is_the_scale_over_the_density():
    dens = np.array([2500.0, 1600.0, 400.0], np.float32)
    np.testing.assert_array_equal(TG.transport_eps(dens), 1.0 / dens.astype(np.float64))
    np.testing.assert_array_equal(TG.transport_eps(dens, 0.5), 0.5 / dens.astype(np.float64))
    assert TG.transport_eps(dens).dtype == np.float64

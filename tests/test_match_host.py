"""Host: the oracle of the one-to-one matching loss (tests/_match_ref.py) and the options that carry the loss -- no device.

(a) assign64 against brute force over ALL injections for every shape with r <= 6, c <= 7, its uniqueness margin against the
    brute-force second best, and against scipy.optimize.linear_sum_assignment where scipy imports.
(b) match64's gradient against its own central differences, with the step and the bound of tests/test_untracked_host.py
    (FD_H = 2^-20, 1e-5 of the largest entry).
(c) THE PRECONDITION OF THE GPU COMPARISONS: on every case of _untracked_ref.chamfer_cases() the optimum of the fp32 cost matrix
    is unique by a margin of at least MARGIN_MIN = 1e-9 -- 10^5 times the double rounding r 2^-52 max C = 1e-14 of these sizes --
    so any exact solver returns assign64's partners.  The smallest over the 14 cases (26 sample pairs) is 2.59e-7, at the
    64 x 64 pair of the B = 3 case.
(d) the option plumbing of train_gnn_dyn: the new names are accepted, 'emd' is still refused, the probes are refused with the
    new losses, match_weight is range-checked, LOSSES is what it was."""
from itertools import permutations

import numpy as np
import pytest

import _match_ref as R
import _untracked_ref as U
from dyn_res_pile_manip_amd import synthetic as syn
from dyn_res_pile_manip_amd import train_gnn_dyn as TG

FD_H = 2.0 ** -20           # tests/test_untracked_host.py
FD_BOUND = 1e-5


# ---- (a) the solver -----------------------------------------------------------------------------------------------------------
def two_best(C):
    """the least and the second least cost over all injections of the rows into the columns"""
    r, c = C.shape
    costs = sorted(float(C[np.arange(r), list(perm)].sum()) for perm in permutations(range(c), r))
    return costs[0], (costs[1] if len(costs) > 1 else np.inf)


@pytest.mark.parametrize('r', range(1, 7))
def test_assign64_against_brute_force(r):
    rng = np.random.default_rng(100 + r)
    for c in range(r, 8):
        for trial in range(2):
            # costs of the clouds' scale as float32 (trial 0), and small integers with many exact ties (trial 1)
            C = (1e-3 * rng.random((r, c))).astype(np.float32) if trial == 0 else rng.integers(0, 4, (r, c)).astype(np.float64)
            col, cost, margin, (u, v) = R.assign64(C)
            best, second = two_best(np.asarray(C, np.float64))
            assert len(set(col.tolist())) == r and col.min() >= 0 and col.max() < c
            assert abs(cost - best) <= 1e-15 * max(best, 1.0), (r, c, trial, cost, best)
            assert abs(cost - R.brute_force(C)) <= 1e-15 * max(best, 1.0)
            want = second - best
            assert (margin == want == np.inf) or abs(margin - want) <= 1e-15 * max(second, 1.0), (r, c, trial, margin, want)
            # the duals certify it: feasible, tight on the pairs, zero on the free columns
            C64 = np.asarray(C, np.float64)
            slack = C64 - u[:, None] - v[None, :]
            assert slack.min() >= -1e-15 and np.abs(slack[np.arange(r), col]).max() <= 1e-15
            free = np.ones(c, bool)
            free[col] = False
            assert (v[free] == 0).all()


def test_solve_pair_takes_the_smaller_cloud_as_rows():
    rng = np.random.default_rng(5)
    C = rng.random((6, 4))
    pq, qp, cost, margin, u, v = R.solve_pair(C)
    assert (pq >= 0).sum() == 4 and (qp >= 0).all() and u.shape == (6,) and v.shape == (4,)
    np.testing.assert_array_equal(pq[qp], np.arange(4))
    assert abs(cost - R.brute_force(C.T)) <= 1e-15
    assert (u[pq < 0] == 0).all()                                    # the larger cloud's unmatched rows


def test_assign64_against_scipy():
    lsa = pytest.importorskip('scipy.optimize').linear_sum_assignment
    rng = np.random.default_rng(9)
    for r, c in ((1, 1), (7, 7), (12, 40), (40, 40), (64, 65), (100, 130)):
        C = rng.random((r, c))
        col, cost, _, _ = R.assign64(C, want_margin=False)
        ri, ci = lsa(C)
        assert abs(cost - C[ri, ci].sum()) <= 1e-12 * cost
    for shape, B in U.chamfer_cases():
        p, q, n_p, n_q = U.chamfer_case(shape, B)
        ref = R.match64(p, q, n_p, n_q, want_margin=False)
        for b in range(B):
            C = R.cost32(p[b, :n_p[b]], q[b, :n_q[b]]).astype(np.float64)
            C = C if C.shape[0] <= C.shape[1] else C.T
            ri, ci = lsa(C)
            assert abs(ref['cost'][b] - C[ri, ci].sum()) <= 1e-12 * ref['cost'][b], (shape, B, b)


def test_cost32_is_float32_arithmetic_in_the_kernels_order():
    p = np.array([[0.1, 0.2, 0.3], [1.0 / 3.0, 2.0 / 3.0, 0.7]], np.float32)
    q = np.array([[0.25, 0.15, 0.35]], np.float32)
    C = R.cost32(p, q)
    for i in range(2):
        d = [np.float32(p[i, k] - q[0, k]) for k in range(3)]
        want = np.float32(np.float32(np.float32(d[0] * d[0]) + np.float32(d[1] * d[1])) + np.float32(d[2] * d[2]))
        assert C[i, 0] == want and C.dtype == np.float32


def test_where_the_matching_is_the_tracked_correspondence_the_term_is_the_mse_term():
    rng = np.random.default_rng(2)
    p = (0.2 + 0.1 * rng.random((1, 40, 3))).astype(np.float32)
    q = (p + 1e-5 * rng.standard_normal(p.shape)).astype(np.float32)
    ref = R.match64(p, q, [40], [40], exact32=False)
    mse = float(((p.astype(np.float64) - q.astype(np.float64)) ** 2).mean())
    np.testing.assert_array_equal(ref['match_pq'][0], np.arange(40))
    assert abs(ref['match'][0] - mse) <= 1e-14 * mse


# ---- (b) central differences ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(5, 3, 8, 8), (3, 5, 8, 8), (70, 130, 70, 130), (64, 64, 64, 64)])
def test_match64_agrees_with_its_central_differences(shape):
    p, q, n_p, n_q = U.chamfer_case(shape, 1)
    p64 = p.astype(np.float64)
    ref = R.match64(p64, q, n_p, n_q, exact32=False)
    g = ref['grad'][0]
    assert (g[n_p[0]:] == 0).all() and (g[:n_p[0]][ref['match_pq'][0, :n_p[0]] < 0] == 0).all()
    worst = 0.0
    order = np.argsort(-np.abs(g).ravel())
    for flat in list(order[:3]) + [order[len(order) // 2]]:
        i, k = np.unravel_index(int(flat), g.shape)
        vals = []
        for sgn in (1.0, -1.0):
            pp = p64.copy()
            pp[0, i, k] += sgn * FD_H
            out = R.match64(pp, q, n_p, n_q, exact32=False, want_margin=False)
            np.testing.assert_array_equal(out['match_pq'], ref['match_pq'])     # the matching is a constant of the derivative
            vals.append(out['match'][0])
        cd = (vals[0] - vals[1]) / (2 * FD_H)
        res = abs(cd - g[i, k]) / np.abs(g).max()
        worst = max(worst, res)
        assert res < FD_BOUND, (shape, i, k, cd, g[i, k])
    print('[match] %s: central differences on 4 entries, worst residual %.3e' % (shape, worst))


# ---- (c) the precondition of the GPU comparisons ----------------------------------------------------------------------------
@pytest.mark.parametrize('shape,B', U.chamfer_cases())
def test_margins_of_the_stand_alone_cases(shape, B):
    p, q, n_p, n_q = U.chamfer_case(shape, B)
    ref = R.match64(p, q, n_p, n_q)
    print('[match] %s B=%d: uniqueness margins %s' % (shape, B, ref['margin']))
    assert ref['margin'].min() >= R.MARGIN_MIN


# ---- (d) the options --------------------------------------------------------------------------------------------------------
def _depth_only_batch():
    z = np.zeros
    batch = TG.PaddedBatch((z((1, 3, 4, 3), np.float32), z((1, 2, 4, 3), np.float32), z((1, 3, 4), np.float32),
                            np.array([4], np.int32), np.array([100.0], np.float32), None, z((1, 2, 5, 3), np.float32),
                            np.array([[5, 5]], np.int32)))
    batch.actions = z((1, 2, 4), np.float32)
    batch.depth_only = True
    return batch


def test_the_new_loss_names_and_their_refusals(tmp_path):
    assert TG.LOSSES == ('mse', 'chamfer')                           # unchanged: the probes work for every member
    assert TG.MATCH_LOSSES == ('match', 'chamfer+match') == R.LOSSES
    config = syn.default_config()
    empty = {'train': [], 'valid': []}
    for loss in TG.MATCH_LOSSES:
        TG.check_loss(loss)                                          # accepted
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
        TG.check_depth_only(_depth_only_batch(), loss, 'actions')
        with pytest.raises(ValueError, match='depth-only'):
            TG.check_depth_only(_depth_only_batch(), loss, 'data')
    with pytest.raises(ValueError, match='contradicts'):
        TG.resolve_data_options('depth', 'mse', None)
    for call in (lambda: TG.train(config, None, empty, loss='emd'), lambda: TG.probe_batch(None, None, loss='emd'),
                 lambda: TG.run_batch(None, None, None, loss='emd'), lambda: TG.check_probe_options('emd', 0, 0)):
        with pytest.raises(ValueError, match='loss must be one of') as e:
            call()
        assert 'chamfer+match' in str(e.value) and 'mse' in str(e.value)     # the message lists both tuples
    for w in (0.0, 1.0, -0.5, 1.5, float('nan')):
        with pytest.raises(ValueError, match='match_weight'):
            TG.train(config, None, empty, loss='chamfer+match', match_weight=w)
        with pytest.raises(ValueError, match='match_weight'):
            TG.run_batch(None, None, None, loss='chamfer+match', match_weight=w)
        with pytest.raises(ValueError, match='match_weight'):
            TG.main(config, data_root=str(tmp_path), train_dir=str(tmp_path / 'run'), loss='chamfer+match', match_weight=w)
        TG.check_loss('match', w)                                    # read by the mix only
    TG.check_loss('chamfer+match', 0.25)
    assert not (tmp_path / 'run').exists()                           # main() refuses before it touches the disk or a device
    for argv in (['--loss', 'emd'], ['--loss', 'chamfer+match', '--match-weight', '1.0'], ['--loss', 'match', '--probe-every', '2']):
        with pytest.raises((SystemExit, ValueError)):
            TG._cli(argv + ['--data-root', str(tmp_path), '--train-dir', str(tmp_path / 'run')])
    assert not (tmp_path / 'run').exists()


def test_track_clouds_refuses_unequal_counts_before_it_touches_the_engine():
    from dyn_res_pile_manip_amd.dataset_gnn_dyn import track_clouds
    clouds = np.zeros((3, 6, 3), np.float32)
    with pytest.raises(ValueError, match='equal'):
        track_clouds(None, clouds, [6, 5, 6])
    with pytest.raises(ValueError):
        track_clouds(None, clouds, [6, 6])

"""CPU: the float64 references of the untracked (Chamfer) loss (tests/_untracked_ref.py), the yardsticks of
tests/test_gpu_chamfer.py and tests/test_gpu_train_untracked.py.

(a) chamfer64 against a triple-loop brute force.
(b) train_untracked64's weight and state gradients against its own central differences in float64 on b2_r5, with the step size
    and the bound tests/test_f64_train_host.py uses for the MSE loss (FD_H = 2^-20, FD_BOUND = 1e-5 of the tensor's largest
    gradient; its reasoning carries over: between two ReLU kinks, with the graph AND the arg-mins constant -- both asserted --
    the Chamfer term is the same kind of polynomial in a weight entry as the MSE term).
(c) THE PRECONDITION OF THE GPU COMPARISONS: for every batch the GPU tests use, every arg-min of the float64 reference wins by
    more than MARGIN_MIN = 1e-7 (squared distance), far above the fp32 rounding of a squared distance and the fp32-vs-float64
    drift of a predicted state -- so the fp32 kernel must pick the same partners.  Asserted, not skipped; a seed that violated it
    would be changed in _untracked_ref (TARGET_SEED, chamfer_case) here, before anything runs on a GPU."""
import numpy as np
import pytest

import _f64_train_ref as T
import _untracked_ref as U
from dyn_res_pile_manip_amd import synthetic as syn
from dyn_res_pile_manip_amd import train_gnn_dyn as TG
from dyn_res_pile_manip_amd.dataset_gnn_dyn import drop_correspondence

FD_H = 2.0 ** -20           # tests/test_f64_train_host.py
FD_BOUND = 1e-5


def brute(p, q, n_p, n_q):
    """three nested loops, the definition read aloud"""
    B, N, _ = p.shape
    fwd, bwd, grad = np.zeros(B), np.zeros(B), np.zeros((B, N, 3))
    for b in range(B):
        n, m = int(n_p[b]), int(n_q[b])
        for i in range(n):
            best, a = None, -1
            for j in range(m):
                d = sum((float(p[b, i, k]) - float(q[b, j, k])) ** 2 for k in range(3))
                if best is None or d < best:
                    best, a = d, j
            fwd[b] += best / (3 * n)
            for k in range(3):
                grad[b, i, k] += 2.0 / (3 * n) * (float(p[b, i, k]) - float(q[b, a, k]))
        for j in range(m):
            best, c = None, -1
            for i in range(n):
                d = sum((float(q[b, j, k]) - float(p[b, i, k])) ** 2 for k in range(3))
                if best is None or d < best:
                    best, c = d, i
            bwd[b] += best / (3 * m)
            for k in range(3):
                grad[b, c, k] += 2.0 / (3 * m) * (float(p[b, c, k]) - float(q[b, j, k]))
    return fwd, bwd, grad


@pytest.mark.parametrize('shape', [(1, 1, 1, 1), (5, 3, 8, 8), (3, 5, 8, 8), (20, 31, 24, 31)])
def test_chamfer64_against_brute_force(shape):
    p, q, n_p, n_q = U.chamfer_case(shape, 3)
    ref = U.chamfer64(p, q, n_p, n_q)
    fwd, bwd, grad = brute(p, q, n_p, n_q)
    np.testing.assert_allclose(ref['fwd'], fwd, rtol=1e-13)
    np.testing.assert_allclose(ref['bwd'], bwd, rtol=1e-13)
    np.testing.assert_allclose(ref['grad'], grad, rtol=0, atol=1e-13 * np.abs(grad).max())
    for b in range(3):
        assert (ref['grad'][b, n_p[b]:] == 0).all() and (ref['nn_pq'][b, n_p[b]:] == -1).all()


def test_chamfer64_ties_take_the_lowest_index():
    q = np.tile(np.array([[0.2, 0.3, 0.5]], np.float32), (6, 1))[None]
    p = np.array([[0.21, 0.3, 0.5], [0.4, 0.1, 0.5], [0.4, 0.1, 0.5], [0.0, 0.0, 0.0]], np.float32)[None]
    ref = U.chamfer64(p, q, [3], [6])
    assert (ref['nn_pq'][0, :3] == 0).all() and (ref['nn_qp'][0] == 0).all()
    q2 = np.array([[0.4, 0.1, 0.51]], np.float32)[None]          # equally far from the coincident rows 1 and 2
    assert U.chamfer64(p, q2, [3], [1])['nn_qp'][0, 0] == 1


def test_where_the_partner_is_the_nearest_fwd_is_the_mse_term():
    rng = np.random.default_rng(0)
    p = (0.2 + 0.1 * rng.random((1, 40, 3))).astype(np.float32)
    q = (p + 1e-5 * rng.standard_normal(p.shape)).astype(np.float32)
    ref = U.chamfer64(p, q, [40], [40])
    assert (ref['nn_pq'][0] == np.arange(40)).all()
    mse = ((p.astype(np.float64) - q.astype(np.float64)) ** 2).mean()
    assert abs(ref['fwd'][0] - mse) <= 1e-14 * mse and abs(ref['bwd'][0] - mse) <= 1e-14 * mse


# ---- (c) the precondition ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,B', U.chamfer_cases())
def test_margins_of_the_stand_alone_cases(shape, B):
    p, q, n_p, n_q = U.chamfer_case(shape, B)
    if B == 3 and min(shape[0], shape[1]) >= 3:
        assert len(set(n_p.tolist())) == 3 or len(set(n_q.tolist())) == 3        # three different counts
    m = U.min_margin(U.chamfer64(p, q, n_p, n_q))
    print('[untracked] shape %s B=%d: smallest arg-min margin %.3e' % (shape, B, m))
    assert m > U.MARGIN_MIN


@pytest.mark.parametrize('name,wset', U.TRAIN_CASES)
def test_margins_of_the_training_cases(golden, name, wset):
    batch = U.untracked_batch(golden, name)
    info = U.reference(golden, name, wset)[4]
    print('[untracked] %s %s: smallest arg-min margin %.3e' % (name, wset, info['margin']))
    assert info['margin'] > U.MARGIN_MIN
    # make_targets does what it is for: a good share of the rows is not matched to the tracked partner's copy
    nums, tnums = batch[3], batch[6]
    assert (tnums >= 1).all() and (tnums <= nums[:, None]).all() and (tnums < nums[:, None]).any()


def test_margins_of_the_other_gpu_batches(golden):
    W = golden.weights_seed0
    for label, batch in (('single point', U.single_point_batch(golden)), ('tiny', U.tiny_batch())):
        info = U.train_untracked64(W, *batch)[4]
        print('[untracked] %s: smallest arg-min margin %.3e' % (label, info['margin']))
        assert info['margin'] > U.MARGIN_MIN
    for name in ('b4_r3', 'b2_r5'):
        lr, beta1 = golden.train[name + '/lr_beta1']
        margin = U.adam_trajectory64(golden, name, float(lr), float(beta1))[3]
        print('[untracked] %s, three Adam steps: smallest arg-min margin %.3e' % (name, margin))
        assert margin > U.MARGIN_MIN


def test_the_single_point_configuration_by_hand(golden):
    """M = 1: fwd is the mean squared distance to the point, bwd the squared distance from the point to its nearest row / 3"""
    batch = U.single_point_batch(golden)
    W = golden.weights_seed0
    loss, terms, _, _, info = U.train_untracked64(W, *batch)
    # the first step's prediction does not depend on the loss
    from _f64_grad_ref import _d, step, weights64
    from oracle.propnet_dense import adjacency
    st, sd, at, dens = _d(batch[0]), _d(batch[1]), _d(batch[2]), _d(batch[4])
    adj, _ = adjacency(st[:, 0].float(), sd[:, 0].float(), 0.08)
    s_pred = step(weights64(W), at[:, 0], st[:, 0], sd[:, 0], dens, adj.double()).numpy()
    B, H = terms.shape[1], terms.shape[0]
    for b in range(B):
        n = int(batch[3][b])
        d = ((s_pred[b, :n] - batch[5][b, 0, 0].astype(np.float64)) ** 2).sum(-1)
        want = (d.mean() / 3 + d.min() / 3) / (H * B)
        assert abs(terms[0, b] - want) <= 1e-12 * want
    assert T.PARAMS == U.PARAMS


# ---- (b) central differences ------------------------------------------------------------------------------------------------
def fd_entries(grads):
    """the largest entries of each of the nine weight tensors, and of three biases (the tensors of tests/test_f64_train_host.py):
    the first of a tensor's three whose interval [-h, h] crosses no ReLU kink is differenced.  The bound's derivation holds
    BETWEEN two kinks; an entry that feeds thousands of edges (a bias of the relation encoder) can have one inside 2^-20.  A kink
    shows in the reference itself: inside one polynomial piece the analytic gradients at -h, 0, h lie on a line up to h^2 times
    the fourth derivative (1e-12 of the gradient by the bound's own estimate), across a kink they do not."""
    keys = [k + '.weight' for k in T.KEYS] + [T.KEYS[1] + '.bias', T.KEYS[4] + '.bias', T.KEYS[6] + '.bias']
    return [(k, [int(i) for i in np.argsort(-np.abs(grads[k]).ravel())[:3]]) for k in keys]


def same_structure(info, info0, nums):
    for a, b in zip(info['graphs'], info0['graphs']):            # the graph of the real rows is a constant of the derivative
        for j, n in enumerate(nums):
            if not np.array_equal(a[j, :n], b[j, :n]):
                return False
    return all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(info['nn'], info0['nn']))   # and the arg-mins


@pytest.mark.parametrize('wset', ['seed0', 'trained'])
def test_train_untracked64_agrees_with_its_central_differences(golden, wset):
    batch = U.untracked_batch(golden, 'b2_r5')
    nums = batch[3]
    W0 = dict((k, v.numpy().copy()) for k, v in U.weights64(U.weights_of(golden, wset)).items())
    loss, _, grads, g_state, info0 = U.train_untracked64(W0, *batch, keep64=True, want_graphs=True)
    worst = 0.0
    for key, cands in fd_entries(grads):
        for flat in cands:
            vals, gpm = [], []
            for sgn in (1.0, -1.0):
                W = dict((k, v.copy()) for k, v in W0.items())
                W[key].reshape(-1)[flat] += sgn * FD_H
                l, _, g, _, info = U.train_untracked64(W, *batch, keep64=True, want_graphs=True)
                assert same_structure(info, info0, nums), 'a neighbour list or an arg-min flips at h = %g in %s' % (FD_H, key)
                vals.append(l)
                gpm.append(g[key].reshape(-1)[flat])
            bend = abs(gpm[0] + gpm[1] - 2 * grads[key].reshape(-1)[flat]) / np.abs(grads[key]).max()
            if bend < 1e-8:                                         # one polynomial piece
                break
            print('[untracked] %s entry %d: a ReLU kink inside +-h (gradient bend %.1e), next entry' % (key, flat, bend))
        else:
            raise AssertionError('no kink-free entry among the three largest of %s' % key)
        cd = (vals[0] - vals[1]) / (2 * FD_H)
        res = abs(cd - grads[key].reshape(-1)[flat]) / np.abs(grads[key]).max()
        worst = max(worst, res)
        assert res < FD_BOUND, (key, flat, cd, grads[key].reshape(-1)[flat])
    print('[untracked] b2_r5 %s: central differences on 12 weight entries, worst residual %.3e' % (wset, worst))
    # the state gradient: the largest entry of the first, a middle and the last step's prediction
    H = g_state.shape[1]
    worst = 0.0
    for t in (0, H // 2, H - 1):
        gs = U.real_rows(g_state, nums)[:, t]
        b, i, k = np.unravel_index(int(np.argmax(np.abs(gs))), gs.shape)
        vals = []
        for sgn in (1.0, -1.0):
            l, _, _, _, info = U.train_untracked64(W0, *batch, keep64=True, want_graphs=True, nudge=(t, b, i, k, sgn * FD_H))
            assert same_structure(info, info0, nums), 'a neighbour list or an arg-min flips at h = %g in step %d' % (FD_H, t)
            vals.append(l)
        cd = (vals[0] - vals[1]) / (2 * FD_H)
        res = abs(cd - gs[b, i, k]) / np.abs(gs).max()
        worst = max(worst, res)
        assert res < FD_BOUND, (t, b, i, k, cd, gs[b, i, k])
    print('[untracked] b2_r5 %s: central differences on 3 state entries, worst residual %.3e' % (wset, worst))


# ---- the host-side pieces ---------------------------------------------------------------------------------------------------
def test_drop_correspondence_and_collate_untracked():
    rng = np.random.default_rng(0)
    data = []
    for n in (5, 9, 3):
        data.append((rng.normal(size=(4, n, 3)), rng.normal(size=(3, n, 3)), np.zeros((4, n)), n, 100.0 + n, None))
    un = [drop_correspondence(d, np.random.default_rng(5 + i)) for i, d in enumerate(data)]
    for d, u in zip(data, un):
        assert len(u) == 7 and len(u[6]) == 3 and u[3] == d[3]
        for t, cloud in enumerate(u[6]):
            n = d[3]
            assert cloud.dtype == np.float32 and cloud.ndim == 2 and 1 <= cloud.shape[0] <= n
            assert int(round(0.6 * n)) <= cloud.shape[0]
            rows = d[0][t + 1].astype(np.float32)                    # every target row is a row of states[t + 1], none twice
            idx = [int(np.flatnonzero((rows == r).all(1))[0]) for r in cloud]
            assert len(set(idx)) == len(idx)
    assert any(not np.array_equal(np.sort(i), i) for i in
               [[int(np.flatnonzero((d[0][1].astype(np.float32) == r).all(1))[0]) for r in u[6][0]] for d, u in zip(data, un)])
    out = TG.collate_untracked(un)
    ref = TG.collate_fn(data)
    for k in range(5):
        np.testing.assert_array_equal(out[k], ref[k])
    targets, tnums = out[6], out[7]
    M = max(c.shape[0] for u in un for c in u[6])
    assert targets.shape == (3, 3, M, 3) and targets.dtype == np.float32 and tnums.shape == (3, 3) and tnums.dtype == np.int32
    want = np.zeros_like(targets)                                    # the per-sample copy loop
    for b, u in enumerate(un):
        for t, cloud in enumerate(u[6]):
            want[b, t, :cloud.shape[0]] = cloud
            assert tnums[b, t] == cloud.shape[0]
    np.testing.assert_array_equal(targets, want)


def test_make_targets_is_seeded_and_jittered(golden):
    batch = U.fixture_batch(golden, 'b4_r3')
    a = U.make_targets(batch[0], batch[3], 0)
    b = U.make_targets(batch[0], batch[3], 0)
    c = U.make_targets(batch[0], batch[3], 1)
    np.testing.assert_array_equal(a[0], b[0])
    assert a[0].shape != c[0].shape or not np.array_equal(a[0], c[0])
    # no target row is a state row any more (the jitter), yet each lies within 6 sigma of one
    st = batch[0][0, 1, :batch[3][0]].astype(np.float64)
    d = np.sqrt(((a[0][0, 0, :a[1][0, 0]].astype(np.float64)[:, None] - st[None]) ** 2).sum(-1)).min(1)
    assert (d > 0).all() and (d < 6 * U.JITTER * np.sqrt(3)).all()


def test_the_probe_is_refused_with_the_chamfer_loss():
    config = syn.default_config()
    with pytest.raises(ValueError):
        TG.train(config, None, {'train': [], 'valid': []}, grad_probe_every=1, loss='chamfer')
    with pytest.raises(ValueError):
        TG.train(config, None, {'train': [], 'valid': []}, loss='emd')

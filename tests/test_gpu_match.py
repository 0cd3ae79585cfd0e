"""GPU: the stand-alone one-to-one matching distance (drp_cloud_match, csrc/k_match.h) through ctypes, against its own optimality
conditions and against assign64 of tests/_match_ref.py on the kernel's fp32 cost matrix (cost32).

Bounds.  tau = r 2^-40 max C for every statement about the duals and the total cost: one dual update per inserted row, each a
double rounding (2^-52) of a quantity of at most max C, with 2^12 to spare -- derived, not measured.  Partners: identical to
assign64's wherever the optimum is unique by MARGIN_MIN = 1e-9 (tests/test_match_host.py holds that margin on every case of
chamfer_cases()).  Term: rtol 1e-12 (double sums of the same fp32 differences in another order).  Gradient: within 1e-6 of its
largest entry, tests/test_gpu_chamfer.py's bound for the same arithmetic.  Every figure is printed before it is asserted."""
import ctypes

import numpy as np
import pytest

import _match_ref as R
import _untracked_ref as U
from dyn_res_pile_manip_amd import synthetic as syn, weights
from dyn_res_pile_manip_amd._lib import DrpError
from dyn_res_pile_manip_amd.engine import Engine

pytestmark = pytest.mark.gpu
I32P = ctypes.POINTER(ctypes.c_int32)
FP = ctypes.POINTER(ctypes.c_float)
DP = ctypes.POINTER(ctypes.c_double)


@pytest.fixture(scope='module')
def eng():
    e = Engine(0)                       # no weights: the metric needs none
    yield e
    e.close()


def extra_case(shape):
    """clouds of chamfer_case's scale for a shape of R.EXTRA_SHAPES, rubbish in the padding"""
    n_p, n_q, N, M = shape
    rng = np.random.default_rng(7 * n_p + 13 * n_q)
    p = (5.0 + rng.standard_normal((1, N, 3))).astype(np.float32)
    q = (-5.0 + rng.standard_normal((1, M, 3))).astype(np.float32)
    side = 0.02 * max(n_p, n_q) ** (1.0 / 3.0)
    p[0, :n_p] = (0.2 + side * rng.random((n_p, 3))).astype(np.float32)
    q[0, :n_q] = (0.2 + side * rng.random((n_q, 3))).astype(np.float32)
    return p, q, np.array([n_p], np.int32), np.array([n_q], np.int32)


def check_valid_and_optimal(got, p, q, n_p, n_q, label):
    """what needs no oracle: a one-to-one matching of r pairs, -1 and +0.0 elsewhere, and the duals' certificate of optimality
    -> the primal cost of every sample (host-summed in double over cost32)"""
    B, N, M = p.shape[0], p.shape[1], q.shape[1]
    costs = np.zeros(B)
    for b in range(B):
        n, m = int(n_p[b]), int(n_q[b])
        r = min(n, m)
        pq, qp = got['match_pq'][b], got['match_qp'][b]
        assert got['r'][b] == r
        assert (pq[n:] == -1).all() and (qp[m:] == -1).all()
        on = np.nonzero(pq[:n] >= 0)[0]
        assert len(on) == r and (np.nonzero(qp[:m] >= 0)[0].size == r)
        assert pq[:n].max() < m and qp[:m].max() < n
        assert len(set(pq[on].tolist())) == r                       # injective
        np.testing.assert_array_equal(qp[pq[on]], on)               # mutually consistent
        off = np.ones(N, bool)
        off[on] = False
        g = got['grad'][b]
        assert (g[off] == 0).all() and not np.signbit(g[off]).any()  # +0.0 exactly
        C = R.cost32(p[b, :n], q[b, :m]).astype(np.float64)
        tau = r * 2.0 ** -40 * C.max()
        u, v = got['u'][b], got['v'][b]
        assert (u[n:] == 0).all() and (v[m:] == 0).all()
        slack = C - u[:n, None] - v[None, :m]
        primal = float(C[on, pq[on]].sum())
        gap = primal - float(u[:n].sum() + v[:m].sum())
        larger_unmatched = v[:m][qp[:m] < 0] if n <= m else u[:n][pq[:n] < 0]
        print('[match] %s sample %d: least slack %.2e, largest slack on a pair %.2e, duality gap %.2e, tau %.2e'
              % (label, b, slack.min(), np.abs(slack[on, pq[on]]).max(), gap, tau))
        assert slack.min() >= -tau
        assert np.abs(slack[on, pq[on]]).max() <= tau
        assert (larger_unmatched == 0).all()
        assert gap <= tau
        costs[b] = primal
    return costs


def check(eng, p, q, n_p, n_q, label, margins=True):
    got = eng.cloud_match(p, q, n_p, n_q, want_grad=True, want_match=True, want_dual=True)
    assert got['grad'].dtype == np.float32 and got['match'].dtype == np.float64
    costs = check_valid_and_optimal(got, p, q, n_p, n_q, label)
    ref = R.match64(p, q, n_p, n_q, want_margin=margins)
    for b in range(p.shape[0]):
        n, m = int(n_p[b]), int(n_q[b])
        tau = min(n, m) * 2.0 ** -40 * float(R.cost32(p[b, :n], q[b, :m]).max())
        print('[match] %s sample %d: cost %.12e, assign64 %.12e, margin %.2e' % (label, b, costs[b], ref['cost'][b], ref['margin'][b]))
        assert abs(costs[b] - ref['cost'][b]) <= tau
        if margins and ref['margin'][b] >= R.MARGIN_MIN:
            np.testing.assert_array_equal(got['match_pq'][b], ref['match_pq'][b])
            np.testing.assert_array_equal(got['match_qp'][b], ref['match_qp'][b])
    # term and gradient against float64 arithmetic on the call's OWN matching (the oracle's, wherever the margin holds)
    own = R.match64(p, q, n_p, n_q, matches=got['match_pq'])
    et = float((np.abs(got['match'] - own['match']) / own['match']).max())
    eg = float(np.abs(got['grad'] - own['grad']).max() / np.abs(own['grad']).max())
    print('[match] %s: term %.2e rel, gradient %.2e of the largest entry' % (label, et, eg))
    assert et <= 1e-12 and eg <= 1e-6
    return got


@pytest.mark.parametrize('shape,B', U.chamfer_cases())
def test_against_assign64(eng, shape, B):
    p, q, n_p, n_q = U.chamfer_case(shape, B)
    ref = R.match64(p, q, n_p, n_q)
    assert ref['margin'].min() >= R.MARGIN_MIN                      # (tests/test_match_host.py: the precondition)
    check(eng, p, q, n_p, n_q, '%s B=%d' % (shape, B))


@pytest.mark.parametrize('shape', R.EXTRA_SHAPES)
def test_the_cap_the_lane_stripe_edges_and_few_rows(eng, shape):
    """held to the optimum by the certificate and by assign64's cost (no uniqueness margin is computed at these sizes, so the
    partners are not compared)"""
    check(eng, *extra_case(shape), label='%s' % (shape,), margins=False)


def test_ties_take_the_lowest_index(eng):
    """the deliberate exception to the margin rule: a lattice whose every point is there twice in the larger cloud -- the optimum
    costs 0 and the first of each pair of duplicates is taken"""
    g = np.stack(np.meshgrid(*[np.arange(3)] * 3, indexing='ij'), -1).reshape(-1, 3)[:20]
    small = (0.2 + 0.02 * g).astype(np.float32)
    large = np.repeat(small, 2, axis=0)                             # rows 2 i and 2 i + 1 are point i
    got = eng.cloud_match(small[None], large[None], want_match=True, want_dual=True, want_grad=True)
    check_valid_and_optimal(got, small[None], large[None], [20], [40], 'ties p < q')
    assert got['match'][0] == 0.0
    np.testing.assert_array_equal(got['match_pq'][0], 2 * np.arange(20))
    got = eng.cloud_match(large[None], small[None], want_match=True, want_dual=True, want_grad=True)
    check_valid_and_optimal(got, large[None], small[None], [40], [20], 'ties p > q')
    assert got['match'][0] == 0.0
    np.testing.assert_array_equal(got['match_qp'][0], 2 * np.arange(20))
    assert (got['grad'] == 0).all() and not np.signbit(got['grad']).any()


def test_same_bits_run_to_run_and_alone_or_in_a_batch(eng):
    p, q, n_p, n_q = U.chamfer_case((300, 257, 300, 300), 3)
    kw = dict(want_grad=True, want_match=True, want_dual=True)
    a = eng.cloud_match(p, q, n_p, n_q, **kw)
    b = eng.cloud_match(p, q, n_p, n_q, **kw)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])
    for s in range(3):
        one = eng.cloud_match(p[s:s + 1], q[s:s + 1], n_p[s:s + 1], n_q[s:s + 1], **kw)
        for k in a:
            np.testing.assert_array_equal(one[k][0], a[k][s], err_msg='%s of sample %d' % (k, s))
    # the outputs are optional, and a single pair may come without the batch axis
    t = eng.cloud_match(p[0, :n_p[0]], q[0, :n_q[0]])
    assert sorted(t) == ['match', 'r'] and t['match'][0] == a['match'][0]


def test_a_permutation_of_the_cloud_is_found(eng):
    rng = np.random.default_rng(11)
    p = (0.2 + 0.06 * rng.random((2, 90, 3))).astype(np.float32)
    perm = np.stack([rng.permutation(90), rng.permutation(90)])
    q = np.stack([p[b][perm[b]] for b in range(2)])                 # q_j = p_perm[j]
    got = eng.cloud_match(p, q, want_match=True, want_grad=True)
    assert (got['match'] == 0.0).all() and (got['grad'] == 0).all()
    np.testing.assert_array_equal(got['match_qp'], perm)
    for b in range(2):
        np.testing.assert_array_equal(got['match_pq'][b][perm[b]], np.arange(90))


def test_refusals(eng):
    p, q, n_p, n_q = U.chamfer_case((5, 3, 8, 8), 1)
    lib, h = eng.lib, eng.h
    terms = np.zeros((1,))
    def call(p_, np_, q_, nq_, B, N, M, t_):
        f = lambda a, T: None if a is None else a.ctypes.data_as(T)
        return lib.drp_cloud_match(h, f(p_, FP), f(np_, I32P), f(q_, FP), f(nq_, I32P), B, N, M, f(t_, DP), None, None, None, None)
    assert call(p, n_p, q, n_q, 1, 8, 8, terms) == 0
    big = np.zeros((1, 1025, 3), np.float32)
    nan_p, inf_q = p.copy(), q.copy()
    nan_p[0, 4, 1] = np.nan                                          # a real row (n_p = 5)
    inf_q[0, 0, 2] = np.inf
    for args in ((None, n_p, q, n_q, 1, 8, 8, terms), (p, None, q, n_q, 1, 8, 8, terms), (p, n_p, None, n_q, 1, 8, 8, terms),
                 (p, n_p, q, None, 1, 8, 8, terms), (p, n_p, q, n_q, 1, 8, 8, None),
                 (p, n_p, q, n_q, 1, 8, 0, terms), (p, n_p, big, n_q, 1, 8, 1025, terms), (big, n_p, q, n_q, 1, 1025, 8, terms),
                 (p, n_p, q, n_q, 0, 8, 8, terms),
                 (p, np.array([0], np.int32), q, n_q, 1, 8, 8, terms), (p, np.array([9], np.int32), q, n_q, 1, 8, 8, terms),
                 (p, n_p, q, np.array([0], np.int32), 1, 8, 8, terms), (p, n_p, q, np.array([9], np.int32), 1, 8, 8, terms),
                 (nan_p, n_p, q, n_q, 1, 8, 8, terms), (p, n_p, inf_q, n_q, 1, 8, 8, terms)):
        assert call(*args) == -1, args[4:7]                          # DRP_EINVAL
    with pytest.raises(DrpError, match='1025'):
        eng.cloud_match(big, q, [5], [3])
    with pytest.raises(DrpError):
        eng.cloud_match(p, q, [0], [3])
    nan_pad = p.copy()
    nan_pad[0, 6] = np.nan                                           # padding is never read as points
    a = eng.cloud_match(p, q, n_p, n_q, want_grad=True, want_match=True)
    b = eng.cloud_match(nan_pad, q, n_p, n_q, want_grad=True, want_match=True)
    for k in a:                                                      # and the context is as usable as before
        np.testing.assert_array_equal(a[k], b[k])


def test_a_gd_session_and_the_dispatch_marks_survive_a_call(golden):
    """drp_cloud_match ends no session and leaves the marks alone: a GD session stepped with calls in between gives the bits of an
    undisturbed one, and last_dispatch() is what it was (tests/test_gpu_chamfer.py's pattern)"""
    from oracle import propnet_sparse as osp
    sd = weights.random_state_dict(seed=0)
    M34 = osp.world2cam_affine(syn.demo_cam_extrinsics(), 24)
    p, q, n_p, n_q = U.chamfer_case((70, 130, 70, 130), 1)
    runs = []
    for disturb in (False, True):
        e = Engine(0)
        e.load_weights(weights.blob_from_state_dict(sd), 0.08)
        e.set_camera(M34, 24.0, syn.demo_cam_params())
        e.set_goal_image(syn.goal_distance_image(syn.goal_mask('I')), 5 * 64, fps_init=0, mode='cv5')
        s0, dens, attr = syn.make_pile(64, 1, seed=0)
        acts = syn.sample_pushes(4, 3, seed=0)
        lo, hi = syn.action_limits()
        e.gd_begin(s0, attr, dens, acts, 0.05, lo, hi)
        out = [e.gd_step()]
        marks = e.last_dispatch()
        if disturb:
            e.cloud_match(p, q, n_p, n_q, want_grad=True, want_dual=True)
            assert e.last_dispatch() == marks
        out.append(e.gd_step())
        if disturb:
            e.cloud_match(p, q, n_p, n_q)
        out.append(e.gd_actions())
        runs.append(out)
        e.close()
    for a, b in zip(runs[0], runs[1]):
        for x, y in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
            np.testing.assert_array_equal(np.asarray(x), np.asarray(y))


def test_an_adam_trajectory_survives_calls(golden):
    """the trainer's state is untouched: three Adam steps with matching calls in between are three undisturbed ones, bit for bit"""
    batch = U.untracked_batch(golden, 'b2_r5')
    p, q, n_p, n_q = U.chamfer_case((70, 130, 70, 130), 1)
    runs = []
    for disturb in (False, True):
        e = Engine(0)
        e.load_weights(weights.blob_from_state_dict(golden.weights_seed0), 0.08)
        e.train_begin(batch[0].shape[1] - 1, 1e-3, 0.9)
        losses = []
        for _ in range(3):
            losses.append(e.train_step_untracked(*batch, mode='update')[0])
            if disturb:
                e.cloud_match(p, q, n_p, n_q, want_grad=True)
        runs.append((losses, e.get_weights().copy()))
        e.close()
    assert runs[0][0] == runs[1][0]
    np.testing.assert_array_equal(runs[0][1], runs[1][1])


def test_the_three_one_shots_share_one_buffer(eng):
    """drp_cloud_chamfer, drp_cloud_match and drp_cloud_chamfer_f64 stage into one device buffer (c->cloud_io): interleaved on one
    context, every output asked for, each call returns the bytes it returns as the first call of a fresh context.  A large call
    before a small one (stale bytes behind a shrunk layout), a small one before a large one (the buffer grows), and 65 against 64
    rows (the matching kernel's lane-stripe edge, the float64 kernel's first partial chunk); every case has a sample whose
    counts lie below the padding."""
    big, small, edge = U.chamfer_case((70, 130, 70, 130), 3), U.chamfer_case((5, 3, 5, 3), 2), U.chamfer_case((65, 60, 65, 64), 1)
    for p, q, n_p, n_q in (big, small, edge):
        assert (n_p < p.shape[1]).any() or (n_q < q.shape[1]).any()
    chamfer = lambda e, c: e.cloud_chamfer(*c, want_grad=True, want_nn=True)
    match = lambda e, c: e.cloud_match(*c, want_grad=True, want_match=True, want_dual=True)
    chamfer64 = lambda e, c: e.cloud_chamfer_f64(*c, want_grad=True, want_nn=True)
    for n, (call, case) in enumerate(((chamfer, big), (match, small), (chamfer64, edge), (chamfer, small), (match, big))):
        got = call(eng, case)
        fresh_eng = Engine(0)
        try:
            fresh = call(fresh_eng, case)
        finally:
            fresh_eng.close()
        assert sorted(got) == sorted(fresh)
        for k in fresh:
            assert got[k].dtype == fresh[k].dtype and got[k].shape == fresh[k].shape
            assert got[k].tobytes() == fresh[k].tobytes(), 'call %d, %s' % (n, k)

"""GPU: the unbalanced Sinkhorn divergence (drp_cloud_divergence_unbalanced; csrc/k_sinkhorn.h: kd_sweeps_unbalanced and
kd_combine<false, true>) through ctypes, against include/drp.h's definition in numpy float64
(tests/_divergence_unbalanced_ref.py) on the kernel's fp32 cost matrices.

Both sides do the same IEEE double operations in the same order; they differ in the order the terms of a sum are added and in
whose exp, expm1 and log they call (tests/test_gpu_divergence.py).  Shapes, denominators and the layout of the cases are that
file's: value against its own value, duals against the sample's largest dual entry, gradient against the sample's largest
entry beyond one fp32 rounding, col_err and self_err against the total mass 1 -- and transported against 1 too.
Parameters: B in {1, 3} (at B = 3 the counts are ragged and eps, rho and w differ per sample), K in {1, 50}, rho / eps in
{4, 25}, w in {1, n_q / n_p}; one 1024 x 1024 case at K = 2.
Bounds: 5 x the worst figure measured on one MI355X over every case below, each below 1e-10:
  MEASURED (worst)   value 1.5e-14   duals 1.2e-15   col_err 5.6e-16   self_err 1.2e-15   transported 1.5e-15   gradient 0 beyond
                     its one fp32 rounding (held to the duals' bound, as in tests/test_gpu_divergence.py)
The value's figure is a little above the balanced kernel's 1.2e-14 (at 1024 x 1024): its four sums are of -expm1(-dual / rho),
which cancel as the duals' sums do, and each term carries one more library call's rounding; it stays far below 1e-10.  self_err's
worst is the 1 x 7 case at w = 7: the target's plan carries 7 times the mass the figure is measured against."""
import ctypes

import numpy as np
import pytest

import _divergence_ref as D
import _divergence_unbalanced_ref as R
import _untracked_ref as U
import test_divergence_unbalanced_host as HOST
import test_gpu_divergence as G
from dyn_res_pile_manip_amd._lib import DrpError
from dyn_res_pile_manip_amd.engine import Engine

pytestmark = pytest.mark.gpu
I32P = ctypes.POINTER(ctypes.c_int32)
FP = ctypes.POINTER(ctypes.c_float)
DP = ctypes.POINTER(ctypes.c_double)

MEASURED = {'value': 1.5e-14, 'dual': 1.2e-15, 'grad': 1.2e-15, 'col': 5.6e-16, 'self': 1.2e-15, 'moved': 1.5e-15}   # the module docstring's line
BOUND = {k: 5 * v for k, v in MEASURED.items()}
SHAPES = G.SHAPES
RATIOS = (4.0, 25.0)
KW = dict(want_grad=True, want_dual=True, want_col_err=True, want_self_err=True, want_transported=True)
K = G.K
EPS = D.GRID_SPACING ** 2


@pytest.fixture(scope='module')
def eng():
    e = Engine(0)                       # no weights: the metric needs none
    yield e
    e.close()


def case_params(n_p, n_q, ratio, by_count):
    """per sample: test_gpu_divergence's eps (a quarter more for every further sample), rho = ratio x eps x (1, 1.5, 2, ...),
    w = 1 or the counts' ratio"""
    eps = G.case_eps(n_p, n_q, 1.0)
    rho = ratio * eps * (1.0 + 0.5 * np.arange(len(n_p)))
    w = n_q.astype(np.float64) / n_p if by_count else np.ones(len(n_p))
    return eps, rho, w


def check(eng, p, q, n_p, n_q, eps, rho, w, iters, label):
    got = eng.cloud_divergence(p, q, n_p, n_q, eps=eps, iters=iters, reach=rho, mass_q=w, **KW)
    assert sorted(got) == sorted(('divergence', 'grad', 'col_err', 'self_err', 'transported') + G.DUALS)
    assert got['grad'].dtype == np.float32 and all(got[k].dtype == np.float64 for k in got if k != 'grad')
    ref = R.divergence64(p, q, n_p, n_q, eps, rho, w, iters)
    dev = G.deviations(got, ref, n_p, n_q)
    dev['moved'] = float(np.abs(got['transported'] - ref['transported']).max() / 1.0)
    print('[unbalanced] %s K=%d rho/eps=%g w=%s: value %.2e, duals %.2e, gradient %.2e (beyond one fp32 rounding), col_err %.2e, '
          'self_err %.2e, transported %.2e; transported itself %s'
          % (label, iters, rho[0] / eps[0], np.round(w, 3), dev['value'], dev['dual'], dev['grad'], dev['col'], dev['self'], dev['moved'],
             np.round(ref['transported'], 4)))
    for k in dev:
        assert dev[k] <= BOUND[k] < 1e-10, (label, iters, k, dev[k])
    return got


@pytest.mark.parametrize('ratio', RATIOS)
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('shape', SHAPES)
def test_against_the_float64_definition(eng, shape, B, ratio):
    p, q, n_p, n_q = U.chamfer_case(shape, B, seed=0)
    for by_count in (False, True):
        eps, rho, w = case_params(n_p, n_q, ratio, by_count)
        for iters in (1, K):
            check(eng, p, q, n_p, n_q, eps, rho, w, iters, '%s B=%d' % (shape, B))


def test_the_cap_once(eng):
    p, q, n_p, n_q = U.chamfer_case((1024, 1024, 1024, 1024), 1, seed=0)
    eps, rho, w = case_params(n_p, n_q, 4.0, False)
    got = check(eng, p, q, n_p, n_q, eps, rho, w, 2, '1024 x 1024')
    assert (np.abs(got['grad'][0]).max(axis=1) > 0).all()


# ---- bits ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(5, 3, 8, 8), (65, 63, 65, 64), (257, 300, 260, 300)])
def test_an_infinite_reach_has_the_balanced_kernels_bits(eng, shape):
    p, q, n_p, n_q = U.chamfer_case(shape, 3, seed=0)
    eps = G.case_eps(n_p, n_q, 1.0)
    for iters in (1, K):
        want = eng.cloud_divergence(p, q, n_p, n_q, eps=eps, iters=iters, **G.KW)
        got = eng.cloud_divergence(p, q, n_p, n_q, eps=eps, iters=iters, reach=np.inf, mass_q=1.0, **KW)
        for k in want:
            assert got[k].tobytes() == want[k].tobytes(), (shape, iters, k)
        assert np.abs(got['transported'] - 1.0).max() <= 4e-16
    # a batch may mix the two: the sample with the infinite reach keeps the balanced bits
    rho = np.array([4 * eps[0], np.inf, 25 * eps[2]])
    mixed = eng.cloud_divergence(p, q, n_p, n_q, eps=eps, iters=K, reach=rho, mass_q=[0.75, 1.0, 1.0], **KW)
    for k in want:
        assert mixed[k][1].tobytes() == want[k][1].tobytes(), (shape, k)
    for k in ('divergence', 'f', 'grad'):                            # (and its neighbours are not the balanced problem)
        assert mixed[k][0].tobytes() != want[k][0].tobytes() and mixed[k][2].tobytes() != want[k][2].tobytes(), (shape, k)


def test_same_bits_run_to_run_alone_or_in_a_batch_and_under_more_padding(eng):
    p, q, n_p, n_q = U.chamfer_case((257, 300, 260, 300), 3, seed=0)
    eps, rho, w = case_params(n_p, n_q, 4.0, True)
    a = eng.cloud_divergence(p, q, n_p, n_q, eps=eps, iters=K, reach=rho, mass_q=w, **KW)
    b = eng.cloud_divergence(p, q, n_p, n_q, eps=eps, iters=K, reach=rho, mass_q=w, **KW)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    for s in range(3):
        one = eng.cloud_divergence(p[s:s + 1], q[s:s + 1], n_p[s:s + 1], n_q[s:s + 1], eps=eps[s:s + 1], iters=K, reach=rho[s:s + 1],
                                   mass_q=w[s:s + 1], **KW)
        for k in a:
            assert one[k][0].tobytes() == a[k][s].tobytes(), '%s of sample %d' % (k, s)
    N, M = p.shape[1], q.shape[1]
    wide_p, wide_q = np.full((3, N + 37, 3), 9.0, np.float32), np.full((3, M + 5, 3), -9.0, np.float32)
    wide_p[:, :N], wide_q[:, :M] = p, q
    wd = eng.cloud_divergence(wide_p, wide_q, n_p, n_q, eps=eps, iters=K, reach=rho, mass_q=w, **KW)
    for k in ('divergence', 'col_err', 'self_err', 'transported'):
        assert wd[k].tobytes() == a[k].tobytes(), k
    for s in range(3):
        n, m = int(n_p[s]), int(n_q[s])
        assert wd['grad'][s, :n].tobytes() == a['grad'][s, :n].tobytes()
        for k, real in (('f', n), ('g', m), ('h_p', n), ('h_q', m)):
            assert wd[k][s, :real].tobytes() == a[k][s, :real].tobytes(), k
    G.assert_padding(wd, n_p, n_q)
    # the outputs are optional -- asked for or not, the value's bits are the same
    t = eng.cloud_divergence(p[0, :n_p[0]], q[0, :n_q[0]], eps=eps[0], iters=K, reach=rho[0], mass_q=w[0])
    assert sorted(t) == ['divergence'] and t['divergence'][0] == a['divergence'][0]


# ---- the property, on the device ---------------------------------------------------------------------------------------------------
def test_a_finite_reach_leaves_the_unseen_side_and_the_seen_interior_alone(eng):
    p, q, col = R.half_seen_pile()
    P, Q = np.zeros((1, 80, 3), np.float32), np.zeros((1, 40, 3), np.float32)
    P[0, :72], Q[0, :36] = p, q
    n_p, n_q = np.array([72], np.int32), np.array([36], np.int32)
    balanced = eng.cloud_divergence(P, Q, n_p, n_q, eps=EPS, iters=K, want_grad=True)
    got = eng.cloud_divergence(P, Q, n_p, n_q, eps=EPS, iters=K, reach=4 * EPS, mass_q=36 / 72, want_grad=True, want_col_err=True,
                               want_transported=True)
    HOST.half_seen_thresholds(balanced['grad'][0, :72], got['grad'][0, :72], col, got['col_err'][0], 'device:')
    assert (np.abs(got['grad'][0, :72]).max(axis=1) > 0).all()       # every real row has a gradient ...
    pad = got['grad'][0, 72:]
    assert (pad == 0).all() and not np.signbit(pad).any()            # ... and the padding exactly +0.0
    assert 0.0 < got['transported'][0] <= 1.0


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals(eng):
    p, q, n_p, n_q = U.chamfer_case((5, 3, 8, 8), 1, seed=0)
    lib, h = eng.lib, eng.h
    terms = np.zeros((1,))
    e64 = lambda v: np.array([v], np.float64)
    eps, rho, w = e64(4e-4), e64(16e-4), e64(0.6)
    good = eng.cloud_divergence(p, q, n_p, n_q, eps=eps, iters=7, reach=rho, mass_q=w, **KW)

    def call(p_, np_, q_, nq_, B, N, M, eps_, rho_, w_, iters, t_):
        f = lambda a, T_: None if a is None else a.ctypes.data_as(T_)
        return lib.drp_cloud_divergence_unbalanced(h, f(p_, FP), f(np_, I32P), f(q_, FP), f(nq_, I32P), B, N, M, f(eps_, DP), f(rho_, DP),
                                                   f(w_, DP), iters, f(t_, DP), None, None, None, None, None)
    assert call(p, n_p, q, n_q, 1, 8, 8, eps, rho, w, 7, terms) == 0 and terms[0] == good['divergence'][0]
    big = np.zeros((1, 1025, 3), np.float32)
    nan_p, inf_q = p.copy(), q.copy()
    nan_p[0, 4, 1] = np.nan                                          # a real row (n_p = 5)
    inf_q[0, 0, 2] = np.inf
    one = e64(1.0)
    for args, word in (((p, n_p, q, n_q, 1, 8, 8, eps, None, w, 7, terms), 'null'), ((p, n_p, q, n_q, 1, 8, 8, eps, rho, None, 7, terms), 'null'),
                       ((p, n_p, q, n_q, 1, 8, 8, eps, e64(0.0), w, 7, terms), 'rho'), ((p, n_p, q, n_q, 1, 8, 8, eps, e64(-16e-4), w, 7, terms), 'rho'),
                       ((p, n_p, q, n_q, 1, 8, 8, eps, e64(4e-4 / 1025), w, 7, terms), 'rho'),     # below eps / 1024
                       ((p, n_p, q, n_q, 1, 8, 8, eps, e64(np.nan), w, 7, terms), 'rho'), ((p, n_p, q, n_q, 1, 8, 8, eps, e64(-np.inf), w, 7, terms), 'rho'),
                       ((p, n_p, q, n_q, 1, 8, 8, eps, rho, e64(0.1249), 7, terms), 'mass_q'), ((p, n_p, q, n_q, 1, 8, 8, eps, rho, e64(8.001), 7, terms), 'mass_q'),
                       ((p, n_p, q, n_q, 1, 8, 8, eps, rho, e64(np.nan), 7, terms), 'mass_q'), ((p, n_p, q, n_q, 1, 8, 8, eps, rho, e64(0.0), 7, terms), 'mass_q'),
                       ((p, n_p, q, n_q, 1, 8, 8, eps, e64(np.inf), w, 7, terms), 'balanced'),      # w != 1 without a finite reach
                       ((nan_p, n_p, q, n_q, 1, 8, 8, eps, rho, w, 7, terms), 'finite'), ((p, n_p, inf_q, n_q, 1, 8, 8, eps, rho, w, 7, terms), 'finite'),
                       ((p, n_p, big, n_q, 1, 8, 1025, eps, rho, w, 7, terms), '1025'), ((big, n_p, q, n_q, 1, 1025, 8, eps, rho, w, 7, terms), '1025'),
                       ((p, n_p, q, n_q, 1, 8, 8, e64(0.0), rho, w, 7, terms), 'eps'), ((p, n_p, q, n_q, 1, 8, 8, eps, rho, w, 0, terms), 'iters'),
                       ((p, n_p, q, n_q, 1, 8, 8, eps, rho, w, 7, None), 'null')):
        eng.dispatch_reset()
        eng.probe_begin('loss')
        assert call(*args) == -1, word                               # DRP_EINVAL ...
        assert word in eng.lib.drp_last_error(h).decode(), (word, eng.lib.drp_last_error(h))      # ... with a message ...
        assert eng.probe_read()[1] == 0                              # ... and no kernel
        eng.probe_begin(None)
        again = eng.cloud_divergence(p, q, n_p, n_q, eps=eps, iters=7, reach=rho, mass_q=w, **KW)
        for k in good:
            assert again[k].tobytes() == good[k].tobytes(), (word, k)
    # the edges of the ranges are served
    assert call(p, n_p, q, n_q, 1, 8, 8, eps, e64(4e-4 / 1024), e64(0.125), 7, terms) == 0
    assert call(p, n_p, q, n_q, 1, 8, 8, eps, rho, e64(8.0), 7, terms) == 0
    assert call(p, n_p, q, n_q, 1, 8, 8, eps, e64(np.inf), one, 7, terms) == 0
    with pytest.raises(DrpError, match='rho'):
        eng.cloud_divergence(p, q, n_p, n_q, eps=4e-4, iters=7, reach=-1.0)
    with pytest.raises(DrpError, match='mass_q'):
        eng.cloud_divergence(p, q, n_p, n_q, eps=4e-4, iters=7, reach=16e-4, mass_q=9.0)
    with pytest.raises(DrpError, match='1025'):
        eng.cloud_divergence(big, q, [5], [3], eps=4e-4, iters=7, reach=16e-4)

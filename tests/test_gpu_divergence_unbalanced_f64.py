"""GPU: the float64 yardstick of the unbalanced Sinkhorn divergence stand-alone (drp_cloud_divergence_unbalanced_f64;
csrc/k_sinkhorn.h: kd64_sweeps_unbalanced and kd64_combine_unbalanced) through ctypes, against
tests/_divergence_unbalanced_f64_ref.py's divergence64_wide: include/drp.h's definition in numpy float64 with nothing in fp32.

p carries bits no float32 has (tests/test_gpu_divergence_f64.py's wide_case), q is float32.  Both sides do the same IEEE double
operations in the same order; they differ in the order the terms of a sum are added and in whose exp, expm1 and log they call.
Denominators as tests/test_gpu_divergence_f64.py: value against its own value, duals against the sample's largest dual entry,
gradient against the sample's largest entry with NO fp32-rounding allowance, col_err, self_err and transported against the
total mass 1.
Parameters: tests/test_gpu_divergence.py's shapes, B in {1, 3} (at B = 3 the counts are ragged and eps, rho and w all differ per
sample, so a wrong index shows), K in {1, 50}, rho / eps in {4, 25}, w in {1, n_q / n_p}; one 1024 x 1024 case at K = 2.
Bounds: 5 x the worst figure measured on one MI355X over every case below, each below 1e-10:
  MEASURED (worst)   value 5.8e-14   duals 1.1e-15   gradient 2.7e-15   col_err 1.8e-15   self_err 1.2e-15   transported 1.5e-15
The value's worst is the 1024 x 1024 case (K = 2): four sums of 1024 terms -expm1(-dual / rho) that cancel, against the value that is
left; every other case stays below 3e-14.  col_err's and self_err's worst are the 1 x 7 cases at w = 7 (and 7, 5, 3): the target's
plan carries up to 7 times the mass the figures are measured against."""
import ctypes

import numpy as np
import pytest

import _divergence_ref as D
import _divergence_unbalanced_f64_ref as RU
import _divergence_unbalanced_ref as UB
import _untracked_ref as U
import test_divergence_unbalanced_host as HOST
import test_gpu_divergence as G
import test_gpu_divergence_f64 as F
from dyn_res_pile_manip_amd._lib import DrpError
from dyn_res_pile_manip_amd.engine import Engine

pytestmark = pytest.mark.gpu
I32P = ctypes.POINTER(ctypes.c_int32)
FP = ctypes.POINTER(ctypes.c_float)
DP = ctypes.POINTER(ctypes.c_double)

MEASURED = {'value': 5.8e-14, 'dual': 1.1e-15, 'grad': 2.7e-15, 'col': 1.8e-15, 'self': 1.2e-15, 'moved': 1.5e-15}   # the module docstring's line
BOUND = {k: 5 * v for k, v in MEASURED.items()}
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
    got = eng.cloud_divergence_f64(p, q, n_p, n_q, eps=eps, iters=iters, reach=rho, mass_q=w, **KW)
    assert sorted(got) == sorted(('divergence', 'grad', 'col_err', 'self_err', 'transported') + G.DUALS)
    assert all(got[k].dtype == np.float64 for k in got)
    ref = RU.divergence64_wide(p, q, n_p, n_q, eps, rho, w, iters)
    dev = F.deviations(got, ref, n_p, n_q)                           # (the padding too: +0.0 rows, zero duals beyond the counts)
    dev['moved'] = float(np.abs(got['transported'] - ref['transported']).max() / 1.0)
    print('[unbalanced-f64] %s K=%d rho/eps=%g w=%s: value %.2e, duals %.2e, gradient %.2e, col_err %.2e, self_err %.2e, '
          'transported %.2e; transported itself %s'
          % (label, iters, rho[0] / eps[0], np.round(w, 3), dev['value'], dev['dual'], dev['grad'], dev['col'], dev['self'], dev['moved'],
             np.round(ref['transported'], 4)))
    for k in dev:
        assert dev[k] <= BOUND[k] < 1e-10, (label, iters, k, dev[k])
    return got


@pytest.mark.parametrize('ratio', RATIOS)
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('shape', G.SHAPES)
def test_against_the_float64_definition(eng, shape, B, ratio):
    p, q, n_p, n_q = F.wide_case(shape, B)
    for by_count in (False, True):
        eps, rho, w = case_params(n_p, n_q, ratio, by_count)
        if B == 3:
            assert len(set(eps)) == 3 and len(set(rho)) == 3
        for iters in (1, K):
            check(eng, p, q, n_p, n_q, eps, rho, w, iters, '%s B=%d' % (shape, B))


def test_the_cap_once(eng):
    p, q, n_p, n_q = F.wide_case((1024, 1024, 1024, 1024), 1)
    eps, rho, w = case_params(n_p, n_q, 4.0, False)
    got = check(eng, p, q, n_p, n_q, eps, rho, w, 2, '1024 x 1024')
    assert (np.abs(got['grad'][0]).max(axis=1) > 0).all()
    with pytest.raises(DrpError, match='1025'):
        eng.cloud_divergence_f64(np.zeros((1, 1025, 3)), q[:, :8], [5], [3], eps=4e-4, iters=7, reach=16e-4)
    with pytest.raises(DrpError, match='1025'):
        eng.cloud_divergence_f64(p[:, :8], np.zeros((1, 1025, 3), np.float32), [5], [3], eps=4e-4, iters=7, reach=16e-4)


def test_the_non_fp32_bits_of_p_reach_the_result(eng):
    """the same clouds with p rounded to fp32 give another value, and the device follows the reference on both"""
    p, q, n_p, n_q = F.wide_case((64, 64, 70, 66), 1)
    eps = G.case_eps(n_p, n_q, 0.01)
    rho, w = 4.0 * eps, np.array([1.0])
    p32 = p.astype(np.float32).astype(np.float64)
    a = check(eng, p, q, n_p, n_q, eps, rho, w, K, '64 x 64 double p')
    b = check(eng, p32, q, n_p, n_q, eps, rho, w, K, '64 x 64 rounded p')
    ref_a, ref_b = (RU.divergence64_wide(x, q, n_p, n_q, eps, rho, w, K) for x in (p, p32))
    shift, ref_shift = a['divergence'][0] - b['divergence'][0], ref_a['divergence'][0] - ref_b['divergence'][0]
    print('[unbalanced-f64] 64 x 64, eps scale 0.01: value shift under fp32 rounding of p %.3e, reference %.3e' % (shift, ref_shift))
    assert shift != 0 and abs(shift - ref_shift) <= 1e-3 * abs(ref_shift) + 1e-10 * abs(ref_a['divergence'][0])


# ---- bits ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(5, 3, 8, 8), (65, 63, 65, 64), (257, 300, 260, 300)])
def test_an_infinite_reach_has_the_balanced_kernels_bits(eng, shape):
    p, q, n_p, n_q = F.wide_case(shape, 3)
    eps = G.case_eps(n_p, n_q, 1.0)
    for iters in (1, K):
        want = eng.cloud_divergence_f64(p, q, n_p, n_q, eps=eps, iters=iters, **G.KW)
        got = eng.cloud_divergence_f64(p, q, n_p, n_q, eps=eps, iters=iters, reach=np.inf, mass_q=1.0, **KW)
        for k in want:
            assert got[k].tobytes() == want[k].tobytes(), (shape, iters, k)
        # the sum of a itself -- n terms 1 / n x exp(-0) in the block sum's order: 1 to the rounding of that sum
        assert np.abs(got['transported'] - 1.0).max() <= 4e-16
    # a batch may mix the two: the sample with the infinite reach keeps the balanced bits
    rho = np.array([4 * eps[0], np.inf, 25 * eps[2]])
    mixed = eng.cloud_divergence_f64(p, q, n_p, n_q, eps=eps, iters=K, reach=rho, mass_q=[0.75, 1.0, 1.0], **KW)
    for k in want:
        assert mixed[k][1].tobytes() == want[k][1].tobytes(), (shape, k)
    for k in ('divergence', 'f', 'grad'):                            # (and its neighbours are not the balanced problem)
        assert mixed[k][0].tobytes() != want[k][0].tobytes() and mixed[k][2].tobytes() != want[k][2].tobytes(), (shape, k)


def test_same_bits_run_to_run_alone_or_in_a_batch_and_under_more_padding(eng):
    p, q, n_p, n_q = F.wide_case((257, 300, 260, 300), 3)
    eps, rho, w = case_params(n_p, n_q, 4.0, True)
    call = lambda *a, **k: eng.cloud_divergence_f64(*a, iters=K, **dict(KW, **k))
    a = call(p, q, n_p, n_q, eps=eps, reach=rho, mass_q=w)
    b = call(p, q, n_p, n_q, eps=eps, reach=rho, mass_q=w)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    for s in range(3):
        one = call(p[s:s + 1], q[s:s + 1], n_p[s:s + 1], n_q[s:s + 1], eps=eps[s:s + 1], reach=rho[s:s + 1], mass_q=w[s:s + 1])
        for k in a:
            assert one[k][0].tobytes() == a[k][s].tobytes(), '%s of sample %d' % (k, s)
    N, M = p.shape[1], q.shape[1]
    wide_p, wide_q = np.full((3, N + 37, 3), 9.0, np.float64), np.full((3, M + 5, 3), -9.0, np.float32)
    wide_p[:, :N], wide_q[:, :M] = p, q
    wd = call(wide_p, wide_q, n_p, n_q, eps=eps, reach=rho, mass_q=w)
    for k in ('divergence', 'col_err', 'self_err', 'transported'):
        assert wd[k].tobytes() == a[k].tobytes(), k
    for s in range(3):
        n, m = int(n_p[s]), int(n_q[s])
        assert wd['grad'][s, :n].tobytes() == a['grad'][s, :n].tobytes()
        for k, real in (('f', n), ('g', m), ('h_p', n), ('h_q', m)):
            assert wd[k][s, :real].tobytes() == a[k][s, :real].tobytes(), k
    F.assert_padding(wd, n_p, n_q)
    # the outputs are optional -- asked for or not, the value's bits are the same
    t = eng.cloud_divergence_f64(p[0, :n_p[0]], q[0, :n_q[0]], eps=eps[0], iters=K, reach=rho[0], mass_q=w[0])
    assert sorted(t) == ['divergence'] and t['divergence'][0] == a['divergence'][0]


# ---- the property, on the device ---------------------------------------------------------------------------------------------------
def test_a_finite_reach_leaves_the_unseen_side_and_the_seen_interior_alone(eng):
    p, q, col = UB.half_seen_pile()
    P, Q = np.zeros((1, 80, 3), np.float64), np.zeros((1, 40, 3), np.float32)
    P[0, :72], Q[0, :36] = p, q
    n_p, n_q = np.array([72], np.int32), np.array([36], np.int32)
    balanced = eng.cloud_divergence_f64(P, Q, n_p, n_q, eps=EPS, iters=K, want_grad=True)
    got = eng.cloud_divergence_f64(P, Q, n_p, n_q, eps=EPS, iters=K, reach=4 * EPS, mass_q=36 / 72, want_grad=True, want_col_err=True,
                                   want_transported=True)
    HOST.half_seen_thresholds(balanced['grad'][0, :72], got['grad'][0, :72], col, got['col_err'][0], 'float64 device:')
    ref = UB.pair64(None, q, EPS, 4 * EPS, 36 / 72, K, p64=p.astype(np.float64))
    assert abs(got['transported'][0] - ref[8]) <= BOUND['moved']
    assert (np.abs(got['grad'][0, :72]).max(axis=1) > 0).all()       # every real row has a gradient ...
    pad = got['grad'][0, 72:]
    assert (pad == 0).all() and not np.signbit(pad).any()            # ... and the padding exactly +0.0
    print('[unbalanced-f64] half-seen pile: transported %.4f' % got['transported'][0])
    assert 0.0 < got['transported'][0] <= 0.75                       # well below 1: half of the pile has nothing to pair with


# ---- nothing else is disturbed -----------------------------------------------------------------------------------------------------
def test_it_leaves_the_other_divergence_calls_and_the_dispatch_marks_alone(eng):
    p, q, n_p, n_q = U.chamfer_case((5, 3, 8, 8), 1, seed=0)
    calls = (lambda: eng.cloud_divergence(p, q, n_p, n_q, eps=4e-4, iters=7, **G.KW),
             lambda: eng.cloud_divergence(p, q, n_p, n_q, eps=4e-4, iters=7, reach=16e-4, mass_q=0.6, **KW),
             lambda: eng.cloud_divergence_f64(p, q, n_p, n_q, eps=4e-4, iters=7, **G.KW))
    before = [c() for c in calls]
    eng.dispatch_reset()
    marks = eng.last_dispatch()
    eng.cloud_divergence_f64(p, q, n_p, n_q, eps=4e-4, iters=7, reach=16e-4, mass_q=0.6, **KW)
    assert eng.last_dispatch() == marks
    for was, c in zip(before, calls):
        now = c()
        for k in was:
            assert was[k].tobytes() == now[k].tobytes(), k


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals(eng):
    p, q, n_p, n_q = F.wide_case((5, 3, 8, 8), 1)
    lib, h = eng.lib, eng.h
    terms = np.zeros((1,))
    e64 = lambda v: np.array([v], np.float64)
    eps, rho, w = e64(4e-4), e64(16e-4), e64(0.6)
    good = eng.cloud_divergence_f64(p, q, n_p, n_q, eps=eps, iters=7, reach=rho, mass_q=w, **KW)

    def call(p_, np_, q_, nq_, B, N, M, eps_, rho_, w_, iters, t_):
        f = lambda a, T_: None if a is None else a.ctypes.data_as(T_)
        return lib.drp_cloud_divergence_unbalanced_f64(h, f(p_, DP), f(np_, I32P), f(q_, FP), f(nq_, I32P), B, N, M, f(eps_, DP),
                                                       f(rho_, DP), f(w_, DP), iters, f(t_, DP), None, None, None, None, None)
    assert call(p, n_p, q, n_q, 1, 8, 8, eps, rho, w, 7, terms) == 0 and terms[0] == good['divergence'][0]
    big_p, big_q = np.zeros((1, 1025, 3), np.float64), np.zeros((1, 1025, 3), np.float32)
    nan_p, inf_q = p.copy(), q.copy()
    nan_p[0, 4, 1] = np.nan                                          # a real row (n_p = 5)
    inf_q[0, 0, 2] = np.inf
    i32 = lambda v: np.array([v], np.int32)
    one = e64(1.0)
    std = (p, n_p, q, n_q, 1, 8, 8, eps, rho, w, 7, terms)
    with_ = lambda i, v: std[:i] + (v,) + std[i + 1:]
    for args, word in ((with_(8, None), 'null'), (with_(9, None), 'null'),
                       (with_(8, e64(0.0)), 'rho'), (with_(8, e64(-16e-4)), 'rho'), (with_(8, e64(4e-4 / 1025)), 'rho'),   # below eps / 1024
                       (with_(8, e64(np.nan)), 'rho'), (with_(8, e64(-np.inf)), 'rho'),
                       (with_(9, e64(0.1249)), 'mass_q'), (with_(9, e64(8.001)), 'mass_q'), (with_(9, e64(np.nan)), 'mass_q'),
                       (with_(9, e64(0.0)), 'mass_q'),
                       (with_(8, e64(np.inf)), 'balanced'),          # w != 1 without a finite reach
                       # ... and everything drp_cloud_divergence_f64 refuses
                       (with_(0, None), 'null'), (with_(1, None), 'null'), (with_(2, None), 'null'), (with_(3, None), 'null'),
                       (with_(7, None), 'null'), (with_(11, None), 'null'),
                       (with_(0, nan_p), 'finite'), (with_(2, inf_q), 'finite'),
                       ((p, n_p, big_q, n_q, 1, 8, 1025, eps, rho, w, 7, terms), '1025'),
                       ((big_p, n_p, q, n_q, 1, 1025, 8, eps, rho, w, 7, terms), '1025'),
                       (with_(1, i32(0)), ''), (with_(1, i32(9)), ''), (with_(3, i32(0)), ''), (with_(3, i32(9)), ''),
                       (with_(4, 0), ''), (with_(5, 0), ''), (with_(6, 0), ''),
                       (with_(7, e64(0.0)), 'eps'), (with_(7, e64(np.inf)), 'eps'), (with_(10, 0), 'iters'),
                       (with_(10, F.TRANSPORT_MAX_ITERS + 1), 'iters')):
        eng.dispatch_reset()
        eng.probe_begin('loss')
        assert call(*args) == -1, word                               # DRP_EINVAL ...
        assert word in eng.lib.drp_last_error(h).decode(), (word, eng.lib.drp_last_error(h))      # ... with a message ...
        assert eng.probe_read()[1] == 0                              # ... and no kernel
        eng.probe_begin(None)
        again = eng.cloud_divergence_f64(p, q, n_p, n_q, eps=eps, iters=7, reach=rho, mass_q=w, **KW)
        for k in good:
            assert again[k].tobytes() == good[k].tobytes(), (word, k)
    # the edges of the ranges are served
    assert call(p, n_p, q, n_q, 1, 8, 8, eps, e64(4e-4 / 1024), e64(0.125), 7, terms) == 0
    assert call(p, n_p, q, n_q, 1, 8, 8, eps, rho, e64(8.0), 7, terms) == 0
    assert call(p, n_p, q, n_q, 1, 8, 8, eps, e64(np.inf), one, 7, terms) == 0
    with pytest.raises(DrpError, match='rho'):
        eng.cloud_divergence_f64(p, q, n_p, n_q, eps=4e-4, iters=7, reach=-1.0)
    with pytest.raises(DrpError, match='mass_q'):
        eng.cloud_divergence_f64(p, q, n_p, n_q, eps=4e-4, iters=7, reach=16e-4, mass_q=9.0)
    with pytest.raises(DrpError, match='balanced'):
        eng.cloud_divergence_f64(p, q, n_p, n_q, eps=4e-4, iters=7, reach=np.inf, mass_q=1.5)
    with pytest.raises(ValueError, match='give reach'):
        eng.cloud_divergence_f64(p, q, n_p, n_q, eps=4e-4, iters=7, mass_q=1.5)

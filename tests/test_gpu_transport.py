"""GPU: the stand-alone entropy-regularised transport distance (drp_cloud_transport, csrc/k_sinkhorn.h) through ctypes, against
include/drp.h's definition in numpy float64 (tests/_transport_ref.py) on the kernel's fp32 cost matrix.

Both sides do the same IEEE double operations in the same order; they differ in the order the terms of a log-sum-exp are added
(the kernel: ascending within each of the lanes that share a sum, then an xor butterfly) and in whose exp and log they call.  A
Sinkhorn sweep is a contraction, so those last-place differences do not build up over the sweeps.

What each deviation is measured against (printed before it is asserted):
  term     its own value;
  f, g     the sample's largest |f_i|, |g_j|: a dual passes through zero, only its size against the costs means anything;
  gradient the sample's largest entry, as for the other cloud losses, plus one fp32 rounding (2^-24 of that entry);
  col_err  the total mass 1: it is a sum of differences of masses b_j that add up to 1, and falls to their rounding when K is
           enough -- measured against itself the bound would be a statement about cancellation, not about the kernel.
Bounds: 5 x the worst figure measured on one MI355X over every case, sweep count and eps below (README: bounds pinned at 5 x the
measured error), each at most 1e-10, the bound of the project's other float64 device calls:
  MEASURED (worst)   term 9.1e-16   duals 2.2e-15   col_err 4.5e-16   gradient 0 beyond its one fp32 rounding
The gradient's double part measured 0 -- every device entry is the reference's entry rounded to fp32 or its neighbour -- and a
bound of 5 x 0 would promise the bits of two libraries' exp.  Its rows are sums over the plan entries the term sums, weighted by
differences instead of costs, and the plan is exp of the duals: it is held to the duals' bound, the largest of the three.
The sizes: 1 x 1 and 1 x 7; 5 x 3 and 3 x 5; 64 x 64 and 65 x 63 (a wavefront and the 256-thread workgroup are crossed by the
(row, part) items); 257 x 300; 1024 x 1024 once at K = 10.  B in {1, 3}: at B = 3 the counts are ragged and lie below the padding
on both sides, and eps differs per sample.  K in {1, the default}; eps = 1 and 1/100 of the squared spacing."""
import ctypes

import numpy as np
import pytest

import _transport_ref as T
import _untracked_ref as U
from dyn_res_pile_manip_amd import train_gnn_dyn as TG
from dyn_res_pile_manip_amd._lib import DrpError
from dyn_res_pile_manip_amd.engine import Engine

pytestmark = pytest.mark.gpu
I32P = ctypes.POINTER(ctypes.c_int32)
FP = ctypes.POINTER(ctypes.c_float)
DP = ctypes.POINTER(ctypes.c_double)

MEASURED = {'term': 9.1e-16, 'dual': 2.2e-15, 'grad': 2.2e-15, 'col': 4.5e-16}      # the module docstring's line (grad: the duals')
BOUND = {k: 5 * v for k, v in MEASURED.items()}
FP32_ROUND = 2.0 ** -24

SHAPES = [(1, 1, 1, 1), (1, 7, 4, 9), (5, 3, 8, 8), (3, 5, 8, 8), (64, 64, 70, 66), (65, 63, 65, 64), (257, 300, 260, 300)]
EPS_SCALES = (1.0, 0.01)
KW = dict(want_grad=True, want_dual=True, want_col_err=True)


@pytest.fixture(scope='module')
def eng():
    e = Engine(0)                       # no weights: the metric needs none
    yield e
    e.close()


def case_eps(n_p, n_q, scale):
    """per sample: the squared spacing of the case's clouds times `scale`, a quarter more for every further sample"""
    return T.case_eps(n_p, n_q, scale) * (1.0 + 0.25 * np.arange(len(n_p)))


def deviations(got, ref, n_p, n_q):
    """-> the worst relative deviations {'term', 'dual', 'grad', 'col'} over the samples, by the module docstring's denominators"""
    dev = {'term': 0.0, 'dual': 0.0, 'grad': 0.0, 'col': 0.0}
    for b in range(len(n_p)):
        n, m = int(n_p[b]), int(n_q[b])
        dev['term'] = max(dev['term'], abs(got['transport'][b] - ref['transport'][b]) / ref['transport'][b])
        size = max(np.abs(ref['f'][b]).max(), np.abs(ref['g'][b]).max())
        dev['dual'] = max(dev['dual'], max(np.abs(got['f'][b] - ref['f'][b]).max(), np.abs(got['g'][b] - ref['g'][b]).max()) / size)
        gmax = np.abs(ref['grad'][b]).max()
        dev['grad'] = max(dev['grad'], max(0.0, np.abs(got['grad'][b].astype(np.float64) - ref['grad'][b]).max() / gmax - FP32_ROUND))
        dev['col'] = max(dev['col'], abs(got['col_err'][b] - ref['col_err'][b]) / 1.0)
        # padding: duals 0, gradient +0.0 exactly
        assert (got['f'][b, n:] == 0).all() and (got['g'][b, m:] == 0).all()
        pad = got['grad'][b, n:]
        assert (pad == 0).all() and not np.signbit(pad).any()
    return dev


def check(eng, p, q, n_p, n_q, eps, K, label):
    got = eng.cloud_transport(p, q, n_p, n_q, eps=eps, iters=K, **KW)
    assert got['grad'].dtype == np.float32 and all(got[k].dtype == np.float64 for k in ('transport', 'f', 'g', 'col_err'))
    ref = T.transport64(p, q, n_p, n_q, eps, K)
    dev = deviations(got, ref, n_p, n_q)
    print('[transport] %s K=%d eps=%.1e: term %.2e, duals %.2e, gradient %.2e (beyond one fp32 rounding), col_err %.2e; col_err '
          'itself %.2e' % (label, K, eps[0], dev['term'], dev['dual'], dev['grad'], dev['col'], ref['col_err'].max()))
    for k in dev:
        assert dev[k] <= BOUND[k] <= 1e-10, (label, K, k, dev[k])
    return got


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('shape', SHAPES)
def test_against_the_float64_definition(eng, shape, B):
    p, q, n_p, n_q = U.chamfer_case(shape, B, seed=0)
    if B == 3 and shape != (1, 1, 1, 1):
        assert (n_p < p.shape[1]).any() and (n_q < q.shape[1]).any()      # counts below the padding on both sides
    for scale in EPS_SCALES:
        for K in (1, TG.TRANSPORT_ITERS):
            check(eng, p, q, n_p, n_q, case_eps(n_p, n_q, scale), K, '%s B=%d' % (shape, B))


def test_the_cap_once(eng):
    p, q, n_p, n_q = U.chamfer_case((1024, 1024, 1024, 1024), 1, seed=0)
    got = check(eng, p, q, n_p, n_q, case_eps(n_p, n_q, 1.0), 10, '1024 x 1024')
    assert (np.abs(got['grad'][0]).max(axis=1) > 0).all()


# ---- bits ------------------------------------------------------------------------------------------------------------------------
def test_same_bits_run_to_run_alone_or_in_a_batch_and_under_more_padding(eng):
    p, q, n_p, n_q = U.chamfer_case((257, 300, 260, 300), 3, seed=0)
    eps = case_eps(n_p, n_q, 1.0)
    K = TG.TRANSPORT_ITERS
    a = eng.cloud_transport(p, q, n_p, n_q, eps=eps, iters=K, **KW)
    b = eng.cloud_transport(p, q, n_p, n_q, eps=eps, iters=K, **KW)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    for s in range(3):
        one = eng.cloud_transport(p[s:s + 1], q[s:s + 1], n_p[s:s + 1], n_q[s:s + 1], eps=eps[s:s + 1], iters=K, **KW)
        for k in a:
            assert one[k][0].tobytes() == a[k][s].tobytes(), '%s of sample %d' % (k, s)
    # the same clouds under a larger padding that holds other rubbish
    N, M = p.shape[1], q.shape[1]
    wide_p, wide_q = np.full((3, N + 37, 3), 9.0, np.float32), np.full((3, M + 5, 3), -9.0, np.float32)
    wide_p[:, :N], wide_q[:, :M] = p, q
    w = eng.cloud_transport(wide_p, wide_q, n_p, n_q, eps=eps, iters=K, **KW)
    assert w['transport'].tobytes() == a['transport'].tobytes() and w['col_err'].tobytes() == a['col_err'].tobytes()
    for s in range(3):
        n, m = int(n_p[s]), int(n_q[s])
        assert w['grad'][s, :n].tobytes() == a['grad'][s, :n].tobytes()
        assert w['f'][s, :n].tobytes() == a['f'][s, :n].tobytes() and w['g'][s, :m].tobytes() == a['g'][s, :m].tobytes()
        pad = w['grad'][s, n:]
        assert (pad == 0).all() and not np.signbit(pad).any()
        assert (w['f'][s, n:] == 0).all() and (w['g'][s, m:] == 0).all()
    # the outputs are optional, and a single pair may come without the batch axis
    t = eng.cloud_transport(p[0, :n_p[0]], q[0, :n_q[0]], eps=eps[0], iters=K)
    assert sorted(t) == ['transport'] and t['transport'][0] == a['transport'][0]


def test_every_real_row_has_a_gradient_where_the_matching_leaves_rows_out(eng):
    """the reason the feature exists: n_p = 40 predicted rows against n_q = 25 targets"""
    p, q, n_p, n_q = U.chamfer_case((40, 25, 44, 30), 1, seed=0)
    got = eng.cloud_transport(p, q, n_p, n_q, eps=case_eps(n_p, n_q, 1.0), iters=TG.TRANSPORT_ITERS, **KW)
    match = eng.cloud_match(p, q, n_p, n_q, want_grad=True)
    rows_t = int((np.abs(got['grad'][0, :40]).max(axis=1) > 0).sum())
    rows_m = int((np.abs(match['grad'][0, :40]).max(axis=1) > 0).sum())
    print('[transport] 40 x 25: rows with a gradient: transport %d, match %d; col_err %.2e' % (rows_t, rows_m, got['col_err'][0]))
    assert rows_t == 40 and rows_m == 25
    pad = got['grad'][0, 40:]
    assert (pad == 0).all() and not np.signbit(pad).any()
    # and the other way round every target's mass is placed: the columns' marginals are met to col_err
    p, q, n_p, n_q = U.chamfer_case((25, 40, 30, 44), 1, seed=0)
    got = eng.cloud_transport(p, q, n_p, n_q, eps=case_eps(n_p, n_q, 1.0), iters=TG.TRANSPORT_ITERS, **KW)
    assert (np.abs(got['grad'][0, :25]).max(axis=1) > 0).all() and got['col_err'][0] <= T.COL_ERR_MAX


def test_it_counts_under_the_loss_class_and_leaves_the_dispatch_marks(eng):
    p, q, n_p, n_q = U.chamfer_case((5, 3, 8, 8), 1, seed=0)
    eng.dispatch_reset()
    marks = eng.last_dispatch()
    eng.probe_begin('loss')
    eng.cloud_transport(p, q, n_p, n_q, eps=4e-4, iters=3, **KW)
    ms, launches = eng.probe_read()
    eng.probe_begin(None)
    assert launches == 1 and ms > 0
    assert eng.last_dispatch() == marks


def test_refusals(eng):
    p, q, n_p, n_q = U.chamfer_case((5, 3, 8, 8), 1, seed=0)
    lib, h = eng.lib, eng.h
    terms = np.zeros((1,))
    eps = np.array([4e-4])
    good = eng.cloud_transport(p, q, n_p, n_q, eps=eps, iters=7, **KW)

    def call(p_, np_, q_, nq_, B, N, M, eps_, K, t_):
        f = lambda a, T_: None if a is None else a.ctypes.data_as(T_)
        return lib.drp_cloud_transport(h, f(p_, FP), f(np_, I32P), f(q_, FP), f(nq_, I32P), B, N, M, f(eps_, DP), K, f(t_, DP),
                                       None, None, None)
    assert call(p, n_p, q, n_q, 1, 8, 8, eps, 7, terms) == 0 and terms[0] == good['transport'][0]
    big = np.zeros((1, 1025, 3), np.float32)
    nan_p, inf_q = p.copy(), q.copy()
    nan_p[0, 4, 1] = np.nan                                          # a real row (n_p = 5)
    inf_q[0, 0, 2] = np.inf
    i32 = lambda v: np.array([v], np.int32)
    e64 = lambda v: np.array([v], np.float64)
    for args in ((None, n_p, q, n_q, 1, 8, 8, eps, 7, terms), (p, None, q, n_q, 1, 8, 8, eps, 7, terms),
                 (p, n_p, None, n_q, 1, 8, 8, eps, 7, terms), (p, n_p, q, None, 1, 8, 8, eps, 7, terms),
                 (p, n_p, q, n_q, 1, 8, 8, None, 7, terms), (p, n_p, q, n_q, 1, 8, 8, eps, 7, None),
                 (p, n_p, q, n_q, 0, 8, 8, eps, 7, terms),
                 (p, n_p, q, n_q, 1, 8, 0, eps, 7, terms), (p, n_p, q, n_q, 1, 0, 8, eps, 7, terms),
                 (p, n_p, big, n_q, 1, 8, 1025, eps, 7, terms), (big, n_p, q, n_q, 1, 1025, 8, eps, 7, terms),
                 (p, i32(0), q, n_q, 1, 8, 8, eps, 7, terms), (p, i32(9), q, n_q, 1, 8, 8, eps, 7, terms),
                 (p, n_p, q, i32(0), 1, 8, 8, eps, 7, terms), (p, n_p, q, i32(9), 1, 8, 8, eps, 7, terms),
                 (p, n_p, q, n_q, 1, 8, 8, e64(0.0), 7, terms), (p, n_p, q, n_q, 1, 8, 8, e64(-4e-4), 7, terms),
                 (p, n_p, q, n_q, 1, 8, 8, e64(np.inf), 7, terms), (p, n_p, q, n_q, 1, 8, 8, e64(np.nan), 7, terms),
                 (p, n_p, q, n_q, 1, 8, 8, eps, 0, terms), (p, n_p, q, n_q, 1, 8, 8, eps, -1, terms),
                 (p, n_p, q, n_q, 1, 8, 8, eps, 1001, terms),
                 (nan_p, n_p, q, n_q, 1, 8, 8, eps, 7, terms), (p, n_p, inf_q, n_q, 1, 8, 8, eps, 7, terms)):
        assert call(*args) == -1, args[4:9]                          # DRP_EINVAL
        again = eng.cloud_transport(p, q, n_p, n_q, eps=eps, iters=7, **KW)     # the context answers with its earlier bits
        for k in good:
            assert again[k].tobytes() == good[k].tobytes(), (args[4:9], k)
    assert call(p, n_p, q, n_q, 1, 8, 8, eps, 1000, terms) == 0      # the cap itself is served
    with pytest.raises(DrpError, match='1025'):
        eng.cloud_transport(big, q, [5], [3], eps=4e-4, iters=7)
    with pytest.raises(DrpError, match='eps'):
        eng.cloud_transport(p, q, n_p, n_q, eps=0.0, iters=7)
    with pytest.raises(DrpError, match='iters'):
        eng.cloud_transport(p, q, n_p, n_q, eps=4e-4, iters=0)
    with pytest.raises(ValueError):
        eng.cloud_transport(p, q, n_p, n_q)
    nan_pad = p.copy()
    nan_pad[0, 6] = np.nan                                           # padding is never read as points
    b = eng.cloud_transport(nan_pad, q, n_p, n_q, eps=eps, iters=7, **KW)
    for k in good:
        assert b[k].tobytes() == good[k].tobytes(), k

"""GPU: the stand-alone Sinkhorn divergence (drp_cloud_divergence, csrc/k_sinkhorn.h) through ctypes, against include/drp.h's
definition in numpy float64 (tests/_divergence_ref.py) on the kernel's fp32 cost matrices.

Both sides do the same IEEE double operations in the same order; they differ in the order the terms of a sum are added (the
kernel: ascending within each of the lanes that share a sum, then an xor butterfly; the value sums over the workgroup) and in whose
exp and log they call.  Every sweep is a contraction, so those last-place differences do not build up.

What each deviation is measured against (printed before it is asserted), as tests/test_gpu_transport.py defines them:
  value    its own value (the clouds are unrelated: it lies well above the cancellation of its four sums);
  duals    f, g, h_p, h_q against the sample's largest dual entry;
  gradient the sample's largest entry, beyond one fp32 rounding (2^-24 of that entry);
  col_err, self_err   the total mass 1.
Bounds: 5 x the worst figure measured on one MI355X over every case, sweep count and eps below, each below 1e-10:
  MEASURED (worst)   value 1.2e-14   duals 3.8e-15   col_err 1.1e-15   self_err 2.9e-16   gradient 0 beyond its one fp32 rounding
The value's figure is larger than the duals' because its four sums cancel (it is a fraction of each of them), not because of
the sweeps.  The gradient's double part measured 0 -- every device entry is the reference's entry rounded to fp32 or its neighbour
-- and 5 x 0 would promise the bits of two libraries' exp: as in tests/test_gpu_transport.py it is held to the duals' bound.
The sizes are tests/test_gpu_transport.py's, with 16 x 17 and 33 x 32 added, which sit on kt_parts' thresholds for the self
problems: a sum is shared by 16 lanes at n = 16 and by 32 at n = 17 (no more lanes than terms), and the 32 lanes x n items fill
two rounds of the workgroup exactly at n = 32 and need a third at n = 33.  B in {1, 3}: at B = 3 the counts are ragged, lie below
the padding on both sides, and eps differs per sample.  K in {1, the default}; eps = 1 and 1/100 of the squared spacing."""
import ctypes

import numpy as np
import pytest

import _divergence_ref as D
import _transport_ref as T
import _untracked_ref as U
from dyn_res_pile_manip_amd import train_gnn_dyn as TG
from dyn_res_pile_manip_amd._lib import DrpError, TRANSPORT_MAX_ITERS
from dyn_res_pile_manip_amd.engine import Engine

pytestmark = pytest.mark.gpu
I32P = ctypes.POINTER(ctypes.c_int32)
FP = ctypes.POINTER(ctypes.c_float)
DP = ctypes.POINTER(ctypes.c_double)

MEASURED = {'value': 1.2e-14, 'dual': 3.8e-15, 'grad': 3.8e-15, 'col': 1.1e-15, 'self': 2.9e-16}      # the module docstring's line (grad: the duals')
BOUND = {k: 5 * v for k, v in MEASURED.items()}
FP32_ROUND = 2.0 ** -24

SHAPES = [(1, 1, 1, 1), (1, 7, 4, 9), (5, 3, 8, 8), (3, 5, 8, 8), (64, 64, 70, 66), (65, 63, 65, 64), (257, 300, 260, 300),
          (16, 17, 20, 20), (33, 32, 40, 40)]
EPS_SCALES = (1.0, 0.01)
DUALS = ('f', 'g', 'h_p', 'h_q')
KW = dict(want_grad=True, want_dual=True, want_col_err=True, want_self_err=True)
K = TG.TRANSPORT_ITERS


@pytest.fixture(scope='module')
def eng():
    e = Engine(0)                       # no weights: the metric needs none
    yield e
    e.close()


def case_eps(n_p, n_q, scale):
    """per sample: the squared spacing of the case's clouds times `scale`, a quarter more for every further sample"""
    return T.case_eps(n_p, n_q, scale) * (1.0 + 0.25 * np.arange(len(n_p)))


def assert_padding(got, n_p, n_q):
    """duals 0, gradient +0.0 exactly"""
    for b in range(len(n_p)):
        n, m = int(n_p[b]), int(n_q[b])
        assert (got['f'][b, n:] == 0).all() and (got['g'][b, m:] == 0).all()
        assert (got['h_p'][b, n:] == 0).all() and (got['h_q'][b, m:] == 0).all()
        pad = got['grad'][b, n:]
        assert (pad == 0).all() and not np.signbit(pad).any()


def deviations(got, ref, n_p, n_q):
    """-> the worst relative deviations over the samples, by the module docstring's denominators"""
    dev = dict((k, 0.0) for k in MEASURED)
    for b in range(len(n_p)):
        dev['value'] = max(dev['value'], abs(got['divergence'][b] - ref['divergence'][b]) / abs(ref['divergence'][b]))
        size = max(np.abs(ref[k][b]).max() for k in DUALS)
        dev['dual'] = max(dev['dual'], max(np.abs(got[k][b] - ref[k][b]).max() for k in DUALS) / size)
        gmax = np.abs(ref['grad'][b]).max()
        dev['grad'] = max(dev['grad'], max(0.0, np.abs(got['grad'][b].astype(np.float64) - ref['grad'][b]).max() / gmax - FP32_ROUND))
        dev['col'] = max(dev['col'], abs(got['col_err'][b] - ref['col_err'][b]) / 1.0)
        dev['self'] = max(dev['self'], np.abs(got['self_err'][b] - ref['self_err'][b]).max() / 1.0)
    assert_padding(got, n_p, n_q)
    return dev


def check(eng, p, q, n_p, n_q, eps, iters, label):
    got = eng.cloud_divergence(p, q, n_p, n_q, eps=eps, iters=iters, **KW)
    assert sorted(got) == sorted(('divergence', 'grad', 'col_err', 'self_err') + DUALS)
    assert got['grad'].dtype == np.float32 and all(got[k].dtype == np.float64 for k in got if k != 'grad')
    ref = D.divergence64(p, q, n_p, n_q, eps, iters)
    dev = deviations(got, ref, n_p, n_q)
    print('[divergence] %s K=%d eps=%.1e: value %.2e, duals %.2e, gradient %.2e (beyond one fp32 rounding), col_err %.2e, self_err '
          '%.2e; self_err itself %.2e' % (label, iters, eps[0], dev['value'], dev['dual'], dev['grad'], dev['col'], dev['self'],
                                          ref['self_err'].max()))
    for k in dev:
        assert dev[k] <= BOUND[k] < 1e-10, (label, iters, k, dev[k])
    return got


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('shape', SHAPES)
def test_against_the_float64_definition(eng, shape, B):
    p, q, n_p, n_q = U.chamfer_case(shape, B, seed=0)
    if B == 3 and shape != (1, 1, 1, 1):
        assert (n_p < p.shape[1]).any() and (n_q < q.shape[1]).any()      # counts below the padding on both sides
    for scale in EPS_SCALES:
        for iters in (1, K):
            check(eng, p, q, n_p, n_q, case_eps(n_p, n_q, scale), iters, '%s B=%d' % (shape, B))


def test_the_cap_once(eng):
    p, q, n_p, n_q = U.chamfer_case((1024, 1024, 1024, 1024), 1, seed=0)
    got = check(eng, p, q, n_p, n_q, case_eps(n_p, n_q, 1.0), 2, '1024 x 1024')
    assert (np.abs(got['grad'][0]).max(axis=1) > 0).all()


# ---- bits ------------------------------------------------------------------------------------------------------------------------
def test_same_bits_run_to_run_alone_or_in_a_batch_and_under_more_padding(eng):
    p, q, n_p, n_q = U.chamfer_case((257, 300, 260, 300), 3, seed=0)
    eps = case_eps(n_p, n_q, 1.0)
    a = eng.cloud_divergence(p, q, n_p, n_q, eps=eps, iters=K, **KW)
    b = eng.cloud_divergence(p, q, n_p, n_q, eps=eps, iters=K, **KW)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    for s in range(3):
        one = eng.cloud_divergence(p[s:s + 1], q[s:s + 1], n_p[s:s + 1], n_q[s:s + 1], eps=eps[s:s + 1], iters=K, **KW)
        for k in a:
            assert one[k][0].tobytes() == a[k][s].tobytes(), '%s of sample %d' % (k, s)
    # the same clouds under a larger padding that holds other rubbish
    N, M = p.shape[1], q.shape[1]
    wide_p, wide_q = np.full((3, N + 37, 3), 9.0, np.float32), np.full((3, M + 5, 3), -9.0, np.float32)
    wide_p[:, :N], wide_q[:, :M] = p, q
    w = eng.cloud_divergence(wide_p, wide_q, n_p, n_q, eps=eps, iters=K, **KW)
    for k in ('divergence', 'col_err', 'self_err'):
        assert w[k].tobytes() == a[k].tobytes(), k
    for s in range(3):
        n, m = int(n_p[s]), int(n_q[s])
        assert w['grad'][s, :n].tobytes() == a['grad'][s, :n].tobytes()
        for k, real in (('f', n), ('g', m), ('h_p', n), ('h_q', m)):
            assert w[k][s, :real].tobytes() == a[k][s, :real].tobytes(), k
    assert_padding(w, n_p, n_q)
    # the outputs are optional -- asked for or not, the value's bits are the same -- and a single pair may come without the batch axis
    t = eng.cloud_divergence(p[0, :n_p[0]], q[0, :n_q[0]], eps=eps[0], iters=K)
    assert sorted(t) == ['divergence'] and t['divergence'][0] == a['divergence'][0]


def test_a_perfect_prediction_is_left_alone_where_transport_pushes_it(eng):
    p = D.grid_cloud(40, 3)[None]
    eps = D.GRID_SPACING ** 2
    div = eng.cloud_divergence(p, p.copy(), eps=eps, iters=K, want_grad=True)
    tra = eng.cloud_transport(p, p.copy(), eps=eps, iters=K, want_grad=True)
    g_div, g_tra = float(np.abs(div['grad']).max()), float(np.abs(tra['grad']).max())
    print('[divergence] q = p, 40 points, K = %d: divergence %.2e, transport term %.2e; largest gradient component %.2e against '
          'transport\'s %.2e' % (K, div['divergence'][0], tra['transport'][0], g_div, g_tra))
    assert g_div <= 1e-2 * g_tra


def test_every_real_row_has_a_gradient_and_the_padding_none(eng):
    p, q, n_p, n_q = U.chamfer_case((40, 25, 44, 30), 1, seed=0)
    got = eng.cloud_divergence(p, q, n_p, n_q, eps=case_eps(n_p, n_q, 1.0), iters=K, **KW)
    rows = int((np.abs(got['grad'][0, :40]).max(axis=1) > 0).sum())
    print('[divergence] 40 x 25: rows with a gradient: %d; col_err %.2e, self_err %s' % (rows, got['col_err'][0], got['self_err'][0]))
    assert rows == 40
    assert_padding(got, n_p, n_q)


def test_it_counts_under_the_loss_class_and_leaves_the_dispatch_marks(eng):
    p, q, n_p, n_q = U.chamfer_case((5, 3, 8, 8), 1, seed=0)
    eng.dispatch_reset()
    marks = eng.last_dispatch()
    eng.probe_begin('loss')
    eng.cloud_divergence(p, q, n_p, n_q, eps=4e-4, iters=3, **KW)
    ms, launches = eng.probe_read()
    eng.probe_begin(None)
    assert launches == 1 and ms > 0                                  # one timed region around the call's two kernels
    assert eng.last_dispatch() == marks


def test_refusals(eng):
    p, q, n_p, n_q = U.chamfer_case((5, 3, 8, 8), 1, seed=0)
    lib, h = eng.lib, eng.h
    terms = np.zeros((1,))
    eps = np.array([4e-4])
    good = eng.cloud_divergence(p, q, n_p, n_q, eps=eps, iters=7, **KW)

    def call(p_, np_, q_, nq_, B, N, M, eps_, iters, t_):
        f = lambda a, T_: None if a is None else a.ctypes.data_as(T_)
        return lib.drp_cloud_divergence(h, f(p_, FP), f(np_, I32P), f(q_, FP), f(nq_, I32P), B, N, M, f(eps_, DP), iters, f(t_, DP),
                                        None, None, None, None)
    assert call(p, n_p, q, n_q, 1, 8, 8, eps, 7, terms) == 0 and terms[0] == good['divergence'][0]
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
                 (p, n_p, big, n_q, 1, 8, 1025, eps, 7, terms), (big, n_p, q, n_q, 1, 1025, 8, eps, 7, terms),      # more than 1024 points
                 (p, i32(0), q, n_q, 1, 8, 8, eps, 7, terms), (p, i32(9), q, n_q, 1, 8, 8, eps, 7, terms),          # an empty cloud
                 (p, n_p, q, i32(0), 1, 8, 8, eps, 7, terms), (p, n_p, q, i32(9), 1, 8, 8, eps, 7, terms),
                 (p, n_p, q, n_q, 1, 8, 8, e64(0.0), 7, terms), (p, n_p, q, n_q, 1, 8, 8, e64(-4e-4), 7, terms),
                 (p, n_p, q, n_q, 1, 8, 8, e64(np.inf), 7, terms), (p, n_p, q, n_q, 1, 8, 8, e64(np.nan), 7, terms),
                 (p, n_p, q, n_q, 1, 8, 8, eps, 0, terms), (p, n_p, q, n_q, 1, 8, 8, eps, -1, terms),
                 (p, n_p, q, n_q, 1, 8, 8, eps, TRANSPORT_MAX_ITERS + 1, terms),
                 (nan_p, n_p, q, n_q, 1, 8, 8, eps, 7, terms), (p, n_p, inf_q, n_q, 1, 8, 8, eps, 7, terms)):
        assert call(*args) == -1, args[4:9]                          # DRP_EINVAL
        again = eng.cloud_divergence(p, q, n_p, n_q, eps=eps, iters=7, **KW)    # the context answers with its earlier bits
        for k in good:
            assert again[k].tobytes() == good[k].tobytes(), (args[4:9], k)
    assert call(p, n_p, q, n_q, 1, 8, 8, eps, TRANSPORT_MAX_ITERS, terms) == 0      # the cap itself is served
    with pytest.raises(DrpError, match='1025'):
        eng.cloud_divergence(big, q, [5], [3], eps=4e-4, iters=7)
    with pytest.raises(DrpError, match='eps'):
        eng.cloud_divergence(p, q, n_p, n_q, eps=0.0, iters=7)
    with pytest.raises(DrpError, match='iters'):
        eng.cloud_divergence(p, q, n_p, n_q, eps=4e-4, iters=0)
    for kw in ({}, {'eps': 4e-4}, {'iters': 7}):                     # both are required
        with pytest.raises(ValueError):
            eng.cloud_divergence(p, q, n_p, n_q, **kw)
    nan_pad = p.copy()
    nan_pad[0, 6] = np.nan                                           # padding is never read as points
    b = eng.cloud_divergence(nan_pad, q, n_p, n_q, eps=eps, iters=7, **KW)
    for k in good:
        assert b[k].tobytes() == good[k].tobytes(), k

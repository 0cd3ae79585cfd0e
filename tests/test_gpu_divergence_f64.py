"""GPU: the float64 yardstick of the Sinkhorn divergence stand-alone (drp_cloud_divergence_f64, csrc/k_sinkhorn.h) through
ctypes, against tests/_divergence_f64_ref.py's divergence64_wide: include/drp.h's definition in numpy float64 with nothing in fp32.

p carries bits no float32 has -- _untracked_ref.chamfer_case's floats plus 1e-9 x a standard normal draw -- as the float64 tape's
predicted state does; q is float32.  Both sides do the same IEEE double operations in the same order; they differ in the order the
terms of a sum are added (the kernel: ascending within each of the lanes that share a sum, then an xor butterfly; the value sums
over the workgroup) and in whose exp and log they call.

What each deviation is measured against (printed before it is asserted), as tests/test_gpu_divergence.py defines them, with NO
fp32-rounding allowance for the gradient -- it is float64 here:
  value    its own value;   duals    f, g, h_p, h_q against the sample's largest dual entry;   gradient   the sample's largest entry;
  col_err, self_err   the total mass 1.
Bounds: 5 x the worst figure measured on one MI355X over every case, sweep count and eps below, each below 1e-10:
  MEASURED (worst)   value 1.3e-14   duals 5.5e-15   gradient 1.8e-14   col_err 6.7e-16   self_err 2.5e-16
The gradient's figure is the largest: it is the difference of two sums, taken against the entry that is left.
The sizes, B, K and eps scales are tests/test_gpu_divergence.py's (16 x 17 and 33 x 32 sit on kt_parts' thresholds), and
1024 x 1024 runs once at K = 2."""
import ctypes

import numpy as np
import pytest

import _divergence_f64_ref as R
import _untracked_ref as U
from dyn_res_pile_manip_amd import train_gnn_dyn as TG
from dyn_res_pile_manip_amd._lib import DrpError, TRANSPORT_MAX_ITERS
from dyn_res_pile_manip_amd.engine import Engine
from test_gpu_divergence import DUALS, EPS_SCALES, KW, SHAPES, case_eps

pytestmark = pytest.mark.gpu
I32P = ctypes.POINTER(ctypes.c_int32)
FP = ctypes.POINTER(ctypes.c_float)
DP = ctypes.POINTER(ctypes.c_double)

MEASURED = {'value': 1.3e-14, 'dual': 5.5e-15, 'grad': 1.8e-14, 'col': 6.7e-16, 'self': 2.5e-16}      # the module docstring's line
BOUND = {k: 5 * v for k, v in MEASURED.items()}
K = TG.TRANSPORT_ITERS


@pytest.fixture(scope='module')
def eng():
    e = Engine(0)                       # no weights: the metric needs none
    yield e
    e.close()


def wide_case(shape, B, seed=0):
    """chamfer_case with p as float64 carrying non-fp32 bits (the padding's rubbish too)"""
    p, q, n_p, n_q = U.chamfer_case(shape, B, seed=seed)
    p64 = p.astype(np.float64) + 1e-9 * np.random.default_rng(4242 + 31 * shape[0] + B).standard_normal(p.shape)
    assert (p64.astype(np.float32).astype(np.float64) != p64).any()
    return p64, q, n_p, n_q


def assert_padding(got, n_p, n_q):
    """duals 0, gradient +0.0 exactly"""
    for b in range(len(n_p)):
        n, m = int(n_p[b]), int(n_q[b])
        assert (got['f'][b, n:] == 0).all() and (got['g'][b, m:] == 0).all()
        assert (got['h_p'][b, n:] == 0).all() and (got['h_q'][b, m:] == 0).all()
        pad = got['grad'][b, n:]
        assert (pad == 0).all() and not np.signbit(pad).any()


def deviations(got, ref, n_p, n_q):
    dev = dict((k, 0.0) for k in MEASURED)
    for b in range(len(n_p)):
        dev['value'] = max(dev['value'], abs(got['divergence'][b] - ref['divergence'][b]) / abs(ref['divergence'][b]))
        size = max(np.abs(ref[k][b]).max() for k in DUALS)
        dev['dual'] = max(dev['dual'], max(np.abs(got[k][b] - ref[k][b]).max() for k in DUALS) / size)
        dev['grad'] = max(dev['grad'], np.abs(got['grad'][b] - ref['grad'][b]).max() / np.abs(ref['grad'][b]).max())
        dev['col'] = max(dev['col'], abs(got['col_err'][b] - ref['col_err'][b]) / 1.0)
        dev['self'] = max(dev['self'], np.abs(got['self_err'][b] - ref['self_err'][b]).max() / 1.0)
    assert_padding(got, n_p, n_q)
    return dev


def check(eng, p, q, n_p, n_q, eps, iters, label):
    got = eng.cloud_divergence_f64(p, q, n_p, n_q, eps=eps, iters=iters, **KW)
    assert sorted(got) == sorted(('divergence', 'grad', 'col_err', 'self_err') + DUALS)
    assert all(got[k].dtype == np.float64 for k in got)
    ref = R.divergence64_wide(p, q, n_p, n_q, eps, iters)
    dev = deviations(got, ref, n_p, n_q)
    print('[divergence-f64] %s K=%d eps=%.1e: value %.2e, duals %.2e, gradient %.2e, col_err %.2e, self_err %.2e'
          % (label, iters, eps[0], dev['value'], dev['dual'], dev['grad'], dev['col'], dev['self']))
    for k in dev:
        assert dev[k] <= BOUND[k] < 1e-10, (label, iters, k, dev[k])
    return got


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('shape', SHAPES)
def test_against_the_float64_definition(eng, shape, B):
    p, q, n_p, n_q = wide_case(shape, B)
    for scale in EPS_SCALES:
        for iters in (1, K):
            check(eng, p, q, n_p, n_q, case_eps(n_p, n_q, scale), iters, '%s B=%d' % (shape, B))


def test_the_cap_once(eng):
    p, q, n_p, n_q = wide_case((1024, 1024, 1024, 1024), 1)
    got = check(eng, p, q, n_p, n_q, case_eps(n_p, n_q, 1.0), 2, '1024 x 1024')
    assert (np.abs(got['grad'][0]).max(axis=1) > 0).all()


def test_the_non_fp32_bits_of_p_reach_the_result(eng):
    """the same clouds with p rounded to fp32 give another value: every bit of p enters the costs"""
    p, q, n_p, n_q = wide_case((64, 64, 70, 66), 1)
    eps = case_eps(n_p, n_q, 0.01)
    a = eng.cloud_divergence_f64(p, q, n_p, n_q, eps=eps, iters=K, want_grad=True)
    b = eng.cloud_divergence_f64(p.astype(np.float32), q, n_p, n_q, eps=eps, iters=K, want_grad=True)
    ref_a, ref_b = (R.divergence64_wide(x, q, n_p, n_q, eps, K) for x in (p, p.astype(np.float32)))
    shift, ref_shift = a['divergence'][0] - b['divergence'][0], ref_a['divergence'][0] - ref_b['divergence'][0]
    print('[divergence-f64] 64 x 64, eps scale 0.01: value shift under fp32 rounding of p %.3e, reference %.3e' % (shift, ref_shift))
    assert shift != 0 and abs(shift - ref_shift) <= 1e-3 * abs(ref_shift) + 1e-10 * abs(ref_a['divergence'][0])


# ---- bits ------------------------------------------------------------------------------------------------------------------------
def test_same_bits_run_to_run_alone_or_in_a_batch_and_under_more_padding(eng):
    p, q, n_p, n_q = wide_case((257, 300, 260, 300), 3)
    eps = case_eps(n_p, n_q, 1.0)
    a = eng.cloud_divergence_f64(p, q, n_p, n_q, eps=eps, iters=K, **KW)
    b = eng.cloud_divergence_f64(p, q, n_p, n_q, eps=eps, iters=K, **KW)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    for s in range(3):
        one = eng.cloud_divergence_f64(p[s:s + 1], q[s:s + 1], n_p[s:s + 1], n_q[s:s + 1], eps=eps[s:s + 1], iters=K, **KW)
        for k in a:
            assert one[k][0].tobytes() == a[k][s].tobytes(), '%s of sample %d' % (k, s)
    N, M = p.shape[1], q.shape[1]
    wide_p, wide_q = np.full((3, N + 37, 3), 9.0, np.float64), np.full((3, M + 5, 3), -9.0, np.float32)
    wide_p[:, :N], wide_q[:, :M] = p, q
    w = eng.cloud_divergence_f64(wide_p, wide_q, n_p, n_q, eps=eps, iters=K, **KW)
    for k in ('divergence', 'col_err', 'self_err'):
        assert w[k].tobytes() == a[k].tobytes(), k
    for s in range(3):
        n, m = int(n_p[s]), int(n_q[s])
        assert w['grad'][s, :n].tobytes() == a['grad'][s, :n].tobytes()
        for k, real in (('f', n), ('g', m), ('h_p', n), ('h_q', m)):
            assert w[k][s, :real].tobytes() == a[k][s, :real].tobytes(), k
    assert_padding(w, n_p, n_q)
    # the outputs are optional -- asked for or not, the value's bits are the same -- and a single pair may come without the batch axis
    t = eng.cloud_divergence_f64(p[0, :n_p[0]], q[0, :n_q[0]], eps=eps[0], iters=K)
    assert sorted(t) == ['divergence'] and t['divergence'][0] == a['divergence'][0]


def test_it_leaves_the_fp32_call_and_the_dispatch_marks_alone(eng):
    p, q, n_p, n_q = U.chamfer_case((5, 3, 8, 8), 1, seed=0)
    before = eng.cloud_divergence(p, q, n_p, n_q, eps=4e-4, iters=7, **KW)
    eng.dispatch_reset()
    marks = eng.last_dispatch()
    eng.cloud_divergence_f64(p, q, n_p, n_q, eps=4e-4, iters=7, **KW)
    assert eng.last_dispatch() == marks
    after = eng.cloud_divergence(p, q, n_p, n_q, eps=4e-4, iters=7, **KW)
    for k in before:
        assert before[k].tobytes() == after[k].tobytes(), k


def test_refusals_leave_the_context_usable(eng):
    p, q, n_p, n_q = wide_case((5, 3, 8, 8), 1)
    lib, h = eng.lib, eng.h
    terms = np.zeros((1,))
    eps = np.array([4e-4])
    good = eng.cloud_divergence_f64(p, q, n_p, n_q, eps=eps, iters=7, **KW)

    def call(p_, np_, q_, nq_, B, N, M, eps_, iters, t_):
        f = lambda a, T_: None if a is None else a.ctypes.data_as(T_)
        return lib.drp_cloud_divergence_f64(h, f(p_, DP), f(np_, I32P), f(q_, FP), f(nq_, I32P), B, N, M, f(eps_, DP), iters, f(t_, DP),
                                            None, None, None, None)
    assert call(p, n_p, q, n_q, 1, 8, 8, eps, 7, terms) == 0 and terms[0] == good['divergence'][0]
    big_p, big_q = np.zeros((1, 1025, 3), np.float64), np.zeros((1, 1025, 3), np.float32)
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
                 (p, n_p, big_q, n_q, 1, 8, 1025, eps, 7, terms), (big_p, n_p, q, n_q, 1, 1025, 8, eps, 7, terms),  # more than 1024 points
                 (p, i32(0), q, n_q, 1, 8, 8, eps, 7, terms), (p, i32(9), q, n_q, 1, 8, 8, eps, 7, terms),
                 (p, n_p, q, i32(0), 1, 8, 8, eps, 7, terms), (p, n_p, q, i32(9), 1, 8, 8, eps, 7, terms),
                 (p, n_p, q, n_q, 1, 8, 8, e64(0.0), 7, terms), (p, n_p, q, n_q, 1, 8, 8, e64(-4e-4), 7, terms),
                 (p, n_p, q, n_q, 1, 8, 8, e64(np.inf), 7, terms), (p, n_p, q, n_q, 1, 8, 8, e64(np.nan), 7, terms),
                 (p, n_p, q, n_q, 1, 8, 8, eps, 0, terms), (p, n_p, q, n_q, 1, 8, 8, eps, -1, terms),
                 (p, n_p, q, n_q, 1, 8, 8, eps, TRANSPORT_MAX_ITERS + 1, terms),
                 (nan_p, n_p, q, n_q, 1, 8, 8, eps, 7, terms), (p, n_p, inf_q, n_q, 1, 8, 8, eps, 7, terms)):
        assert call(*args) == -1, args[4:9]                          # DRP_EINVAL
        again = eng.cloud_divergence_f64(p, q, n_p, n_q, eps=eps, iters=7, **KW)    # the context answers with its earlier bits
        for k in good:
            assert again[k].tobytes() == good[k].tobytes(), (args[4:9], k)
    with pytest.raises(DrpError, match='1025'):
        eng.cloud_divergence_f64(big_p, q, [5], [3], eps=4e-4, iters=7)
    for kw in ({}, {'eps': 4e-4}, {'iters': 7}):                     # both are required
        with pytest.raises(ValueError):
            eng.cloud_divergence_f64(p, q, n_p, n_q, **kw)
    nan_pad = p.copy()
    nan_pad[0, 6] = np.nan                                           # padding is never read as points
    b = eng.cloud_divergence_f64(nan_pad, q, n_p, n_q, eps=eps, iters=7, **KW)
    for k in good:
        assert b[k].tobytes() == good[k].tobytes(), k

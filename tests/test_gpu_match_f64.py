"""GPU: the float64 assignment kernel (drp_cloud_match_f64: ka64_match of csrc/k_match_f64.h) against match64(exact32=False) of
tests/_match_ref.py, on double inputs whose low bits are random (tests/_match_f64_ref.py: wide_case).

Partners are compared everywhere: tests/test_match_f64_host.py holds every case's uniqueness margin above 1e-9, 10^5 times the
solver's rounding.  Term, gradient and duals: relative to the largest entry of the compared array, against bounds pinned at 5 x
the error MEASURED on one MI355X (the figures are the `[match-f64]` lines and DESIGN.md 2), every one below 1e-10, the project's
practice for its float64 kernels:
      term, cost   measured 6.1e-16 (257 x 300; the two sides sum the pairs in different orders)   bound TERM_TOL = 3.1e-15
      grad         measured 2.1e-16 (5 x 3: one rounding of 2 d / (3 r) against 2 d scale / (3 r))    bound GRAD_TOL = 1.1e-15
      duals        measured 0 on all 18 cases: every operation of the solver is one IEEE double operation in the reference's
                   order, so the device's duals are the reference's bits                             bound DUAL_TOL = 0: equality
At the cap (1024 x 1024, 17 x 1023, 1024 x 1) there is no O(n^3) numpy solve: the duals' certificate alone, to r 2^-52 max C;
term and gradient there against term_and_grad on the device's own pairs, the term to r 2^-53 (its r - 1 additions in ascending
row, one rounding each of at most the total; measured 1.3e-15 at r = 1024).
Every figure is printed before it is asserted."""
import ctypes

import numpy as np
import pytest

import _match_f64_ref as F
import _match_ref as R
from dyn_res_pile_manip_amd.engine import Engine

pytestmark = pytest.mark.gpu
TERM_TOL = 3.1e-15
GRAD_TOL = 1.1e-15
DUAL_TOL = 0.0
FP, IP, DP = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)


@pytest.fixture(scope='module')
def eng():
    e = Engine(0)                       # a one-shot: no weights
    yield e
    e.close()


def full(e, p, q, n_p, n_q, **kw):
    return e.cloud_match_f64(p, q, n_p, n_q, want_grad=True, want_match=True, want_dual=True, **kw)


KEYS = ('match', 'cost', 'opt_cost', 'grad', 'match_pq', 'match_qp', 'u', 'v')


def same_bits(a, b, keys=KEYS):
    for k in keys:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
        assert not (np.signbit(a[k]) != np.signbit(b[k])).any(), k


def rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


# ---- 1. against the numpy definition ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B', F.BATCHES)
@pytest.mark.parametrize('shape', F.SHAPES)
def test_against_the_float64_definition(eng, shape, B):
    p, q, n_p, n_q = F.wide_case(shape, B)
    ref = F.one_shot_reference(shape, B)
    out = full(eng, p, q, n_p, n_q)
    assert out['grad'].dtype == np.float64 and out['match'].dtype == np.float64
    np.testing.assert_array_equal(out['r'], np.minimum(n_p, n_q))
    np.testing.assert_array_equal(out['match_pq'], ref['match_pq'])         # everywhere: no case is excluded
    np.testing.assert_array_equal(out['match_qp'], ref['match_qp'])
    np.testing.assert_array_equal(out['cost'], out['opt_cost'])            # no match_in: the same pairs, the same sum
    figures = {'term': rel(out['match'], ref['match']), 'cost': rel(out['cost'], ref['cost']), 'grad': rel(out['grad'], ref['grad']),
               'dual': max(np.abs(out['u'] - ref['u']).max(), np.abs(out['v'] - ref['v']).max())
               / max(np.abs(ref['u']).max(), np.abs(ref['v']).max(), 1e-300)}
    print('[match-f64] %s B=%d: term %.3e cost %.3e grad %.3e duals %.3e' % (shape, B, figures['term'], figures['cost'],
                                                                           figures['grad'], figures['dual']))
    assert figures['term'] <= TERM_TOL and figures['cost'] <= TERM_TOL and figures['grad'] <= GRAD_TOL and figures['dual'] <= DUAL_TOL
    for b in range(B):                                                      # unmatched rows and padding: +0.0 exactly, no partner, no dual
        off = np.ones(p.shape[1], bool)
        off[:n_p[b]] = ref['match_pq'][b, :n_p[b]] < 0
        assert (out['grad'][b, off] == 0).all() and not np.signbit(out['grad'][b, off]).any()
        assert (out['match_pq'][b, n_p[b]:] == -1).all() and (out['match_qp'][b, n_q[b]:] == -1).all()
        assert (out['u'][b, n_p[b]:] == 0).all() and (out['v'][b, n_q[b]:] == 0).all()
        free = out['match_qp'][b, :n_q[b]] < 0                              # the larger cloud's unmatched rows: dual 0
        assert (out['v'][b, :n_q[b]][free] == 0).all()
        assert (out['u'][b, :n_p[b]][out['match_pq'][b, :n_p[b]] < 0] == 0).all()
    short = eng.cloud_match_f64(p, q, n_p, n_q)                             # every output but the terms is optional
    assert sorted(short) == ['cost', 'match', 'opt_cost', 'r']
    np.testing.assert_array_equal(short['match'], out['match'])


# ---- 2. at the cap: the duals' certificate ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', F.BIG_SHAPES)
def test_the_duals_certify_the_optimum_at_the_cap(eng, shape):
    p, q, n_p, n_q = F.wide_case(shape, 1)
    out = full(eng, p, q, n_p, n_q)
    n, m = int(n_p[0]), int(n_q[0])
    c = F.certificate(p[0], q[0], n, m, out['u'][0], out['v'][0], out['match_pq'][0], out['opt_cost'][0])
    bound = c['r'] * 2.0 ** -52
    print('[match-f64] %d x %d: slack %.2e tight %.2e sum %.2e cost %.2e of max C (bound r 2^-52 = %.2e)'
          % (n, m, c['slack'], c['tight'], c['sum'], c['cost'], bound))
    assert c['slack'] <= bound and c['tight'] <= bound and c['sum'] <= bound and c['cost'] <= bound
    inv = out['match_qp'][0]
    on = np.nonzero(out['match_pq'][0] >= 0)[0]
    np.testing.assert_array_equal(inv[out['match_pq'][0][on]], on)          # the two partner arrays are one matching
    assert (inv >= 0).sum() == c['r']
    term, grad = R.term_and_grad(p[0, :n], q[0, :m], out['match_pq'][0, :n].astype(np.int64))
    print('[match-f64] %d x %d: term %.3e grad %.3e of term_and_grad on the same pairs' % (n, m, abs(out['match'][0] - term) / term,
                                                                                         np.abs(out['grad'][0, :n] - grad).max() / np.abs(grad).max()))
    assert abs(out['match'][0] - term) <= max(TERM_TOL, c['r'] * 2.0 ** -53) * term
    assert np.abs(out['grad'][0, :n] - grad).max() <= GRAD_TOL * np.abs(grad).max()


# ---- 3. the tie rule ----------------------------------------------------------------------------------------------------------------
def test_ties_go_to_the_lowest_column(eng):
    p, q, n_p, n_q = F.grid_case()
    ref = R.match64(p, q, n_p, n_q, exact32=False, want_margin=False)
    out = full(eng, p, q, n_p, n_q)
    np.testing.assert_array_equal(out['match_pq'], ref['match_pq'])
    np.testing.assert_array_equal(out['match_qp'], ref['match_qp'])
    np.testing.assert_array_equal(out['u'], ref['u'])                       # exact arithmetic: the duals too
    np.testing.assert_array_equal(out['v'], ref['v'])
    np.testing.assert_array_equal(out['opt_cost'], ref['cost'])


# ---- 4. a matching given by the caller ----------------------------------------------------------------------------------------------
def test_match_in(eng):
    shape = (70, 130, 70, 130)
    p, q, n_p, n_q = F.wide_case(shape, 3)
    ref = F.one_shot_reference(shape, 3)
    own = full(eng, p, q, n_p, n_q)
    fed = full(eng, p, q, n_p, n_q, match_in=ref['match_pq'])
    same_bits(own, fed)                                                     # the optimum fed back: the bits of match_in=None
    swapped = ref['match_pq'].copy().astype(np.int32)
    swapped[:, [0, 1]] = swapped[:, [1, 0]]                                 # valid, and not the optimum (rows 0 and 1 are matched)
    assert (swapped[:, :2] >= 0).all()
    out = full(eng, p, q, n_p, n_q, match_in=swapped)
    print('[match-f64] match_in, two partners swapped: cost - opt_cost %s' % (out['cost'] - out['opt_cost'],))
    assert (out['cost'] > out['opt_cost']).all()
    same_bits(own, out, ('opt_cost', 'match_pq', 'match_qp', 'u', 'v'))    # the solver's own optimum all the same
    for b in range(3):
        n, m = int(n_p[b]), int(n_q[b])
        term, grad = R.term_and_grad(p[b, :n], q[b, :m], swapped[b, :n].astype(np.int64))
        assert abs(out['match'][b] - term) <= TERM_TOL * term
        assert np.abs(out['grad'][b, :n] - grad).max() <= GRAD_TOL * np.abs(grad).max()
        assert (out['grad'][b, n:] == 0).all()
        assert abs(out['cost'][b] - term * 3 * min(n, m)) <= 4 * TERM_TOL * out['cost'][b]


# ---- 5. one value, one order ---------------------------------------------------------------------------------------------------------
def test_same_bits_alone_in_a_batch_and_under_padding(eng):
    shape = (70, 130, 70, 130)
    p, q, n_p, n_q = F.wide_case(shape, 3)
    whole, again = full(eng, p, q, n_p, n_q), full(eng, p, q, n_p, n_q)
    same_bits(whole, again)
    for b in range(3):
        alone = full(eng, p[b:b + 1], q[b:b + 1], n_p[b:b + 1], n_q[b:b + 1])
        for k in KEYS:
            np.testing.assert_array_equal(alone[k][0], whole[k][b], err_msg='%s of sample %d' % (k, b))
    # larger N and M (a different LDS layout and launch size), rubbish in the new padding
    N2, M2 = 200, 257
    p2 = np.full((3, N2, 3), 7.5)
    q2 = np.full((3, M2, 3), -3.25, np.float32)
    p2[:, :70], q2[:, :130] = p, q
    wide = full(eng, p2, q2, n_p, n_q)
    for k in ('match', 'cost', 'opt_cost'):
        np.testing.assert_array_equal(wide[k], whole[k])
    for k, n in (('grad', 70), ('match_pq', 70), ('u', 70), ('match_qp', 130), ('v', 130)):
        np.testing.assert_array_equal(wide[k][:, :n], whole[k], err_msg=k)
    assert (wide['grad'][:, 70:] == 0).all() and (wide['match_pq'][:, 70:] == -1).all() and (wide['v'][:, 130:] == 0).all()


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(eng):
    p, q, n_p, n_q = F.wide_case((5, 3, 8, 8), 3)
    p, q = np.ascontiguousarray(p), np.ascontiguousarray(q)
    B, N, M = 3, 8, 8
    good = full(eng, p, q, n_p, n_q)
    terms = np.empty(B)
    valid = np.ascontiguousarray(good['match_pq'], dtype=np.int32)

    def call(p_=p, n_p_=n_p, q_=q, n_q_=n_q, N_=N, M_=M, match_=None, terms_=terms):
        f = lambda a, T: None if a is None else np.ascontiguousarray(a).ctypes.data_as(T)
        return eng.lib.drp_cloud_match_f64(eng.h, f(p_, DP), f(n_p_, IP), f(q_, FP), f(n_q_, IP), B, N_, M_, f(match_, IP), f(terms_, DP),
                                           None, None, None, None, None)
    assert call() == 0 and call(match_=valid) == 0
    nan_p, inf_q = p.copy(), q.copy()
    nan_p[1, 0, 2] = np.nan
    inf_q[2, 0, 0] = np.inf
    pad_nan = p.copy()
    pad_nan[0, n_p[0]:] = np.nan                                            # rubbish in the padding is allowed
    assert call(p_=pad_nan) == 0
    dup, far, few, pad, neg = (valid.copy() for _ in range(5))
    on0 = np.nonzero(valid[0, :n_p[0]] >= 0)[0]
    dup[0, on0[1]] = dup[0, on0[0]]
    far[1, np.nonzero(valid[1] >= 0)[0][0]] = n_q[1]
    few[0, on0[0]] = -1
    pad[1, N - 1] = 0
    neg[0, 0] = -2
    assert n_p[1] < N
    refused = [('null p', dict(p_=None)), ('null q', dict(q_=None)), ('null n_p', dict(n_p_=None)), ('null n_q', dict(n_q_=None)),
               ('null terms', dict(terms_=None)), ('N = 1025', dict(N_=1025)), ('M = 1025', dict(M_=1025)), ('M = 0', dict(M_=0)),
               ('a count of 0', dict(n_p_=np.array([5, 0, 1], np.int32))), ('a count above M', dict(n_q_=np.array([3, 9, 1], np.int32))),
               ('a row of p that is no number', dict(p_=nan_p)), ('an infinite row of q', dict(q_=inf_q)),
               ('match_in: a duplicate partner', dict(match_=dup)), ('match_in: a partner out of range', dict(match_=far)),
               ('match_in: too few pairs', dict(match_=few)), ('match_in: a partner on padding', dict(match_=pad)),
               ('match_in: below -1', dict(match_=neg))]
    for label, kw in refused:
        rc = call(**kw)
        msg = eng.lib.drp_last_error(eng.h).decode()
        print('[match-f64] refusal, %s: %d (%s)' % (label, rc, msg))
        assert rc == -1, label                                              # DRP_EINVAL
        if label.startswith('match_in'):
            assert 'sample' in msg and 'step' in msg and 'row' in msg
        same_bits(full(eng, p, q, n_p, n_q), good)                          # the context is usable, the result what it was

"""GPU: the stand-alone Chamfer metric in float64 (drp_cloud_chamfer_f64, csrc/k_chamfer_f64.h) against chamfer64 of
tests/_untracked_ref.py on the same fp32 inputs, and against the fp32 metric it is the yardstick of.

Bounds.  Both sides compute a squared distance as dx*dx + dy*dy + dz*dz in double from the same widened inputs, so the arg-mins
are equal exactly -- with or without a margin -- and each margin agrees within 1e-15 absolute (squared distances are about 4e-4:
an ulp is 5e-20); fwd and bwd differ in summation order only, rtol 1e-12; the gradient within 1e-12 of its largest entry.
Padding: exactly 0 / -1.  Against the fp32 metric: the bound of tests/test_gpu_chamfer.py, 1e-6, on cases whose margins
tests/test_untracked_host.py and tests/test_chamfer_f64_host.py hold above 1e-7.  Every figure is printed before it is asserted."""
import ctypes

import numpy as np
import pytest

import _chamfer_f64_cases as C
import _untracked_ref as U
from dyn_res_pile_manip_amd import synthetic as syn, weights
from dyn_res_pile_manip_amd._lib import DrpError
from dyn_res_pile_manip_amd.engine import Engine

pytestmark = pytest.mark.gpu
RTOL = 1e-12
MARGIN_ATOL = 1e-15
REL32 = 1e-6                    # tests/test_gpu_chamfer.py
I32P = ctypes.POINTER(ctypes.c_int32)
FP = ctypes.POINTER(ctypes.c_float)
DP = ctypes.POINTER(ctypes.c_double)


@pytest.fixture(scope='module')
def eng():
    e = Engine(0)                       # no weights: the metric needs none
    yield e
    e.close()


def ref_margin(ref):
    """[B, 2]: the smallest margin of the real rows, p -> q and q -> p (padding holds inf)"""
    return np.stack([ref['margin_pq'].min(axis=1), ref['margin_qp'].min(axis=1)], 1)


def margin_err(got, want):
    """largest absolute difference; inf must sit where inf sits"""
    inf = np.isinf(want)
    assert (np.isinf(got) == inf).all() and (got[inf] > 0).all(), (got, want)
    return float(np.abs(got[~inf] - want[~inf]).max()) if (~inf).any() else 0.0


def check(eng, p, q, n_p, n_q, label):
    ref = U.chamfer64(p, q, n_p, n_q)
    got = eng.cloud_chamfer_f64(p, q, n_p, n_q, want_grad=True, want_nn=True)
    assert got['grad'].dtype == np.float64 and got['fwd'].dtype == np.float64 and got['margin'].shape == (p.shape[0], 2)
    ef = float((np.abs(got['fwd'] - ref['fwd']) / ref['fwd']).max())
    eb = float((np.abs(got['bwd'] - ref['bwd']) / ref['bwd']).max())
    eg = float(np.abs(got['grad'] - ref['grad']).max() / np.abs(ref['grad']).max())
    want_m = ref_margin(ref)
    same_nn = bool((got['nn_pq'] == ref['nn_pq']).all() and (got['nn_qp'] == ref['nn_qp']).all())
    print('[chamfer-f64] %s: fwd %.2e bwd %.2e rel, gradient %.2e of the largest entry, arg-mins equal %s, margins %s (reference %s)'
          % (label, ef, eb, eg, same_nn, got['margin'].min(axis=0), want_m.min(axis=0)))
    np.testing.assert_array_equal(got['nn_pq'], ref['nn_pq'])
    np.testing.assert_array_equal(got['nn_qp'], ref['nn_qp'])
    assert ef <= RTOL and eb <= RTOL and eg <= RTOL
    em = margin_err(got['margin'], want_m)
    print('[chamfer-f64] %s: margins off by %.2e' % (label, em))
    assert em <= MARGIN_ATOL
    np.testing.assert_array_equal(got['total'], got['fwd'] + got['bwd'])
    for b in range(p.shape[0]):
        pad = got['grad'][b, n_p[b]:]
        assert (pad == 0).all() and not np.signbit(pad).any()       # exactly +0.0
    return got, ref


# ---- 1. parity ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,B', U.chamfer_cases())
def test_against_chamfer64(eng, shape, B):
    p, q, n_p, n_q = U.chamfer_case(shape, B)
    check(eng, p, q, n_p, n_q, '%s B=%d' % (shape, B))


# ---- 2. the tiling ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', C.TILING_SHAPES)
def test_around_the_tile_and_chunk_boundaries(eng, shape):
    p, q, n_p, n_q = C.tiling_case(shape)
    got, ref = check(eng, p, q, n_p, n_q, '%d x %d' % shape)
    cr = C.crossings({'nn_pq': got['nn_pq'], 'nn_qp': got['nn_qp']}, shape)
    print('[chamfer-f64] %d x %d: crossings (has, crossed) %s' % (shape + (cr,)))
    for has, crossed in cr.values():                # some arg-min of the DEVICE lies in a later tile / a later 256-row chunk
        assert crossed or not has
    assert float(got['margin'].min()) > U.MARGIN_MIN


# ---- 3. ties and degenerate margins ----------------------------------------------------------------------------------------
def test_ties_take_the_lowest_index_and_give_margin_zero(eng):
    q = np.tile(np.array([[0.2, 0.3, 0.5]], np.float32), (6, 1))[None]
    p = np.array([[0.21, 0.3, 0.5], [0.4, 0.1, 0.5], [0.4, 0.1, 0.5], [9.0, 9.0, 9.0]], np.float32)[None]
    got = eng.cloud_chamfer_f64(p, q, [3], [6], want_nn=True)
    print('[chamfer-f64] six identical targets: nn_pq %s nn_qp %s margin %s' % (got['nn_pq'][0], got['nn_qp'][0], got['margin'][0]))
    np.testing.assert_array_equal(got['nn_pq'][0], [0, 0, 0, -1])
    np.testing.assert_array_equal(got['nn_qp'][0], [0] * 6)
    assert got['margin'][0, 0] == 0.0 and not np.signbit(got['margin'][0, 0])      # a duplicate of the winner: 0 exactly
    ref = U.chamfer64(p, q, [3], [6])
    assert margin_err(got['margin'], ref_margin(ref)) <= MARGIN_ATOL
    # a one-row other cloud: nothing else to lose to
    got = eng.cloud_chamfer_f64(p, q, [3], [1], want_nn=True)
    print('[chamfer-f64] one target row: margin %s' % (got['margin'][0],))
    assert got['margin'][0, 0] == np.inf and np.isfinite(got['margin'][0, 1])
    np.testing.assert_array_equal(got['nn_pq'][0], [0, 0, 0, -1])
    got = eng.cloud_chamfer_f64(p, q, [1], [6], want_nn=True)
    assert got['margin'][0, 1] == np.inf and got['margin'][0, 0] == 0.0
    q2 = np.array([[0.4, 0.1, 0.51], [7.0, 7.0, 7.0]], np.float32)[None]      # equally far from the coincident rows 1 and 2
    got = eng.cloud_chamfer_f64(p, q2, [3], [1], want_nn=True)
    np.testing.assert_array_equal(got['nn_qp'][0], [1, -1])
    assert got['margin'][0, 1] == 0.0


# ---- 4. one value, one order ------------------------------------------------------------------------------------------------
def test_same_bits_run_to_run_and_alone_or_in_a_batch(eng):
    p, q, n_p, n_q = U.chamfer_case((300, 257, 300, 300), 3)
    a = eng.cloud_chamfer_f64(p, q, n_p, n_q, want_grad=True, want_nn=True)
    b = eng.cloud_chamfer_f64(p, q, n_p, n_q, want_grad=True, want_nn=True)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])
    for s in range(3):
        one = eng.cloud_chamfer_f64(p[s:s + 1], q[s:s + 1], n_p[s:s + 1], n_q[s:s + 1], want_grad=True, want_nn=True)
        for k in a:
            np.testing.assert_array_equal(one[k][0], a[k][s], err_msg='%s of sample %d' % (k, s))
    # the outputs are optional, and a single pair may come without the batch axis
    t = eng.cloud_chamfer_f64(p[0, :n_p[0]], q[0, :n_q[0]])
    assert sorted(t) == ['bwd', 'fwd', 'margin', 'total'] and t['fwd'][0] == a['fwd'][0] and t['bwd'][0] == a['bwd'][0]
    np.testing.assert_array_equal(t['margin'][0], a['margin'][0])


# ---- 5. the fp32 metric against its yardstick ---------------------------------------------------------------------------------
def fp32_cases():
    return [('%s B=%d' % (shape, B), lambda shape=shape, B=B: U.chamfer_case(shape, B)) for shape, B in U.chamfer_cases()] + \
           [('258 x 1030', C.boundary_case)]


@pytest.mark.parametrize('label,make', fp32_cases(), ids=[c[0] for c in fp32_cases()])
def test_the_fp32_metric_against_float64(eng, label, make):
    p, q, n_p, n_q = make()
    g64 = eng.cloud_chamfer_f64(p, q, n_p, n_q, want_nn=True)
    g32 = eng.cloud_chamfer(p, q, n_p, n_q, want_nn=True)
    ef = float((np.abs(g32['fwd'] - g64['fwd']) / g64['fwd']).max())
    eb = float((np.abs(g32['bwd'] - g64['bwd']) / g64['bwd']).max())
    print('[chamfer-f64] fp32 against float64, %s: fwd %.2e bwd %.2e rel, smallest float64 margin %.3e'
          % (label, ef, eb, g64['margin'].min()))
    np.testing.assert_array_equal(g32['nn_pq'], g64['nn_pq'])
    np.testing.assert_array_equal(g32['nn_qp'], g64['nn_qp'])
    assert ef <= REL32 and eb <= REL32


# ---- 6. refusals --------------------------------------------------------------------------------------------------------
def test_refusals(eng):
    p, q, n_p, n_q = U.chamfer_case((5, 3, 8, 8), 1)
    lib, h = eng.lib, eng.h
    terms = np.zeros((1, 2))

    def call(p_, np_, q_, nq_, B, N, M, t_):
        f = lambda a, T: None if a is None else a.ctypes.data_as(T)
        return lib.drp_cloud_chamfer_f64(h, f(p_, FP), f(np_, I32P), f(q_, FP), f(nq_, I32P), B, N, M, f(t_, DP), None, None, None, None)
    assert call(p, n_p, q, n_q, 1, 8, 8, terms) == 0
    want = eng.cloud_chamfer_f64(p, q, n_p, n_q, want_grad=True, want_nn=True)
    for args in ((None, n_p, q, n_q, 1, 8, 8, terms), (p, None, q, n_q, 1, 8, 8, terms), (p, n_p, None, n_q, 1, 8, 8, terms),
                 (p, n_p, q, None, 1, 8, 8, terms), (p, n_p, q, n_q, 1, 8, 8, None),
                 (p, n_p, q, n_q, 1, 8, 0, terms), (p, n_p, q, n_q, 1, 8, 4097, terms), (p, n_p, q, n_q, 1, 4097, 8, terms),
                 (p, n_p, q, n_q, 0, 8, 8, terms),
                 (p, np.array([0], np.int32), q, n_q, 1, 8, 8, terms), (p, np.array([9], np.int32), q, n_q, 1, 8, 8, terms),
                 (p, n_p, q, np.array([0], np.int32), 1, 8, 8, terms), (p, n_p, q, np.array([9], np.int32), 1, 8, 8, terms)):
        assert call(*args) == -1, args[4:7]                          # DRP_EINVAL
        got = eng.cloud_chamfer_f64(p, q, n_p, n_q, want_grad=True, want_nn=True)     # the next call works
        for k in want:
            np.testing.assert_array_equal(got[k], want[k])
    with pytest.raises(DrpError):
        eng.cloud_chamfer_f64(p, q, [0], [3])
    assert lib.drp_cloud_chamfer_f64(None, None, None, None, None, 1, 8, 8, None, None, None, None, None) == -1


# ---- 7. isolation -------------------------------------------------------------------------------------------------------
def test_a_gd_session_the_dispatch_marks_and_the_trainer_survive_a_call(golden):
    """drp_cloud_chamfer_f64 ends no session and leaves the marks and the trainer's state alone: a GD session stepped with calls
    in between gives the bits of an undisturbed one, last_dispatch() is what it was, and an Adam trajectory with calls in between
    is the undisturbed one"""
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
            e.cloud_chamfer_f64(p, q, n_p, n_q, want_grad=True)
            assert e.last_dispatch() == marks
        out.append(e.gd_step())
        if disturb:
            e.cloud_chamfer_f64(p, q, n_p, n_q)
        out.append(e.gd_actions())
        # the trainer: three updates, a call before each
        batch = U.untracked_batch(golden, 'b2_r5')
        e.train_begin(batch[0].shape[1] - 1, 1e-3, 0.9)
        for _ in range(3):
            if disturb:
                e.cloud_chamfer_f64(p, q, n_p, n_q, want_nn=True)
            loss, grad = e.train_step_untracked(*batch, mode='update', want_grad=True)
            out += [np.float64(loss), grad, e.get_weights()]
        runs.append(out)
        e.close()
    assert len(runs[0]) == len(runs[1])
    for a, b in zip(runs[0], runs[1]):
        for x, y in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
            np.testing.assert_array_equal(np.asarray(x), np.asarray(y))

"""GPU: the stand-alone Chamfer metric (drp_cloud_chamfer, csrc/k_chamfer.h) through ctypes against chamfer64 of
tests/_untracked_ref.py on the same fp32 inputs.

Bounds.  Arg-min indices: equal exactly (tests/test_untracked_host.py holds every margin of these cases above 1e-7, three orders
above the fp32 rounding of a squared distance).  fwd and bwd: 1e-6 relative -- at most four fp32 roundings of 2^-24 per squared
distance is 2.4e-7, the sum is in double; a margin of 4x.  Gradient: elementwise within 1e-6 of the largest entry.  Padded rows:
exactly 0.  The kernel has one path for every size (tiles of 1024 points), so there is no threshold to straddle; one larger case
crosses the tile and the 256-row chunk boundaries.  Every figure is printed before it is asserted."""
import ctypes

import numpy as np
import pytest

import _untracked_ref as U
from dyn_res_pile_manip_amd import synthetic as syn, weights
from dyn_res_pile_manip_amd._lib import DrpError
from dyn_res_pile_manip_amd.engine import Engine

pytestmark = pytest.mark.gpu
REL = 1e-6
I32P = ctypes.POINTER(ctypes.c_int32)
FP = ctypes.POINTER(ctypes.c_float)
DP = ctypes.POINTER(ctypes.c_double)


@pytest.fixture(scope='module')
def eng():
    e = Engine(0)                       # no weights: the metric needs none
    yield e
    e.close()


def check(eng, p, q, n_p, n_q, label):
    ref = U.chamfer64(p, q, n_p, n_q)
    got = eng.cloud_chamfer(p, q, n_p, n_q, want_grad=True, want_nn=True)
    np.testing.assert_array_equal(got['nn_pq'], ref['nn_pq'])
    np.testing.assert_array_equal(got['nn_qp'], ref['nn_qp'])
    ef = float((np.abs(got['fwd'] - ref['fwd']) / ref['fwd']).max())
    eb = float((np.abs(got['bwd'] - ref['bwd']) / ref['bwd']).max())
    eg = float(np.abs(got['grad'] - ref['grad']).max() / np.abs(ref['grad']).max())
    print('[chamfer] %s: fwd %.2e bwd %.2e rel, gradient %.2e of the largest entry' % (label, ef, eb, eg))
    assert ef <= REL and eb <= REL and eg <= REL
    np.testing.assert_array_equal(got['total'], got['fwd'] + got['bwd'])
    for b in range(p.shape[0]):
        assert (got['grad'][b, n_p[b]:] == 0).all()                 # exactly
    assert got['grad'].dtype == np.float32 and got['fwd'].dtype == np.float64
    return got


@pytest.mark.parametrize('shape,B', U.chamfer_cases())
def test_against_float64(eng, shape, B):
    p, q, n_p, n_q = U.chamfer_case(shape, B)
    check(eng, p, q, n_p, n_q, '%s B=%d' % (shape, B))


def test_across_the_tile_and_chunk_boundaries(eng):
    """n_q = 1030 > the 1024-point tile, n_p = 258 > one 256-row chunk: the arg-min of a row may sit in the second tile.  Clouds on
    jittered lattices of different pitch, so that every margin is far above 1e-7 (asserted here on the reference)."""
    rng = np.random.default_rng(5)
    def lattice(n, pitch, off):
        k = int(np.ceil(n ** (1.0 / 3.0)))
        g = np.stack(np.meshgrid(*[np.arange(k)] * 3, indexing='ij'), -1).reshape(-1, 3)[rng.permutation(k ** 3)[:n]]
        return (0.1 + off + pitch * g + 0.2 * pitch * rng.random((n, 3))).astype(np.float32)
    p, q = lattice(258, 0.031, 0.0)[None], lattice(1030, 0.02, 0.003)[None]
    ref = U.chamfer64(p, q, [258], [1030])
    assert U.min_margin(ref) > U.MARGIN_MIN
    assert (ref['nn_pq'] >= 1024).any() and (ref['nn_qp'] >= 256).any()
    check(eng, p, q, np.array([258], np.int32), np.array([1030], np.int32), '258 x 1030')


def test_ties_take_the_lowest_index(eng):
    """the deliberate exception to the margin rule: exact duplicates"""
    q = np.tile(np.array([[0.2, 0.3, 0.5]], np.float32), (6, 1))[None]
    p = np.array([[0.21, 0.3, 0.5], [0.4, 0.1, 0.5], [0.4, 0.1, 0.5], [9.0, 9.0, 9.0]], np.float32)[None]
    got = eng.cloud_chamfer(p, q, [3], [6], want_nn=True)
    np.testing.assert_array_equal(got['nn_pq'][0], [0, 0, 0, -1])
    np.testing.assert_array_equal(got['nn_qp'][0], [0] * 6)
    q2 = np.array([[0.4, 0.1, 0.51], [7.0, 7.0, 7.0]], np.float32)[None]      # equally far from the coincident rows 1 and 2
    got = eng.cloud_chamfer(p, q2, [3], [1], want_nn=True)
    np.testing.assert_array_equal(got['nn_qp'][0], [1, -1])


def test_same_bits_run_to_run_and_alone_or_in_a_batch(eng):
    p, q, n_p, n_q = U.chamfer_case((300, 257, 300, 300), 3)
    a = eng.cloud_chamfer(p, q, n_p, n_q, want_grad=True, want_nn=True)
    b = eng.cloud_chamfer(p, q, n_p, n_q, want_grad=True, want_nn=True)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])
    for s in range(3):
        one = eng.cloud_chamfer(p[s:s + 1], q[s:s + 1], n_p[s:s + 1], n_q[s:s + 1], want_grad=True, want_nn=True)
        for k in a:
            np.testing.assert_array_equal(one[k][0], a[k][s], err_msg='%s of sample %d' % (k, s))
    # the outputs are optional, and a single pair may come without the batch axis
    t = eng.cloud_chamfer(p[0, :n_p[0]], q[0, :n_q[0]])
    assert sorted(t) == ['bwd', 'fwd', 'total'] and t['fwd'][0] == a['fwd'][0] and t['bwd'][0] == a['bwd'][0]


def test_refusals(eng):
    p, q, n_p, n_q = U.chamfer_case((5, 3, 8, 8), 1)
    lib, h = eng.lib, eng.h
    terms = np.zeros((1, 2))
    def call(p_, np_, q_, nq_, B, N, M, t_):
        f = lambda a, T: None if a is None else a.ctypes.data_as(T)
        return lib.drp_cloud_chamfer(h, f(p_, FP), f(np_, I32P), f(q_, FP), f(nq_, I32P), B, N, M, f(t_, DP), None, None, None)
    assert call(p, n_p, q, n_q, 1, 8, 8, terms) == 0
    for args in ((None, n_p, q, n_q, 1, 8, 8, terms), (p, None, q, n_q, 1, 8, 8, terms), (p, n_p, None, n_q, 1, 8, 8, terms),
                 (p, n_p, q, None, 1, 8, 8, terms), (p, n_p, q, n_q, 1, 8, 8, None),
                 (p, n_p, q, n_q, 1, 8, 0, terms), (p, n_p, q, n_q, 1, 8, 4097, terms), (p, n_p, q, n_q, 1, 4097, 8, terms),
                 (p, n_p, q, n_q, 0, 8, 8, terms),
                 (p, np.array([0], np.int32), q, n_q, 1, 8, 8, terms), (p, np.array([9], np.int32), q, n_q, 1, 8, 8, terms),
                 (p, n_p, q, np.array([0], np.int32), 1, 8, 8, terms), (p, n_p, q, np.array([9], np.int32), 1, 8, 8, terms)):
        assert call(*args) == -1, args[4:7]                          # DRP_EINVAL
    with pytest.raises(DrpError):
        eng.cloud_chamfer(p, q, [0], [3])


def test_a_gd_session_and_the_dispatch_marks_survive_a_call(golden):
    """drp_cloud_chamfer ends no session and leaves the marks alone: a GD session stepped with calls in between gives the bits
    of an undisturbed one, and last_dispatch() is what it was"""
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
            e.cloud_chamfer(p, q, n_p, n_q, want_grad=True)
            assert e.last_dispatch() == marks
        out.append(e.gd_step())
        if disturb:
            e.cloud_chamfer(p, q, n_p, n_q)
        out.append(e.gd_actions())
        runs.append(out)
        e.close()
    for a, b in zip(runs[0], runs[1]):
        for x, y in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
            np.testing.assert_array_equal(np.asarray(x), np.asarray(y))

"""CPU: what the float64 Chamfer yardstick's GPU tests (tests/test_gpu_chamfer_f64.py, tests/test_gpu_train_f64_untracked.py) take
for granted, and the host side of the feature.

(a) the trainer's probe options: probe_every is valid for every loss, refuses an unknown one and refuses to be combined with
    grad_probe_every; probe_batch hands the batch's targets (and pushes) to Engine.train_gradient_probe.
(b) THE PRECONDITION of the stand-alone shapes the GPU tests add (tests/_chamfer_f64_cases.py): every arg-min of chamfer64 wins by
    more than MARGIN_MIN, and where a shape has a second 1024-point tile or a second 256-row chunk some arg-min lies in it.
    Asserted here, where the seeds were picked; nothing is skipped at run time.
(c) tr_blocks (csrc/train_host.h) for the one upload of the float64 trainer calls, against sizes summed by hand; the function is
    plain C++, so tools/train_host_check.cpp is built for the host and asked."""
import os
import subprocess

import numpy as np
import pytest

import _chamfer_f64_cases as C
import _untracked_ref as U
from dyn_res_pile_manip_amd import synthetic as syn
from dyn_res_pile_manip_amd import train_gnn_dyn as TG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- (a) the options ------------------------------------------------------------------------------------------------------
def test_probe_every_refuses_an_unknown_loss_and_both_schedules():
    config = syn.default_config()
    loaders = {'train': [], 'valid': []}
    with pytest.raises(ValueError, match='loss must be one of'):
        TG.train(config, None, loaders, probe_every=1, loss='emd')
    for loss in TG.LOSSES:
        with pytest.raises(ValueError, match='not both'):
            TG.train(config, None, loaders, probe_every=2, grad_probe_every=2, loss=loss)
        with pytest.raises(ValueError, match='not both'):
            TG.main(config, probe_every=1, grad_probe_every=3, loss=loss)
    with pytest.raises(ValueError, match='probe_every'):        # the old option keeps its refusal and now names the new one
        TG.train(config, None, loaders, grad_probe_every=1, loss='chamfer')
    with pytest.raises(ValueError, match='loss must be one of'):
        TG.probe_batch(None, None, loss='emd')
    with pytest.raises(ValueError, match='impulses must be one of'):
        TG.probe_batch(None, None, impulses='pushes', loss='chamfer')
    TG.check_probe_options('chamfer', 0, 3)
    TG.check_probe_options('mse', 3, 0)
    TG.check_probe_options('mse', 0, 3)


class StubEngine(object):
    def __init__(self):
        self.calls = []

    def train_gradient_probe(self, *args, **kw):
        self.calls.append((args, kw))
        return {'rel': 0.0}


class StubModel(object):
    def __init__(self):
        self.engine = StubEngine()
        self.claimed = 0

    def _claim(self):
        self.claimed += 1


def test_probe_batch_hands_targets_and_pushes_to_the_engine():
    rng = np.random.default_rng(0)
    B, H, N, M = 2, 3, 5, 4
    six = (rng.random((B, H + 1, N, 3)), rng.random((B, H, N, 3)), np.zeros((B, H + 1, N)), np.array([5, 3]), np.array([300.0, 250.0]),
           None)
    targets, tnums = rng.random((B, H, M, 3)).astype(np.float64), np.array([[4, 3, 2], [1, 4, 4]], np.int64)
    acts = rng.random((B, H, 4))
    data = TG.PaddedBatch(six + (targets, tnums))
    model = StubModel()
    # the tracked loss: today's call, no target arguments at all
    assert TG.probe_batch(model, data) == {'rel': 0.0}
    args, kw = model.engine.calls[-1]
    assert len(args) == 5 and kw == {'actions': None} and model.claimed == 1
    assert args[0].dtype == np.float32 and args[3].dtype == np.int32
    # the Chamfer loss, data impulses
    TG.probe_batch(model, data, loss='chamfer')
    args, kw = model.engine.calls[-1]
    assert sorted(kw) == ['actions', 'target_nums', 'targets'] and kw['actions'] is None
    assert kw['targets'].dtype == np.float32 and kw['target_nums'].dtype == np.int32
    np.testing.assert_array_equal(kw['targets'], targets.astype(np.float32))
    np.testing.assert_array_equal(kw['target_nums'], tnums)
    # pushes need a batch that carries them
    with pytest.raises(ValueError, match='actions'):
        TG.probe_batch(model, data, impulses='actions', loss='chamfer')
    data.actions = acts
    TG.probe_batch(model, data, impulses='actions', loss='chamfer')
    args, kw = model.engine.calls[-1]
    np.testing.assert_array_equal(kw['actions'], acts.astype(np.float32))
    np.testing.assert_array_equal(kw['targets'], targets.astype(np.float32))
    TG.probe_batch(model, data, impulses='actions')
    args, kw = model.engine.calls[-1]
    assert sorted(kw) == ['actions'] and kw['actions'].shape == (B, H, 4)


# ---- (b) the stand-alone shapes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', C.TILING_SHAPES)
def test_tiling_shapes_have_their_margins_and_cross_their_boundaries(shape):
    p, q, n_p, n_q = C.tiling_case(shape)
    assert p.shape == (1, shape[0], 3) and q.shape == (1, shape[1], 3) and p.dtype == np.float32
    ref = U.chamfer64(p, q, n_p, n_q)
    m_pq, m_qp = float(ref['margin_pq'].min()), float(ref['margin_qp'].min())
    cr = C.crossings(ref, shape)
    print('[chamfer-f64 host] %s: margins p->q %.3e q->p %.3e, crossings %s' % (shape, m_pq, m_qp, cr))
    assert min(m_pq, m_qp) > U.MARGIN_MIN
    if shape[0] == 1:
        assert m_qp == np.inf                       # a one-row other cloud
    for has, crossed in cr.values():
        assert crossed or not has
    assert cr['tile'][0] == (max(shape) > 1024) and cr['chunk'][0] == (shape[0] > 256)


def test_some_tiling_shape_crosses_each_boundary_in_each_direction():
    seen = {'a_tile': False, 'c_tile': False, 'c_chunk': False, 'third_tile': False}
    for shape in C.TILING_SHAPES:
        ref = U.chamfer64(*C.tiling_case(shape))
        seen['a_tile'] |= bool((ref['nn_pq'] >= 1024).any())
        seen['c_tile'] |= bool((ref['nn_qp'] >= 1024).any())
        seen['c_chunk'] |= bool((ref['nn_qp'] >= 256).any())
        seen['third_tile'] |= bool((ref['nn_pq'] >= 2048).any() or (ref['nn_qp'] >= 2048).any())
    assert all(seen.values()), seen


def test_the_boundary_case_is_the_fp32_tests_draw():
    """258 x 1030: the clouds tests/test_gpu_chamfer.py builds inline, with the margin it asserts"""
    p, q, n_p, n_q = C.boundary_case()
    ref = U.chamfer64(p, q, n_p, n_q)
    assert U.min_margin(ref) > U.MARGIN_MIN
    assert (ref['nn_pq'] >= 1024).any() and (ref['nn_qp'] >= 256).any()


def test_degenerate_margins_of_the_reference():
    """what the device is held to for ties: a duplicate of the winner gives 0 exactly, a one-row other cloud inf"""
    q = np.tile(np.array([[0.2, 0.3, 0.5]], np.float32), (6, 1))[None]
    p = np.array([[0.21, 0.3, 0.5], [0.4, 0.1, 0.5], [0.4, 0.1, 0.5], [9.0, 9.0, 9.0]], np.float32)[None]
    ref = U.chamfer64(p, q, [3], [6])
    np.testing.assert_array_equal(ref['nn_pq'][0], [0, 0, 0, -1])
    np.testing.assert_array_equal(ref['margin_pq'][0, :3], 0.0)
    ref = U.chamfer64(p, q, [3], [1])
    assert (ref['margin_pq'][0, :3] == np.inf).all() and np.isfinite(ref['margin_qp'][0, 0])


# ---- (c) the upload's layout ---------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def host_check(tmp_path_factory):
    import __graft_entry__ as g
    exe = str(tmp_path_factory.mktemp('host_check') / 'train_host_check')
    subprocess.check_call([g.HIPCC, '-x', 'c++', '-std=c++17', '-O1', os.path.join(ROOT, 'tools', 'train_host_check.cpp'), '-o', exe])
    return exe


@pytest.mark.parametrize('B,H,N,M,actions', [(4, 3, 64, 50, 0), (3, 5, 23, 17, 1), (2, 1, 7, 0, 0)])
def test_float64_upload_is_the_hand_summed_size(host_check, B, H, N, M, actions):
    out = subprocess.check_output([host_check, 'layout'] + [str(v) for v in (B, H, N, M, actions, 0, 0, 0, 1, 0)]).decode().split()
    states, sdelta, attr, dens, nums, targets, tnums, nbytes = [int(v) for v in out[:8]]
    assert [int(v) for v in out[8:]] == [0] * 5             # no eps, rho, mass_q, seed or match_in was asked for

    def up(v):
        return (v + 15) // 16 * 16
    n_st = B * (H + 1) * N * 3 * 4
    n_imp = (B * H * 4 if actions else B * H * N * 3) * 4
    at_attr = up(n_st) + up(n_imp)
    at_dens = at_attr + up(B * N * 4)                       # a_cur = attrs[:, 0] alone
    assert (states, sdelta, attr, dens, nums) == (0, up(n_st), at_attr, at_dens, at_dens + up(B * 4))
    head = at_dens + 2 * up(B * 4)                          # drp_train_grad_f64's whole upload
    if M > 0:
        assert targets == head and tnums == head + up(B * H * M * 3 * 4) and nbytes == tnums + up(B * H * 4)
    else:
        assert targets == 0 and tnums == 0 and nbytes == head


def test_the_host_check_program_passes(host_check):
    out = subprocess.check_output([host_check]).decode()
    assert 'all checks passed' in out

"""GPU: training with the entropy-regularised transport loss (drp_train_step_transport: kt_transport<true> of csrc/k_sinkhorn.h
where drp_train_step_untracked launches kc_chamfer<true>; everything behind the loss gradient unchanged) through the C ABI, at
B = 2, H = 2, N = 9 (counts 9 and 6), M = 12 (target counts 12, 7 / 5, 10: above and below the predictions') on both tapes and
both impulse sources (tests/_transport_ref.py: train_batch).

The predicted states are the call's own (the trainer's `train_states` buffer, as tests/test_gpu_train_actions.py reads it):
  - the loss is the sum, step-major then sample, of cloud_transport's terms on them / (H B), to 1e-12 relative (the same kernel;
    one more rounding by the scale and the host's sum), and col_err_out is cloud_transport's col_err bit for bit;
  - the weight gradients are those of the float64 restatement (train_transport64) with the plan of every problem computed from
    those states by the host reference and held constant, as the kernel holds it: the loss within 1e-4 relative and every tensor
    within 2e-4 x max |ref| + 1e-9, tests/test_gpu_train_untracked.py's bounds for the same reverse pass.
Every figure is printed before it is asserted."""
import ctypes

import numpy as np
import pytest

import _train_actions_ref as A
import _transport_ref as T
import _untracked_ref as U
from dyn_res_pile_manip_amd import synthetic as syn
from dyn_res_pile_manip_amd import train_gnn_dyn as TG
from dyn_res_pile_manip_amd import weights
from dyn_res_pile_manip_amd._lib import DrpError
from dyn_res_pile_manip_amd.engine import Engine
from dyn_res_pile_manip_amd.gnn_dyn import PropNetDiffDenModel

pytestmark = pytest.mark.gpu
LOSS_REL = 1e-4
GRAD_REL = 2e-4
K = TG.TRANSPORT_ITERS


def new_engine(w, engine=None):
    e = Engine(0)
    e.load_weights(weights.blob_from_state_dict(w), 0.08)
    e.set_camera(*A.camera_args())
    if engine is not None:
        e.set_engine(engine)
    return e


def case(impulses):
    """-> (the keyword arguments of Engine.train_step_transport, the batch)"""
    st, sd, ac, at, nums, dens, tg, tn = T.train_batch()
    kw = dict(states=st, attrs=at, particle_nums=nums, particle_dens=dens, targets=tg, target_nums=tn, eps=TG.transport_eps(dens), iters=K)
    kw.update(dict(states_delta=sd) if impulses == 'data' else dict(actions=ac))
    return kw


@pytest.mark.parametrize('impulses', ['data', 'actions'])
@pytest.mark.parametrize('tape', ['fused', 'mfma'])
def test_loss_col_err_and_gradients(golden, tape, impulses):
    kw = case(impulses)
    st, nums, tg, tn, eps = kw['states'], kw['particle_nums'], kw['targets'], kw['target_nums'], kw['eps']
    B, H, N = st.shape[0], st.shape[1] - 1, st.shape[2]
    label = '%s %s' % (tape, impulses)
    e = new_engine(golden.weights_seed0, tape)
    e.train_begin(H, 1e-3, 0.9)
    e.dispatch_reset()
    loss, grad, col_err = e.train_step_transport(mode='grad', want_grad=True, want_col_err=True, **kw)
    ran = e.last_dispatch()
    pred = e.debug_fetch('train_states', (B, H, N, 3))
    loss_eval, none = e.train_step_transport(mode='eval', **kw)
    loss2, grad2, col_err2 = e.train_step_transport(mode='grad', want_grad=True, want_col_err=True, **kw)
    # the stand-alone metric on the call's own predictions
    total, plans = 0.0, []
    for t in range(H):
        one = e.cloud_transport(pred[:, t], tg[:, t], nums, tn[:, t], eps=eps, iters=K, want_col_err=True)
        assert one['col_err'].tobytes() == col_err[t].tobytes(), (label, t)
        for b in range(B):
            total += one['transport'][b] / (H * B)
        plans.append([T.pair64(pred[b, t, :nums[b]], tg[b, t, :tn[b, t]], float(eps[b]), K)[5] for b in range(B)])
    e.close()
    rel = abs(loss - total) / total
    print('[transport] %s: loss %.15e, cloud_transport on the predicted states %.15e, rel %.2e; col_err %s' % (label, loss, total, rel, col_err.ravel()))
    assert rel <= 1e-12
    assert none is None and abs(loss_eval - loss) < 1e-9            # tests/test_gpu_train_untracked.py's statement of `the same loss`
    assert ('k_aggregate_tape' in ran) == (tape == 'mfma'), ran
    assert not any('transport' in name for name in ran)             # no dispatch variant
    assert loss2 == loss and col_err2.tobytes() == col_err.tobytes()
    np.testing.assert_array_equal(grad2, grad)
    # the float64 restatement with those plans
    ref_loss, _, grads, _ = T.train_transport64(golden.weights_seed0, st, kw.get('states_delta'), kw['attrs'], nums, kw['particle_dens'],
                                                tg, tn, plans, actions=kw.get('actions'))
    rel = abs(loss - ref_loss) / ref_loss
    print('[transport] %s: float64 restatement %.9e, rel %.2e' % (label, ref_loss, rel))
    assert rel < LOSS_REL
    ref_blob = U.blob64(grads)
    off = 0
    for key, shape in weights.STATE_DICT_KEYS:
        n = int(np.prod(shape))
        a, b = grad[off:off + n].astype(np.float64), np.asarray(ref_blob[off:off + n], np.float64)
        scale = max(np.abs(b).max(), 1e-8)
        err = float(np.abs(a - b).max())
        print('[transport] %s %-45s %.3e of the largest gradient' % (label, key, err / scale))
        assert err < GRAD_REL * scale + 1e-9, (label, key, err / scale)
        off += n


def test_updates_move_the_weights_and_the_loss_stays_finite(golden):
    kw = case('actions')
    e = new_engine(golden.weights_seed0)
    e.train_begin(kw['states'].shape[1] - 1, 1e-3, 0.9)
    w0 = e.get_weights().copy()
    losses = [e.train_step_transport(mode='update', **kw)[0] for _ in range(3)]
    w1 = e.get_weights().copy()
    e.close()
    print('[transport] three updates: %s' % losses)
    assert np.isfinite(losses).all() and np.isfinite(w1).all()
    assert np.abs(w1 - w0).max() > 1e-4


def test_the_other_losses_keep_their_bits_around_a_transport_step(golden):
    """drp_train_step_loss with kinds 1..3 (and the MSE step) gives, before and after transport steps, the bits it gave before"""
    batch = U.untracked_batch(golden, 'b2_r5')
    st, sd, at, nums, dens, tg, tn = batch
    kw = dict(states=st, attrs=at, particle_nums=nums, particle_dens=dens, targets=tg, target_nums=tn, states_delta=sd)
    H = st.shape[1] - 1
    e = new_engine(golden.weights_seed0)
    e.train_begin(H, 1e-3, 0.9)

    def others():
        out = [e.train_step_loss(loss=kind, match_weight=0.3, mode='grad', want_grad=True, **kw) for kind in ('chamfer', 'match', 'chamfer+match')]
        return out + [e.train_step(*batch[:5], mode='grad', want_grad=True)]
    before = others()
    e.dispatch_reset()
    marks = e.last_dispatch()
    for mode in ('grad', 'eval'):
        e.train_step_loss(loss='chamfer', mode=mode, want_grad=True, **kw)
    ran_chamfer = e.last_dispatch()
    e.dispatch_reset()
    for mode in ('grad', 'eval'):
        e.train_step_transport(eps=TG.transport_eps(dens), iters=K, mode=mode, want_grad=True, want_col_err=True, **kw)
    ran = e.last_dispatch()
    assert ran == ran_chamfer                                       # the trainer's own marks, none of the new call's
    after = others()
    # a refused transport step in between changes nothing either
    with pytest.raises(DrpError, match='iters'):
        e.train_step_transport(eps=TG.transport_eps(dens), iters=0, **kw)
    again = others()
    e.close()
    assert marks == [] and not any('transport' in name for name in ran)
    for a, b, c in zip(before, after, again):
        assert a[0] == b[0] == c[0]
        np.testing.assert_array_equal(a[1], b[1])
        np.testing.assert_array_equal(a[1], c[1])


def test_refusals(golden):
    kw = case('data')
    st, sd, at, nums, dens, tg, tn, eps = [np.ascontiguousarray(kw[k]) for k in ('states', 'states_delta', 'attrs', 'particle_nums',
                                                                                   'particle_dens', 'targets', 'target_nums', 'eps')]
    acts = np.ascontiguousarray(case('actions')['actions'])
    B, T1, N, _ = st.shape
    H, M = T1 - 1, tg.shape[2]
    e = new_engine(golden.weights_seed0)
    e._n_rollout = H
    FP, IP, DP = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
    loss = ctypes.c_double()

    def call(sd_=sd, acts_=None, tg_=tg, tn_=tn, M_=M, eps_=eps, iters=K, N_=N, st_=st, at_=at, mode=0):
        f = lambda a, T_: None if a is None else a.ctypes.data_as(T_)
        return e.lib.drp_train_step_transport(e.h, f(st_, FP), f(sd_, FP), f(acts_, FP), f(at_, FP), f(nums, IP), f(dens, FP), B, N_,
                                              f(tg_, FP), f(tn_, IP), M_, f(eps_, DP), iters, mode, ctypes.byref(loss), None, None)
    assert call() == -2                                             # DRP_ESTATE before train_begin
    e.train_begin(H, 1e-3, 0.9)
    assert call() == 0
    good = loss.value
    zero, big = tn.copy(), tn.copy()
    zero[1, 1], big[0, 0] = 0, M + 1
    wide_t = np.zeros((B, H, 1025, 3), np.float32)
    wide_s, wide_d, wide_a = np.zeros((B, H + 1, 1025, 3), np.float32), np.zeros((B, H, 1025, 3), np.float32), np.zeros((B, H + 1, 1025), np.float32)
    bad_eps = lambda v: np.array([eps[0], v], np.float64)
    for kwargs in (dict(tg_=None), dict(tn_=None), dict(tn_=zero), dict(tn_=big), dict(M_=0),
                   dict(tg_=wide_t, M_=1025),                        # refused on the host: no kernel sees 1025 points
                   dict(st_=wide_s, sd_=wide_d, at_=wide_a, N_=1025),
                   dict(eps_=None), dict(eps_=bad_eps(0.0)), dict(eps_=bad_eps(-1.0)), dict(eps_=bad_eps(np.inf)), dict(eps_=bad_eps(np.nan)),
                   dict(iters=0), dict(iters=-1), dict(iters=1001),
                   dict(mode=3), dict(mode=-1),
                   dict(sd_=sd, acts_=acts), dict(sd_=None, acts_=None)):    # both or neither impulse source
        assert call(**kwargs) == -1, kwargs                          # DRP_EINVAL
        assert call() == 0 and loss.value == good, kwargs            # the context is as it was
    assert call(sd_=None, acts_=acts) == 0
    # drp_train_step_loss keeps refusing kind 4 and every other kind outside 1..3
    for kind in (4, 0, 5, -1):
        assert e.lib.drp_train_step_loss(e.h, st.ctypes.data_as(FP), sd.ctypes.data_as(FP), None, at.ctypes.data_as(FP), nums.ctypes.data_as(IP),
                                         dens.ctypes.data_as(FP), B, N, tg.ctypes.data_as(FP), tn.ctypes.data_as(IP), M, kind, 0.5, 0,
                                         ctypes.byref(loss), None, None) == -1, kind
    with pytest.raises(DrpError, match='1025'):
        e.train_step_transport(st, at, nums, dens, wide_t, tn, eps, K, states_delta=sd)
    with pytest.raises(ValueError):
        e.train_step_transport(st, at, nums, dens, tg, tn, eps, K, states_delta=sd, actions=acts)
    with pytest.raises(ValueError, match='loss must be one of'):
        e.train_step_loss(st, at, nums, dens, tg, tn, states_delta=sd, loss='transport')       # no kind of that call
    e.close()


# ---- the training loop ------------------------------------------------------------------------------------------------------------
def _model(golden):
    import torch
    model = PropNetDiffDenModel(syn.default_config(), True)
    model.load_state_dict({k[2:]: torch.from_numpy(golden.weights_seed0[k]) for k in golden.weights_seed0.files
                           if k.startswith('w/')}, strict=False)
    return model


def test_run_batch_is_the_engine_call_with_eps_from_the_densities(golden):
    st, sd, ac, at, nums, dens, tg, tn = T.train_batch()
    model = _model(golden)
    model.engine.set_camera(*A.camera_args())
    opt = TG.DeviceAdam(model, 1e-3, betas=(0.9, 0.999), n_rollout=st.shape[1] - 1)
    data = TG.PaddedBatch((st, sd, at, nums, dens, None, tg, tn))
    data.actions = ac
    for impulses, extra in (('data', dict(states_delta=sd)), ('actions', dict(actions=ac))):
        for scale, iters in ((1.0, K), (0.5, 7)):
            got = TG.run_batch(model, opt, data, 'valid', loss='transport', impulses=impulses, transport_eps_scale=scale, transport_iters=iters)
            want = model.engine.train_step_transport(st, at, nums, dens, tg, tn, scale / dens.astype(np.float64), iters, mode='eval', **extra)[0]
            assert got == want and np.isfinite(got), (impulses, scale, iters)
    with pytest.raises(ValueError, match='no float64 yardstick'):
        TG.probe_batch(model, data, loss='transport')
    model.engine.close()


@pytest.fixture(scope='module')
def depth_episodes(tmp_path_factory):
    """tests/test_gpu_gnn_frames.py's episodes: depth PNGs and actions.p alone"""
    import os
    import shutil
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
    import make_golden_gnn_frames as mk
    full = str(tmp_path_factory.mktemp('transport_tracked'))
    syn.write_episodes(full, **mk.EPISODES)
    d = str(tmp_path_factory.mktemp('transport_depth'))
    for ep in os.listdir(full):
        os.makedirs(os.path.join(d, ep))
        for f in os.listdir(os.path.join(full, ep)):
            if not (f.endswith('_particles.npy') or f.endswith('_color.png')):
                shutil.copy(os.path.join(full, ep, f), os.path.join(d, ep, f))
    return d


def test_train_on_a_depth_dataset(depth_episodes):
    """train(..., loss='transport') for 2 epochs on a DepthDataset of the tiny fixture episodes, impulses='actions': finite losses;
    a depth-only batch is refused with any other impulse source"""
    import dyn_res_pile_manip_amd.planners as P
    from dyn_res_pile_manip_amd.dataset_gnn_dyn import DepthDataset, DeviceLoader
    cam = (syn.demo_cam_params(), syn.demo_cam_extrinsics())
    cfg = TG.default_config()
    cfg['dataset'].update(n_episode=4, n_timestep=6)
    cfg['train'].update(n_rollout=2, batch_size=4, train_valid_ratio=0.5, lr=2e-4, ckp_per_iter=2, log_per_iter=1, adam_beta1=0.9)
    eng = Engine(0)
    model = PropNetDiffDenModel(cfg, engine=eng)
    model.load_state_dict(weights.random_state_dict(seed=0, predictor_scale=1.0))
    eng.set_camera(P.world2cam_affine(np.asarray(cam[1], dtype=np.float64)), 24.0, cam[0])
    datasets = {ph: DepthDataset(depth_episodes, cfg, ph, cam, engine=eng, target_den_scale=1.5) for ph in ('train', 'valid')}
    loaders = {ph: DeviceLoader(datasets[ph], 4, shuffle=False, chunk=16, threads=4) for ph in ('train', 'valid')}
    first = next(iter(loaders['train']))
    assert first.depth_only
    with pytest.raises(ValueError, match='depth-only'):
        TG.run_batch(model, None, first, 'valid', 2, loss='transport', impulses='data')
    w0 = eng.get_weights().copy()
    lines = []
    res = TG.train(cfg, model, loaders, n_epoch=2, loss='transport', impulses='actions', log=lines.append)
    rmse = [r for (_, ph, r) in res['history'] if ph in ('train', 'valid')]
    print('[transport] depth episodes, 2 epochs: rmse %s' % rmse)
    assert len(rmse) == 4 and np.isfinite(rmse).all() and np.isfinite(res['best_valid_loss'])
    assert np.abs(eng.get_weights() - w0).max() > 0
    eng.close()

"""GPU: training against untracked clouds (drp_train_step_untracked: the Chamfer loss of csrc/k_chamfer.h where drp_train_step
launches kt_mse_grad, everything behind the loss gradient unchanged) through the C ABI, against train_untracked64 of
tests/_untracked_ref.py.

Bounds: the loss within 1e-4 relative and each of the 18 parameter tensors within 2e-4 x max |ref| + 1e-9, the yardstick
tests/test_gpu_train.py holds the trainer to; tests/test_untracked_host.py holds every arg-min margin of the batches used here
above 1e-7, so the fp32 pass picks the reference's partners.  Every figure is printed before it is asserted."""
import ctypes

import numpy as np
import pytest

import _untracked_ref as U
from dyn_res_pile_manip_amd import synthetic as syn
from dyn_res_pile_manip_amd import train_gnn_dyn as TG
from dyn_res_pile_manip_amd import weights
from dyn_res_pile_manip_amd._lib import DrpError
from dyn_res_pile_manip_amd.dataset_gnn_dyn import drop_correspondence
from dyn_res_pile_manip_amd.engine import Engine
from dyn_res_pile_manip_amd.gnn_dyn import PropNetDiffDenModel

pytestmark = pytest.mark.gpu
LOSS_REL = 1e-4
GRAD_REL = 2e-4


def new_engine(w, engine=None):
    e = Engine(0)
    e.load_weights(weights.blob_from_state_dict(w), 0.08)
    if engine is not None:
        e.set_engine(engine)
    return e


def _model(golden):
    import torch
    model = PropNetDiffDenModel(syn.default_config(), True)
    model.load_state_dict({k[2:]: torch.from_numpy(golden.weights_seed0[k]) for k in golden.weights_seed0.files
                           if k.startswith('w/')}, strict=False)
    return model


def assert_grads(grad, ref_blob, label):
    off, worst = 0, 0.0
    for key, shape in weights.STATE_DICT_KEYS:
        n = int(np.prod(shape))
        a, b = grad[off:off + n].astype(np.float64), ref_blob[off:off + n]
        scale = max(np.abs(b).max(), 1e-8)
        err = float(np.abs(a - b).max())
        print('[untracked] %s %-45s %.3e of the largest gradient' % (label, key, err / scale))
        worst = max(worst, err / scale)
        assert err < GRAD_REL * scale + 1e-9, (label, key, err / scale)
        off += n
    return worst


@pytest.mark.parametrize('tape', ['fused', 'mfma'])
@pytest.mark.parametrize('name,wset', U.TRAIN_CASES)
def test_loss_and_gradients_against_float64(golden, name, wset, tape):
    batch = U.untracked_batch(golden, name)
    ref_loss, ref_terms, ref_blob, _, _ = U.reference(golden, name, wset)
    e = new_engine(U.weights_of(golden, wset), tape)
    e.train_begin(batch[0].shape[1] - 1, 1e-3, 0.9)
    e.dispatch_reset()
    loss, grad = e.train_step_untracked(*batch, mode='grad', want_grad=True)
    ran = e.last_dispatch()
    loss_eval, none = e.train_step_untracked(*batch, mode='eval')
    loss2, grad2 = e.train_step_untracked(*batch, mode='grad', want_grad=True)
    e.close()
    # the marks of an MSE step of the same shape, at the same point of an engine's life
    e = new_engine(U.weights_of(golden, wset), tape)
    e.train_begin(batch[0].shape[1] - 1, 1e-3, 0.9)
    e.dispatch_reset()
    e.train_step(*batch[:5], mode='grad')
    ran_mse = e.last_dispatch()
    e.close()
    assert ('k_aggregate_tape' in ran) == (tape == 'mfma'), ran
    rel = abs(loss - ref_loss) / ref_loss
    print('[untracked] %s %s %s: loss %.9e, float64 %.9e, rel %.2e' % (name, wset, tape, loss, ref_loss, rel))
    assert rel < LOSS_REL
    assert none is None and abs(loss_eval - loss) < 1e-9
    assert_grads(grad, ref_blob, '%s %s %s' % (name, wset, tape))
    assert loss2 == loss
    np.testing.assert_array_equal(grad2, grad)                      # bit-equal from run to run
    assert ran == ran_mse


def test_single_point_targets(golden):
    """target_nums all 1, M = 1 (the hand-checkable configuration: tests/test_untracked_host.py checks the reference by hand)"""
    batch = U.single_point_batch(golden)
    ref_loss, _, grads, _, _ = U.train_untracked64(golden.weights_seed0, *batch)
    e = new_engine(golden.weights_seed0)
    e.train_begin(batch[0].shape[1] - 1, 1e-3, 0.9)
    loss, grad = e.train_step_untracked(*batch, mode='grad', want_grad=True)
    e.close()
    print('[untracked] single point: loss rel %.2e' % (abs(loss - ref_loss) / ref_loss))
    assert abs(loss - ref_loss) < LOSS_REL * ref_loss
    assert_grads(grad, U.blob64(grads), 'single point')


def test_tiny_unpadded_batch(golden):
    batch = U.tiny_batch()
    assert batch[0].shape == (1, 2, 5, 3) and batch[5].shape == (1, 1, 3, 3)
    ref_loss, _, grads, _, _ = U.train_untracked64(golden.weights_seed0, *batch)
    e = new_engine(golden.weights_seed0)
    e.train_begin(1, 1e-3, 0.9)
    loss, grad = e.train_step_untracked(*batch, mode='grad', want_grad=True)
    e.close()
    print('[untracked] tiny: loss rel %.2e' % (abs(loss - ref_loss) / ref_loss))
    assert abs(loss - ref_loss) < LOSS_REL * ref_loss
    assert_grads(grad, U.blob64(grads), 'tiny')


@pytest.mark.parametrize('name', ['b4_r3', 'b2_r5'])
def test_adam_trajectory(golden, name):
    """three Adam steps on the device follow train_untracked64 with a numpy Adam (the bounds of tests/test_gpu_train.py's
    test_adam_trajectory)"""
    batch = U.untracked_batch(golden, name)
    lr, beta1 = [float(v) for v in golden.train[name + '/lr_beta1']]
    ref_losses, ref_blob, g0, _ = U.adam_trajectory64(golden, name, lr, beta1)
    model = _model(golden)
    opt = TG.DeviceAdam(model, lr, betas=(beta1, 0.999), n_rollout=batch[0].shape[1] - 1)
    data = batch[:5] + [None] + batch[5:]                           # collate_untracked's layout
    losses = [TG.run_batch(model, opt, data, 'train', loss='chamfer') for _ in range(3)]
    got = model.engine.get_weights().astype(np.float64)
    model.engine.close()
    print('[untracked] %s losses %s, float64 %s' % (name, losses, ref_losses))
    np.testing.assert_allclose(losses, ref_losses, rtol=2e-3)
    off = 0
    for key, shape in weights.STATE_DICT_KEYS:
        n = int(np.prod(shape))
        gr = g0[off:off + n]
        firm = np.abs(gr) > 1e-3 * np.abs(gr).max()               # Adam's first steps are +-lr: sign of tiny gradients is noise
        d = np.abs(got[off:off + n] - ref_blob[off:off + n])
        assert d[firm].max() < 2e-5, key
        assert d.max() < 3.5 * lr, key
        off += n


def test_training_lowers_the_chamfer_loss_and_valid_phase_leaves_weights(golden):
    """a fixed batch trained as in test_training_reduces_the_loss_and_valid_phase_leaves_weights: same iteration count and lr"""
    model = _model(golden)
    config = syn.default_config()
    config['train'].update({'n_rollout': 3, 'n_history': 1, 'lr': 2e-4, 'adam_beta1': 0.9, 'log_per_iter': 50, 'n_epoch': 6})
    batch = U.untracked_batch(golden, 'b4_r3')
    data = batch[:5] + [None] + batch[5:]                           # collate_untracked's layout
    w0 = model.engine.get_weights().copy()
    res = TG.train(config, model, {'train': [data] * 4, 'valid': [data]}, loss='chamfer')
    rmse_valid = [h[2] for h in res['history'] if h[1] == 'valid']
    print('[untracked] valid rmse per epoch %s' % rmse_valid)
    assert rmse_valid[-1] < 0.99 * rmse_valid[0] and min(rmse_valid) == rmse_valid[-1]
    assert np.abs(model.engine.get_weights() - w0).max() > 1e-4
    w1 = model.engine.get_weights()
    l_a = TG.run_batch(model, None, data, 'valid', loss='chamfer')
    l_b = TG.run_batch(model, None, data, 'valid', loss='chamfer')
    assert l_a == l_b
    np.testing.assert_array_equal(model.engine.get_weights(), w1)
    model.engine.close()


def test_train_and_collate_untracked_end_to_end(golden):
    """synthetic.push_batch samples through drop_correspondence and collate_untracked into train(loss='chamfer')"""
    rng = np.random.default_rng(0)
    loaders = {'train': [], 'valid': []}
    for it in range(3):
        st, sd, at, nums, dens = syn.push_batch(it, batch_size=2, n_rollout=2)
        data = [drop_correspondence((st[b, :, :n], sd[b, :, :n], at[b, :, :n], int(n), float(dens[b]), None), rng)
                for b, n in enumerate(nums)]
        out = TG.collate_untracked(data)
        np.testing.assert_array_equal(out[0], st)
        np.testing.assert_array_equal(out[3], nums)
        for b, d in enumerate(data):                                # against a per-sample copy loop
            for t, cloud in enumerate(d[6]):
                assert out[7][b, t] == cloud.shape[0]
                np.testing.assert_array_equal(out[6][b, t, :cloud.shape[0]], cloud)
                assert (out[6][b, t, cloud.shape[0]:] == 0).all()
        loaders['train' if it < 2 else 'valid'].append(out)
    model = _model(golden)
    config = syn.default_config()
    config['train'].update({'n_rollout': 2, 'n_history': 1, 'lr': 2e-4, 'adam_beta1': 0.9, 'log_per_iter': 50, 'n_epoch': 2})
    w0 = model.engine.get_weights().copy()
    with pytest.raises(ValueError):
        TG.train(config, model, loaders, grad_probe_every=1, loss='chamfer')
    res = TG.train(config, model, loaders, loss='chamfer')
    assert len([h for h in res['history'] if h[1] == 'valid']) == 2 and np.isfinite(res['best_valid_loss'])
    assert np.abs(model.engine.get_weights() - w0).max() > 1e-4
    model.engine.close()


def test_chamfer_steps_leave_the_mse_and_f64_paths_their_bits(golden):
    batch = U.untracked_batch(golden, 'b2_r5')
    H = batch[0].shape[1] - 1
    runs = []
    for disturb in (False, True):
        e = new_engine(golden.weights_seed0)
        e.train_begin(H, 1e-3, 0.9)
        if disturb:
            for _ in range(2):
                e.train_step_untracked(*batch, mode='grad', want_grad=True)
            e.train_step_untracked(*batch, mode='eval')
        mse = e.train_step(*batch[:5], mode='grad', want_grad=True)
        f64 = e.train_grad_f64(*batch[:5])
        runs.append((mse, f64))
        e.close()
    assert runs[0][0][0] == runs[1][0][0]
    np.testing.assert_array_equal(runs[0][0][1], runs[1][0][1])
    assert runs[0][1][0] == runs[1][1][0]
    np.testing.assert_array_equal(runs[0][1][1], runs[1][1][1])
    np.testing.assert_array_equal(runs[0][1][2], runs[1][1][2])


def test_a_timed_out_barrier_moves_nothing_and_the_chamfer_step_runs_again(golden, monkeypatch):
    """DRP_DEBUG_FORCE_GIVEUP=1 as tests/test_gpu_train.py sets it: the first Chamfer update ends as if kmb_step_bwd's barrier had
    timed out, moves nothing, and runs again with one workgroup per group -- the bits of an engine that ran so from the start"""
    batch = U.untracked_batch(golden, 'b4_r3')
    lr, beta1 = [float(v) for v in golden.train['b4_r3/lr_beta1']]
    runs = {}
    for name, env in (('retry', {'DRP_DEBUG_FORCE_GIVEUP': '1'}), ('one', {'DRP_TRAIN_PARTS': '1'})):
        for k in ('DRP_DEBUG_FORCE_GIVEUP', 'DRP_TRAIN_PARTS'):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        model = _model(golden)
        eng = model.engine
        eng.train_begin(batch[0].shape[1] - 1, lr, beta1)
        eng.dispatch_reset()
        # the FIRST call is an update: its first pass gives up, Adam moves nothing (weights, moments, iteration count), the pass
        # runs again and the update is that of an engine whose first pass was never disturbed
        loss, grad = eng.train_step_untracked(*batch, mode='update', want_grad=True)
        w1 = eng.get_weights().copy()
        losses = [eng.train_step_untracked(*batch, mode='update')[0] for _ in range(2)]
        runs[name] = (loss, grad, losses, eng.get_weights(), eng.last_dispatch(), w1)
        eng.close()
    assert any('barrier gave up' in v for v in runs['retry'][4]), runs['retry'][4]
    assert not any('barrier gave up' in v for v in runs['one'][4])
    assert runs['retry'][0] == runs['one'][0] and runs['retry'][2] == runs['one'][2]
    np.testing.assert_array_equal(runs['retry'][1], runs['one'][1])
    np.testing.assert_array_equal(runs['retry'][3], runs['one'][3])
    np.testing.assert_array_equal(runs['retry'][5], runs['one'][5])
    assert np.abs(runs['retry'][5] - weights.blob_from_state_dict(golden.weights_seed0)).max() > 0


def test_refusals(golden):
    batch = U.untracked_batch(golden, 'b2_r5')
    H = batch[0].shape[1] - 1
    e = new_engine(golden.weights_seed0)
    e._n_rollout = H
    with pytest.raises(DrpError):                                   # DRP_ESTATE before train_begin
        e.train_step_untracked(*batch, mode='eval')
    st, sd, at, nums, dens, tg, tn = [np.ascontiguousarray(a) for a in batch]
    B, _, N, _ = st.shape
    M = tg.shape[2]
    FP, IP = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32)
    loss = ctypes.c_double()

    def call(tg_, tn_, M_):
        f = lambda a, T: None if a is None else a.ctypes.data_as(T)
        return e.lib.drp_train_step_untracked(e.h, f(st, FP), f(sd, FP), f(at, FP), f(nums, IP), f(dens, FP), B, N, f(tg_, FP),
                                              f(tn_, IP), M_, 0, ctypes.byref(loss), None)
    assert call(tg, tn, M) == -2                                    # DRP_ESTATE
    e.train_begin(H, 1e-3, 0.9)
    assert call(tg, tn, M) == 0
    zero, big = tn.copy(), tn.copy()
    zero[1, 2], big[0, 0] = 0, M + 1
    for args in ((None, tn, M), (tg, None, M), (tg, zero, M), (tg, big, M), (tg, tn, 0), (tg, tn, 4097)):
        assert call(*args) == -1, args[2]                           # DRP_EINVAL
    assert call(tg, tn, M) == 0
    e.close()

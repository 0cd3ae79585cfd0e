"""GPU: training with the Sinkhorn divergence (drp_train_step_divergence: kd_sweeps and kd_combine<true> of csrc/k_sinkhorn.h
where drp_train_step_transport launches kt_transport<true>; everything behind the loss gradient unchanged) through the C ABI, on
tests/_transport_ref.py's train_batch: B = 2, H = 2, N = 9 (counts 9 and 6), M = 12 (target counts 12, 7 / 5, 10: above and below
the predictions'), on both tapes and both impulse sources.

The predicted states are the call's own (the trainer's `train_states` buffer):
  - the loss is the sum, step-major then sample, of cloud_divergence's terms on them / (H B), to 1e-12 relative (the same kernels;
    one more rounding by the scale and the host's sum), and col_err and self_err are cloud_divergence's bit for bit;
  - the weight gradients are those of the float64 restatement (_divergence_ref.train_divergence64) with the cross plan and the
    self plan of every problem computed from those states by the host reference and held constant, as the kernel holds them.
Bounds: tests/test_gpu_train_transport.py's for the same reverse pass were 1e-4 (loss) and 2e-4 x max |ref| + 1e-9 (every tensor);
here they are 5 x the worst figure measured on one MI355X over the four cases:
  MEASURED (worst)   loss 6.5e-16 relative (the reported term is the duals' value on both sides)   weight gradients 8.6e-7 of a
                     tensor's largest entry (the fp32 reverse pass)
Every figure is printed before it is asserted."""
import numpy as np
import pytest

import _divergence_ref as D
import _train_actions_ref as A
import _transport_ref as T
import _untracked_ref as U
from dyn_res_pile_manip_amd import synthetic as syn
from dyn_res_pile_manip_amd import train_gnn_dyn as TG
from dyn_res_pile_manip_amd import weights
from dyn_res_pile_manip_amd.engine import Engine
from dyn_res_pile_manip_amd.gnn_dyn import PropNetDiffDenModel

pytestmark = pytest.mark.gpu
MEASURED = {'loss': 6.5e-16, 'grad': 8.6e-7}                         # the module docstring's line
LOSS_REL = 5 * MEASURED['loss']
GRAD_REL = 5 * MEASURED['grad']
assert LOSS_REL <= 1e-4 and GRAD_REL <= 2e-4                         # no wider than the transport step's
K = TG.TRANSPORT_ITERS


def new_engine(w, engine=None):
    e = Engine(0)
    e.load_weights(weights.blob_from_state_dict(w), 0.08)
    e.set_camera(*A.camera_args())
    if engine is not None:
        e.set_engine(engine)
    return e


def case(impulses):
    """-> the keyword arguments of Engine.train_step_divergence"""
    st, sd, ac, at, nums, dens, tg, tn = T.train_batch()
    kw = dict(states=st, attrs=at, particle_nums=nums, particle_dens=dens, targets=tg, target_nums=tn, eps=TG.transport_eps(dens), iters=K)
    kw.update(dict(states_delta=sd) if impulses == 'data' else dict(actions=ac))
    return kw


@pytest.mark.parametrize('impulses', ['data', 'actions'])
@pytest.mark.parametrize('tape', ['fused', 'mfma'])
def test_loss_certificates_and_gradients(golden, tape, impulses):
    kw = case(impulses)
    st, nums, tg, tn, eps = kw['states'], kw['particle_nums'], kw['targets'], kw['target_nums'], kw['eps']
    B, H, N = st.shape[0], st.shape[1] - 1, st.shape[2]
    label = '%s %s' % (tape, impulses)
    e = new_engine(golden.weights_seed0, tape)
    e.train_begin(H, 1e-3, 0.9)
    e.dispatch_reset()
    loss, grad, col_err, self_err = e.train_step_divergence(mode='grad', want_grad=True, want_err=True, **kw)
    ran = e.last_dispatch()
    pred = e.debug_fetch('train_states', (B, H, N, 3))
    w0 = e.get_weights().copy()
    loss_eval, none = e.train_step_divergence(mode='eval', **kw)
    loss2, grad2, col_err2, self_err2 = e.train_step_divergence(mode='grad', want_grad=True, want_err=True, **kw)
    assert col_err.shape == (H, B) and self_err.shape == (H, B, 2)
    # the stand-alone metric on the call's own predictions
    total, plans = 0.0, []
    for t in range(H):
        one = e.cloud_divergence(pred[:, t], tg[:, t], nums, tn[:, t], eps=eps, iters=K, want_col_err=True, want_self_err=True)
        assert one['col_err'].tobytes() == col_err[t].tobytes(), (label, t)
        assert one['self_err'].tobytes() == self_err[t].tobytes(), (label, t)
        for b in range(B):
            total += one['divergence'][b] / (H * B)
        row = []
        for b in range(B):
            out = D.pair64(pred[b, t, :nums[b]], tg[b, t, :tn[b, t]], float(eps[b]), K, want_plans=True)
            row.append((out[8], out[9], out[0]))
        plans.append(row)
    np.testing.assert_array_equal(e.get_weights(), w0)              # neither mode moved the weights
    e.close()
    rel = abs(loss - total) / total
    print('[divergence] %s: loss %.15e, cloud_divergence on the predicted states %.15e, rel %.2e; col_err %s self_err %s'
          % (label, loss, total, rel, col_err.ravel(), self_err.ravel()))
    assert rel <= 1e-12
    assert none is None and abs(loss_eval - loss) < 1e-9
    assert ('k_aggregate_tape' in ran) == (tape == 'mfma'), ran
    assert not any('divergence' in name or 'sweeps' in name for name in ran)      # no dispatch variant
    assert loss2 == loss and col_err2.tobytes() == col_err.tobytes() and self_err2.tobytes() == self_err.tobytes()
    np.testing.assert_array_equal(grad2, grad)
    # the float64 restatement with those plans
    ref_loss, _, grads, _ = D.train_divergence64(golden.weights_seed0, st, kw.get('states_delta'), kw['attrs'], nums, kw['particle_dens'],
                                                 tg, tn, plans, actions=kw.get('actions'))
    rel = abs(loss - ref_loss) / ref_loss
    print('[divergence] %s: float64 restatement %.9e, rel %.2e' % (label, ref_loss, rel))
    assert rel < LOSS_REL
    ref_blob = U.blob64(grads)
    off, worst = 0, 0.0
    for key, shape in weights.STATE_DICT_KEYS:
        n = int(np.prod(shape))
        a, b = grad[off:off + n].astype(np.float64), np.asarray(ref_blob[off:off + n], np.float64)
        scale = max(np.abs(b).max(), 1e-8)
        err = float(np.abs(a - b).max())
        worst = max(worst, err / scale)
        print('[divergence] %s %-45s %.3e of the largest gradient' % (label, key, err / scale))
        assert err < GRAD_REL * scale + 1e-9, (label, key, err / scale)
        off += n
    print('[divergence] %s: worst tensor %.3e' % (label, worst))


def test_eval_leaves_the_session_alone_and_updates_move_the_weights(golden):
    kw = case('actions')
    e = new_engine(golden.weights_seed0)
    e.train_begin(kw['states'].shape[1] - 1, 1e-3, 0.9)
    w0 = e.get_weights().copy()
    first = e.train_step_divergence(mode='update', **kw)[0]          # Adam state and iteration count now hold one step
    w1 = e.get_weights().copy()
    evals = [e.train_step_divergence(mode='eval', **kw)[0] for _ in range(2)]
    np.testing.assert_array_equal(e.get_weights(), w1)
    # had the evaluations touched the moments or the count, this update would differ from the one of a session without them
    second = e.train_step_divergence(mode='update', **kw)[0]
    w2 = e.get_weights().copy()
    e.close()
    e = new_engine(golden.weights_seed0)
    e.train_begin(kw['states'].shape[1] - 1, 1e-3, 0.9)
    plain = [e.train_step_divergence(mode='update', **kw)[0] for _ in range(2)]
    w2_plain = e.get_weights().copy()
    e.close()
    print('[divergence] updates: %s, evaluations in between: %s' % ([first, second], evals))
    assert evals[0] == evals[1] == second and plain == [first, second]
    np.testing.assert_array_equal(w2, w2_plain)
    assert np.isfinite([first, second]).all() and np.isfinite(w2).all()
    assert np.abs(w1 - w0).max() > 1e-4 and np.abs(w2 - w1).max() > 1e-5


def test_a_non_finite_predicted_state_ends_in_a_nan_loss(golden):
    """one rollout step, evaluation only: the prediction is read by the loss kernels alone.  A NaN in the predictor's last bias
    makes every predicted coordinate NaN; the sweeps run their K n_p n_q steps and the call returns NaN"""
    st, sd, ac, at, nums, dens, tg, tn = T.train_batch()
    w = dict((k, np.array(golden.weights_seed0[k])) for k in golden.weights_seed0.files)
    key = [k for k in w if k.endswith('particle_predictor.linear_1.bias')]
    assert len(key) == 1
    w[key[0]] = np.full_like(w[key[0]], np.nan)
    e = new_engine(w)
    e.train_begin(1, 1e-3, 0.9)
    kw = dict(states=st[:, :2], attrs=at[:, :2], particle_nums=nums, particle_dens=dens, targets=tg[:, :1], target_nums=tn[:, :1],
              eps=TG.transport_eps(dens), iters=K, states_delta=sd[:, :1])
    loss, none, col_err, self_err = e.train_step_divergence(mode='eval', want_err=True, **kw)
    pred = e.debug_fetch('train_states', (2, 1, st.shape[2], 3))
    e.close()
    assert np.isnan(pred[0, 0, :nums[0]]).all()
    assert np.isnan(loss) and none is None
    assert np.isnan(col_err).all() and np.isnan(self_err[..., 0]).all()
    assert np.isfinite(self_err[..., 1]).all()                       # the targets' own problem never saw the prediction


# ---- the training loop ------------------------------------------------------------------------------------------------------------
def _model(golden):
    import torch
    model = PropNetDiffDenModel(syn.default_config(), True)
    model.load_state_dict({k[2:]: torch.from_numpy(golden.weights_seed0[k]) for k in golden.weights_seed0.files
                           if k.startswith('w/')}, strict=False)
    return model


def test_run_batch_is_the_engine_call_and_train_runs_untracked_batches(golden):
    st, sd, ac, at, nums, dens, tg, tn = T.train_batch()
    model = _model(golden)
    model.engine.set_camera(*A.camera_args())
    H = st.shape[1] - 1
    opt = TG.DeviceAdam(model, 1e-3, betas=(0.9, 0.999), n_rollout=H)
    data = TG.PaddedBatch((st, sd, at, nums, dens, None, tg, tn))
    data.actions = ac
    for impulses, extra in (('data', dict(states_delta=sd)), ('actions', dict(actions=ac))):
        for scale, iters in ((1.0, K), (0.5, 7)):
            got = TG.run_batch(model, opt, data, 'valid', loss='sinkhorn', impulses=impulses, transport_eps_scale=scale, transport_iters=iters)
            want = model.engine.train_step_divergence(st, at, nums, dens, tg, tn, scale / dens.astype(np.float64), iters, mode='eval', **extra)[0]
            assert got == want and np.isfinite(got), (impulses, scale, iters)
    with pytest.raises(ValueError, match='no float64 yardstick'):
        TG.probe_batch(model, data, loss='sinkhorn')
    # train(): two batches a phase of collate_untracked's layout (the batch above and its samples swapped), one epoch
    swap = TG.PaddedBatch(tuple(None if x is None else np.ascontiguousarray(x[::-1]) for x in (st, sd, at, nums, dens, None, tg, tn)))
    swap.actions = np.ascontiguousarray(ac[::-1])
    cfg = TG.default_config()
    cfg['train'].update(n_rollout=H, lr=2e-4, ckp_per_iter=10, log_per_iter=1, adam_beta1=0.9)
    loaders = {'train': [data, swap], 'valid': [data, swap]}
    w0 = model.engine.get_weights().copy()
    lines = []
    res = TG.train(cfg, model, loaders, n_epoch=1, loss='sinkhorn', impulses='actions', log=lines.append)
    phases = [ph for (_, ph, _) in res['history']]
    rmse = [r for (_, _, r) in res['history']]
    print('[divergence] train(loss=\'sinkhorn\'): history %s' % (res['history'],))
    assert phases == ['train', 'valid'] and np.isfinite(rmse).all() and np.isfinite(res['best_valid_loss'])
    assert np.abs(model.engine.get_weights() - w0).max() > 0
    model.engine.close()

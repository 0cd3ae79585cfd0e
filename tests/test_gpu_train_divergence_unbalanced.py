"""GPU: training with the unbalanced Sinkhorn divergence (drp_train_step_divergence_unbalanced: kd_sweeps_unbalanced and
kd_combine<true, true> of csrc/k_sinkhorn.h where drp_train_step_divergence launches the balanced pair; everything behind the
loss gradient unchanged) through the C ABI, on tests/_transport_ref.py's train_batch -- B = 2, H = 2, N = 9 (counts 9 and 6),
M = 12 (target counts 12, 7 / 5, 10) -- on both tapes, both impulse sources, the seed-0 and the trained weights, at
rho = 4 eps with the targets' masses 1 ('unit') and target_nums / particle_nums ('count').

As tests/test_gpu_train_divergence.py, on the call's own predicted states:
  - the loss is the sum, step-major then sample, of cloud_divergence(reach=...)'s terms on them / (H B), to 1e-12 relative, and
    col_err, self_err and transported are that call's bit for bit;
  - the weight gradients are those of the float64 restatement (_divergence_unbalanced_ref.train_divergence64) fed the reference's
    own plans of those states.
Bounds: that file's, unchanged -- everything behind the loss gradient is the same code: loss 5 x 6.5e-16 relative, every tensor
5 x 8.6e-7 of its largest entry + 1e-9.
  MEASURED (worst of the 16 cases, one MI355X)   loss 2.7e-15 relative (fused, pushes, trained weights, unit masses; the balanced
                     step's 6.5e-16 times the cancellation of the value's expm1 sums)   weight gradients 1.6e-6 of a tensor's
                     largest entry (fused, pushes, seed-0 weights, count masses)
Every figure is printed before it is asserted."""
import numpy as np
import pytest

import _divergence_unbalanced_ref as R
import _train_actions_ref as A
import _transport_ref as T
import _untracked_ref as U
import test_gpu_train_divergence as GT
from dyn_res_pile_manip_amd import train_gnn_dyn as TG
from dyn_res_pile_manip_amd import weights
from dyn_res_pile_manip_amd._lib import DrpError

pytestmark = pytest.mark.gpu
LOSS_REL, GRAD_REL = GT.LOSS_REL, GT.GRAD_REL                        # the balanced step's bounds
K = TG.TRANSPORT_ITERS
REACH_SCALE = 4.0


def case(impulses, mass):
    """-> the keyword arguments of Engine.train_step_divergence with a reach"""
    kw = GT.case(impulses)
    kw['reach'] = TG.sinkhorn_reach(kw['particle_dens'], REACH_SCALE)
    kw['mass_q'] = TG.sinkhorn_mass_q(mass, kw['particle_nums'], kw['target_nums'])
    return kw


def weight_set(golden, wset):
    return golden.weights_seed0 if wset == 'seed0' else golden.weights_trained


@pytest.mark.parametrize('mass', TG.SINKHORN_MASSES)
@pytest.mark.parametrize('wset', ['seed0', 'trained'])
@pytest.mark.parametrize('impulses', ['data', 'actions'])
@pytest.mark.parametrize('tape', ['fused', 'mfma'])
def test_loss_certificates_and_gradients(golden, tape, impulses, wset, mass):
    kw = case(impulses, mass)
    st, nums, tg, tn, eps, rho, w = (kw[k] for k in ('states', 'particle_nums', 'targets', 'target_nums', 'eps', 'reach', 'mass_q'))
    B, H, N = st.shape[0], st.shape[1] - 1, st.shape[2]
    label = '%s %s %s %s' % (tape, impulses, wset, mass)
    W = weight_set(golden, wset)
    e = GT.new_engine(W, tape)
    e.train_begin(H, 1e-3, 0.9)
    e.dispatch_reset()
    loss, grad, col_err, self_err, moved = e.train_step_divergence(mode='grad', want_grad=True, want_err=True, **kw)
    ran = e.last_dispatch()
    pred = e.debug_fetch('train_states', (B, H, N, 3))
    w0 = e.get_weights().copy()
    loss_eval, none = e.train_step_divergence(mode='eval', **kw)
    loss2, grad2, col_err2, self_err2, moved2 = e.train_step_divergence(mode='grad', want_grad=True, want_err=True, **kw)
    assert col_err.shape == (H, B) and self_err.shape == (H, B, 2) and moved.shape == (H, B)
    total, plans = 0.0, []
    for t in range(H):
        one = e.cloud_divergence(pred[:, t], tg[:, t], nums, tn[:, t], eps=eps, iters=K, reach=rho, mass_q=w[t], want_col_err=True,
                                 want_self_err=True, want_transported=True)
        assert one['col_err'].tobytes() == col_err[t].tobytes(), (label, t)
        assert one['self_err'].tobytes() == self_err[t].tobytes(), (label, t)
        assert one['transported'].tobytes() == moved[t].tobytes(), (label, t)
        for b in range(B):
            total += one['divergence'][b] / (H * B)
        row = []
        for b in range(B):
            out = R.pair64(pred[b, t, :nums[b]], tg[b, t, :tn[b, t]], float(eps[b]), float(rho[b]), float(w[t, b]), K, want_plans=True)
            row.append((out[9], out[10], out[0]))
        plans.append(row)
    np.testing.assert_array_equal(e.get_weights(), w0)              # neither mode moved the weights
    e.close()
    rel = abs(loss - total) / abs(total)
    print('[unbalanced] %s: loss %.15e, cloud_divergence on the predicted states %.15e, rel %.2e; col_err %s self_err %s transported %s'
          % (label, loss, total, rel, col_err.ravel(), self_err.ravel(), moved.ravel()))
    assert rel <= 1e-12
    assert none is None and abs(loss_eval - loss) < 1e-9
    assert ('k_aggregate_tape' in ran) == (tape == 'mfma'), ran
    assert not any('divergence' in name or 'sweeps' in name for name in ran)      # no dispatch variant
    assert loss2 == loss and col_err2.tobytes() == col_err.tobytes() and self_err2.tobytes() == self_err.tobytes()
    assert moved2.tobytes() == moved.tobytes()
    np.testing.assert_array_equal(grad2, grad)
    if mass == 'unit':
        assert ((moved > 0) & (moved <= 1)).all(), moved
    ref_loss, _, grads, _ = R.train_divergence64(W, st, kw.get('states_delta'), kw['attrs'], nums, kw['particle_dens'], tg, tn, plans,
                                                 actions=kw.get('actions'))
    rel = abs(loss - ref_loss) / abs(ref_loss)
    print('[unbalanced] %s: float64 restatement %.9e, rel %.2e' % (label, ref_loss, rel))
    ref_blob = U.blob64(grads)
    off, worst = 0, 0.0
    failed = []
    for key, shape in weights.STATE_DICT_KEYS:
        n = int(np.prod(shape))
        a, b = grad[off:off + n].astype(np.float64), np.asarray(ref_blob[off:off + n], np.float64)
        scale = max(np.abs(b).max(), 1e-8)
        err = float(np.abs(a - b).max())
        worst = max(worst, err / scale)
        print('[unbalanced] %s %-45s %.3e of the largest gradient' % (label, key, err / scale))
        if not err < GRAD_REL * scale + 1e-9:
            failed.append((key, err / scale))
        off += n
    print('[unbalanced] %s: worst tensor %.3e' % (label, worst))
    assert rel < LOSS_REL
    assert not failed, (label, failed)


def test_an_infinite_reach_is_the_balanced_step_bit_for_bit(golden):
    for impulses in ('data', 'actions'):
        kw = GT.case(impulses)
        H = kw['states'].shape[1] - 1
        e = GT.new_engine(golden.weights_seed0)
        e.train_begin(H, 1e-3, 0.9)
        want = e.train_step_divergence(mode='grad', want_grad=True, want_err=True, **kw)
        got = e.train_step_divergence(mode='grad', want_grad=True, want_err=True, reach=np.inf, mass_q=1.0, **kw)
        e.close()
        assert got[0] == want[0]
        for a, b in zip(got[1:4], want[1:]):
            assert a.tobytes() == b.tobytes()
        assert np.abs(got[4] - 1.0).max() <= 4e-16


def test_eval_leaves_the_session_alone_and_updates_move_the_weights(golden):
    kw = case('actions', 'count')
    H = kw['states'].shape[1] - 1
    e = GT.new_engine(golden.weights_seed0)
    e.train_begin(H, 1e-3, 0.9)
    w0 = e.get_weights().copy()
    first = e.train_step_divergence(mode='update', **kw)[0]          # Adam state and iteration count now hold one step
    w1 = e.get_weights().copy()
    evals = [e.train_step_divergence(mode='eval', **kw)[0] for _ in range(2)]
    np.testing.assert_array_equal(e.get_weights(), w1)
    second = e.train_step_divergence(mode='update', **kw)[0]
    w2 = e.get_weights().copy()
    e.close()
    e = GT.new_engine(golden.weights_seed0)
    e.train_begin(H, 1e-3, 0.9)
    plain = [e.train_step_divergence(mode='update', **kw)[0] for _ in range(2)]
    w2_plain = e.get_weights().copy()
    e.close()
    print('[unbalanced] updates: %s, evaluations in between: %s' % ([first, second], evals))
    assert evals[0] == evals[1] == second and plain == [first, second]
    np.testing.assert_array_equal(w2, w2_plain)
    assert np.isfinite([first, second]).all() and np.isfinite(w2).all()
    assert np.abs(w1 - w0).max() > 1e-4 and np.abs(w2 - w1).max() > 1e-5
    # the balanced step from the same weights moves them elsewhere: the reach reached the kernels
    e = GT.new_engine(golden.weights_seed0)
    e.train_begin(H, 1e-3, 0.9)
    balanced = e.train_step_divergence(mode='update', **GT.case('actions'))[0]
    e.close()
    assert balanced != first


def test_refusals_reach_no_kernel(golden):
    kw = case('data', 'unit')
    H, B = kw['states'].shape[1] - 1, kw['states'].shape[0]
    e = GT.new_engine(golden.weights_seed0)
    e.train_begin(H, 1e-3, 0.9)
    good = e.train_step_divergence(mode='eval', **kw)[0]
    w0 = e.get_weights().copy()
    eps = kw['eps']
    bad_w = np.ones((H, B))
    bad_w[1, 0] = 8.5
    for change, word in ((dict(reach=0.0), 'rho'), (dict(reach=eps / 1025), 'rho'), (dict(reach=np.nan), 'rho'), (dict(mass_q=bad_w), 'mass_q'),
                         (dict(mass_q=0.1), 'mass_q'), (dict(reach=np.inf, mass_q=0.6), 'balanced')):
        e.dispatch_reset()
        marks = e.last_dispatch()
        with pytest.raises(DrpError, match=word):
            e.train_step_divergence(mode='update', **dict(kw, **change))
        assert e.last_dispatch() == marks                             # refused on the host: not even the forward pass ran
        np.testing.assert_array_equal(e.get_weights(), w0)
        assert e.train_step_divergence(mode='eval', **kw)[0] == good
    e.close()


def test_run_batch_and_train_carry_the_reach_and_log_the_transported_share(golden):
    st, sd, ac, at, nums, dens, tg, tn = T.train_batch()
    model = GT._model(golden)
    model.engine.set_camera(*A.camera_args())
    H = st.shape[1] - 1
    opt = TG.DeviceAdam(model, 1e-3, betas=(0.9, 0.999), n_rollout=H)
    data = TG.PaddedBatch((st, sd, at, nums, dens, None, tg, tn))
    data.actions = ac
    eps = TG.transport_eps(dens)
    for mass in TG.SINKHORN_MASSES:
        stats = {}
        got = TG.run_batch(model, opt, data, 'valid', loss='sinkhorn', impulses='actions', sinkhorn_reach_scale=REACH_SCALE,
                           sinkhorn_mass=mass, stats=stats)
        want = model.engine.train_step_divergence(st, at, nums, dens, tg, tn, eps, K, actions=ac, mode='eval', want_err=True,
                                                  reach=REACH_SCALE * eps, mass_q=TG.sinkhorn_mass_q(mass, nums, tn))
        assert got == want[0] and np.isfinite(got) and stats['transported'] == float(want[4].mean()), mass
    assert got != TG.run_batch(model, opt, data, 'valid', loss='sinkhorn', impulses='actions')
    cfg = TG.default_config()
    cfg['train'].update(n_rollout=H, lr=2e-4, ckp_per_iter=10, log_per_iter=1, adam_beta1=0.9)
    w0 = model.engine.get_weights().copy()
    lines = []
    res = TG.train(cfg, model, {'train': [data], 'valid': [data]}, n_epoch=1, loss='sinkhorn', impulses='actions', log=lines.append,
                   sinkhorn_reach_scale=REACH_SCALE, sinkhorn_mass='count')
    print('[unbalanced] train(sinkhorn_reach_scale=4, sinkhorn_mass=\'count\'): %s' % (lines,))
    assert len(lines) == 2 and all(', transported 0.' in line for line in lines)
    assert np.isfinite([r for (_, _, r) in res['history']]).all()
    assert np.abs(model.engine.get_weights() - w0).max() > 0
    lines = []
    TG.train(cfg, model, {'train': [data], 'valid': [data]}, n_epoch=1, loss='sinkhorn', impulses='actions', log=lines.append)
    assert not any('transported' in line for line in lines)          # the balanced run's log line is what it was
    model.engine.close()

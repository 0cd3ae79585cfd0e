"""GPU: training with the one-to-one matching loss (drp_train_step_loss: ka_match<true> of csrc/k_match.h where drp_train_step
launches kt_mse_grad, alone or behind kc_chamfer<true> for the mix; everything behind the loss gradient unchanged) through the C
ABI, against train_match64 of tests/_match_ref.py.

The matching is a discrete choice, so the float64 restatement takes the CALL'S OWN matching (match_out) for the loss and the 18
tensors, and the matching itself is held to the restatement's optimum separately: its cost on the restatement's float64
predictions may exceed the optimum there by at most 2 r 4e-8 -- 4e-8 is the fp32-vs-float64 drift of a squared distance of a
predicted state that tests/_untracked_ref.py states, and each of the r pairs of either matching can move by that much.
Bounds of the rest: the loss within 1e-4 relative and each tensor within 2e-4 x max |ref| + 1e-9, tests/test_gpu_train_untracked.py's
for the same reverse pass.  The call returns the loss, not its [H][B] terms: the terms are compared through their sum.  Every
figure is printed before it is asserted."""
import ctypes

import numpy as np
import pytest

import _match_ref as R
import _train_actions_ref as A
import _untracked_ref as U
from dyn_res_pile_manip_amd import synthetic as syn
from dyn_res_pile_manip_amd import train_gnn_dyn as TG
from dyn_res_pile_manip_amd import weights
from dyn_res_pile_manip_amd._lib import DrpError
from dyn_res_pile_manip_amd.dataset_gnn_dyn import track_clouds
from dyn_res_pile_manip_amd.engine import Engine
from dyn_res_pile_manip_amd.gnn_dyn import PropNetDiffDenModel

pytestmark = pytest.mark.gpu
LOSS_REL = 1e-4
GRAD_REL = 2e-4


def new_engine(w, engine=None):
    e = Engine(0)
    e.load_weights(weights.blob_from_state_dict(w), 0.08)
    e.set_camera(*A.camera_args())
    if engine is not None:
        e.set_engine(engine)
    return e


def _model(golden):
    import torch
    model = PropNetDiffDenModel(syn.default_config(), True)
    model.load_state_dict({k[2:]: torch.from_numpy(golden.weights_seed0[k]) for k in golden.weights_seed0.files
                           if k.startswith('w/')}, strict=False)
    return model


def case(golden, name, impulses):
    """-> the keyword arguments of Engine.train_step_loss for a fixture batch with data impulses or with pushes"""
    if impulses == 'data':
        st, sd, at, nums, dens, tg, tn = U.untracked_batch(golden, name)
        return dict(states=st, attrs=at, particle_nums=nums, particle_dens=dens, targets=tg, target_nums=tn, states_delta=sd)
    st, acts, at, nums, dens = A.batch(golden, name)
    tg, tn = A.targets_of(golden, name)
    return dict(states=st, attrs=at, particle_nums=nums, particle_dens=dens, targets=tg, target_nums=tn, actions=acts)


def reference(kw, W, matches, kind, weight):
    return R.train_match64(W, kw['states'], kw.get('states_delta'), kw['attrs'], kw['particle_nums'], kw['particle_dens'],
                           kw['targets'], kw['target_nums'], matches=matches, kind=kind, weight=weight, actions=kw.get('actions'))


def assert_grads(grad, ref_blob, label, tag='match'):
    off, worst = 0, 0.0
    for key, shape in weights.STATE_DICT_KEYS:
        n = int(np.prod(shape))
        a, b = grad[off:off + n].astype(np.float64), np.asarray(ref_blob[off:off + n], np.float64)
        scale = max(np.abs(b).max(), 1e-8)
        err = float(np.abs(a - b).max())
        print('[%s] %s %-45s %.3e of the largest gradient' % (tag, label, key, err / scale))
        worst = max(worst, err / scale)
        assert err < GRAD_REL * scale + 1e-9, (label, key, err / scale)
        off += n
    return worst


def assert_matching(match, kw, info, label):
    """a one-to-one matching of r pairs per (step, sample), -1 elsewhere; and no worse than the restatement's own optimum by more
    than the drift of 2 r squared distances"""
    nums, tn = kw['particle_nums'], kw['target_nums']
    H, B, N = match.shape
    for t in range(H):
        for b in range(B):
            n, m = int(nums[b]), int(tn[b, t])
            row = match[t, b]
            on = row[:n][row[:n] >= 0]
            assert (row[n:] == -1).all() and len(on) == min(n, m) and len(set(on.tolist())) == len(on) and on.max() < m
    excess = info['cost'] - info['opt_cost']
    allowed = 2 * info['r'] * R.DRIFT
    print('[match] %s: cost over the float64 optimum, worst %.3e of the %.3e allowed (r = %s); identical to it in %d of %d problems'
          % (label, excess.max(), allowed.flat[int(np.argmax(excess))], info['r'].flat[int(np.argmax(excess))],
             int((excess == 0).sum()), excess.size))
    assert (excess <= allowed).all()


def run_and_check(golden, kw, W, kind, weight, label, tape=None):
    H = kw['states'].shape[1] - 1
    e = new_engine(W, tape)
    e.train_begin(H, 1e-3, 0.9)
    args = dict(kw, loss=kind, match_weight=weight)
    e.dispatch_reset()
    loss, grad, match = e.train_step_loss(mode='grad', want_grad=True, want_match=True, **args)
    ran = e.last_dispatch()
    loss_eval, none, match_eval = e.train_step_loss(mode='eval', want_match=True, **args)
    loss2, grad2, match2 = e.train_step_loss(mode='grad', want_grad=True, want_match=True, **args)
    e.close()
    ref_loss, _, grads, _, info = reference(kw, W, match, kind, weight)
    rel = abs(loss - ref_loss) / ref_loss
    print('[match] %s: loss %.9e, float64 on the same matching %.9e, rel %.2e; eval - grad %.2e' % (label, loss, ref_loss, rel, loss_eval - loss))
    assert rel < LOSS_REL
    assert none is None and abs(loss_eval - loss) < 1e-9             # tests/test_gpu_train_untracked.py's statement of `the same loss`
    np.testing.assert_array_equal(match_eval, match)
    assert_grads(grad, R.blob64(grads), label)
    assert_matching(match, kw, info, label)
    assert loss2 == loss                                            # bit-equal from run to run
    np.testing.assert_array_equal(grad2, grad)
    np.testing.assert_array_equal(match2, match)
    return ran


@pytest.mark.parametrize('kind', R.LOSSES)
@pytest.mark.parametrize('impulses', ['data', 'actions'])
@pytest.mark.parametrize('tape', ['fused', 'mfma'])
@pytest.mark.parametrize('name,wset', U.TRAIN_CASES)
def test_loss_and_gradients_against_float64(golden, name, wset, tape, impulses, kind):
    kw = case(golden, name, impulses)
    ran = run_and_check(golden, kw, U.weights_of(golden, wset), kind, 0.25, '%s %s %s %s %s' % (name, wset, tape, impulses, kind), tape)
    assert ('k_aggregate_tape' in ran) == (tape == 'mfma'), ran


def _kw(batch):
    st, sd, at, nums, dens, tg, tn = batch
    return dict(states=st, attrs=at, particle_nums=nums, particle_dens=dens, targets=tg, target_nums=tn, states_delta=sd)


@pytest.mark.parametrize('kind', R.LOSSES)
def test_single_point_targets(golden, kind):
    """target_nums all 1, M = 1: one predicted row per (step, sample) is matched, every other row's share of the term is 0"""
    run_and_check(golden, _kw(U.single_point_batch(golden)), golden.weights_seed0, kind, 0.5, 'single point ' + kind)


@pytest.mark.parametrize('kind', R.LOSSES)
def test_tiny_unpadded_batch(golden, kind):
    batch = U.tiny_batch()
    assert batch[0].shape == (1, 2, 5, 3) and batch[5].shape == (1, 1, 3, 3)
    run_and_check(golden, _kw(batch), golden.weights_seed0, kind, 0.5, 'tiny ' + kind)


@pytest.mark.parametrize('kind', R.LOSSES)
def test_targets_larger_than_the_prediction(golden, kind):
    """the other orientation: n_q > n_p, every predicted row has a partner and target rows are left over"""
    batch = U.fixture_batch(golden, 'b4_r3')
    tg, tn = R.dense_targets(batch[0], batch[3])
    assert (tn > np.asarray(batch[3])[:, None]).all()
    run_and_check(golden, _kw(batch + [tg, tn]), golden.weights_seed0, kind, 0.5, 'dense targets ' + kind)


# ---- the loss kinds against each other ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('impulses', ['data', 'actions'])
def test_the_chamfer_kind_has_the_bits_of_the_calls_it_generalises(golden, impulses):
    kw = case(golden, 'b4_r3', impulses)
    H = kw['states'].shape[1] - 1
    e = new_engine(golden.weights_seed0)
    e.train_begin(H, 1e-3, 0.9)
    new = e.train_step_loss(loss='chamfer', mode='grad', want_grad=True, **kw)
    pos = (kw['states'], kw['states_delta'] if impulses == 'data' else kw['actions'], kw['attrs'], kw['particle_nums'], kw['particle_dens'],
           kw['targets'], kw['target_nums'])
    old = (e.train_step_untracked if impulses == 'data' else e.train_step_actions)(*pos, mode='grad', want_grad=True)
    new_eval = e.train_step_loss(loss='chamfer', mode='eval', **kw)
    old_eval = (e.train_step_untracked if impulses == 'data' else e.train_step_actions)(*pos, mode='eval')
    e.close()
    assert new[0] == old[0] and new_eval[0] == old_eval[0]
    np.testing.assert_array_equal(new[1], old[1])


@pytest.mark.parametrize('w', [0.5, 0.25, 0.3])
@pytest.mark.parametrize('impulses', ['data', 'actions'])
def test_the_mix_is_the_weighted_sum_of_the_two_losses(golden, impulses, w):
    """(1 - w) chamfer + w match of the two single-loss mode='grad' calls: the loss to rtol 1e-12 for any w (the matching kernel
    weighs a Chamfer-only step's terms in double), the gradient blob within 2e-4 of each tensor's largest entry of the same
    combination"""
    kw = case(golden, 'b2_r5', impulses)
    H = kw['states'].shape[1] - 1
    e = new_engine(golden.weights_seed0)
    e.train_begin(H, 1e-3, 0.9)
    lc, gc = e.train_step_loss(loss='chamfer', mode='grad', want_grad=True, **kw)
    lm, gm, mm = e.train_step_loss(loss='match', mode='grad', want_grad=True, want_match=True, **kw)
    lx, gx, mx = e.train_step_loss(loss='chamfer+match', match_weight=w, mode='grad', want_grad=True, want_match=True, **kw)
    e.close()
    want = (1.0 - w) * lc + w * lm
    print('[match] mix %s w=%g: loss %.15e, combination %.15e, rel %.2e' % (impulses, w, lx, want, abs(lx - want) / want))
    assert abs(lx - want) <= 1e-12 * want
    np.testing.assert_array_equal(mx, mm)                           # the same forward pass, the same matching
    assert_grads(gx, (1.0 - w) * gc.astype(np.float64) + w * gm.astype(np.float64), 'mix %s w=%g' % (impulses, w))


# ---- the optimiser and the training loop --------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['b4_r3', 'b2_r5'])
def test_adam_trajectory(golden, name):
    """three Adam steps on the device follow train_match64 with a numpy Adam (the helper's recipe and the bounds of
    tests/test_gpu_train_untracked.py's test_adam_trajectory)"""
    batch = U.untracked_batch(golden, name)
    lr, beta1 = [float(v) for v in golden.train[name + '/lr_beta1']]
    ref_losses, ref_blob, g0, margin = R.adam_trajectory64(golden, name, lr, beta1)
    model = _model(golden)
    opt = TG.DeviceAdam(model, lr, betas=(beta1, 0.999), n_rollout=batch[0].shape[1] - 1)
    data = batch[:5] + [None] + batch[5:]                           # collate_untracked's layout
    losses = [TG.run_batch(model, opt, data, 'train', loss='match') for _ in range(3)]
    got = model.engine.get_weights().astype(np.float64)
    model.engine.close()
    print('[match] %s losses %s, float64 %s (smallest uniqueness margin on the way %.2e)' % (name, losses, ref_losses, margin))
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


def test_training_lowers_the_matching_loss_and_valid_phase_leaves_weights(golden):
    """tests/test_gpu_train_untracked.py's fixed-batch test with loss='match': same iteration count and lr"""
    model = _model(golden)
    config = syn.default_config()
    config['train'].update({'n_rollout': 3, 'n_history': 1, 'lr': 2e-4, 'adam_beta1': 0.9, 'log_per_iter': 50, 'n_epoch': 6})
    batch = U.untracked_batch(golden, 'b4_r3')
    data = batch[:5] + [None] + batch[5:]
    w0 = model.engine.get_weights().copy()
    with pytest.raises(ValueError, match='no float64 yardstick'):
        TG.train(config, model, {'train': [data], 'valid': [data]}, loss='match', probe_every=1)
    np.testing.assert_array_equal(model.engine.get_weights(), w0)
    res = TG.train(config, model, {'train': [data] * 4, 'valid': [data]}, loss='match')
    rmse_valid = [h[2] for h in res['history'] if h[1] == 'valid']
    print('[match] valid rmse per epoch %s' % rmse_valid)
    assert rmse_valid[-1] < 0.99 * rmse_valid[0] and min(rmse_valid) == rmse_valid[-1]
    assert np.abs(model.engine.get_weights() - w0).max() > 1e-4
    w1 = model.engine.get_weights()
    for loss in R.LOSSES:
        l_a = TG.run_batch(model, None, data, 'valid', loss=loss, match_weight=0.3)
        l_b = TG.run_batch(model, None, data, 'valid', loss=loss, match_weight=0.3)
        assert l_a == l_b
    np.testing.assert_array_equal(model.engine.get_weights(), w1)
    model.engine.close()


@pytest.fixture(scope='module')
def depth_episodes(tmp_path_factory):
    """tests/test_gpu_gnn_frames.py's episodes: depth PNGs and actions.p alone"""
    import os
    import shutil
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
    import make_golden_gnn_frames as mk
    full = str(tmp_path_factory.mktemp('match_tracked'))
    syn.write_episodes(full, **mk.EPISODES)
    d = str(tmp_path_factory.mktemp('match_depth'))
    for ep in os.listdir(full):
        os.makedirs(os.path.join(d, ep))
        for f in os.listdir(os.path.join(full, ep)):
            if not (f.endswith('_particles.npy') or f.endswith('_color.png')):
                shutil.copy(os.path.join(full, ep, f), os.path.join(d, ep, f))
    return d


def test_main_on_depth_episodes_with_the_mix(depth_episodes, tmp_path):
    """main(data='depth', loss='chamfer+match') end to end, then a fixed depth batch: 24 updates lower its loss (the count and lr
    of tests/test_gpu_gnn_frames.py's fixed-batch test) and the valid phase leaves the weights alone"""
    import os
    import dyn_res_pile_manip_amd.planners as P
    from dyn_res_pile_manip_amd.dataset_gnn_dyn import DepthDataset
    cam = (syn.demo_cam_params(), syn.demo_cam_extrinsics())
    cfg = TG.default_config()
    cfg['dataset'].update(n_episode=4, n_timestep=6)
    cfg['train'].update(n_rollout=2, batch_size=4, train_valid_ratio=0.5, lr=2e-4, ckp_per_iter=2, log_per_iter=1)
    out = str(tmp_path / 'run')
    eng = Engine(0)
    with pytest.raises(ValueError, match='no float64 yardstick'):
        TG.main(cfg, data_root=depth_episodes, train_dir=out, engine=eng, data='depth', loss='chamfer+match', probe_every=2)
    with pytest.raises(ValueError, match='contradicts'):
        TG.main(cfg, data_root=depth_episodes, train_dir=out, engine=eng, data='depth', loss='mse')
    assert not os.path.exists(out)
    result, d = TG.main(cfg, data_root=depth_episodes, train_dir=out, threads=4, n_epoch=1, engine=eng, data='depth',
                        loss='chamfer+match', match_weight=0.4)
    assert d == out and os.path.exists(os.path.join(out, 'net_best.pth'))
    rmse = [r for (_, ph, r) in result['history'] if ph in ('train', 'valid')]
    assert len(rmse) == 2 and np.isfinite(rmse).all() and np.isfinite(result['best_valid_loss'])
    # a fixed batch
    cfg['train'].update(n_rollout=3, adam_beta1=0.9)
    model = PropNetDiffDenModel(cfg, engine=eng)
    model.load_state_dict(weights.random_state_dict(seed=0, predictor_scale=1.0))
    ds = DepthDataset(depth_episodes, cfg, 'train', cam, engine=eng)
    eng.set_camera(P.world2cam_affine(np.asarray(cam[1], dtype=np.float64)), 24.0, cam[0])
    np.random.seed(2)
    data = ds.get_batch([0, 2, 5, 7])
    assert data.depth_only
    opt = TG.DeviceAdam(model, 2e-4, betas=(0.9, 0.999), n_rollout=3)
    kw = dict(n_rollout=3, loss='chamfer+match', impulses='actions', match_weight=0.4)
    with pytest.raises(ValueError, match='depth-only'):
        TG.run_batch(model, opt, data, 'train', 3, loss='match')           # zero impulses are never trained on
    w0 = model.engine.get_weights().copy()
    before = TG.run_batch(model, opt, data, 'valid', **kw)
    np.testing.assert_array_equal(model.engine.get_weights(), w0)          # the valid phase leaves the weights alone
    losses = [TG.run_batch(model, opt, data, 'train', **kw) for _ in range(24)]
    after = TG.run_batch(model, opt, data, 'valid', **kw)
    print('[match] depth batch %s x %s: eval loss %.6e -> %.6e after 24 updates' % (data[0].shape, data[6].shape, before, after))
    assert np.isfinite(losses).all() and after < before
    assert np.abs(model.engine.get_weights() - w0).max() > 1e-4
    eng.close()


def test_matching_steps_leave_the_mse_and_chamfer_steps_their_bits(golden):
    batch = U.untracked_batch(golden, 'b2_r5')
    kw = _kw(batch)
    H = batch[0].shape[1] - 1
    runs = []
    for disturb in (False, True):
        e = new_engine(golden.weights_seed0)
        e.train_begin(H, 1e-3, 0.9)
        first = e.train_step_untracked(*batch, mode='grad', want_grad=True)
        if disturb:
            for kind in R.LOSSES:
                e.train_step_loss(loss=kind, match_weight=0.3, mode='grad', want_grad=True, want_match=True, **kw)
                e.train_step_loss(loss=kind, match_weight=0.3, mode='eval', **kw)
        mse = e.train_step(*batch[:5], mode='grad', want_grad=True)
        cham = e.train_step_untracked(*batch, mode='grad', want_grad=True)
        upd = [e.train_step_untracked(*batch, mode='update')[0] for _ in range(2)]
        runs.append((first, mse, cham, upd, e.get_weights().copy()))
        e.close()
    for a, b in zip(runs[0][:3], runs[1][:3]):
        assert a[0] == b[0]
        np.testing.assert_array_equal(a[1], b[1])
    assert runs[0][3] == runs[1][3]
    np.testing.assert_array_equal(runs[0][4], runs[1][4])
    assert runs[0][0][0] == runs[0][2][0]
    np.testing.assert_array_equal(runs[0][0][1], runs[0][2][1])


# ---- what the feature is for --------------------------------------------------------------------------------------------------
def test_a_collapse_that_chamfer_cannot_see():
    """A target lattice of 64 points.  The prediction's first half lies on the lattice's first 32 points, off by a fixed few
    millimetres; its second half crowds around ONE target (half the mass on one point), within 5e-4 of it.  Collapsing the clump
    further, to within 5e-5, changes cloud_chamfer's fwd by less than 1 % -- every crowded row has its near target either way --
    and bwd not at all in its first four digits: the 32 targets without a predicted row are as far from the pile as before, and
    that is all bwd says.  The matching distance pairs the 32 crowded rows with those 32 empty targets: it is two hundred
    times fwd, and it RISES as the rows leave them."""
    g = np.stack(np.meshgrid(*[np.arange(4)] * 3, indexing='ij'), -1).reshape(-1, 3)
    q = (0.2 + 0.02 * g).astype(np.float32)                         # 64 targets, pitch 0.02
    rng = np.random.default_rng(4)
    noise = (0.008 * (rng.random((32, 3)) - 0.5)).astype(np.float32)
    spread = (rng.random((32, 3)) - 0.5).astype(np.float32)
    def pred(radius):
        p = q.copy()
        p[:32] += noise
        p[32:] = q[0] + np.float32(radius) * spread                 # rows 32.. crowd around target 0
        return p
    e = Engine(0)
    loose, tight = pred(5e-4), pred(5e-5)
    cl, ct = e.cloud_chamfer(loose, q), e.cloud_chamfer(tight, q)
    ml, mt = e.cloud_match(loose, q), e.cloud_match(tight, q)
    e.close()
    df = abs(ct['fwd'][0] - cl['fwd'][0]) / cl['fwd'][0]
    dt = abs(ct['total'][0] - cl['total'][0]) / cl['total'][0]
    print('[match] collapse: chamfer fwd %.6e -> %.6e (%.3f %%), total %.6e -> %.6e (%.4f %%); match %.6e -> %.6e'
          % (cl['fwd'][0], ct['fwd'][0], 100 * df, cl['total'][0], ct['total'][0], 100 * dt, ml['match'][0], mt['match'][0]))
    assert df < 0.01 and dt < 0.01
    assert mt['match'][0] > ml['match'][0]
    assert ml['match'][0] > 100 * cl['fwd'][0]


def _window(frames, rng):
    """frames [T, n, 3] -> (clouds [T, n + 3, 3]: every frame after the first moved by JITTER and shuffled, rubbish in the padding;
    inv [T, n]: the row of frame t that holds particle i)"""
    T, n, _ = frames.shape
    shuffles = np.stack([np.arange(n)] + [rng.permutation(n) for _ in range(T - 1)])
    clouds = np.zeros((T, n + 3, 3), np.float32)
    clouds[:, n:] = 7.0                                             # padding is never read
    for t in range(T):
        clouds[t, :n] = (frames[t] + (U.JITTER * rng.standard_normal((n, 3)) if t else 0.0))[shuffles[t]]
    return clouds, np.argsort(shuffles, axis=1)


def test_track_clouds_recovers_a_shuffled_window(golden):
    """A recorded frame seen four times, each view shuffled and moved by JITTER (a resting pile re-sampled): the chained partners
    ARE the shuffles, wherever the host oracle finds each pair's matching unique by MARGIN_MIN (asserted here on the reference),
    and the window is tracked again.  A recorded window whose pile MOVES between frames by more than its spacing: the partners
    are the oracle's optimum still, chained -- the least-cost correspondence, which is then not the physical one (printed).
    Unequal counts are refused."""
    st, _, _, nums, _ = U.fixture_batch(golden, 'b4_r3')
    rng = np.random.default_rng(12)
    e = Engine(0)
    for b in (1, 3):                                                # the two samples of 64 particles
        n, T = int(nums[b]), st.shape[1]
        for moving in (False, True):
            frames = st[b, :, :n] if moving else np.repeat(st[b, :1, :n], T, axis=0)
            clouds, inv = _window(frames, rng)
            ref = R.match64(clouds[:-1], clouds[1:], [n] * (T - 1), [n] * (T - 1))
            assert ref['margin'].min() >= R.MARGIN_MIN
            perms = track_clouds(e, clouds, [n] * T)
            chain = [np.arange(n)]
            for t in range(1, T):
                chain.append(ref['match_pq'][t - 1][chain[-1]])
            np.testing.assert_array_equal(perms, np.stack(chain))   # the oracle's partners, chained
            print('[match] window of sample %d, %s: uniqueness margins %s, %d of %d rows are the physical particle'
                  % (b, 'moving' if moving else 'resting', ref['margin'], int((perms == inv).sum()), inv.size))
            if not moving:
                np.testing.assert_array_equal(perms, inv)           # and they are the particles
                tracked = np.stack([clouds[t, perms[t]] for t in range(T)])
                assert np.abs(tracked - frames).max() < 6 * U.JITTER
    with pytest.raises(ValueError, match='equal'):
        track_clouds(e, clouds, [n, n - 1, n, n])
    e.close()


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals(golden):
    batch = U.untracked_batch(golden, 'b2_r5')
    H = batch[0].shape[1] - 1
    e = new_engine(golden.weights_seed0)
    e._n_rollout = H
    st, sd, at, nums, dens, tg, tn = [np.ascontiguousarray(a) for a in batch]
    acts = np.ascontiguousarray(A.batch(golden, 'b2_r5')[1])
    B, _, N, _ = st.shape
    M = tg.shape[2]
    FP, IP = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32)
    loss = ctypes.c_double()

    def call(sd_=sd, acts_=None, tg_=tg, tn_=tn, M_=M, kind=2, w=0.5, N_=N, st_=st, at_=at):
        f = lambda a, T: None if a is None else a.ctypes.data_as(T)
        return e.lib.drp_train_step_loss(e.h, f(st_, FP), f(sd_, FP), f(acts_, FP), f(at_, FP), f(nums, IP), f(dens, FP), B, N_, f(tg_, FP),
                                         f(tn_, IP), M_, kind, w, 0, ctypes.byref(loss), None, None)
    assert call() == -2                                             # DRP_ESTATE before train_begin
    e.train_begin(H, 1e-3, 0.9)
    assert call() == 0
    good = loss.value
    zero, big = tn.copy(), tn.copy()
    zero[1, 2], big[0, 0] = 0, M + 1
    wide_t = np.zeros((B, H, 1025, 3), np.float32)
    wide_s, wide_d, wide_a = np.zeros((B, H + 1, 1025, 3), np.float32), np.zeros((B, H, 1025, 3), np.float32), np.zeros((B, H + 1, 1025), np.float32)
    for kwargs in (dict(tg_=None), dict(tn_=None), dict(tn_=zero), dict(tn_=big), dict(M_=0),
                   dict(tg_=wide_t, M_=1025),                        # a count above KA_MAX_POINTS ...
                   dict(st_=wide_s, sd_=wide_d, at_=wide_a, N_=1025),
                   dict(tg_=wide_t, M_=1025, kind=3),
                   dict(kind=0), dict(kind=4), dict(kind=-1),        # the MSE has its own call
                   dict(kind=3, w=0.0), dict(kind=3, w=1.0), dict(kind=3, w=-0.1), dict(kind=3, w=float('nan')),
                   dict(sd_=sd, acts_=acts), dict(sd_=None, acts_=None)):    # both or neither impulse source
        assert call(**kwargs) == -1, kwargs                          # DRP_EINVAL
    assert call(tg_=wide_t, M_=1025, kind=1) == 0                   # (the Chamfer kind keeps its own limit of 4096)
    assert call(kind=2, w=7.0) == 0 and loss.value == good          # match_weight is read by the mix only; the context is as it was
    assert call(kind=3, w=0.5) == 0
    assert call(sd_=None, acts_=acts) == 0
    with pytest.raises(DrpError, match='1025'):
        e.train_step_loss(st, at, nums, dens, wide_t, tn, states_delta=sd, loss='match')
    with pytest.raises(ValueError):
        e.train_step_loss(st, at, nums, dens, tg, tn, states_delta=sd, actions=acts)
    with pytest.raises(ValueError, match='loss must be one of'):
        e.train_step_loss(st, at, nums, dens, tg, tn, states_delta=sd, loss='emd')
    e.close()

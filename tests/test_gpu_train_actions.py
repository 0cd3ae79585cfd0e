"""GPU: training through the push (drp_train_step_actions, drp_train_grad_f64_actions) through the C ABI, against train_actions64 of
tests/_train_actions_ref.py.

Bounds: the loss within 1e-4 relative and each of the 18 parameter tensors within 2e-4 x max |ref| + 1e-9 (the bounds of
tests/test_gpu_train_untracked.py); the float64 call within 1e-10 x the largest magnitude of the compared tensor (row y3's
bound, tests/test_gpu_train_f64.py).  tests/test_train_actions_host.py holds, for every batch used here, every row's distance to
a decision of gen_s_delta above 1e-5 and every Chamfer arg-min margin above 1e-7, so the fp32 pass takes the reference's
branches.  Every figure is printed before it is asserted."""
import ctypes

import numpy as np
import pytest

import _train_actions_ref as A
from dyn_res_pile_manip_amd import synthetic as syn
from dyn_res_pile_manip_amd import train_gnn_dyn as TG
from dyn_res_pile_manip_amd import weights
from dyn_res_pile_manip_amd._lib import DrpError
from dyn_res_pile_manip_amd.engine import Engine
from dyn_res_pile_manip_amd.gnn_dyn import PropNetDiffDenModel

pytestmark = pytest.mark.gpu
LOSS_REL = A.LOSS_REL
GRAD_REL = A.GRAD_REL
TOL64 = 1e-10


def new_engine(w, engine=None, camera=True):
    e = Engine(0)
    e.load_weights(weights.blob_from_state_dict(w), 0.08)
    if camera:
        e.set_camera(*A.camera_args())
    if engine is not None:
        e.set_engine(engine)
    return e


def _model(golden):
    import torch
    model = PropNetDiffDenModel(syn.default_config(), True)
    model.load_state_dict({k[2:]: torch.from_numpy(golden.weights_seed0[k]) for k in golden.weights_seed0.files
                           if k.startswith('w/')}, strict=False)
    model.engine.set_camera(*A.camera_args())
    return model


def grad_errors(grad, ref_blob):
    """per tensor: (key, max |err|, max |ref|)"""
    out, off = [], 0
    for key, shape in weights.STATE_DICT_KEYS:
        n = int(np.prod(shape))
        a, b = np.asarray(grad[off:off + n], np.float64), ref_blob[off:off + n]
        out.append((key, float(np.abs(a - b).max()), float(np.abs(b).max())))
        off += n
    return out


def assert_grads(grad, ref_blob, label):
    worst = 0.0
    for key, err, ref in grad_errors(grad, ref_blob):
        scale = max(ref, 1e-8)
        print('[train-actions] %s %-45s %.3e of the largest gradient' % (label, key, err / scale))
        worst = max(worst, err / scale)
    for key, err, ref in grad_errors(grad, ref_blob):
        assert err < GRAD_REL * max(ref, 1e-8) + 1e-9, (label, key, err / max(ref, 1e-8))
    return worst


def full_batch(golden, name, loss):
    b = A.batch(golden, name)
    return b + (A.targets_of(golden, name) if loss == 'chamfer' else [None, None])


# ---- 1, 6: against float64, the same bits from run to run, the eval loss, an MSE step's marks ---------------------------------
@pytest.mark.parametrize('loss', ['mse', 'chamfer'])
@pytest.mark.parametrize('tape', ['fused', 'mfma'])
@pytest.mark.parametrize('name,wset', A.TRAIN_CASES)
def test_loss_and_gradients_against_float64(golden, name, wset, tape, loss):
    b = full_batch(golden, name, loss)
    ref_loss, _, ref_blob, _, _ = A.reference(golden, name, wset, loss)
    H = b[0].shape[1] - 1
    e = new_engine(A.weights_of(golden, wset), tape)
    e.train_begin(H, 1e-3, 0.9)
    e.dispatch_reset()
    got, grad = e.train_step_actions(*b, mode='grad', want_grad=True)
    ran = e.last_dispatch()
    loss_eval, none = e.train_step_actions(*b, mode='eval')
    got2, grad2 = e.train_step_actions(*b, mode='grad', want_grad=True)
    e.close()
    rel = abs(got - ref_loss) / ref_loss
    print('[train-actions] %s %s %s %s: loss %.9e, float64 %.9e, rel %.2e' % (name, wset, tape, loss, got, ref_loss, rel))
    assert ('k_aggregate_tape' in ran) == (tape == 'mfma'), ran
    assert rel < LOSS_REL
    # The forward without the tape is another instantiation of the step kernels and not bit-equal (measured: the same bits in
    # most cases, 2.9e-13 apart in one), so no equality.  The bound is every predicted coordinate one fp32 ulp off in the same
    # direction (coordinates are below 1: 2^-24): a mean of squared distances d moves by at most 2 ulp mean|d| <= 2 ulp sqrt(loss),
    # and the Chamfer loss is two such means.
    drift = 4 * 2.0 ** -24 * np.sqrt(got)
    print('[train-actions] eval loss - grad-mode loss: %.3e (bound %.3e)' % (loss_eval - got, drift))
    assert none is None and abs(loss_eval - got) <= drift
    assert_grads(grad, ref_blob, '%s %s %s %s' % (name, wset, tape, loss))
    assert got2 == got
    np.testing.assert_array_equal(grad2, grad)                      # bit-equal from run to run
    if loss == 'mse':                                               # no dispatch variant of its own: an MSE step's marks
        sd = np.zeros(b[0].shape[:1] + (H,) + b[0].shape[2:], np.float32)
        e = new_engine(A.weights_of(golden, wset), tape)
        e.train_begin(H, 1e-3, 0.9)
        e.dispatch_reset()
        e.train_step(b[0], sd, b[2], b[3], b[4], mode='grad')
        ran_mse = e.last_dispatch()
        e.close()
        assert ran == ran_mse


# ---- 2: the mask -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tape', ['fused', 'mfma'])
def test_the_mask(golden, tape):
    """every push runs from (-3, 0) to (3, 0), over the camera-frame origin where collate_fn's zero rows sit; sample 1's real
    rows lie around them (z = 0), so the zero rows are in real rows' neighbour lists and a moved one would show in the
    gradients as well as in the predicted states"""
    b = A.batch(golden, 'mask')
    st, ac, at, nums, dens = b
    B, T1, N, _ = st.shape
    H = T1 - 1
    ref_loss, _, ref_blob, _, _ = A.reference(golden, 'mask', 'trained')
    e = new_engine(golden.weights_trained, tape)
    e.train_begin(H, 1e-3, 0.9)
    got, grad = e.train_step_actions(*b, mode='grad', want_grad=True)
    states = e.debug_fetch('train_states', (B, H, N, 3))
    sdelta = e.debug_fetch('train_sdelta', (H, B, N, 3))
    # the data path fed these impulses: zero on the padded rows, so every row of every predicted state must have the same bits
    loss_data, _ = e.train_step(st, np.ascontiguousarray(sdelta.transpose(1, 0, 2, 3)), at, nums, dens, mode='grad')
    states_data = e.debug_fetch('train_states', (B, H, N, 3))
    e.close()
    for j, n in enumerate(nums):
        assert (sdelta[:, j, n:].view(np.uint32) == 0).all()        # +0.0f exactly
    assert np.abs(sdelta).max() > 0.05                              # and the push did move real rows
    np.testing.assert_array_equal(states, states_data)
    assert got == loss_data
    rel = abs(got - ref_loss) / ref_loss
    print('[train-actions] mask %s: loss rel %.2e' % (tape, rel))
    assert rel < LOSS_REL
    assert_grads(grad, ref_blob, 'mask ' + tape)


def test_an_unmasked_pass_would_fail_the_bounds(golden):
    """the float64 loop with the zero rows given gen_s_delta's impulse (what an unmasked kernel computes) fails case 1's bounds:
    sample 1 of the mask case lies around the camera-frame origin, its zero rows are senders of real rows
    (tests/test_train_actions_host.py counts the edges), so an impulse on them reaches the loss and every weight"""
    _, _, ref_blob, _, _ = A.reference(golden, 'mask', 'trained')
    bad_loss, _, bad_blob, _, info = A.reference(golden, 'mask', 'trained', masked=False)
    nums = A.batch(golden, 'mask')[3]
    assert max(np.abs(info['sdelta'][j, :, n:]).max() for j, n in enumerate(nums) if n < 24) > 0.05    # the zero rows did move
    bad = grad_errors(bad_blob, ref_blob)
    print('[train-actions] mask: an unmasked pass is off by %.3e of a tensor\'s largest gradient'
          % max(err / max(ref, 1e-8) for _, err, ref in bad))
    assert any(err >= GRAD_REL * max(ref, 1e-8) + 1e-9 for _, err, ref in bad)


# ---- 3: the same bits as data at H = 1 -------------------------------------------------------------------------------------
@pytest.mark.parametrize('tape', ['fused', 'mfma'])
def test_same_bits_as_data_at_one_step(golden, tape):
    st, ac, at, nums, dens = A.batch(golden, 'b3_n24')
    st, ac, at = np.ascontiguousarray(st[:, :2]), np.ascontiguousarray(ac[:, :1]), np.ascontiguousarray(at[:, :2])
    e = new_engine(golden.weights_trained, tape)
    e.train_begin(1, 1e-3, 0.9)
    sd = e.gen_s_delta(st[:, 0], ac[:, 0])
    for j, n in enumerate(nums):
        sd[j, n:] = 0.0
    la, ga = e.train_step_actions(st, ac, at, nums, dens, mode='grad', want_grad=True)
    ld, gd = e.train_step(st, sd[:, None], at, nums, dens, mode='grad', want_grad=True)
    e.close()
    assert np.abs(sd).max() > 0.01
    assert la == ld
    np.testing.assert_array_equal(ga, gd)


# ---- 4: strided loops and the state chain; the smallest batch ------------------------------------------------------------------
@pytest.mark.parametrize('name,wset', [('n300', 'seed0'), ('n300', 'trained'), ('tiny', 'trained')])
def test_large_and_tiny_batches(golden, name, wset):
    b = A.batch(golden, name)
    assert b[0].shape[:3] == ((2, 3, 300) if name == 'n300' else (1, 2, 5))
    ref_loss, _, ref_blob, _, _ = A.reference(golden, name, wset)
    e = new_engine(A.weights_of(golden, wset))
    e.train_begin(b[0].shape[1] - 1, 1e-3, 0.9)
    got, grad = e.train_step_actions(*b, mode='grad', want_grad=True)
    e.close()
    rel = abs(got - ref_loss) / ref_loss
    print('[train-actions] %s %s: loss rel %.2e' % (name, wset, rel))
    assert rel < LOSS_REL
    assert_grads(grad, ref_blob, '%s %s' % (name, wset))


# ---- 5: a push that misses every particle ------------------------------------------------------------------------------------
def test_a_push_that_misses_is_the_data_path_with_zero_impulses(golden):
    st, ac, at, nums, dens = A.batch(golden, 'b3_n24')
    ac = np.empty_like(ac)
    ac[:] = np.array([4.9, 4.9, 6.0, 6.0], np.float32)              # starts beyond every pile and points away: u < 0 on every row
    H = ac.shape[1]
    e = new_engine(golden.weights_trained)
    e.train_begin(H, 1e-3, 0.9)
    la, ga = e.train_step_actions(st, ac, at, nums, dens, mode='grad', want_grad=True)
    sdelta = e.debug_fetch('train_sdelta', (H,) + st.shape[:1] + st.shape[2:])
    ld, gd = e.train_step(st, np.zeros(st.shape[:1] + (H,) + st.shape[2:], np.float32), at, nums, dens, mode='grad', want_grad=True)
    e.close()
    assert (sdelta == 0).all()
    assert la == ld
    np.testing.assert_array_equal(ga, gd)


# ---- 6: an actions step leaves the MSE and float64 paths their bits -------------------------------------------------------------
def test_actions_steps_leave_the_mse_and_f64_paths_their_bits(golden):
    b = A.batch(golden, 'b2_r5')
    data = A.U.fixture_batch(golden, 'b2_r5')
    H = b[0].shape[1] - 1
    runs = []
    for disturb in (False, True):
        e = new_engine(golden.weights_seed0)
        e.train_begin(H, 1e-3, 0.9)
        mse0 = e.train_step(*data, mode='grad', want_grad=True)
        f0 = e.train_grad_f64(*data)
        if disturb:
            e.train_step_actions(*b, mode='grad', want_grad=True)
            e.train_step_actions(*(b + A.targets_of(golden, 'b2_r5')), mode='eval')
            e.train_grad_f64_actions(*b)
        mse = e.train_step(*data, mode='grad', want_grad=True)
        f64 = e.train_grad_f64(*data)
        runs.append((mse, f64))
        assert mse0[0] == mse[0] and f0[0] == f64[0]
        np.testing.assert_array_equal(mse0[1], mse[1])
        np.testing.assert_array_equal(f0[2], f64[2])
        e.close()
    assert runs[0][0][0] == runs[1][0][0] and runs[0][1][0] == runs[1][1][0]
    np.testing.assert_array_equal(runs[0][0][1], runs[1][0][1])
    np.testing.assert_array_equal(runs[0][1][1], runs[1][1][1])
    np.testing.assert_array_equal(runs[0][1][2], runs[1][1][2])


# ---- 7: the float64 call and the probe ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,wset', A.TRAIN_CASES + [('mask', 'trained')])
def test_f64_call_matches_the_float64_reference(golden, name, wset):
    b = A.batch(golden, name)
    ref_loss, ref_terms, ref_blob, ref_gs, _ = A.reference(golden, name, wset)
    e = new_engine(A.weights_of(golden, wset))
    loss, terms, grad, gs = e.train_grad_f64_actions(*b, want_state=True)
    loss2, _, grad2 = e.train_grad_f64_actions(*b)
    e.close()
    gs = A.real_rows(gs, b[3])
    figures = [('loss', abs(loss - ref_loss) / abs(ref_loss)), ('loss_terms', np.abs(terms - ref_terms).max() / np.abs(ref_terms).max()),
               ('grad_state', np.abs(gs - ref_gs).max() / np.abs(ref_gs).max())]
    figures += [(k, err / max(ref, 1e-300)) for k, err, ref in grad_errors(grad, ref_blob)]
    for k, v in figures:
        print('[train-actions] f64 %s %s %-45s %.3e' % (name, wset, k, v))
    for k, v in figures:
        assert v <= TOL64, (k, v)
    assert loss2 == loss
    np.testing.assert_array_equal(grad2, grad)


@pytest.mark.parametrize('tape', ['fused', 'mfma'])
def test_train_gradient_probe_with_actions(golden, tape):
    b = A.batch(golden, 'b3_n24')
    e = new_engine(golden.weights_trained, tape)
    e.train_begin(b[0].shape[1] - 1, 1e-3, 0.9)
    w0 = e.get_weights().copy()
    pr = e.train_gradient_probe(b[0], None, b[2], b[3], b[4], actions=b[1])
    np.testing.assert_array_equal(e.get_weights(), w0)
    e.close()
    assert pr['tape'] == tape and len(pr['tensors']) == 18
    for key, t in pr['tensors'].items():
        print('[train-actions] probe %s %-45s %.3e' % (tape, key, t['rel']))
    for key, t in pr['tensors'].items():
        assert t['max_abs_err'] < GRAD_REL * t['max_abs_ref'] + 1e-9, key
    assert pr['loss_diff'] < LOSS_REL * pr['loss64']


# ---- 8: the reference fixture ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tape', ['fused', 'mfma'])
def test_reference_fixture(golden, tape):
    g = golden.train_actions
    b = [g[k] for k in ('states', 'actions', 'attrs', 'particle_nums', 'particle_dens')]
    ref_blob = np.concatenate([g['grad/' + k].astype(np.float64).ravel() for k in A.PARAMS])
    e = new_engine(golden.weights_seed0, tape)
    e.train_begin(b[0].shape[1] - 1, 1e-3, 0.9)
    got, grad = e.train_step_actions(*b, mode='grad', want_grad=True)
    e.close()
    rel = abs(got - float(g['loss'])) / float(g['loss'])
    print('[train-actions] fixture %s: loss %.9e, reference %.9e, rel %.2e' % (tape, got, float(g['loss']), rel))
    assert rel < LOSS_REL
    assert_grads(grad, ref_blob, 'fixture ' + tape)


# ---- 9: Adam -----------------------------------------------------------------------------------------------------------------
def _padded(b, extra=()):
    data = TG.PaddedBatch((b[0], None, b[2], b[3], b[4], None) + tuple(extra))
    data.actions = b[1]
    return data


def test_adam_trajectory(golden):
    """three Adam steps on the device follow train_actions64 with a numpy Adam (the bounds of tests/test_gpu_train.py's
    test_adam_trajectory)"""
    b = A.batch(golden, 'b3_n24')
    lr, beta1 = [float(v) for v in golden.train['b4_r3/lr_beta1']]
    ref_losses, ref_blob, g0, _ = A.adam_trajectory64(golden, 'b3_n24', lr, beta1)
    model = _model(golden)
    opt = TG.DeviceAdam(model, lr, betas=(beta1, 0.999), n_rollout=b[0].shape[1] - 1)
    data = _padded(b)
    losses = [TG.run_batch(model, opt, data, 'train', impulses='actions') for _ in range(3)]
    got = model.engine.get_weights().astype(np.float64)
    model.engine.close()
    print('[train-actions] adam losses %s, float64 %s' % (losses, ref_losses))
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


# ---- 10: end to end ----------------------------------------------------------------------------------------------------------
def test_loader_and_training_end_to_end(tmp_path):
    """written synthetic episodes through ParticleDataset, DeviceLoader and UntrackedLoader (batch.actions: the pickled pushes) into
    main(impulses='actions', loss='chamfer'): the validation loss falls, the valid phase leaves the weights alone"""
    import pickle
    from dyn_res_pile_manip_amd.dataset_gnn_dyn import DeviceLoader, ParticleDataset, UntrackedLoader
    root = str(tmp_path / 'episodes')
    syn.write_episodes(root, n_episode=4, n_timestep=4, seed=3)
    cfg = TG.default_config()
    cfg['dataset'].update(n_episode=4, n_timestep=4)
    cfg['train'].update(n_rollout=2, batch_size=2, train_valid_ratio=0.75, lr=2e-4, log_per_iter=50, ckp_per_iter=1000, n_epoch=4)
    cam = (syn.demo_cam_params(), syn.demo_cam_extrinsics())
    eng = Engine(0)
    ds = ParticleDataset(root, cfg, 'train', cam, engine=eng)
    np.random.seed(0)
    direct = ds.get_batch([0, 4])
    loader = DeviceLoader(ds, 2, shuffle=False, chunk=4, threads=2)
    first = next(iter(loader))
    wrapped = next(iter(UntrackedLoader(loader, seed=1)))
    for batch, idx in ((direct, [0, 4]), (first, [0, 1]), (wrapped, [0, 1])):
        assert batch.actions.shape == (2, 2, 4) and batch.actions.dtype == np.float32 and len(batch) in (6, 8)
        for j, i in enumerate(idx):
            ep, t0 = ds.locate(i)
            with open('%s/%d/actions.p' % (root, ep), 'rb') as fp:
                acts = np.asarray(pickle.load(fp))
            np.testing.assert_array_equal(batch.actions[j], acts[t0:t0 + 2].astype(np.float32))
    with pytest.raises(ValueError):
        TG.run_batch(None, None, TG.PaddedBatch(tuple(first)), 'valid', impulses='actions')      # a batch without .actions
    with pytest.raises(ValueError):
        TG.main(cfg, data_root=root, train_dir=str(tmp_path / 'probe'), engine=eng, grad_probe_every=1, loss='chamfer',
                impulses='actions')
    result, _ = TG.main(cfg, data_root=root, train_dir=str(tmp_path / 'run'), chunk=8, threads=2, engine=eng, loss='chamfer',
                        impulses='actions')
    rmse_valid = [h[2] for h in result['history'] if h[1] == 'valid']
    print('[train-actions] valid rmse per epoch %s' % rmse_valid)
    assert len(rmse_valid) == 4 and np.isfinite(rmse_valid).all() and rmse_valid[-1] < rmse_valid[0]
    w1 = eng.get_weights().copy()
    l_a = eng.train_step_actions(wrapped[0], wrapped.actions, wrapped[2], wrapped[3], wrapped[4], wrapped[6], wrapped[7], mode='eval')[0]
    l_b = eng.train_step_actions(wrapped[0], wrapped.actions, wrapped[2], wrapped[3], wrapped[4], wrapped[6], wrapped[7], mode='eval')[0]
    assert l_a == l_b and np.isfinite(l_a)
    np.testing.assert_array_equal(eng.get_weights(), w1)
    eng.close()


# ---- 11: refusals ------------------------------------------------------------------------------------------------------------
def test_refusals(golden):
    b = A.batch(golden, 'b3_n24')
    st, ac, at, nums, dens = [np.ascontiguousarray(a) for a in b]
    B, T1, N, _ = st.shape
    H = T1 - 1
    FP, IP = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32)
    fresh = new_engine(golden.weights_seed0)
    fresh.train_begin(H, 1e-3, 0.9)
    want = fresh.train_step_actions(*b, mode='grad', want_grad=True)
    fresh.close()

    def call(e, ac_):
        loss = ctypes.c_double()
        f = lambda a, T: None if a is None else a.ctypes.data_as(T)
        return e.lib.drp_train_step_actions(e.h, f(st, FP), f(ac_, FP), f(at, FP), f(nums, IP), f(dens, FP), B, N, None, None, 0, 1,
                                            ctypes.byref(loss), None)

    def call64(e, ac_):
        f = lambda a, T: None if a is None else a.ctypes.data_as(T)
        return e.lib.drp_train_grad_f64_actions(e.h, f(st, FP), f(ac_, FP), f(at, FP), f(nums, IP), f(dens, FP), B, N, H, None, None,
                                                None, None)
    zero = ac.copy()
    zero[1, 1, 2:] = zero[1, 1, :2]                                 # a zero-length push in the middle of the batch
    e = new_engine(golden.weights_seed0, camera=False)
    assert call(e, ac) == -2                                        # DRP_ESTATE: no drp_train_begin
    e.train_begin(H, 1e-3, 0.9)
    assert call(e, ac) == -2 and call64(e, ac) == -2                # DRP_ESTATE: no camera
    with pytest.raises(DrpError):
        e.train_step_actions(*b, mode='eval')
    e.set_camera(*A.camera_args())
    got = e.train_step_actions(*b, mode='grad', want_grad=True)
    assert got[0] == want[0]
    np.testing.assert_array_equal(got[1], want[1])
    for bad in (None, zero):
        assert call(e, bad) == -1 and call64(e, bad) == -1          # DRP_EINVAL
        got = e.train_step_actions(*b, mode='grad', want_grad=True)
        assert got[0] == want[0]
        np.testing.assert_array_equal(got[1], want[1])              # the bits of a fresh context
    assert np.isfinite(e.get_weights()).all()
    e.close()

"""GPU: training on a loss of the caller's -- drp_train_predict / drp_train_step_seeded, their float64 pair, the Python composition
(Engine.train_step_custom, train_gradient_probe_custom) and the trainer's callable loss.

Bounds.  The fp32 seam is held to BITS: the forward of drp_train_predict is the forward of drp_train_step_seeded and of
drp_train_step, and behind a seed that has the bits of kt_mse_grad's own everything is the same code, so the gradient blob and the
weights five Adam steps leave are equal bit for bit.  The float64 pair is held to 1e-10 of each tensor's largest entry (the TOL of
tests/test_gpu_train_f64.py: the same expressions in double, another summation order) against the built-in float64 yardstick and
against the restatement with the loss as an argument (tests/_seeded_ref.py).  The probe is held to 2e-4 of each tensor's largest
gradient, the PROBE_TOL every other loss is held to.  Every figure is printed before it is asserted."""
import ctypes

import numpy as np
import pytest

import _f64_train_ref as T
import _seeded_ref as S
import _train_actions_ref as A
from dyn_res_pile_manip_amd import _lib, losses, synthetic as syn, train_gnn_dyn as TG, weights
from dyn_res_pile_manip_amd._lib import DrpError
from dyn_res_pile_manip_amd.engine import Engine
from dyn_res_pile_manip_amd.gnn_dyn import PropNetDiffDenModel
from test_gpu_train_f64 import fixture_batch, hand_made

pytestmark = pytest.mark.gpu
TOL = 1e-10
PROBE_TOL = 2e-4
TAPES = ('fused', 'mfma')
HAND = {'n3_h2': ((3,), 2), 'n5_17_16_h3': ((5, 17, 16), 3), 'n33_h1': ((33,), 1)}


def weights_of(golden, wset):
    return golden.weights_seed0 if wset == 'seed0' else golden.weights_trained


def new_engine(w):
    e = Engine(0)
    e.load_weights(weights.blob_from_state_dict(w), 0.08)
    e.set_camera(*A.camera_args())
    return e


@pytest.fixture(scope='module')
def engines(golden):
    es = {'seed0': new_engine(golden.weights_seed0), 'trained': new_engine(golden.weights_trained)}
    yield es
    for e in es.values():
        e.close()


_batches = {}


def batch_of(golden, name, by_actions):
    """[states, impulses, attrs, nums, dens]: the fixtures and the hand-made batches of tests/test_gpu_train_f64.py with data
    impulses; with pushes the fixtures of tests/_train_actions_ref.py and its synthetic piles in the hand-made counts"""
    key = (name, by_actions)
    if key not in _batches:
        if name in HAND:
            nums, H = HAND[name]
            out = A.synthetic_batch(list(nums), H, 90, kinds=('blob',)) if by_actions else hand_made(list(nums), H)
        else:
            out = A.batch(golden, name) if by_actions else fixture_batch(golden, name)
        out = [np.ascontiguousarray(a) for a in out]
        for a in out:
            a.setflags(write=False)
        _batches[key] = out
    return list(_batches[key])


def split(batch, by_actions):
    """-> ((states, attrs, nums, dens), {the impulse keyword})"""
    st, imp, at, nums, dens = batch
    return (st, at, nums, dens), ({'actions': imp} if by_actions else {'states_delta': imp})


def builtin_grad(e, batch, by_actions, mode='grad'):
    """the built-in MSE step -> (loss, blob)"""
    if by_actions:
        return e.train_step_actions(*batch, mode=mode, want_grad=True)
    return e.train_step(*batch, mode=mode, want_grad=True)


def mse_seed32(pred, batch):
    """kt_mse_grad's seed with its own fp32 arithmetic: inv = (1 / (H B)) / (3 n_b), seed = (2 (p - q)) inv on real rows"""
    st, nums = batch[0], batch[3]
    B, H = pred.shape[:2]
    seed = np.zeros_like(pred)
    for b in range(B):
        n = int(nums[b])
        inv = np.float32(np.float32(1) / np.float32(H * B)) / np.float32(3 * n)
        seed[b, :, :n] = (np.float32(2) * (pred[b, :, :n] - st[b, 1:, :n])) * inv
    assert seed.dtype == np.float32
    return seed


def mse_seed64(pred, batch):
    st, nums = batch[0], batch[3]
    B, H = pred.shape[:2]
    seed = np.zeros_like(pred)
    for b in range(B):
        n = int(nums[b])
        seed[b, :, :n] = 2.0 * (pred[b, :, :n] - st[b, 1:, :n].astype(np.float64)) / (3.0 * n * H * B)
    return seed


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def real_bits(a, nums):
    """[B, H, N, 3] -> the bit patterns of the real rows, sample by sample"""
    return [bits(a[b, :, :int(n)]) for b, n in enumerate(nums)]


def assert_same_real_rows(a, b, nums, label):
    for q, (x, y) in enumerate(zip(real_bits(a, nums), real_bits(b, nums))):
        differ = int((x != y).sum())
        if differ:
            print('[seeded] %s: sample %d: %d values differ' % (label, q, differ))
        assert differ == 0, (label, q, differ)


def per_tensor(g, ref):
    off, out = 0, {}
    for key, shape in weights.STATE_DICT_KEYS:
        n = int(np.prod(shape))
        out[key] = float(np.abs(g[off:off + n].astype(np.float64) - ref[off:off + n]).max() / max(np.abs(ref[off:off + n]).max(), 1e-300))
        off += n
    return out


CASES = [(n, a) for n in ('b4_r3', 'b2_r5') + tuple(HAND) for a in (False, True)]
IDS = ['%s-%s' % (n, 'actions' if a else 'data') for n, a in CASES]


# ---- 1. the forward is the seeded call's forward --------------------------------------------------------------------------
@pytest.mark.parametrize('tape', TAPES)
@pytest.mark.parametrize('name,by_actions', CASES, ids=IDS)
def test_predict_is_the_forward_of_the_seeded_and_of_the_built_in_step(engines, golden, name, by_actions, tape):
    e = engines['seed0']
    batch = batch_of(golden, name, by_actions)
    args, kw = split(batch, by_actions)
    B, T1, N, _ = batch[0].shape
    e.set_engine(tape)
    try:
        e.train_begin(T1 - 1, 1e-3, 0.9)
        e.dispatch_reset()
        pred = e.train_predict(*args, **kw)
        assert pred.dtype == np.float32 and pred.shape == (B, T1 - 1, N, 3)
        assert ('k_aggregate_tape' in e.last_dispatch()) == (tape == 'mfma')
        assert_same_real_rows(e.debug_fetch('train_states', pred.shape), pred, batch[3], 'tap after predict')
        e.train_step_seeded(*args, mse_seed32(pred, batch), mode='grad', **kw)
        assert_same_real_rows(e.debug_fetch('train_states', pred.shape), pred, batch[3], 'tap after the seeded step')
        builtin_grad(e, batch, by_actions)
        assert_same_real_rows(e.debug_fetch('train_states', pred.shape), pred, batch[3], 'tap after the built-in step')
        assert_same_real_rows(e.train_predict(*args, **kw), pred, batch[3], 'a second predict')
        print('[seeded] %s %s %s: predict = both steps\' forward on %d real rows, bit for bit'
              % (name, 'actions' if by_actions else 'data', tape, int(batch[3].sum()) * (T1 - 1)))
    finally:
        e.set_engine('fused')


# ---- 2. the seam is exact ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tape', TAPES)
@pytest.mark.parametrize('name,by_actions', CASES, ids=IDS)
def test_the_mse_seed_gives_the_built_in_blob_bit_for_bit(engines, golden, name, by_actions, tape):
    e = engines['trained' if name == 'b2_r5' else 'seed0']
    batch = batch_of(golden, name, by_actions)
    args, kw = split(batch, by_actions)
    e.set_engine(tape)
    try:
        e.train_begin(batch[0].shape[1] - 1, 1e-3, 0.9)
        _, want = builtin_grad(e, batch, by_actions)
        pred = e.train_predict(*args, **kw)
        seed = mse_seed32(pred, batch)
        got = e.train_step_seeded(*args, seed, mode='grad', want_grad=True, **kw)
        differ = int((bits(got) != bits(want)).sum())
        print('[seeded] %s %s %s: %d of 38403 gradient entries differ from the built-in step\'s' %
              (name, 'actions' if by_actions else 'data', tape, differ))
        if differ:                                  # which side: the seed as the device holds it, against the built-in loss's
            builtin_grad(e, batch, by_actions, mode='eval')
            tap = e.debug_fetch('train_seed', (pred.shape[1], pred.shape[0]) + pred.shape[2:]).transpose(1, 0, 2, 3)
            print('[seeded]     seed entries that differ from the eval pass\'s train_seed tap: %d' % int((bits(tap) != bits(seed)).sum()))
        assert differ == 0
        assert e.train_step_seeded(*args, seed, mode='grad', **kw) is None
    finally:
        e.set_engine('fused')


@pytest.mark.parametrize('tape', TAPES)
@pytest.mark.parametrize('by_actions', [False, True], ids=['data', 'actions'])
def test_five_updates_of_each_kind_leave_the_same_weights(engines, golden, by_actions, tape):
    e = engines['seed0']
    batch = batch_of(golden, 'b2_r5', by_actions)
    args, kw = split(batch, by_actions)
    blob = weights.blob_from_state_dict(golden.weights_seed0)
    e.set_engine(tape)
    try:
        out = []
        for seeded in (False, True):
            e.load_weights(blob, 0.08)
            e.train_begin(batch[0].shape[1] - 1, 1e-3, 0.9)
            for _ in range(5):
                if seeded:
                    assert e.train_step_seeded(*args, mse_seed32(e.train_predict(*args, **kw), batch), mode='update', **kw) is None
                else:
                    builtin_grad(e, batch, by_actions, mode='update')
            out.append(e.get_weights())
        moved = int((bits(out[0]) != bits(blob)).sum())
        differ = int((bits(out[0]) != bits(out[1])).sum())
        print('[seeded] five updates, %s %s: %d weights moved, %d differ between the two kinds' %
              ('actions' if by_actions else 'data', tape, moved, differ))
        assert moved > 38403 // 2 and differ == 0             # (the attribute columns' weights have no gradient and stay)
    finally:
        e.set_engine('fused')
        e.load_weights(blob, 0.08)


# ---- 3. padding and refusals ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['n5_17_16_h3', 'b4_r3'])
def test_garbage_on_padded_seed_rows_changes_nothing(engines, golden, name):
    e = engines['seed0']
    batch = batch_of(golden, name, False)
    args, kw = split(batch, False)
    nums = batch[3]
    e.train_begin(batch[0].shape[1] - 1, 1e-3, 0.9)
    seed = mse_seed32(e.train_predict(*args, **kw), batch)
    want = e.train_step_seeded(*args, seed, mode='grad', want_grad=True, **kw)
    dirty = seed.copy()
    n_pad = 0
    for b, n in enumerate(nums):
        pad = dirty[b, :, int(n):]
        n_pad += pad.size
        pad[...] = np.float32(1e30)
        pad[:, ::2] = np.nan
        pad[:, 1::3] = -np.inf
    got = e.train_step_seeded(*args, dirty, mode='grad', want_grad=True, **kw)
    differ = int((bits(got) != bits(want)).sum())
    print('[seeded] %s: %d padded seed values of NaN, inf and 1e30: %d gradient entries differ' % (name, n_pad, differ))
    assert differ == 0
    if name in HAND:
        assert n_pad > 0
        # ... and on the device they are +0.0: the last step's slice of the seed buffer has no later step's share added
        tap = e.debug_fetch('train_seed', (seed.shape[1], seed.shape[0]) + seed.shape[2:])
        for b, n in enumerate(nums):
            assert (bits(tap[-1, b, int(n):]) == 0).all()
            np.testing.assert_array_equal(bits(tap[-1, b, :int(n)]), bits(seed[b, -1, :int(n)]))


def test_refusals_leave_the_trainer_as_it_was(engines, golden):
    e = engines['seed0']
    batch = batch_of(golden, 'n5_17_16_h3', False)
    args, kw = split(batch, False)
    st, sd, at, nums, dens = batch
    acts = batch_of(golden, 'n5_17_16_h3', True)[1]
    B, T1, N, _ = st.shape
    H = T1 - 1
    e.train_begin(H, 1e-3, 0.9)
    _, before = builtin_grad(e, batch, False)
    seed = mse_seed32(e.train_predict(*args, **kw), batch)

    def unchanged(what):
        _, again = builtin_grad(e, batch, False)
        assert (bits(again) == bits(before)).all(), what

    bad = seed.copy()
    bad[1, 2, 3, 1] = np.nan
    with pytest.raises(DrpError, match='drp error -1: seed: sample 1 step 2 row 3 is not finite'):
        e.train_step_seeded(*args, bad, mode='grad', **kw)
    unchanged('a NaN on a real row')
    bad = seed.copy()
    bad[2, 0, 15, 2] = np.inf                       # the last real row of the last sample
    with pytest.raises(DrpError, match='seed: sample 2 step 0 row 15'):
        e.train_step_seeded(*args, bad, mode='update', **kw)
    unchanged('an inf on a real row')
    with pytest.raises(DrpError, match='drp error -1: .*drp_train_predict'):
        e.train_step_seeded(*args, seed, mode='eval', **kw)
    unchanged('mode eval')
    f32, i32 = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32)
    p = [a.ctypes.data_as(f32) for a in (st, sd, acts, at, dens, seed)]
    pn = nums.ctypes.data_as(i32)
    out = np.empty((B, H, N, 3), np.float32)
    for delta, act in ((p[1], p[2]), (None, None)):
        assert e.lib.drp_train_step_seeded(e.h, p[0], delta, act, p[3], pn, p[4], B, N, p[5], 1, None) == -1
        assert 'exactly one of states_delta and actions' in e.lib.drp_last_error(e.h).decode()
        assert e.lib.drp_train_predict(e.h, p[0], delta, act, p[3], pn, p[4], B, N, out.ctypes.data_as(f32)) == -1
        assert 'exactly one of states_delta and actions' in e.lib.drp_last_error(e.h).decode()
        unchanged('both or neither impulse source')
    assert e.lib.drp_train_step_seeded(e.h, p[0], p[1], None, p[3], pn, p[4], B, N, None, 1, None) == -1
    assert 'null argument' in e.lib.drp_last_error(e.h).decode()
    with pytest.raises(ValueError, match='exactly one'):
        e.train_step_seeded(*args, seed, states_delta=sd, actions=acts)
    with pytest.raises(DrpError, match='particle_nums'):
        e.train_predict(st, at, np.array([5, 18, 16], np.int32), dens, **kw)
    unchanged('a count beyond N')
    fresh = Engine(0)
    try:
        fresh.load_weights(weights.blob_from_state_dict(golden.weights_seed0), 0.08)
        fresh._n_rollout = H                        # (the wrapper's own shape check; the library has seen no drp_train_begin)
        with pytest.raises(DrpError, match='drp error -2: drp_train_begin not called'):
            fresh.train_predict(*args, **kw)
        with pytest.raises(DrpError, match='drp error -2: drp_train_begin not called'):
            fresh.train_step_seeded(*args, seed, mode='grad', **kw)
        fresh.train_begin(H, 1e-3, 0.9)
        with pytest.raises(DrpError, match='drp error -2: camera not set'):
            fresh.train_predict(*args, actions=acts)
        _, g = builtin_grad(fresh, batch, False)
        assert (bits(g) == bits(before)).all()
    finally:
        fresh.close()


# ---- 4. float64 against the built-in yardstick ------------------------------------------------------------------------------
@pytest.mark.parametrize('name,by_actions', [c for c in CASES if not (c[0] in HAND and c[1])],
                         ids=[i for c, i in zip(CASES, IDS) if not (c[0] in HAND and c[1])])
def test_f64_seeded_with_the_mse_seed_is_the_f64_yardstick(engines, golden, name, by_actions):
    e = engines['trained' if name == 'b4_r3' else 'seed0']
    batch = batch_of(golden, name, by_actions)
    args, kw = split(batch, by_actions)
    nums = batch[3]
    if by_actions:
        _, _, rg, rgs = e.train_grad_f64_actions(*batch, want_state=True)
    else:
        _, _, rg, rgs = e.train_grad_f64(*batch, want_state=True)
    pred = e.train_predict_f64(*args, **kw)
    assert pred.dtype == np.float64
    seed = mse_seed64(pred, batch)
    for b, n in enumerate(nums):
        seed[b, :, int(n):] = np.nan                # padded rows of the seed are ignored here too
    g, gs = e.train_grad_f64_seeded(*args, seed, want_state=True, **kw)
    figures = per_tensor(g, rg)
    figures['grad_state'] = float(np.abs(T.real_rows(gs, nums) - T.real_rows(rgs, nums)).max() / np.abs(T.real_rows(rgs, nums)).max())
    worst = max(figures, key=lambda k: figures[k])
    print('[seeded-f64] %s %s: worst %s %.2e of the tensor\'s largest entry' % (name, 'actions' if by_actions else 'data', worst, figures[worst]))
    for k, v in figures.items():
        assert v <= TOL, (k, v)
    # the same bits from run to run and in chunks of one sample
    again = e.train_grad_f64_seeded(*args, seed, want_state=True, **kw)
    try:
        e.set_f64_cap(1)
        single = e.train_grad_f64_seeded(*args, seed, want_state=True, **kw)
        pred1 = e.train_predict_f64(*args, **kw)
    finally:
        e.set_f64_cap(0)
    for a, b, c in zip((g, gs), again, single):
        assert (bits(a) == bits(b)).all() and (bits(a) == bits(c)).all()
    assert_same_real_rows(pred1, pred, nums, 'predict_f64 under a cap of one sample')
    assert_same_real_rows(e.train_predict_f64(*args, **kw), pred, nums, 'predict_f64 again')
    assert (g,)[0].shape == (38403,) and len(e.train_grad_f64_seeded(*args, seed, **kw)) == 1


def test_f64_refusals(engines, golden):
    e = engines['seed0']
    batch = batch_of(golden, 'n5_17_16_h3', False)
    args, kw = split(batch, False)
    seed = mse_seed64(e.train_predict_f64(*args, **kw), batch)
    good = e.train_grad_f64_seeded(*args, seed, **kw)[0]
    bad = seed.copy()
    bad[1, 1, 16, 0] = np.nan
    with pytest.raises(DrpError, match='drp error -1: seed: sample 1 step 1 row 16 is not finite'):
        e.train_grad_f64_seeded(*args, bad, **kw)
    with pytest.raises(ValueError, match='exactly one'):
        e.train_predict_f64(*args)
    assert (bits(e.train_grad_f64_seeded(*args, seed, **kw)[0]) == bits(good)).all()


# ---- 5. float64 against the restatement, for a new loss ---------------------------------------------------------------------
_ref = {}


def restated(golden, name, wset):
    if (name, wset) not in _ref:
        out = S.train_loss_and_grads64_custom(weights_of(golden, wset), batch_of(golden, name, False), S.pseudo_huber_torch)
        for v in out[2:]:
            v.setflags(write=False)
        _ref[(name, wset)] = out
    return _ref[(name, wset)]


@pytest.mark.parametrize('wset', ['seed0', 'trained'])
@pytest.mark.parametrize('name', ['b4_r3', 'b2_r5', 'n5_17_16_h3'])
def test_pseudo_huber_through_torch_loss_matches_the_restatement(engines, golden, name, wset):
    e = engines[wset]
    batch = batch_of(golden, name, False)
    args, kw = split(batch, False)
    nums = batch[3]
    loss_fn = losses.torch_loss(S.pseudo_huber_torch)
    pred = e.train_predict_f64(*args, **kw)
    value, seed = loss_fn(pred, batch)
    assert seed.dtype == np.float64
    g, gs = e.train_grad_f64_seeded(*args, seed, want_state=True, **kw)
    rloss, rgrads, rgs, rpred, rseed = restated(golden, name, wset)
    figures = per_tensor(g, T.blob64(rgrads))
    figures['loss'] = abs(value - rloss) / abs(rloss)
    for key, a, b in (('pred', pred, rpred), ('seed', seed, rseed), ('grad_state', gs, rgs)):
        a, b = T.real_rows(a, nums), T.real_rows(b, nums)
        figures[key] = float(np.abs(a - b).max() / np.abs(b).max())
    worst = max(figures, key=lambda k: figures[k])
    print('[seeded-f64] pseudo-Huber %s %s: worst %s %.2e of the tensor\'s largest entry (loss %.6e)' % (name, wset, worst, figures[worst], value))
    for k, v in figures.items():
        assert v <= TOL, (k, v)


# ---- 6. the probe -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tape', TAPES)
@pytest.mark.parametrize('by_actions', [False, True], ids=['data', 'actions'])
@pytest.mark.parametrize('name,wset', [(b, w) for b in ('b4_r3', 'b2_r5') for w in ('seed0', 'trained')])
def test_custom_probe_is_what_numpy_computes_and_within_the_probe_bound(engines, golden, name, wset, by_actions, tape):
    e = engines[wset]
    batch = batch_of(golden, name, by_actions)
    args, kw = split(batch, by_actions)
    fn = losses.pseudo_huber_loss
    blob = e.get_weights()
    e.set_engine(tape)
    try:
        e.train_begin(batch[0].shape[1] - 1, 1e-3, 0.9)
        p = e.train_gradient_probe_custom(fn, *args, context=batch, **kw)
        assert p['tape'] == tape and p['loss_kind'] == 'custom'
        pred32 = e.train_predict(*args, **kw)
        loss32, seed32 = fn(pred32, batch)
        g32 = e.train_step_seeded(*args, seed32, mode='grad', want_grad=True, **kw)
        pred64 = e.train_predict_f64(*args, **kw)
        loss64, seed64 = fn(pred64, batch)
        g64, = e.train_grad_f64_seeded(*args, seed64, **kw)
        assert seed32.dtype == np.float32 and seed64.dtype == np.float64
        assert p['loss32'] == loss32 and p['loss64'] == loss64 and p['loss_diff'] == abs(loss32 - loss64)
        assert p['seed_rel'] == np.abs(seed32.astype(np.float64) - seed64).max() / np.abs(seed64).max()
        off, rels = 0, {}
        for key, shape in weights.STATE_DICT_KEYS:
            n = int(np.prod(shape))
            err = np.abs(g32[off:off + n].astype(np.float64) - g64[off:off + n]).max()
            ref = np.abs(g64[off:off + n]).max()
            t = p['tensors'][key]
            assert t['max_abs_err'] == err and t['max_abs_ref'] == ref and t['rel'] == err / max(ref, 1e-300)
            rels[key] = t['rel']
            off += n
        assert p['worst'] == max(rels, key=lambda k: rels[k]) and p['rel'] == rels[p['worst']]
        print('[seeded-probe] %s %s %s %s: worst %s rel %.3e, seed_rel %.3e, loss diff %.3e'
              % (name, wset, 'actions' if by_actions else 'data', tape, p['worst'], p['rel'], p['seed_rel'], p['loss_diff']))
        assert (bits(e.get_weights()) == bits(blob)).all()
        for key, r in rels.items():
            assert r <= PROBE_TOL, (key, r, 'seed_rel %.3e' % p['seed_rel'])
    finally:
        e.set_engine('fused')


# ---- 7. the trainer ---------------------------------------------------------------------------------------------------------
def test_the_trainer_on_mse_loss_ends_on_the_bits_of_loss_mse(golden):
    import torch
    config = syn.default_config()
    config['train'].update({'n_rollout': 3, 'n_history': 1, 'lr': 2e-4, 'adam_beta1': 0.9, 'log_per_iter': 1, 'n_epoch': 1})
    batches = [hand_made([12, 9], 3, seed=s) + [None] for s in range(4)]
    res, lines = {}, {}
    for key, kw in (('mse', {'loss': 'mse'}), ('fn', {'loss': losses.mse_loss}), ('probed', {'loss': losses.mse_loss, 'custom_probe_every': 2})):
        model = PropNetDiffDenModel(config, True)
        model.load_state_dict({k[2:]: torch.from_numpy(golden.weights_seed0[k]) for k in golden.weights_seed0.files
                               if k.startswith('w/')}, strict=False)
        lines[key] = []
        r = TG.train(config, model, {'train': batches, 'valid': batches[:1]}, log=lines[key].append, **kw)
        res[key] = (r, model.engine.get_weights().copy())
        model.engine.close()
    for key in ('fn', 'probed'):
        differ = int((bits(res[key][1]) != bits(res['mse'][1])).sum())
        print('[seeded-trainer] %s: %d of 38403 weights differ from loss=\'mse\' after four updates' % (key, differ))
        print('[seeded-trainer] %s history %s' % (key, [h for h in res[key][0]['history'] if h[1] != 'grad_probe']))
    print('[seeded-trainer] mse history %s' % (res['mse'][0]['history'],))
    for key in ('fn', 'probed'):
        assert (bits(res[key][1]) == bits(res['mse'][1])).all()
        assert [h for h in res[key][0]['history'] if h[1] != 'grad_probe'] == res['mse'][0]['history']
        assert [ln for ln in lines[key] if not ln.startswith('grad_probe')] == lines['mse']
    assert res['fn'][0]['best_valid_loss'] == res['mse'][0]['best_valid_loss']
    probes = [h for h in res['probed'][0]['history'] if h[1] == 'grad_probe']
    logged = [ln for ln in lines['probed'] if ln.startswith('grad_probe')]
    for ln in logged:
        print('[seeded-trainer] ' + ln)
    assert len(probes) == 2 and all(0 < h[2] < PROBE_TOL for h in probes)
    assert len(logged) == 2 and all('seed_rel' in ln for ln in logged)
    assert not [ln for ln in lines['fn'] if ln.startswith('grad_probe')]


def test_sessions_engine_dispatch_and_taps_are_left_alone_by_the_f64_pair(engines, golden):
    from dyn_res_pile_manip_amd.planners import world2cam_affine
    batch = batch_of(golden, 'b2_r5', False)
    args, kw = split(batch, False)
    G = syn.goal_field(syn.goal_distance_image(syn.goal_mask('I')))
    lo, hi = syn.action_limits()

    def f64_pair(e):
        pred = e.train_predict_f64(*args, **kw)
        e.train_grad_f64_seeded(*args, mse_seed64(pred, batch), **kw)

    def gd_run(disturbed):
        e = Engine(0)
        out = []
        try:
            e.load_weights(weights.blob_from_state_dict(golden.weights_seed0), 0.08)
            e.set_camera(world2cam_affine(syn.demo_cam_extrinsics()), 24.0, syn.demo_cam_params())
            e.set_goal(G, syn.goal_coor_strided(syn.goal_distance_image(syn.goal_mask('I')), 200))
            s0, dens, attr = syn.make_pile(40, 1, seed=0)
            e.gd_begin(s0, attr, dens, syn.sample_pushes(4, 2, seed=0), 0.05, lo, hi)
            for _ in range(3):
                out.append(e.gd_step())
                if disturbed:
                    f64_pair(e)
            out.append(e.gd_actions())
            assert e.engine_id == _lib.ENGINE_FUSED
        finally:
            e.close()
        return out
    for a, b in zip(gd_run(False), gd_run(True)):
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b))
    e = engines['seed0']
    e.set_engine('split')
    try:
        s, dens, attr = syn.make_pile(20, 2, seed=1)
        sd = 0.004 * np.random.default_rng(1).standard_normal(s.shape).astype(np.float32)
        e.dispatch_reset()
        e.step(attr, s, sd, dens)
        e.step_f64(attr, s, sd, dens)
        marks, tap = e.last_dispatch(), e.f64_tap('effect_1')
        f64_pair(e)
        assert e.engine_id == _lib.ENGINES['split'] and e.last_dispatch() == marks
        np.testing.assert_array_equal(e.f64_tap('effect_1'), tap)      # taps of the earlier call are still answered
    finally:
        e.set_engine('fused')
    # ... and an Adam trajectory with the pair and the custom probe in between is the undisturbed one
    out = {}
    blob = weights.blob_from_state_dict(golden.weights_seed0)
    try:
        for disturbed in (False, True):
            e.load_weights(blob, 0.08)
            e.train_begin(batch[0].shape[1] - 1, 1e-3, 0.9)
            for it in range(3):
                if disturbed:
                    f64_pair(e)
                    e.train_gradient_probe_custom(losses.pseudo_huber_loss, *args, context=batch, **kw)
                    e.train_step_seeded(*args, mse_seed32(e.train_predict(*args, **kw), batch), mode='grad', **kw)
                e.train_step(*batch, mode='update')
            out[disturbed] = e.get_weights()
        assert (bits(out[False]) == bits(out[True])).all()
    finally:
        e.load_weights(blob, 0.08)

"""GPU, row u1's yardstick: the training loop body with the Chamfer loss in float64 on the device (drp_train_grad_f64_untracked:
kc64_chamfer of csrc/k_chamfer_f64.h where drp_train_grad_f64 launches kt64_mse, everything behind the seed unchanged), the probe
that holds the fp32 tapes against it, and the trainer's hook.

Tolerances are the project's own.  The device against the float64 host references (train_untracked64 of tests/_untracked_ref.py,
train_actions64(targets=...) of tests/_train_actions_ref.py; both pinned on the CPU): 1e-10 x the largest magnitude of the
compared tensor, the comparison of tests/test_gpu_train_f64.py -- both sides take their arg-mins in double on the double
prediction and differ in summation order only; the smallest margin agrees within 1e-10 absolute.  The fp32 tapes against float64:
GRAD_REL = 2e-4 of each tensor's largest gradient and LOSS_REL = 1e-4 (tests/_train_actions_ref.py), with min_margin above
MARGIN_MIN = 1e-7 (tests/_untracked_ref.py), which tests/test_untracked_host.py and tests/test_train_actions_host.py hold for
every batch used here.  Every figure is printed before it is asserted."""
import ctypes

import numpy as np
import pytest

import _train_actions_ref as A
import _untracked_ref as U
from dyn_res_pile_manip_amd import synthetic as syn
from dyn_res_pile_manip_amd import train_gnn_dyn as TG
from dyn_res_pile_manip_amd import weights
from dyn_res_pile_manip_amd._lib import DrpError
from dyn_res_pile_manip_amd.engine import Engine
from dyn_res_pile_manip_amd.gnn_dyn import PropNetDiffDenModel

pytestmark = pytest.mark.gpu
TOL = 1e-10
GRAD_REL = A.GRAD_REL
LOSS_REL = A.LOSS_REL
FP, IP, DP = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)


def new_engine(w, engine=None, camera=True):
    e = Engine(0)
    e.load_weights(weights.blob_from_state_dict(w), 0.08)
    if camera:
        e.set_camera(*A.camera_args())
    if engine is not None:
        e.set_engine(engine)
    return e


@pytest.fixture(scope='module')
def engines(golden):
    es = {'seed0': new_engine(golden.weights_seed0), 'trained': new_engine(golden.weights_trained)}
    yield es
    for e in es.values():
        e.close()


def push_args(golden, name):
    """a push case -> (states, None, attrs, nums, dens, targets, target_nums), actions"""
    st, ac, at, nums, dens = A.batch(golden, name)
    tg, tn = A.targets_of(golden, name)
    return [st, None, at, nums, dens, tg, tn], ac


def assert_close(got, want, nums, label):
    """got: train_grad_f64_untracked(..., want_state=True); want: a reference()'s (loss, terms, blob, g_state on real rows, info)"""
    loss, terms, grad, margin, gs = got
    rl, rt, rg, rgs, info = want
    figures = [('loss', abs(loss - rl) / abs(rl))]
    assert terms.dtype == np.float64 and terms.shape == rt.shape and margin.shape == rt.shape
    figures.append(('loss_terms', float(np.abs(terms - rt).max() / np.abs(rt).max())))
    assert grad.dtype == np.float64 and grad.shape == (38403,)
    off = 0
    for key, shape in weights.STATE_DICT_KEYS:
        n = int(np.prod(shape))
        a, b = grad[off:off + n], rg[off:off + n]
        figures.append((key, float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))))
        np.testing.assert_array_equal(a[b == 0], 0.0)       # identically zero inputs (the attribute columns): exactly zero
        off += n
    assert len(figures) == 2 + 18
    figures.append(('grad_state', float(np.abs(U.real_rows(gs, nums) - rgs).max() / np.abs(rgs).max())))
    dm = abs(float(margin.min()) - info['margin']) if np.isfinite(info['margin']) else (0.0 if margin.min() == info['margin'] else np.inf)
    for k, v in figures:
        print('[train-f64-untracked] %s %-45s %.3e' % (label, k, v))
    print('[train-f64-untracked] %s smallest margin %.6e, reference %.6e, apart %.2e' % (label, margin.min(), info['margin'], dm))
    for k, v in figures:
        assert v <= TOL, (label, k, v)
    assert dm <= TOL
    for b, n in enumerate(nums):                            # padded rows of the state gradient: exactly 0
        assert (gs[b, :, n:] == 0).all()


# ---- 1. data impulses ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,wset', U.TRAIN_CASES)
def test_data_impulses_match_the_float64_reference(engines, golden, name, wset):
    batch = U.untracked_batch(golden, name)
    e = engines[wset]
    got = e.train_grad_f64_untracked(*batch, want_state=True)
    assert_close(got, U.reference(golden, name, wset), batch[3], '%s %s' % (name, wset))
    short = e.train_grad_f64_untracked(*batch)       # the state gradient is optional
    assert len(short) == 4 and short[0] == got[0]
    np.testing.assert_array_equal(short[2], got[2])
    np.testing.assert_array_equal(short[3], got[3])


# ---- 2. pushes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,wset', A.TRAIN_CASES)
def test_pushes_match_the_float64_reference(engines, golden, name, wset):
    args, ac = push_args(golden, name)
    got = engines[wset].train_grad_f64_untracked(*args, actions=ac, want_state=True)
    assert_close(got, A.reference(golden, name, wset, loss='chamfer'), args[3], 'push %s %s' % (name, wset))


# ---- 3. degenerate batches ----------------------------------------------------------------------------------------------------
def host_reference(w, batch):
    loss, terms, grads, gs, info = U.train_untracked64(w, *batch)
    return loss, terms, U.blob64(grads), U.real_rows(gs, batch[3]), info


def test_single_point_targets(engines, golden):
    """M = 1: no target has a second candidate in the direction p -> q (margin inf there); the margin is q -> p's"""
    batch = U.single_point_batch(golden)
    got = engines['seed0'].train_grad_f64_untracked(*batch, want_state=True)
    want = host_reference(golden.weights_seed0, batch)
    assert np.isfinite(want[4]['margin']) and np.isfinite(got[3]).all()
    assert_close(got, want, batch[3], 'single point')


def test_tiny_unpadded_batch(engines, golden):
    batch = U.tiny_batch()
    assert batch[0].shape == (1, 2, 5, 3) and batch[5].shape == (1, 1, 3, 3)
    got = engines['seed0'].train_grad_f64_untracked(*batch, want_state=True)
    assert_close(got, host_reference(golden.weights_seed0, batch), batch[3], 'tiny')


# ---- 4. one value, one order ------------------------------------------------------------------------------------------------
def test_same_bits_from_run_to_run_and_under_a_one_sample_cap(engines, golden):
    e = engines['seed0']
    calls = [lambda: e.train_grad_f64_untracked(*U.untracked_batch(golden, 'b4_r3'), want_state=True),
             lambda: e.train_grad_f64_untracked(*U.untracked_batch(golden, 'b2_r5'), want_state=True)]
    args, ac = push_args(golden, 'b3_n24')
    calls.append(lambda: e.train_grad_f64_untracked(*args, actions=ac, want_state=True))
    for call in calls:
        whole, again = call(), call()
        try:
            e.set_f64_cap(1)                                    # one sample is the smallest chunk: B chunks
            single = call()
        finally:
            e.set_f64_cap(0)
        assert len(whole) == 5
        for a, b, c in zip(whole, again, single):
            np.testing.assert_array_equal(np.asarray(a), np.asarray(b))
            np.testing.assert_array_equal(np.asarray(a), np.asarray(c))


# ---- 5. the MSE yardstick is untouched ---------------------------------------------------------------------------------------
def test_the_mse_yardsticks_keep_their_bits_and_the_taps_stay_answered(golden):
    batch = U.untracked_batch(golden, 'b2_r5')
    args, ac = push_args(golden, 'b3_n24')
    st, _, at, nums, dens = args[:5]

    def mse(e):
        return list(e.train_grad_f64(*batch[:5], want_state=True)) + list(e.train_grad_f64_actions(st, ac, at, nums, dens, want_state=True))
    fresh = new_engine(golden.weights_seed0)
    try:
        want = mse(fresh)
    finally:
        fresh.close()
    e = new_engine(golden.weights_seed0)
    try:
        before = mse(e)
        s, d, attr = syn.make_pile(20, 2, seed=1)
        sd = 0.004 * np.random.default_rng(1).standard_normal(s.shape).astype(np.float32)
        e.dispatch_reset()
        e.step(attr, s, sd, d)
        e.step_f64(attr, s, sd, d)
        marks, tap = e.last_dispatch(), e.f64_tap('effect_1')
        e.train_grad_f64_untracked(*batch, want_state=True)
        e.train_grad_f64_untracked(*args, actions=ac)
        assert e.last_dispatch() == marks
        np.testing.assert_array_equal(e.f64_tap('effect_1'), tap)      # taps of the earlier call are still answered
        after = mse(e)
    finally:
        e.close()
    assert len(want) == len(before) == len(after) == 8
    for a, b, c in zip(want, before, after):
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b))
        np.testing.assert_array_equal(np.asarray(a), np.asarray(c))


# ---- 6. the probe -------------------------------------------------------------------------------------------------------------
def assert_probe(p, tape, label):
    assert p['tape'] == tape and p['loss_kind'] == 'chamfer' and len(p['tensors']) == 18
    rel_loss = p['loss_diff'] / abs(p['loss64'])
    print('[chamfer-probe] %s %s: worst %s rel %.3e, loss rel %.3e, min_margin %.3e' % (label, tape, p['worst'], p['rel'], rel_loss,
                                                                                       p['min_margin']))
    for key, t in p['tensors'].items():
        print('[chamfer-probe]     %-45s %.3e' % (key, t['rel']))
    assert p['min_margin'] > U.MARGIN_MIN
    for key, t in p['tensors'].items():
        assert t['max_abs_err'] <= GRAD_REL * t['max_abs_ref'], (key, t['rel'])
    assert p['rel'] == max(t['rel'] for t in p['tensors'].values())
    assert rel_loss <= LOSS_REL


@pytest.mark.parametrize('tape', ['fused', 'mfma'])
@pytest.mark.parametrize('name,wset', U.TRAIN_CASES)
def test_probe_with_data_impulses(golden, name, wset, tape):
    batch = U.untracked_batch(golden, name)
    H = batch[0].shape[1] - 1
    plain = new_engine(U.weights_of(golden, wset), tape)
    try:
        plain.train_begin(H, 1e-3, 0.9)
        plain.train_step_untracked(*batch, mode='update')
        want = plain.get_weights().copy()
    finally:
        plain.close()
    e = new_engine(U.weights_of(golden, wset), tape)
    try:
        e.train_begin(H, 1e-3, 0.9)
        w0 = e.get_weights().copy()
        p = e.train_gradient_probe(*batch[:5], targets=batch[5], target_nums=batch[6])
        np.testing.assert_array_equal(e.get_weights(), w0)
        # the probe is what its two halves give
        loss32, g32 = e.train_step_untracked(*batch, mode='grad', want_grad=True)
        loss64, _, g64, margin = e.train_grad_f64_untracked(*batch)
        assert p['loss32'] == loss32 and p['loss64'] == loss64 and p['min_margin'] == margin.min()
        off = 0
        for key, shape in weights.STATE_DICT_KEYS:
            n = int(np.prod(shape))
            assert p['tensors'][key]['max_abs_err'] == np.abs(g32[off:off + n].astype(np.float64) - g64[off:off + n]).max()
            assert p['tensors'][key]['max_abs_ref'] == np.abs(g64[off:off + n]).max()
            off += n
        e.train_step_untracked(*batch, mode='update')
        np.testing.assert_array_equal(e.get_weights(), want)       # the update it would have been, bit for bit
    finally:
        e.close()
    assert_probe(p, tape, '%s %s data' % (name, wset))


@pytest.mark.parametrize('tape', ['fused', 'mfma'])
@pytest.mark.parametrize('name,wset', A.TRAIN_CASES)
def test_probe_with_pushes(golden, name, wset, tape):
    args, ac = push_args(golden, name)
    H = args[0].shape[1] - 1
    e = new_engine(A.weights_of(golden, wset), tape)
    try:
        e.train_begin(H, 1e-3, 0.9)
        w0 = e.get_weights().copy()
        p = e.train_gradient_probe(*args[:5], actions=ac, targets=args[5], target_nums=args[6])
        np.testing.assert_array_equal(e.get_weights(), w0)
    finally:
        e.close()
    assert_probe(p, tape, '%s %s pushes' % (name, wset))


def test_probe_without_targets_is_todays(engines, golden):
    batch = U.untracked_batch(golden, 'b2_r5')
    e = engines['seed0']
    e.train_begin(batch[0].shape[1] - 1, 1e-3, 0.9)
    p = e.train_gradient_probe(*batch[:5])
    assert sorted(p) == ['loss32', 'loss64', 'loss_diff', 'rel', 'tape', 'tensors', 'worst']
    loss64, _, g64 = e.train_grad_f64(*batch[:5])
    assert p['loss64'] == loss64


# ---- 7. the trainer's hook ------------------------------------------------------------------------------------------------------
def _model(golden):
    import torch
    model = PropNetDiffDenModel(syn.default_config(), True)
    model.load_state_dict({k[2:]: torch.from_numpy(golden.weights_seed0[k]) for k in golden.weights_seed0.files
                           if k.startswith('w/')}, strict=False)
    model.engine.set_camera(*A.camera_args())
    return model


def hook_batches(impulses):
    """four collate_untracked-shaped batches of two rollout steps"""
    out = []
    for it in range(4):
        if impulses == 'actions':
            st, ac, at, nums, dens = A.synthetic_batch([12, 9], 2, 90 + it)
            sd = None
        else:
            st, sd, at, nums, dens = syn.push_batch(it, batch_size=2, n_rollout=2)
            ac = None
        tg, tn = U.make_targets(st, nums, 40 + it)
        data = TG.PaddedBatch((st, sd, at, nums, dens, None, tg, tn))
        data.actions = ac
        out.append(data)
    return out


@pytest.mark.parametrize('impulses', ['data', 'actions'])
def test_the_trainers_hook_changes_no_weight(golden, impulses):
    config = syn.default_config()
    config['train'].update({'n_rollout': 2, 'n_history': 1, 'lr': 2e-4, 'adam_beta1': 0.9, 'log_per_iter': 1, 'n_epoch': 1})
    batches = hook_batches(impulses)
    res, lines = {}, {}
    for every in (0, 2):
        model = _model(golden)
        lines[every] = []
        r = TG.train(config, model, {'train': batches, 'valid': batches[:1]}, log=lines[every].append, loss='chamfer',
                     impulses=impulses, probe_every=every)
        res[every] = (r, model.engine.get_weights().copy())
        model.engine.close()
    np.testing.assert_array_equal(res[0][1], res[2][1])
    probes = [h for h in res[2][0]['history'] if h[1] == 'grad_probe']
    probe_lines = [ln for ln in lines[2] if ln.startswith('grad_probe')]
    for ln in probe_lines:
        print('[chamfer-probe] hook %s: %s' % (impulses, ln))
    assert len(probes) == 2 and all(np.isfinite(h[2]) and h[2] > 0 for h in probes)
    assert [h for h in res[2][0]['history'] if h[1] != 'grad_probe'] == res[0][0]['history']
    assert [ln for ln in lines[2] if not ln.startswith('grad_probe')] == lines[0]
    assert len(probe_lines) == 2 and all('min_margin' in ln for ln in probe_lines)


def test_probe_every_with_the_mse_is_grad_probe_every(golden):
    config = syn.default_config()
    config['train'].update({'n_rollout': 2, 'n_history': 1, 'lr': 2e-4, 'adam_beta1': 0.9, 'log_per_iter': 1, 'n_epoch': 1})
    batches = [tuple(b[:6]) for b in hook_batches('data')]
    out = {}
    for opt in ('grad_probe_every', 'probe_every'):
        model = _model(golden)
        lines = []
        r = TG.train(config, model, {'train': batches, 'valid': batches[:1]}, log=lines.append, **{opt: 2})
        out[opt] = (r['history'], lines, model.engine.get_weights().copy())
        model.engine.close()
    assert out['probe_every'][0] == out['grad_probe_every'][0] and out['probe_every'][1] == out['grad_probe_every'][1]
    np.testing.assert_array_equal(out['probe_every'][2], out['grad_probe_every'][2])
    assert not any('min_margin' in ln for ln in out['probe_every'][1])


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(golden):
    batch = [np.ascontiguousarray(a) for a in U.untracked_batch(golden, 'b2_r5')]
    st, sd, at, nums, dens, tg, tn = batch
    B, T1, N, _ = st.shape
    H, M = T1 - 1, tg.shape[2]
    ac = np.ascontiguousarray(A.fixture_actions(st, nums, 0))

    def call(e, sd_=sd, ac_=None, tg_=tg, tn_=tn, M_=M, nums_=nums, H_=H):
        f = lambda a, T: None if a is None else a.ctypes.data_as(T)
        return e.lib.drp_train_grad_f64_untracked(e.h, f(st, FP), f(sd_, FP), f(ac_, FP), f(at, FP), f(nums_, IP), f(dens, FP), B, N, H_,
                                                  f(tg_, FP), f(tn_, IP), M_, None, None, None, None, None)
    e = Engine(0)
    try:
        assert call(e) == -2 and 'weights not loaded' in e.lib.drp_last_error(e.h).decode()        # DRP_ESTATE
        e.load_weights(weights.blob_from_state_dict(golden.weights_seed0), 0.08)
        good = e.train_grad_f64_untracked(*batch, want_state=True)                                 # no train_begin needed

        def still_works():
            for a, b in zip(e.train_grad_f64_untracked(*batch, want_state=True), good):
                np.testing.assert_array_equal(np.asarray(a), np.asarray(b))
        zero_t, big_t = tn.copy(), tn.copy()
        zero_t[1, 2], big_t[0, 0] = 0, M + 1
        zero_push = ac.copy()
        zero_push[1, 1, 2:] = zero_push[1, 1, :2]
        refused = [('both impulse sources', dict(ac_=ac), -1), ('neither impulse source', dict(sd_=None), -1),
                   ('pushes without a camera', dict(sd_=None, ac_=ac), -2),
                   ('null targets', dict(tg_=None), -1), ('null target_nums', dict(tn_=None), -1),
                   ('M = 0', dict(M_=0), -1), ('M = 4097', dict(M_=4097), -1),
                   ('a target count of 0', dict(tn_=zero_t), -1), ('a target count above M', dict(tn_=big_t), -1),
                   ('a particle count of 0', dict(nums_=np.array([nums[0], 0], np.int32)), -1),
                   ('n_rollout = 0', dict(H_=0), -1), ('n_rollout = 65', dict(H_=65), -1)]
        for label, kw, rc in refused:
            got = call(e, **kw)
            print('[train-f64-untracked] refusal, %s: %d (%s)' % (label, got, e.lib.drp_last_error(e.h).decode()))
            assert got == rc, label
            still_works()
        e.set_camera(*A.camera_args())
        assert call(e, sd_=None, ac_=ac) == 0
        got = call(e, sd_=None, ac_=zero_push)
        print('[train-f64-untracked] refusal, a zero-length push: %d (%s)' % (got, e.lib.drp_last_error(e.h).decode()))
        assert got == -1 and 'push of length' in e.lib.drp_last_error(e.h).decode()
        still_works()
        with pytest.raises(DrpError, match='exactly one'):
            e._ck(call(e, ac_=ac))
        still_works()
        assert_close(good, U.reference(golden, 'b2_r5', 'seed0'), nums, 'after the refusals')
    finally:
        e.close()

"""GPU: the trainer's optimiser seam -- drp_train_accumulate, drp_train_apply, drp_train_get_state / drp_train_set_state, and the
trainer's accum_steps / clip_norm / save_optimizer on top of them.

Bounds.  Almost everything is held to BITS: a gradient accumulated once with weight 1 and applied with scale 1 is the gradient,
so the Adam step is drp_train_step's own arithmetic on the same float32 values; an accumulator fed power-of-two weights holds the
exact sum, and the float32 gradient of an apply is what numpy forms from the returned blobs in float64 (tests/_optim_ref.py).
The norm is held to 1e-13 of numpy's sqrt(sum((scale acc)^2)) -- both float64, two summation orders of 38 403 squares -- and the
clip factor to 1e-15 of max_norm / (norm + 1e-6) evaluated from the returned norm (one division and one addition).  The
accumulated gradient of two half batches is held, per tensor, to 2e-4 of the tensor's largest entry of the float64 yardstick on
the whole batch, the project's standing per-tensor bound.  Every figure is printed before it is asserted."""
import os
import shutil

import numpy as np
import pytest

import _optim_ref as R
import _train_actions_ref as A
import _untracked_ref as U
from dyn_res_pile_manip_amd import _lib, synthetic as syn, train_gnn_dyn as TG, weights
from dyn_res_pile_manip_amd._lib import DrpError
from dyn_res_pile_manip_amd.engine import Engine
from dyn_res_pile_manip_amd.gnn_dyn import PropNetDiffDenModel
from test_gpu_train_f64 import fixture_batch, hand_made
from test_gpu_train_seeded import mse_seed32

pytestmark = pytest.mark.gpu
PROBE_TOL = 2e-4
NORM_TOL = 1e-13
CLIP_TOL = 1e-15
TAPES = ('fused', 'mfma')
WSET = {'b4_r3': 'seed0', 'b2_r5': 'trained'}
SINKHORN_ITERS = 10
LR, BETA1 = 1e-3, 0.9


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same(a, b):
    return bool((bits(a) == bits(b)).all())


def blob_of(golden, wset):
    return weights.blob_from_state_dict(golden.weights_seed0 if wset == 'seed0' else golden.weights_trained)


@pytest.fixture(scope='module')
def eng():
    e = Engine(0)
    e.set_camera(*A.camera_args())
    yield e
    e.close()


class Surface(object):
    """One trainer entry point on one batch: step(e, mode, want_grad) -> the gradient blob or None; eval_loss(e) -> a loss."""

    def __init__(self, golden, kind, name):
        self.kind, self.name = kind, name
        self.data = fixture_batch(golden, name)
        self.H = self.data[0].shape[1] - 1
        self.B = self.data[0].shape[0]
        if kind == 'actions':
            self.batch = A.batch(golden, name)
        elif kind == 'divergence':
            self.batch = U.untracked_batch(golden, name)

    def step(self, e, mode, want_grad=False):
        st, sd, at, nums, dens = self.data
        if self.kind == 'data':
            return e.train_step(*self.data, mode=mode, want_grad=want_grad)[1]
        if self.kind == 'actions':
            return e.train_step_actions(*self.batch, mode=mode, want_grad=want_grad)[1]
        if self.kind == 'divergence':
            tg, tn = self.batch[5], self.batch[6]
            return e.train_step_divergence(st, at, nums, dens, tg, tn, TG.transport_eps(dens), SINKHORN_ITERS, states_delta=sd,
                                           mode=mode, want_grad=want_grad)[1]
        assert self.kind == 'seeded'
        pred = e.train_predict(st, at, nums, dens, states_delta=sd)
        return e.train_step_seeded(st, at, nums, dens, mse_seed32(pred, self.data), states_delta=sd, mode=mode, want_grad=want_grad)

    def eval_loss(self, e):
        return np.float64(e.train_step(*self.data, mode='eval')[0])


def start(e, blob, H, tape='fused'):
    e.set_engine(tape)
    e.load_weights(blob, 0.08)
    e.train_begin(H, LR, BETA1)


def snapshot(e, surface=None):
    """-> [weights, m, v, iter(, the next eval loss)]"""
    m, v, it = e.train_get_state()
    out = [e.get_weights(), m, v, np.int64(it)]
    if surface is not None:
        out.append(surface.eval_loss(e))
    return out


def assert_same_snapshot(a, b, label):
    names = ('weights', 'm', 'v', 'iter', 'eval loss')
    differ = {n: int((bits(np.atleast_1d(x)) != bits(np.atleast_1d(y))).sum()) for n, x, y in zip(names, a, b)}
    print('[optim] %s: entries that differ %s' % (label, differ))
    assert not any(differ.values()), (label, differ)


# ---- 1. bit identity with the built-in update ---------------------------------------------------------------------------------
IDENTITY = [(k, n, t) for t in TAPES for k in ('data', 'actions') for n in ('b4_r3', 'b2_r5')] + \
           [('divergence', 'b4_r3', 'fused'), ('seeded', 'b2_r5', 'fused')]


@pytest.mark.parametrize('kind,name,tape', IDENTITY, ids=['%s-%s-%s' % c for c in IDENTITY])
def test_accumulate_and_apply_are_the_built_in_update(eng, golden, kind, name, tape):
    s = Surface(golden, kind, name)
    blob = blob_of(golden, WSET[name])
    try:
        runs = {}
        for seam in (False, True):
            start(eng, blob, s.H, tape)
            snaps = []
            for it in range(5):
                if seam:
                    g = s.step(eng, 'grad', want_grad=True)
                    eng.train_accumulate(1)
                    out = eng.train_apply(1.0, None, want_grad=True)
                    assert out['applied'] and out['clip'] == 1.0 and out['grad'].dtype == np.float32
                    assert same(out['grad'], g), 'grad_out is the grad pass\'s blob'
                    assert abs(out['norm'] - R.norm(g, 1.0)) <= NORM_TOL * out['norm']
                else:
                    s.step(eng, 'update')
                if it in (0, 4):
                    snaps.append(snapshot(eng, s))
            runs[seam] = snaps
        for k, label in enumerate(('one step', 'five steps')):
            assert_same_snapshot(runs[True][k], runs[False][k], '%s %s %s, %s' % (kind, name, tape, label))
        assert runs[True][1][3] == 5
        moved = int((bits(runs[True][1][0]) != bits(blob)).sum())
        assert moved > 1000, moved                   # (dead units and the attribute columns have no gradient and stay)
    finally:
        eng.set_engine('fused')


# ---- 2. accumulation is the exact sum -------------------------------------------------------------------------------------------
def test_two_half_batches_accumulate_to_the_exact_sum_and_the_whole_batch_gradient(eng, golden):
    s = Surface(golden, 'data', 'b4_r3')
    start(eng, blob_of(golden, 'seed0'), s.H)
    g64 = eng.train_grad_f64(*s.data)[2]                    # at the weights the halves are taken at, before the apply moves them
    halves = []
    for lo in (0, 2):
        halves.append(eng.train_step(*[a[lo:lo + 2] for a in s.data], mode='grad', want_grad=True)[1])      # (the same padding)
        eng.train_accumulate(2)
    out = eng.train_apply(0.25, None, want_grad=True)
    acc = R.accumulate(R.accumulate(None, halves[0], 2), halves[1], 2)
    np.testing.assert_array_equal(acc, 2.0 * halves[0].astype(np.float64) + 2.0 * halves[1].astype(np.float64))
    want = R.scaled_gradient(acc, 0.25)
    differ = int((bits(out['grad']) != bits(want)).sum())
    print('[optim] two halves of b4_r3: %d of 38403 entries differ from numpy\'s ((2 g1 + 2 g2) 0.25).astype(float32)' % differ)
    assert differ == 0 and out['applied'] and out['clip'] == 1.0
    off, rels = 0, {}
    for key, shape in weights.STATE_DICT_KEYS:
        n = int(np.prod(shape))
        rels[key] = float(np.abs(out['grad'][off:off + n].astype(np.float64) - g64[off:off + n]).max()
                          / max(np.abs(g64[off:off + n]).max(), 1e-300))
        off += n
    worst = max(rels, key=lambda k: rels[k])
    print('[optim] accumulated halves against the float64 whole-batch gradient: worst %s %.3e of the tensor\'s largest entry'
          % (worst, rels[worst]))
    for key, r in rels.items():
        assert r <= PROBE_TOL, (key, r)


@pytest.mark.parametrize('name', ['b4_r3', 'b2_r5'])
def test_the_same_batch_twice_is_the_single_update(eng, golden, name):
    s = Surface(golden, 'data', name)
    blob = blob_of(golden, WSET[name])
    start(eng, blob, s.H)
    s.step(eng, 'update')
    single = snapshot(eng, s)
    start(eng, blob, s.H)
    for _ in range(2):
        s.step(eng, 'grad')
        eng.train_accumulate(s.B)
    out = eng.train_apply(1.0 / (2 * s.B), None)
    assert out['applied']
    assert_same_snapshot(snapshot(eng, s), single, '%s twice, weights %d and %d, scale 1/%d' % (name, s.B, s.B, 2 * s.B))


# ---- 3. clipping ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['b4_r3', 'b2_r5'])
def test_clipping_is_torchs_and_a_host_scaled_twin_ends_on_the_same_bits(eng, golden, name):
    s = Surface(golden, 'data', name)
    blob = blob_of(golden, WSET[name])
    w, scale = float(s.B), 1.0 / s.B

    def run(scale_, max_norm):
        start(eng, blob, s.H)
        g = s.step(eng, 'grad', want_grad=True)
        eng.train_accumulate(w)
        out = eng.train_apply(scale_, max_norm, want_grad=True)
        return g, out, snapshot(eng)

    g, free, snap_free = run(scale, None)
    ref_norm = R.norm(R.accumulate(None, g, w), scale)
    assert free['clip'] == 1.0 and free['applied']
    _, clipped, snap_clipped = run(scale, 0.5 * free['norm'])
    max_norm = 0.5 * free['norm']
    norm_rel = abs(clipped['norm'] - ref_norm) / ref_norm
    want_clip = max_norm / (clipped['norm'] + 1e-6)
    clip_rel = abs(clipped['clip'] - want_clip) / want_clip
    print('[optim] %s: norm %.17g, numpy %.17g, rel %.2e; clip %.17g, from the returned norm %.17g, rel %.2e'
          % (name, clipped['norm'], ref_norm, norm_rel, clipped['clip'], want_clip, clip_rel))
    assert norm_rel <= NORM_TOL and abs(free['norm'] - ref_norm) / ref_norm <= NORM_TOL
    assert clip_rel <= CLIP_TOL and 0.0 < clipped['clip'] < 1.0
    assert same(clipped['grad'], R.scaled_gradient(R.accumulate(None, g, w), scale, clipped['clip']))
    assert not same(snap_clipped[0], snap_free[0])
    # a twin that applies without clipping, the factor folded into its scale on the host
    _, twin, snap_twin = run(scale * clipped['clip'], None)
    assert twin['clip'] == 1.0
    assert_same_snapshot(snap_twin, snap_clipped, '%s: clipped on the device against scale x clip from the host' % name)
    # a bound above the norm clips nothing
    _, loose, snap_loose = run(scale, 2.0 * free['norm'])
    assert loose['clip'] == 1.0
    assert_same_snapshot(snap_loose, snap_free, '%s: max_norm above the norm against no clipping' % name)
    # the same bits from run to run
    _, again, snap_again = run(scale, max_norm)
    assert same(np.float64(again['norm']), np.float64(clipped['norm'])) and same(np.float64(again['clip']), np.float64(clipped['clip']))
    assert same(again['grad'], clipped['grad'])
    assert_same_snapshot(snap_again, snap_clipped, '%s: the clipped apply, a second run' % name)


# ---- 4. a norm that is not finite moves nothing ---------------------------------------------------------------------------------
def test_a_norm_that_is_not_finite_moves_nothing(eng, golden):
    s = Surface(golden, 'data', 'b4_r3')
    blob = blob_of(golden, 'seed0')
    start(eng, blob, s.H)
    s.step(eng, 'update')                                   # (moments that are not zero)
    before = snapshot(eng, s)
    s.step(eng, 'grad')
    eng.train_accumulate(1e300)                             # the squares overflow to +inf
    out = eng.train_apply()
    print('[optim] weight 1e300: norm %r, clip %r, applied %r' % (out['norm'], out['clip'], out['applied']))
    assert out['applied'] is False and not np.isfinite(out['norm'])
    assert_same_snapshot(snapshot(eng, s), before, 'after the skipped apply')
    with pytest.raises(DrpError, match='drp error -2: nothing accumulated'):
        eng.train_apply()
    # the accumulator was cleared all the same: the next group is the built-in update
    s.step(eng, 'grad')
    eng.train_accumulate(1)
    assert eng.train_apply()['applied']
    seam = snapshot(eng, s)
    start(eng, blob, s.H)
    s.step(eng, 'update')
    s.step(eng, 'update')
    assert_same_snapshot(seam, snapshot(eng, s), 'an update, a skipped apply, a group of one against two updates')


# ---- 5. state round trip --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['b4_r3', 'b2_r5'])
def test_a_resumed_run_with_adams_state_is_the_uninterrupted_one(eng, golden, name):
    s = Surface(golden, 'data', name)
    blob = blob_of(golden, WSET[name])
    start(eng, blob, s.H)
    for _ in range(5):
        s.step(eng, 'update')
    straight = snapshot(eng, s)
    start(eng, blob, s.H)
    for _ in range(3):
        s.step(eng, 'update')
    w3, (m3, v3, it3) = eng.get_weights(), eng.train_get_state()
    assert it3 == 3 and m3.shape == v3.shape == (38403,) and (v3 >= 0).all() and np.abs(m3).max() > 0
    ends = {}
    for with_state in (True, False):
        fresh = Engine(0)
        try:
            fresh.load_weights(w3, 0.08)
            fresh.train_begin(s.H, LR, BETA1)
            if with_state:
                fresh.train_set_state(m3, v3, it3)
                back = fresh.train_get_state()
                assert same(back[0], m3) and same(back[1], v3) and back[2] == 3
            for _ in range(2):
                s.step(fresh, 'update')
            ends[with_state] = snapshot(fresh, s)
        finally:
            fresh.close()
    assert_same_snapshot(ends[True], straight, '%s: three updates, a fresh context with set_state, two more' % name)
    forgot = int((bits(ends[False][0]) != bits(straight[0])).sum())
    print('[optim] %s: the same resume without set_state: %d of 38403 weights differ' % (name, forgot))
    assert forgot > 1000 and ends[False][3] == 2


# ---- 6. refusals and isolation --------------------------------------------------------------------------------------------------
def test_refusals_leave_the_trainer_as_it_was(eng, golden):
    s = Surface(golden, 'data', 'b4_r3')
    st, sd, at, nums, dens = s.data
    blob = blob_of(golden, 'seed0')
    fresh = Engine(0)
    try:
        fresh.load_weights(blob, 0.08)
        for call in (lambda: fresh.train_accumulate(1), lambda: fresh.train_apply(), lambda: fresh.train_get_state(),
                     lambda: fresh.train_set_state(np.zeros(38403, np.float32), np.zeros(38403, np.float32), 0)):
            with pytest.raises(DrpError, match='drp error -2: drp_train_begin not called'):
                call()
    finally:
        fresh.close()
    start(eng, blob, s.H)
    before = s.step(eng, 'grad', want_grad=True)
    state = snapshot(eng)

    def no_fresh_gradient(what):
        with pytest.raises(DrpError, match='drp error -2: no fresh gradient'):
            eng.train_accumulate(1)
        assert same(s.step(eng, 'grad', want_grad=True), before), what
        assert_same_snapshot(snapshot(eng), state, what)

    start(eng, blob, s.H)
    no_fresh_gradient('right after train_begin')
    with pytest.raises(DrpError, match='drp error -2: nothing accumulated'):
        eng.train_apply()
    s.step(eng, 'eval')
    no_fresh_gradient('after an eval pass')
    eng.train_predict(st, at, nums, dens, states_delta=sd)
    no_fresh_gradient('after train_predict')
    with pytest.raises(DrpError, match='particle_nums'):
        eng.train_step(st, sd, at, np.array([5, 99, 16, 3], np.int32), dens, mode='grad')
    no_fresh_gradient('after a refused grad call')
    eng.load_weights(blob, 0.08)
    no_fresh_gradient('after a weight load')
    # bad arguments are refused with the gradient still fresh and nothing accumulated
    for bad in (0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(DrpError, match='drp error -1: weight='):
            eng.train_accumulate(bad)
    with pytest.raises(DrpError, match='drp error -2: nothing accumulated'):
        eng.train_apply()
    eng.train_accumulate(1)
    with pytest.raises(DrpError, match='drp error -2: no fresh gradient'):         # a pass is accumulated once
        eng.train_accumulate(1)
    for bad in (0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(DrpError, match='drp error -1: scale='):
            eng.train_apply(scale=bad)
    for bad in (0.0, -1.0, float('nan'), float('-inf')):
        with pytest.raises(DrpError, match='drp error -1: max_norm='):
            eng.train_apply(max_norm=bad)
    assert_same_snapshot(snapshot(eng), state, 'after the refused accumulate and apply calls')
    out = eng.train_apply(want_grad=True)                    # ... and the one accumulated pass is still there, whole
    assert out['applied'] and same(out['grad'], before)
    seam = snapshot(eng)
    start(eng, blob, s.H)
    s.step(eng, 'update')
    assert_same_snapshot(seam, snapshot(eng), 'the apply behind the refusals against the built-in update')
    with pytest.raises(DrpError, match='drp error -2: no fresh gradient'):         # (after an update pass)
        eng.train_accumulate(1)
    # set_state
    good = eng.train_get_state()
    for m, v, it, word in ((np.where(np.arange(38403) == 7, np.nan, good[0]).astype(np.float32), good[1], 1, r'm\[7\]'),
                           (good[0], np.where(np.arange(38403) == 38402, np.inf, good[1]).astype(np.float32), 1, r'v\[38402\]'),
                           (good[0], np.where(np.arange(38403) == 0, -1e-30, good[1]).astype(np.float32), 1, r'v\[0\]'),
                           (good[0], good[1], -1, 'iter=-1')):
        with pytest.raises(DrpError, match='drp error -1: ' + word):
            eng.train_set_state(m, v, it)
    with pytest.raises(ValueError):
        eng.train_set_state(good[0][:-1], good[1], 1)
    back = eng.train_get_state()
    assert same(back[0], good[0]) and same(back[1], good[1]) and back[2] == good[2] == 1


def skipped_group(e, s):
    """a gradient pass, accumulated so that its norm overflows, and the apply that therefore moves nothing"""
    s.step(e, 'grad')
    e.train_accumulate(1e300)
    assert e.train_apply()['applied'] is False


def test_an_adam_trajectory_a_gd_session_and_the_dispatch_marks_are_not_disturbed(golden):
    from dyn_res_pile_manip_amd.planners import world2cam_affine
    s = Surface(golden, 'data', 'b2_r5')
    blob = blob_of(golden, 'seed0')

    def adam_trajectory(disturbed):                 # the recipe of tests/test_gpu_train_f64.py::adam_trajectory
        e = Engine(0)
        out = []
        try:
            e.load_weights(blob, 0.08)
            e.train_begin(s.H, LR, BETA1)
            for it in range(6):
                if disturbed:
                    skipped_group(e, s)
                loss, grad = e.train_step(*s.data, mode='update', want_grad=True)
                out += [np.float64(loss), grad, e.get_weights()]
        finally:
            e.close()
        return out

    plain, mixed = adam_trajectory(False), adam_trajectory(True)
    assert len(plain) == len(mixed) == 18
    for a, b in zip(plain, mixed):
        np.testing.assert_array_equal(a, b)

    G = syn.goal_field(syn.goal_distance_image(syn.goal_mask('I')))
    lo, hi = syn.action_limits()

    def gd_run(disturbed):
        e = Engine(0)
        out = []
        try:
            e.load_weights(blob, 0.08)
            e.set_camera(world2cam_affine(syn.demo_cam_extrinsics()), 24.0, syn.demo_cam_params())
            e.set_goal(G, syn.goal_coor_strided(syn.goal_distance_image(syn.goal_mask('I')), 200))
            e.train_begin(s.H, LR, BETA1)
            s.step(e, 'grad')                       # the fresh gradient the session's first disturbance takes
            s0, dens, attr = syn.make_pile(40, 1, seed=0)
            e.gd_begin(s0, attr, dens, syn.sample_pushes(4, 2, seed=0), 0.05, lo, hi)
            for it in range(3):
                out.append(e.gd_step())
                if disturbed and it == 0:
                    e.train_accumulate(1e300)
                    assert e.train_apply()['applied'] is False
                elif disturbed:
                    with pytest.raises(DrpError, match='drp error -2'):
                        e.train_accumulate(1)
                    with pytest.raises(DrpError, match='drp error -2'):
                        e.train_apply()
            out.append(e.gd_actions())
        finally:
            e.close()
        return out
    for a, b in zip(gd_run(False), gd_run(True)):
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b))

    e = Engine(0)
    try:
        e.load_weights(blob, 0.08)
        e.train_begin(s.H, LR, BETA1)
        s.step(e, 'grad')
        pile, dens, attr = syn.make_pile(20, 2, seed=1)
        sd = 0.004 * np.random.default_rng(1).standard_normal(pile.shape).astype(np.float32)
        e.dispatch_reset()
        e.step(attr, pile, sd, dens)
        marks = e.last_dispatch()
        e.train_accumulate(1)
        assert e.train_apply()['applied'] and e.last_dispatch() == marks and e.engine_id == _lib.ENGINE_FUSED
    finally:
        e.close()


# ---- 7. the trainer -------------------------------------------------------------------------------------------------------------
def trainer_config():
    config = syn.default_config()
    config['train'].update({'n_rollout': 3, 'n_history': 1, 'lr': 2e-4, 'adam_beta1': 0.9, 'log_per_iter': 1, 'n_epoch': 1})
    return config


def run_trainer(golden, batches, **kw):
    """-> (train()'s result, the log lines, the final weights, Adam's step count)"""
    import torch
    config = trainer_config()
    model = PropNetDiffDenModel(config, True)
    model.load_state_dict({k[2:]: torch.from_numpy(golden.weights_seed0[k]) for k in golden.weights_seed0.files
                           if k.startswith('w/')}, strict=False)
    lines = []
    try:
        r = TG.train(config, model, {'train': batches, 'valid': batches[:1]}, log=lines.append, **kw)
        return r, lines, model.engine.get_weights().copy(), model.engine.train_get_state()[2]
    finally:
        model.engine.close()


def test_the_trainer_accumulates_clips_and_keeps_todays_path_by_default(golden):
    batch = hand_made([12, 9], 3, seed=0) + [None]
    four = [hand_made([12, 9], 3, seed=k) + [None] for k in range(4)]
    plain = run_trainer(golden, four)
    defaults = run_trainer(golden, four, accum_steps=1, clip_norm=None)
    assert defaults[0] == plain[0] and defaults[1] == plain[1] and same(defaults[2], plain[2]) and plain[3] == 4
    assert 'skipped_updates' not in plain[0] and not any('GradNorm' in ln for ln in plain[1])
    # two batches per step on the same batch four times: the gradient of each group is the batch's own, bit for bit
    two = run_trainer(golden, [batch] * 2)
    grouped = run_trainer(golden, [batch] * 4, accum_steps=2)
    differ = int((bits(grouped[2]) != bits(two[2])).sum())
    print('[optim-trainer] accum_steps=2 on [batch] * 4 against plain training on [batch] * 2: %d of 38403 weights differ' % differ)
    assert differ == 0 and grouped[3] == two[3] == 2 and grouped[0]['skipped_updates'] == 0
    marked = [ln for ln in grouped[1] if 'GradNorm' in ln]
    assert [ln.split(' LR:')[0] for ln in marked] == ['train [0][1]', 'train [0][3]'], grouped[1]
    assert all(', Clip 1.0000' in ln for ln in marked)
    assert [h[:2] for h in grouped[0]['history']] == [(0, 'train'), (0, 'valid')]
    # a remainder group is applied at the end of the phase
    rest = run_trainer(golden, [batch] * 3, accum_steps=2)
    assert rest[3] == 2 and rest[0]['skipped_updates'] == 0
    assert [ln for ln in rest[1] if 'the last 1 batches applied' in ln and 'GradNorm' in ln], rest[1]
    # clipping: groups of one, every factor at most 1 and the norm in the log
    def logged(run):
        marked = [ln for ln in run[1] if ln.startswith('train') and 'GradNorm' in ln]
        return [float(ln.split('GradNorm ')[1].split(',')[0]) for ln in marked], [float(ln.split('Clip ')[1]) for ln in marked]

    measured = run_trainer(golden, four, clip_norm=float('inf'))           # measured and logged, never clipped
    norms, clips = logged(measured)
    assert len(norms) == 4 and all(n > 0 for n in norms) and clips == [1.0] * 4 and same(measured[2], plain[2])
    bound = 0.5 * min(norms)
    clipped = run_trainer(golden, four, clip_norm=bound)
    norms_c, clips_c = logged(clipped)
    print('[optim-trainer] unclipped GradNorm %s; clip_norm=%.3e: GradNorm %s Clip %s' % (norms, bound, norms_c, clips_c))
    assert len(clips_c) == 4 and clipped[3] == 4 and all(0.0 < c < 1.0 for c in clips_c) and norms_c[0] == norms[0]
    assert clips_c[0] <= 0.5
    assert not same(clipped[2], plain[2])
    with pytest.raises(ValueError, match='accum_steps'):
        run_trainer(golden, four, accum_steps=0)


class _Phase(object):
    def __init__(self, data_root, config, phase, cam, engine=None):
        self.phase = phase


def test_main_saves_adams_state_and_a_resumed_run_is_the_uninterrupted_one(eng, golden, tmp_path, monkeypatch):
    """main() over fixed batches (the loaders are replaced: what the files hold is the subject, not the data path): two epochs in
    one run against one epoch, then a run resumed from its last checkpoint over the same batches again"""
    from dyn_res_pile_manip_amd import dataset_gnn_dyn
    train_batches = [hand_made([12, 9], 3, seed=k) + [None] for k in range(3)]
    loaders = {'train': train_batches, 'valid': train_batches[:1]}
    monkeypatch.setattr(dataset_gnn_dyn, 'ParticleDataset', _Phase)
    monkeypatch.setattr(dataset_gnn_dyn, 'DeviceLoader', lambda ds, batch_size, **kw: loaders[ds.phase])

    def config(resume=None):
        c = TG.default_config()
        c['train'].update({'n_rollout': 3, 'log_per_iter': 1, 'ckp_per_iter': 1, 'lr': 2e-4})
        if resume is not None:
            c['train']['particle']['resume'] = {'active': True, 'epoch': resume[0], 'iter': resume[1], 'folder': 'x'}
        return c

    def weights_at(d, epoch, i):
        return weights.load_checkpoint(os.path.join(d, 'net_epoch_%d_iter_%d.pth' % (epoch, i)))

    d_u, d_a, d_c = (str(tmp_path / n) for n in 'uac')
    TG.main(config(), data_root='unused', train_dir=d_u, n_epoch=2, engine=eng, save_optimizer=True)
    TG.main(config(), data_root='unused', train_dir=d_a, n_epoch=1, engine=eng, save_optimizer=True)
    for e, i in ((0, 0), (0, 1), (0, 2)):
        assert os.path.exists(os.path.join(d_a, 'opt_epoch_%d_iter_%d.npz' % (e, i)))
    with np.load(os.path.join(d_a, 'opt_epoch_0_iter_2.npz')) as z:
        assert sorted(z.files) == ['iter', 'm', 'v'] and int(z['iter']) == 3 and z['m'].shape == z['v'].shape == (38403,)
        assert z['m'].dtype == z['v'].dtype == np.float32
    assert same(weights_at(d_a, 0, 2), weights_at(d_u, 0, 2))
    shutil.copytree(d_a, d_c)
    for f in os.listdir(d_c):
        if f.endswith('.npz'):
            os.remove(os.path.join(d_c, f))
    TG.main(config((0, 2)), data_root='unused', train_dir=d_a, n_epoch=1, engine=eng, save_optimizer=True)
    TG.main(config((0, 2)), data_root='unused', train_dir=d_c, n_epoch=1, engine=eng)
    want = weights_at(d_u, 1, 2)
    differ = int((bits(weights_at(d_a, 0, 2)) != bits(want)).sum())
    forgot = int((bits(weights_at(d_c, 0, 2)) != bits(want)).sum())
    print('[optim-main] resumed with Adam\'s state: %d of 38403 weights differ from the uninterrupted run; without it: %d' % (differ, forgot))
    assert differ == 0 and forgot > 1000
    with np.load(os.path.join(d_a, 'opt_epoch_0_iter_2.npz')) as z, np.load(os.path.join(d_u, 'opt_epoch_1_iter_2.npz')) as u:
        assert int(z['iter']) == int(u['iter']) == 6 and same(z['m'], u['m']) and same(z['v'], u['v'])
    assert not [f for f in os.listdir(d_c) if f.endswith('.npz')]          # off by default: the files a run writes are what they were
    assert 'resumed Adam' in open(os.path.join(d_a, 'log_resume_epoch_0_iter_2.txt')).read()

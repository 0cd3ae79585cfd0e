"""GPU, row y3: the training loop body in float64 on the device (drp_train_grad_f64), the probe that holds the trainer's fp32
gradients against it, and the trainer's hook.

Tolerance of the device against the float64 restatement (tests/_f64_train_ref.py; pinned to the reference's own model in double
and to its central differences by tests/test_f64_train_host.py): 1e-10 x the largest magnitude of the compared tensor, the
bound of tests/test_gpu_f64.py and tests/test_gpu_gd_f64.py -- both sides evaluate the same expressions in double on the same
graph and differ in summation order only.  Every figure is printed before it is asserted.

The probe's bound is the one tests/test_gpu_train.py already holds the trainer to against the reference's fp32 autograd:
2e-4 x max |g| per tensor."""
import numpy as np
import pytest

import _f64_train_ref as T
from dyn_res_pile_manip_amd import _lib, synthetic as syn, train_gnn_dyn as TG, weights
from dyn_res_pile_manip_amd._lib import DrpError
from dyn_res_pile_manip_amd.engine import Engine
from dyn_res_pile_manip_amd.gnn_dyn import PropNetDiffDenModel

pytestmark = pytest.mark.gpu
TOL = 1e-10
PROBE_TOL = 2e-4
BATCH_KEYS = ('states', 'states_delta', 'attrs', 'particle_nums', 'particle_dens')
CASES = [(b, w) for b in ('b4_r3', 'b2_r5') for w in ('seed0', 'trained')]


def weights_of(golden, wset):
    return golden.weights_seed0 if wset == 'seed0' else golden.weights_trained


def new_engine(w):
    e = Engine(0)
    if w is not None:
        e.load_weights(weights.blob_from_state_dict(w), 0.08)
    return e


@pytest.fixture(scope='module')
def engines(golden):
    es = {'seed0': new_engine(golden.weights_seed0), 'trained': new_engine(golden.weights_trained)}
    yield es
    for e in es.values():
        e.close()


def fixture_batch(golden, name):
    return [golden.train[name + '/' + k] for k in BATCH_KEYS]


_ref_cache = {}


def reference(golden, name, wset):
    """the restatement's (loss, terms, gradient blob, state gradient on real rows) of a fixture case, computed once"""
    if (name, wset) not in _ref_cache:
        batch = fixture_batch(golden, name)
        out = restate(weights_of(golden, wset), batch)
        for v in out[1:]:
            v.setflags(write=False)
        _ref_cache[(name, wset)] = out
    return _ref_cache[(name, wset)]


def restate(w, batch):
    loss, terms, grads, gs, graphs = T.train_loss_and_grads64(w, *batch, want_graphs=True)
    for adj in graphs:                          # the premise of the padded mode: no padded row is tied to a real one
        for b, n in enumerate(batch[3]):
            assert not adj[b, :n, n:].any() and not adj[b, n:, :n].any()
    return loss, terms, T.blob64(grads), T.real_rows(gs, batch[3])


def assert_close(got, want, nums, label):
    """got: train_grad_f64(..., want_state=True); want: restate(...)"""
    loss, terms, grad, gs = got
    rl, rt, rg, rgs = want
    worst = abs(loss - rl) / abs(rl)
    assert worst <= TOL, (label, 'loss', worst)
    assert terms.dtype == np.float64 and terms.shape == rt.shape
    err = float(np.abs(terms - rt).max() / np.abs(rt).max())
    assert err <= TOL, (label, 'loss_terms', err)
    assert grad.dtype == np.float64 and grad.shape == (38403,)
    off = 0
    for key, shape in weights.STATE_DICT_KEYS:
        n = int(np.prod(shape))
        a, b = grad[off:off + n], rg[off:off + n]
        err = float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))
        worst = max(worst, err)
        assert err <= TOL, (label, key, err)
        # inputs that are identically zero (the attribute columns) have exactly zero gradient
        np.testing.assert_array_equal(a[b == 0], 0.0)
        off += n
    gsr = T.real_rows(gs, nums)
    err = float(np.abs(gsr - rgs).max() / np.abs(rgs).max())
    worst = max(worst, err)
    assert err <= TOL, (label, 'grad_state', err)
    print('[train-f64] %s: worst error %.2e of a tensor\'s largest value' % (label, worst))
    return worst


# ---- 1. against the restatement ------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,wset', CASES)
def test_matches_the_float64_restatement(engines, golden, name, wset):
    e = engines[wset]
    batch = fixture_batch(golden, name)
    got = e.train_grad_f64(*batch, want_state=True)
    assert_close(got, reference(golden, name, wset), batch[3], '%s %s' % (name, wset))
    loss, terms, grad = e.train_grad_f64(*batch)                # the state gradient is optional
    assert loss == got[0]
    np.testing.assert_array_equal(grad, got[2])


def hand_made(nums, H, seed=0):
    """collate_fn's layout by hand (the construction of test_gpu_train.py): piles away from the origin, where the padding sits"""
    rng = np.random.default_rng(seed)
    B, N = len(nums), max(nums)
    states = np.zeros((B, H + 1, N, 3), np.float32)
    sdelta = np.zeros((B, H, N, 3), np.float32)
    attrs = np.zeros((B, H + 1, N), np.float32)
    dens = np.array([300.0 + 50 * b for b in range(B)], np.float32)
    for b, n in enumerate(nums):
        s, _, _ = syn.make_pile(n, 1, seed=5 + b + seed, kind='blob')
        for t in range(H + 1):
            states[b, t, :n] = s[0] * 0.3 + 0.002 * t * rng.standard_normal((n, 3)).astype(np.float32) + [0, 0, 0.52]
        sdelta[b, :, :n] = 0.004 * rng.standard_normal((H, n, 3)).astype(np.float32)
    return [states, sdelta, attrs, np.asarray(nums, np.int32), dens]


@pytest.mark.parametrize('nums,H', [((3,), 2), ((5, 17, 16), 1), ((5, 17, 16), 3), ((20, 20), 3), ((33,), 1)])
def test_tile_and_count_edges(engines, golden, nums, H):
    """one sample of 3 particles (fewer than the in-degree cap); row counts of 5, 16 and 17 (x 10 slots) around the 16-row tiles
    and the 4-row k-steps, padded to 17; an unpadded batch; a single rollout step"""
    batch = hand_made(list(nums), H)
    got = engines['seed0'].train_grad_f64(*batch, want_state=True)
    assert_close(got, restate(golden.weights_seed0, batch), batch[3], 'nums=%s H=%d' % (nums, H))


# ---- 2. one value, one order ------------------------------------------------------------------------------------------
def test_same_bits_from_run_to_run_and_under_any_cap(engines, golden):
    e = engines['seed0']
    for name in ('b4_r3', 'b2_r5'):
        batch = fixture_batch(golden, name)
        whole = e.train_grad_f64(*batch, want_state=True)
        again = e.train_grad_f64(*batch, want_state=True)
        try:
            e.set_f64_cap(1)                                    # one sample is the smallest chunk: B chunks
            single = e.train_grad_f64(*batch, want_state=True)
        finally:
            e.set_f64_cap(0)
        for a, b, c in zip(whole, again, single):
            np.testing.assert_array_equal(np.asarray(a), np.asarray(b))
            np.testing.assert_array_equal(np.asarray(a), np.asarray(c))
    batch = fixture_batch(golden, 'b4_r3')                      # 4 samples of 64 rows and 3 steps: two samples a chunk
    whole = e.train_grad_f64(*batch)
    try:
        one = _lib_cap_for(e, batch, 2)
        e.set_f64_cap(one)
        for a, b in zip(whole, e.train_grad_f64(*batch)):
            np.testing.assert_array_equal(np.asarray(a), np.asarray(b))
    finally:
        e.set_f64_cap(0)


def _lib_cap_for(e, batch, samples):
    """a cap that holds `samples` samples of this batch but not one more, from the figures include/drp.h gives: tape 24 KB per
    particle and step, the reverse pass and the weight gradients' operands 42 KB per particle (rounded up to 52), 307 KB of
    accumulators per sample"""
    B, T1, N, _ = batch[0].shape
    per = (24 * 1024 * (T1 - 1) + 52 * 1024) * N + 307 * 1024
    return int(per * (samples + 0.5))


# ---- 3. the weights an optimiser step left ----------------------------------------------------------------------------
def test_the_gradient_uses_the_weights_an_optimiser_step_left(golden):
    batch = fixture_batch(golden, 'b2_r5')
    e = new_engine(golden.weights_seed0)
    try:
        before = e.train_grad_f64(*batch)
        e.train_begin(batch[0].shape[1] - 1, 1e-3, 0.9)
        e.train_step(*batch, mode='update')
        after = e.train_grad_f64(*batch, want_state=True)
        assert np.abs(after[2] - before[2]).max() > 0
        assert_close(after, restate(weights.state_dict_from_blob(e.get_weights()), batch), batch[3], 'after an optimiser step')
    finally:
        e.close()


# ---- 4. isolation -----------------------------------------------------------------------------------------------------
def adam_trajectory(golden, disturbed):
    batch = fixture_batch(golden, 'b2_r5')
    other = hand_made([5, 17, 16], 5, seed=3)
    e = new_engine(golden.weights_seed0)
    out = []
    try:
        e.train_begin(batch[0].shape[1] - 1, 1e-3, 0.9)
        for it in range(6):
            if disturbed:
                e.train_grad_f64(*(batch if it % 2 else other))
                e.train_gradient_probe(*batch)
            loss, grad = e.train_step(*batch, mode='update', want_grad=True)
            out += [np.float64(loss), grad, e.get_weights()]
    finally:
        e.close()
    return out


def test_an_adam_trajectory_is_not_disturbed(golden):
    plain, mixed = adam_trajectory(golden, False), adam_trajectory(golden, True)
    assert len(plain) == len(mixed) == 18
    for a, b in zip(plain, mixed):
        np.testing.assert_array_equal(a, b)


def test_sessions_engine_dispatch_and_taps_are_left_alone(engines, golden):
    from dyn_res_pile_manip_amd.planners import world2cam_affine
    batch = fixture_batch(golden, 'b2_r5')
    G = syn.goal_field(syn.goal_distance_image(syn.goal_mask('I')))
    lo, hi = syn.action_limits()

    def gd_run(disturbed):
        e = new_engine(golden.weights_seed0)
        out = []
        try:
            e.set_camera(world2cam_affine(syn.demo_cam_extrinsics()), 24.0, syn.demo_cam_params())
            e.set_goal(G, syn.goal_coor_strided(syn.goal_distance_image(syn.goal_mask('I')), 200))
            s0, dens, attr = syn.make_pile(40, 1, seed=0)
            e.gd_begin(s0, attr, dens, syn.sample_pushes(4, 2, seed=0), 0.05, lo, hi)
            for _ in range(3):
                out.append(e.gd_step())
                if disturbed:
                    e.train_grad_f64(*batch)
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
        e.train_grad_f64(*batch)
        assert e.engine_id == _lib.ENGINES['split'] and e.last_dispatch() == marks
        np.testing.assert_array_equal(e.f64_tap('effect_1'), tap)      # taps of the earlier call are still answered
    finally:
        e.set_engine('fused')


# ---- 5. refusals ----------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(golden):
    batch = fixture_batch(golden, 'b2_r5')
    st, sd, at, nums, dens = batch
    e = Engine(0)
    try:
        with pytest.raises(DrpError, match='weights not loaded'):
            e.train_grad_f64(*batch)
        e.load_weights(weights.blob_from_state_dict(golden.weights_seed0), 0.08)
        good = e.train_grad_f64(*batch, want_state=True)          # no train_begin needed
        with pytest.raises(DrpError, match='bad shape'):
            e.train_grad_f64(st[:0], sd[:0], at[:0], nums[:0], dens[:0])
        with pytest.raises(DrpError, match='bad shape'):
            e.train_grad_f64(st[:, :, :0], sd[:, :, :0], at[:, :, :0], nums, dens)
        with pytest.raises(DrpError, match='bad n_rollout'):
            e.train_grad_f64(st[:, :1], sd[:, :0], at[:, :1], nums, dens)
        long = [np.zeros((1, 66, 2, 3), np.float32), np.zeros((1, 65, 2, 3), np.float32), np.zeros((1, 66, 2), np.float32),
                np.array([2], np.int32), np.ones(1, np.float32)]
        with pytest.raises(DrpError, match='bad n_rollout'):
            e.train_grad_f64(*long)
        big = [np.zeros((1, 2, 5000, 3), np.float32), np.zeros((1, 1, 5000, 3), np.float32), np.zeros((1, 2, 5000), np.float32),
               np.array([5000], np.int32), np.ones(1, np.float32)]
        with pytest.raises(DrpError, match='N <= 4096'):
            e.train_grad_f64(*big)
        for bad in (0, -1, st.shape[2] + 1):
            with pytest.raises(DrpError, match='particle_nums'):
                e.train_grad_f64(st, sd, at, np.array([nums[0], bad], np.int32), dens)
        rc = e.lib.drp_train_grad_f64(e.h, None, None, None, None, None, 2, 30, 5, None, None, None, None)
        assert rc == -1 and 'null argument' in e.lib.drp_last_error(e.h).decode()     # DRP_EINVAL
        for a, b in zip(e.train_grad_f64(*batch, want_state=True), good):
            np.testing.assert_array_equal(np.asarray(a), np.asarray(b))
        assert_close(good, reference(golden, 'b2_r5', 'seed0'), nums, 'after the refusals')
    finally:
        e.close()


# ---- 6. the probe -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tape', ['fused', 'mfma'])
@pytest.mark.parametrize('name,wset', CASES)
def test_train_gradient_probe_is_what_numpy_computes(engines, golden, name, wset, tape):
    e = engines[wset]
    batch = fixture_batch(golden, name)
    e.set_engine(tape)
    try:
        e.train_begin(batch[0].shape[1] - 1, 1e-3, 0.9)
        p = e.train_gradient_probe(*batch)
        assert p['tape'] == tape
        loss32, g32 = e.train_step(*batch, mode='grad', want_grad=True)
        loss64, _, g64 = e.train_grad_f64(*batch)
        assert p['loss32'] == loss32 and p['loss64'] == loss64 and p['loss_diff'] == abs(loss32 - loss64)
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
        print('[train-probe] %s %s %s: worst %s rel %.3e, loss diff %.3e' % (name, wset, tape, p['worst'], p['rel'], p['loss_diff']))
        for key, r in rels.items():
            print('[train-probe]     %-45s %.3e' % (key, r))
            assert r <= PROBE_TOL, (key, r)
    finally:
        e.set_engine('fused')


# ---- 7. the trainer's hook ----------------------------------------------------------------------------------------------
def test_the_trainers_probe_hook_changes_no_weight(golden):
    import torch
    config = syn.default_config()
    config['train'].update({'n_rollout': 3, 'n_history': 1, 'lr': 2e-4, 'adam_beta1': 0.9, 'log_per_iter': 1, 'n_epoch': 1})
    batches = [hand_made([12, 9], 3, seed=s) + [None] for s in range(4)]
    res, lines = {}, {}
    for every in (0, 2):
        model = PropNetDiffDenModel(config, True)
        model.load_state_dict({k[2:]: torch.from_numpy(golden.weights_seed0[k]) for k in golden.weights_seed0.files
                               if k.startswith('w/')}, strict=False)
        lines[every] = []
        r = TG.train(config, model, {'train': batches, 'valid': batches[:1]}, log=lines[every].append, grad_probe_every=every)
        res[every] = (r, model.engine.get_weights().copy())
        model.engine.close()
    np.testing.assert_array_equal(res[0][1], res[2][1])
    probes = [h for h in res[2][0]['history'] if h[1] == 'grad_probe']
    assert len(probes) == 2 and all(0 < h[2] < PROBE_TOL for h in probes)
    assert [h for h in res[2][0]['history'] if h[1] != 'grad_probe'] == res[0][0]['history']
    assert [ln for ln in lines[2] if not ln.startswith('grad_probe')] == lines[0]
    assert len([ln for ln in lines[2] if ln.startswith('grad_probe')]) == 2


# ---- 8. the planner's float64 gradient shares this call's buffers -----------------------------------------------------
def test_interleaved_with_gd_grad_f64_on_one_engine(golden):
    """drp_gd_grad_f64 and drp_train_grad_f64 carve their workspaces from the same two buffers of the context: called in turn on
    one engine, with shapes that make every call find the buffers as another layout left them, each result is the bits of the
    same call on a fresh engine that has made no other float64 call"""
    from test_gpu_gd_f64 import M34, CAM, args_of, synthetic_case
    G = syn.goal_field(syn.goal_distance_image(syn.goal_mask('I')))
    case = synthetic_case(17, 3, 2, seed=17)

    def gd(e):
        return e.gd_grad_f64(*args_of(case), want_state_grad=True)
    calls = [gd, lambda e: e.train_grad_f64(*hand_made([5, 17, 16], 3), want_state=True), gd,
             lambda e: e.train_grad_f64(*hand_made([33], 1), want_state=True)]

    def engine():
        e = new_engine(golden.weights_seed0)
        e.set_camera(M34, 24.0, CAM)
        e.set_goal(G, case['goal_coor'])
        return e
    shared = engine()
    try:
        for q, call in enumerate(calls):
            got = call(shared)
            fresh = engine()
            try:
                want = call(fresh)
            finally:
                fresh.close()
            assert len(got) == len(want)
            for a, b in zip(got, want):
                np.testing.assert_array_equal(np.asarray(a), np.asarray(b), err_msg='call %d' % q)
    finally:
        shared.close()

"""GPU, row y2: one iteration of the gradient-descent planner in float64 on the device (drp_gd_grad_f64), the gradient probe
that holds the tape engines against it, and the guard of load_weights(max_grad_rel=...).

Tolerance of the device against the float64 restatement (tests/_f64_grad_ref.py; pinned to the reference's own autograd by
tests/test_f64_grad_host.py): 1e-10 x the largest magnitude of the compared array, the derived float64 tolerance of
tests/test_gpu_f64.py -- both sides evaluate the same expressions in double on the same graph and differ in summation order
only; the argument there (error ~ depth x width x 2^-53 x the activations' growth) carries over with twice the layer depth per
step, forward and reverse.  Measured: at most 2.7e-15 on the nine fixture cases.

The probe's bounds are 5 x the worst measured `rel` per weight set and tape, measured against the float64 call."""
import warnings

import numpy as np
import pytest

import _f64_grad_ref as R
from dyn_res_pile_manip_amd import _lib, synthetic as syn, weights
from dyn_res_pile_manip_amd._lib import DrpError
from dyn_res_pile_manip_amd.engine import Engine
from dyn_res_pile_manip_amd.planners import world2cam_affine
from test_f64_grad_host import case_inputs

pytestmark = pytest.mark.gpu
TOL = 1e-10
CASES = [('seed0', 'h1'), ('seed0', 'h2'), ('seed0', 'h1_n100'), ('stress', 'seed1_attr_h1'), ('stress', 'big_attr_h2'),
         ('trained', 'n20_h1'), ('trained', 'n20_h2'), ('trained', 'n50_h2'), ('trained', 'n100_h2')]
# 5 x the worst measured rel = max |g32 - g64| / max |g64| of gradient_probe per weight set and tape
# measured: seed-0 8.1e-7 / 1.03e-6, stress 1.29e-6 / 1.05e-6, trained 7.5e-6 / 1.95e-6 (fused / mfma)
PROBE_BOUND = {('seed0', 'fused'): 4.1e-6, ('seed0', 'mfma'): 5.2e-6, ('stress', 'fused'): 6.5e-6, ('stress', 'mfma'): 5.3e-6,
               ('trained', 'fused'): 3.8e-5, ('trained', 'mfma'): 9.8e-6}
M34 = world2cam_affine(syn.demo_cam_extrinsics())
CAM = syn.demo_cam_params()
LO, HI = syn.action_limits()


@pytest.fixture(scope='module')
def G():
    return syn.goal_field(syn.goal_distance_image(syn.goal_mask('I')))


def new_engine(w):
    e = Engine(0)
    if w is not None:
        e.load_weights(weights.blob_from_state_dict(w), 0.08)
    e.set_camera(M34, 24.0, CAM)
    return e


@pytest.fixture(scope='module')
def engines(golden):
    """one context per weight set that has a single blob; the stress cases bring their own"""
    es = {'seed0': new_engine(golden.weights_seed0), 'trained': new_engine(golden.weights_trained)}
    yield es
    for e in es.values():
        e.close()


_ref_cache = {}


def reference(golden, G, wset, case):
    """(weights, inputs, restatement's (reward, grad_act, grad_state)) of a fixture case, computed once"""
    if (wset, case) not in _ref_cache:
        w, c = case_inputs(golden, wset, case)
        out = R.gd_loss_and_grads64(w, c['s_cur'], c['dens'], c['attr'], c['act_seqs'], G, CAM, c['goal_coor'], M34, 24.0)
        for v in out:
            v.setflags(write=False)
        _ref_cache[(wset, case)] = (w, c, out)
    return _ref_cache[(wset, case)]


def engine_for(engines, golden, G, wset, case):
    w, c, _ = reference(golden, G, wset, case)
    e = engines[wset] if wset in engines else new_engine(w)
    e.set_goal(G, c['goal_coor'])
    return e, wset not in engines


def args_of(c):
    return c['s_cur'], c['attr'], c['dens'], c['act_seqs']


def assert_close(got, want, label):
    worst = 0.0
    for name, a, b in zip(('reward', 'grad_act', 'grad_state'), got, want):
        assert a.dtype == np.float64 and a.shape == b.shape, (label, name)
        err = float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))
        worst = max(worst, err)
        assert err <= TOL, (label, name, err)
    print('[gd-f64] %s: worst error %.2e of the largest value' % (label, worst))
    return worst


# ---- 1. against the restatement ------------------------------------------------------------------------------------
@pytest.mark.parametrize('wset,case', CASES)
def test_matches_the_float64_restatement(engines, golden, G, wset, case):
    e, own = engine_for(engines, golden, G, wset, case)
    try:
        _, c, ref = reference(golden, G, wset, case)
        assert_close(e.gd_grad_f64(*args_of(c), want_state_grad=True), ref, '%s %s' % (wset, case))
        r, ga = e.gd_grad_f64(*args_of(c))                      # the state gradient is optional
        np.testing.assert_array_equal(ga, e.gd_grad_f64(*args_of(c), want_state_grad=True)[1])
    finally:
        if own:
            e.close()


# ---- 2. tile and count edges ------------------------------------------------------------------------------------------
def synthetic_case(N, B, H, seed, clump=False, acts=None):
    s0, dens, attr = syn.make_pile(N, 1, seed=seed)
    if clump:       # every particle drawn towards the first until each list is full (the construction of test_gpu_f64.py)
        s0[0, :, :2] = s0[0, :1, :2] + 1e-3 * (s0[0, :, :2] - s0[0, :1, :2])
    acts = syn.sample_pushes(B, H, seed=seed).astype(np.float32) if acts is None else acts
    coor = syn.goal_coor_strided(syn.goal_distance_image(syn.goal_mask('I')), 5 * N)
    return {'s_cur': s0, 'dens': dens, 'attr': attr, 'act_seqs': acts, 'goal_coor': coor}


def restate(w, c, G, **kw):
    return R.gd_loss_and_grads64(w, c['s_cur'], c['dens'], c['attr'], c['act_seqs'], G, CAM, c['goal_coor'], M34, 24.0, **kw)


@pytest.mark.parametrize('N,B,H,clump', [(5, 1, 1, False), (17, 3, 2, False), (64, 2, 3, False), (24, 2, 1, True)])
def test_tile_and_count_edges(engines, golden, G, N, B, H, clump):
    e = engines['seed0']
    c = synthetic_case(N, B, H, seed=N, clump=clump)
    e.set_goal(G, c['goal_coor'])
    if clump:
        sd = e.gen_s_delta(np.repeat(c['s_cur'], B, 0), c['act_seqs'][:, 0])
        assert e.build_graph(np.repeat(c['s_cur'], B, 0), sd)[1].min() == 10          # every list is full
    assert_close(e.gd_grad_f64(*args_of(c), want_state_grad=True), restate(golden.weights_seed0, c, G),
                 'N=%d B=%d H=%d%s' % (N, B, H, ' clump' if clump else ''))


def test_a_push_that_misses_the_pile(engines, golden, G):
    """the pile lies within +-0.2 camera units of the origin: a short push in a corner of the workspace moves nothing, so
    nothing reaches the push through s_delta -- the gradient is exactly zero -- while the reward and its gradient are as ever"""
    e = engines['seed0']
    acts = np.array([[[7.5, 7.5, 7.9, 7.9]], [[-7.5, 7.0, -7.9, 7.4]]], np.float32)
    c = synthetic_case(33, 2, 1, seed=5, acts=acts)
    e.set_goal(G, c['goal_coor'])
    ref = restate(golden.weights_seed0, c, G, want_decisions=True)
    assert not ref[3][1].any()                                                        # the hard mask is off everywhere
    r, ga, gs = e.gd_grad_f64(*args_of(c), want_state_grad=True)
    assert_close((r, ga, gs), ref[:3], 'a push that misses')
    assert np.all(ga == 0) and np.all(np.isfinite(r)) and np.all(np.isfinite(gs)) and np.abs(gs).max() > 0


# ---- 3. directional derivative on the device, independent of any restatement ----------------------------------------------
@pytest.mark.parametrize('wset,case', [('trained', 'n20_h1'), ('seed0', 'h2')])
def test_directional_derivative_of_the_devices_own_rewards(engines, golden, G, wset, case):
    """(sum r(a + h d) - sum r(a - h d)) / 2h from the call's own float64 rewards against -g . d, on points that are exact in
    fp32 (R.fd_point / fd_direction); bound: 10 x the residual the host test recorded for the restatement at the same h -- both
    are double evaluations of the same function.  A direction along which a discrete decision flips (read from the
    restatement at the same points) is redrawn, at most 2 of them."""
    e, _ = engine_for(engines, golden, G, wset, case)
    w, c, _ = reference(golden, G, wset, case)

    def fn(a):
        assert np.array_equal(a.astype(np.float32).astype(np.float64), a)
        r, ga = e.gd_grad_f64(c['s_cur'], c['attr'], c['dens'], a.astype(np.float32))
        return r, ga, restate(w, dict(c, act_seqs=a), G, want_decisions=True)[3]
    res = R.fd_check(fn, c['act_seqs'], n_dir=4, max_redraw=2)
    gnorm = float(np.linalg.norm(fn(R.fd_point(c['act_seqs']))[1]))
    worst = max(abs(cd - an) for cd, an in res) / gnorm
    print('[gd-f64] %s %s: directional derivative, worst residual %.3e of |g| (host: %.3e)' % (wset, case, worst, R.FD_RESIDUAL[case]))
    assert worst <= 10 * R.FD_RESIDUAL[case]


# ---- 4. one value, one order ------------------------------------------------------------------------------------------
def test_same_bits_alone_in_any_batch_run_and_chunking(engines, golden, G):
    e, _ = engine_for(engines, golden, G, 'seed0', 'h1')
    _, c, _ = reference(golden, G, 'seed0', 'h1')                      # 30 rows = 10 pushes x 3 piles
    full = e.gd_grad_f64(*args_of(c), want_state_grad=True)
    again = e.gd_grad_f64(*args_of(c), want_state_grad=True)
    # row 7 = push 2 on pile 1: alone, and in a batch of 8 with that pile only
    alone = e.gd_grad_f64(c['s_cur'][1:2], c['attr'][1:2], c['dens'][1:2], c['act_seqs'][7:8], want_state_grad=True)
    eight = e.gd_grad_f64(c['s_cur'][1:2], c['attr'][1:2], c['dens'][1:2], c['act_seqs'][[1, 4, 7, 10, 13, 16, 19, 22]],
                          want_state_grad=True)
    for a, b, o, f in zip(full, again, alone, eight):
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(o[0], a[7])
        np.testing.assert_array_equal(f[2], a[7])
    e2, _ = engine_for(engines, golden, G, 'seed0', 'h2')
    _, c2, _ = reference(golden, G, 'seed0', 'h2')                     # 8 rows, H = 2
    whole = e2.gd_grad_f64(*args_of(c2), want_state_grad=True)
    try:
        e2.set_f64_cap(1)                                              # one row is the smallest chunk: 8 chunks
        for a, b in zip(whole, e2.gd_grad_f64(*args_of(c2), want_state_grad=True)):
            np.testing.assert_array_equal(a, b)
        e2.set_f64_cap(7 << 20)                                        # 2.1 MB a row at 32 particles and 2 steps: 3 rows a chunk
        for a, b in zip(whole, e2.gd_grad_f64(*args_of(c2), want_state_grad=True)):
            np.testing.assert_array_equal(a, b)
    finally:
        e2.set_f64_cap(0)


# ---- 5. isolation -----------------------------------------------------------------------------------------------------
def run_sessions(w, G, disturbed, c):
    e = new_engine(w)
    out = []
    try:
        e.set_goal(G, c['goal_coor'])
        s0, dens, attr = syn.make_pile(40, 1, seed=0)
        e.gd_begin(s0, attr, dens, syn.sample_pushes(4, 2, seed=0), 0.05, LO, HI)
        for _ in range(3):
            out.append(e.gd_step())
            if disturbed:
                e.gd_grad_f64(*args_of(c))
        out.append(e.gd_actions())
        e.mpc_begin(s0, attr, dens, syn.nominal_pushes(2, seed=0), n_sample=8, sigma=0.6, beta_filter=0.7, reward_weight=0.1,
                    act_lo=LO, act_hi=HI, seed=1)
        for it in range(2):
            e.mpc_sample(it)
            if disturbed:
                e.gd_grad_f64(*args_of(c))
            e.mpc_rollout()
            if disturbed:
                e.gd_grad_f64(*args_of(c))
            out.append(e.mpc_update(e.mpc_partials()))
        out.append(e.mpc_get(rewards=True, states=True)['rewards'])
        assert e.engine_id == _lib.ENGINE_FUSED
    finally:
        e.close()
    return out


def test_sessions_engine_dispatch_and_taps_are_left_alone(engines, golden, G):
    _, c, _ = reference(golden, G, 'seed0', 'h2')
    plain = run_sessions(golden.weights_seed0, G, False, c)
    mixed = run_sessions(golden.weights_seed0, G, True, c)
    assert len(plain) == len(mixed)
    for a, b in zip(plain, mixed):
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b))
    e, _ = engine_for(engines, golden, G, 'seed0', 'h2')
    e.set_engine('split')
    try:
        s, dens, attr = syn.make_pile(20, 2, seed=1)
        sd = e.gen_s_delta(s, syn.sample_pushes(2, 1, seed=1)[:, 0])
        e.dispatch_reset()
        e.step(attr, s, sd, dens)
        e.step_f64(attr, s, sd, dens)
        marks, tap = e.last_dispatch(), e.f64_tap('effect_1')
        e.gd_grad_f64(*args_of(c))
        assert e.engine_id == _lib.ENGINES['split'] and e.last_dispatch() == marks
        np.testing.assert_array_equal(e.f64_tap('effect_1'), tap)      # taps of the earlier call are still answered
    finally:
        e.set_engine('fused')


def test_the_gradient_uses_the_weights_an_optimiser_step_left(golden, G):
    g = golden.train
    batch = [g['b4_r3/' + k] for k in ('states', 'states_delta', 'attrs', 'particle_nums', 'particle_dens')]
    _, c, ref = reference(golden, G, 'seed0', 'h2')
    e = new_engine(golden.weights_seed0)
    try:
        e.set_goal(G, c['goal_coor'])
        before = e.gd_grad_f64(*args_of(c))
        e.train_begin(batch[0].shape[1] - 1, 1e-3, 0.9)
        e.train_step(*batch, mode='update')
        after = e.gd_grad_f64(*args_of(c), want_state_grad=True)
        assert np.abs(after[1] - before[1]).max() > 0
        assert_close(after, restate(weights.state_dict_from_blob(e.get_weights()), c, G), 'after an optimiser step')
    finally:
        e.close()


# ---- 6. refusals ----------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(golden, G):
    _, c, ref = reference(golden, G, 'seed0', 'h2')
    a = args_of(c)
    e = Engine(0)
    try:
        with pytest.raises(DrpError, match='weights not loaded'):
            e.gd_grad_f64(*a)
        e.load_weights(weights.blob_from_state_dict(golden.weights_seed0), 0.08)
        with pytest.raises(DrpError, match='camera not set'):
            e.gd_grad_f64(*a)
        e.set_camera(M34, 24.0, CAM)
        with pytest.raises(DrpError, match='goal'):
            e.gd_grad_f64(*a)
        with pytest.raises(ValueError, match='max_grad_rel needs the camera and a goal'):
            e.load_weights(weights.blob_from_state_dict(golden.weights_seed0), 0.08, probe=True, max_grad_rel=1.0)
        with pytest.raises(DrpError, match='goal'):                                 # the probe has invented none
            e.gd_grad_f64(*a)
        e.set_goal(G, c['goal_coor'])
        good = e.gd_grad_f64(*a, want_state_grad=True)
        with pytest.raises(DrpError, match='multiple of n_batch'):
            e.gd_grad_f64(a[0], a[1], a[2], a[3][:7])
        with pytest.raises(DrpError, match='bad shape'):
            e.gd_grad_f64(a[0], a[1], a[2], a[3][:0])
        with pytest.raises(DrpError, match='bad shape'):
            e.gd_grad_f64(a[0][:, :0], a[1][:, :0], a[2], a[3])
        with pytest.raises(DrpError, match='bad horizon'):
            e.gd_grad_f64(a[0], a[1], a[2], a[3][:, :0])
        with pytest.raises(DrpError, match='multiple of n_batch'):
            e.gd_grad_f64(a[0][:0], a[1][:0], a[2][:0], a[3])
        big = np.zeros((1, 5000, 3), np.float32)
        with pytest.raises(DrpError, match='N <= 4096'):
            e.gd_grad_f64(big, np.zeros((1, 5000), np.float32), np.ones(1, np.float32), a[3][:1])
        for x, y in zip(e.gd_grad_f64(*a, want_state_grad=True), good):
            np.testing.assert_array_equal(x, y)
        assert_close(good, ref, 'after the refusals')
    finally:
        e.close()


# ---- 7. the probe and the guard ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('tape', ['fused', 'mfma'])
@pytest.mark.parametrize('wset,case', CASES)
def test_gradient_probe_is_what_numpy_computes(engines, golden, G, wset, case, tape):
    e, own = engine_for(engines, golden, G, wset, case)
    try:
        _, c, _ = reference(golden, G, wset, case)
        e.set_engine(tape)
        p = e.gradient_probe(*args_of(c), LO, HI)
        assert p['tape'] == tape
        r32, g32, _ = e.gd_grad()                                   # the probe's session is still there: the same tape
        r64, g64 = e.gd_grad_f64(*args_of(c))
        err = np.abs(g32.astype(np.float64) - g64)
        assert p['abs'] == err.max() and p['scale'] == np.abs(g64).max() and p['rel'] == err.max() / np.abs(g64).max()
        assert p['worst'] == int(np.argmax(err.ravel()))
        assert p['reward_rel'] == np.abs(r32.astype(np.float64) - r64).max() / np.abs(r64).max()
        print('[grad-probe] %s %s %s: rel %.3e reward_rel %.3e' % (wset, case, tape, p['rel'], p['reward_rel']))
        assert p['rel'] < PROBE_BOUND[(wset, tape)]
    finally:
        e.set_engine('fused')
        if own:
            e.close()


def test_lite_selected_probes_the_fused_tape(engines, golden, G):
    e, _ = engine_for(engines, golden, G, 'seed0', 'h2')
    _, c, _ = reference(golden, G, 'seed0', 'h2')
    fused = e.gradient_probe(*args_of(c), LO, HI)
    e.set_engine('lite')
    try:
        lite = e.gradient_probe(*args_of(c), LO, HI)
    finally:
        e.set_engine('fused')
    assert lite['tape'] == 'fused' and lite == fused                # the tape does not depend on the choice


def test_the_guard_of_load_weights(golden, G):
    """No threshold is asserted BETWEEN the two tapes: on the guard's own batch their measured figures are within 2 x of each
    other on every weight set (seed-0 4.0e-7 fused / 7.2e-7 fp32, trained 8.8e-7 / 5.5e-7), so no threshold would
    separate them robustly.  The fallback and its single warning are exercised by the threshold neither tape can meet."""
    blob = weights.blob_from_state_dict(golden.weights_seed0)
    _, c, _ = reference(golden, G, 'seed0', 'h2')
    e = new_engine(None)
    try:
        e.set_goal(G, c['goal_coor'])
        e.set_engine('fused')
        with warnings.catch_warnings():
            warnings.simplefilter('error')
            e.load_weights(blob, 0.08, probe=True, max_grad_rel=1.0)
        gp = e.range_info()['grad_probe']
        assert gp['tape'] == 'fused' and 0 < gp['rel'] < 1.0 and e.engine_id == _lib.ENGINE_FUSED
        assert 'probe' in e.range_info()
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter('always')
            with pytest.raises(DrpError, match='nowhere to fall back'):
                e.load_weights(blob, 0.08, probe=True, max_grad_rel=1e-12)
        assert len([x for x in rec if issubclass(x.category, RuntimeWarning)]) == 1
        assert e.range_info()['grad_probe']['tape'] == 'mfma'
        e.load_weights(blob, 0.08)                                  # a plain load restores the caller's choice
        assert e.engine_id == _lib.ENGINE_FUSED and 'grad_probe' not in e.range_info()
    finally:
        e.close()

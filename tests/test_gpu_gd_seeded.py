"""GPU: the GD planner on a cost of the caller's -- drp_gd_begin_cost, drp_gd_predict, drp_gd_grad_seeded, drp_gd_step_seeded.

Bounds.  The seam is held to NUMBERS EQUAL: with a seed that is zero but for the last step, where it is drp_gd_grad's own
d loss / d state_{H-1}, the seeded calls return what drp_gd_grad / drp_gd_step return (np.array_equal: a zero may differ in
sign, x + 0.0 turns -0.0 into +0.0), on both tapes, both weight sets and every shape; drp_gd_predict is held to bits.  With
seeds on every step (costs.quadratic_cost) the fp32 gradient is held against drp_gd_grad_f64_seeded on the widened seed:
ALL_STEP_BOUND is 5 x the worst measured max |g32 - g64| / max |g64| per weight set and tape, as PROBE_BOUND of
tests/test_gpu_gd_f64.py is, and refused above 1e-4, load_weights(max_grad_rel=)'s default guard.

Shapes: nb = 2, B = 4; N in {17 (a partial tile), 20 (the small-pile rows kernel), 65 (one past a 64-row tile)}; H in {1 (the
rev_built branch, no intermediate seed), 2, 3 (two intermediate seeds)}."""
import ctypes

import numpy as np
import pytest

import _gd_seeded_ref as S
from dyn_res_pile_manip_amd import costs, synthetic as syn, weights
from dyn_res_pile_manip_amd._lib import DrpError
from dyn_res_pile_manip_amd.engine import Engine
from dyn_res_pile_manip_amd.planners import world2cam_affine

pytestmark = pytest.mark.gpu
M34 = world2cam_affine(syn.demo_cam_extrinsics())
CAM = syn.demo_cam_params()
LO, HI = syn.action_limits()
SHAPES = [(N, H) for N in (17, 20, 65) for H in (1, 2, 3)]
WSETS = ('seed0', 'trained')
TAPES = ('fused', 'mfma')
# 5 x the worst measured max |g32 - g64| / max |g64| over SHAPES, seeds on every step
# measured: seed-0 9.61e-7 / 2.07e-6, trained 3.10e-6 / 5.12e-6 (fused / mfma)
ALL_STEP_BOUND = {('seed0', 'fused'): 4.8e-6, ('seed0', 'mfma'): 1.03e-5, ('trained', 'fused'): 1.55e-5, ('trained', 'mfma'): 2.56e-5}
f32p = ctypes.POINTER(ctypes.c_float)


@pytest.fixture(scope='module')
def G():
    return syn.goal_field(syn.goal_distance_image(syn.goal_mask('I')))


def new_engine(w, goal=None):
    e = Engine(0)
    e.load_weights(weights.blob_from_state_dict(w), 0.08)
    e.set_camera(M34, 24.0, CAM)
    if goal is not None:
        e.set_goal(*goal)
    return e


@pytest.fixture(scope='module')
def engines(golden):
    """per weight set: a context, its twin, and one that never sees a goal"""
    ws = {'seed0': golden.weights_seed0, 'trained': golden.weights_trained}
    es = {k: (new_engine(w), new_engine(w), new_engine(w)) for k, w in ws.items()}
    yield es
    for trio in es.values():
        for e in trio:
            e.close()


_cases = {}


def case(N, H):
    if (N, H) not in _cases:
        c = S.make_case(N, H)
        for v in c.values():
            v.setflags(write=False)
        _cases[(N, H)] = c
    return _cases[(N, H)]


def begin(e, c, G, tape, cost=False, lr=0.05):
    e.set_engine(tape)
    if cost:
        e.gd_begin_cost(c['s_cur'], c['attr'], c['dens'], c['act_seqs'], lr, LO, HI)
    else:
        e.set_goal(G, c['goal_coor'])
        e.gd_begin(c['s_cur'], c['attr'], c['dens'], c['act_seqs'], lr, LO, HI)


def last_step_seed(gs):
    seed = np.zeros_like(gs)
    seed[:, -1] = gs[:, -1]
    return seed


def quadratic(c):
    return costs.quadratic_cost(c['targets'], c['weights'])


# ---- 1. identity with the built-in reward ------------------------------------------------------------------------------------
@pytest.mark.parametrize('tape', TAPES)
@pytest.mark.parametrize('wset', WSETS)
@pytest.mark.parametrize('N,H', SHAPES)
def test_the_rewards_own_seed_gives_the_rewards_own_gradients(engines, G, wset, tape, N, H):
    e, c = engines[wset][0], case(N, H)
    begin(e, c, G, tape)
    r, g, gs = e.gd_grad(want_state_grad=True)
    assert np.abs(g).max() > 0 and np.all(np.isfinite(gs))
    g2, gs2 = e.gd_grad_seeded(last_step_seed(gs), want_state_grad=True)
    assert np.array_equal(g2, g) and np.array_equal(gs2, gs)
    g3, none = e.gd_grad_seeded(last_step_seed(gs))           # the state gradient is optional
    assert none is None and np.array_equal(g3, g)
    # and the built-in call is what it was, behind the seeded ones
    r4, g4, gs4 = e.gd_grad(want_state_grad=True)
    assert r4.tobytes() == r.tobytes() and g4.tobytes() == g.tobytes() and gs4.tobytes() == gs.tobytes()


@pytest.mark.parametrize('tape', TAPES)
@pytest.mark.parametrize('wset', WSETS)
@pytest.mark.parametrize('N,H', [(17, 1), (20, 3), (65, 2)])
def test_five_seeded_steps_leave_the_pushes_of_five_built_in_steps(engines, G, wset, tape, N, H):
    """context a: gd_step; its twin b: gd_step_seeded on the seed the host re-derives each iteration from a's gd_grad"""
    a, b, _ = engines[wset]
    c = case(N, H)
    begin(a, c, G, tape)
    begin(b, c, G, tape, cost=True)
    for it in range(5):
        _, _, gs = a.gd_grad(want_state_grad=True)
        a.gd_step()
        pushes = b.gd_step_seeded(last_step_seed(gs))
        assert np.array_equal(pushes, a.gd_actions()), it
        assert np.array_equal(b.gd_actions(), pushes), it
    assert not np.array_equal(pushes, c['act_seqs'])


# ---- 2. the prediction -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tape', TAPES)
@pytest.mark.parametrize('N,H', [(17, 2), (20, 1), (65, 3)])
def test_predict_keeps_its_bits_and_is_the_forward_gd_grad_runs(engines, G, tape, N, H):
    e, c = engines['trained'][0], case(N, H)
    begin(e, c, G, tape)
    p0 = e.gd_predict()
    assert p0.shape == (4, H, N, 3) and np.all(np.isfinite(p0))
    assert e.gd_predict().tobytes() == p0.tobytes()
    _, seed = quadratic(c)(p0, None, True)
    e.gd_grad_seeded(seed)
    assert e.gd_predict().tobytes() == p0.tobytes()
    r, _, _ = e.gd_grad()
    np.testing.assert_allclose(e.reward(p0[:, H - 1]), r, rtol=1e-5)
    assert np.array_equal(e.gd_actions(), c['act_seqs'])                # nothing moved


# ---- 3. seeds on every step, against float64 ---------------------------------------------------------------------------------
@pytest.mark.parametrize('tape', TAPES)
@pytest.mark.parametrize('wset', WSETS)
def test_all_step_seeds_against_float64(engines, G, wset, tape):
    e = engines[wset][2]
    worst = 0.0
    for N, H in SHAPES:
        c = case(N, H)
        begin(e, c, G, tape, cost=True)
        pred = e.gd_predict()
        _, seed = quadratic(c)(pred, None, True)
        assert all(np.abs(seed[:, t]).max() > 0 for t in range(H))
        g32, gs32 = e.gd_grad_seeded(seed, want_state_grad=True)
        g64, gs64 = e.gd_grad_f64_seeded(c['s_cur'], c['attr'], c['dens'], c['act_seqs'], seed.astype(np.float64), want_state_grad=True)
        rel = float(np.abs(g32 - g64).max() / np.abs(g64).max())
        rel_s = float(np.abs(gs32 - gs64).max() / np.abs(gs64).max())
        print('[gd-seeded] %s %s N=%d H=%d: grad_act rel %.3e, grad_state rel %.3e' % (wset, tape, N, H, rel, rel_s))
        worst = max(worst, rel)
    print('[gd-seeded] %s %s: worst rel %.3e (bound %.1e)' % (wset, tape, worst, ALL_STEP_BOUND[(wset, tape)]))
    assert ALL_STEP_BOUND[(wset, tape)] <= 1e-4
    assert worst <= ALL_STEP_BOUND[(wset, tape)]


# ---- 4. refusals and isolation -------------------------------------------------------------------------------------------------
def session_bits(e):
    return e.gd_predict().tobytes(), e.gd_actions().tobytes()


def test_refusals_leave_the_session_as_it_was(engines, G, golden):
    e, c = engines['seed0'][0], case(20, 2)
    B, H, N = 4, 2, 20
    begin(e, c, G, 'fused', cost=True)
    e.gd_step_seeded(np.ones((B, H, N, 3), np.float32))            # Adam has state
    before = session_bits(e)
    seed = np.zeros((B, H, N, 3), np.float32)
    out = np.empty((B, H, 4), np.float32)
    # a null seed, a null output
    assert e.lib.drp_gd_grad_seeded(e.h, None, out.ctypes.data_as(f32p), None) == -1
    assert e.lib.drp_gd_step_seeded(e.h, None, None) == -1
    assert e.lib.drp_gd_predict(e.h, None) == -1
    assert session_bits(e) == before
    # a seed value that is no number: the message names row, step and particle
    for bad in (np.nan, np.inf, -np.inf):
        s = seed.copy()
        s[2, 1, 7, 1] = bad
        with pytest.raises(DrpError, match=r'drp error -1: .*row 2, step 1, particle 7'):
            e.gd_grad_seeded(s)
        with pytest.raises(DrpError, match=r'drp error -1: .*row 2, step 1, particle 7'):
            e.gd_step_seeded(s)
        assert session_bits(e) == before
    # the built-in reward's calls in a cost session
    for call in (e.gd_grad, e.gd_step, lambda: e.gd_step_async(0), lambda: e.gd_wait(0)):
        with pytest.raises(DrpError, match=r'drp error -2: .*drp_gd_begin_cost.*drp_gd_step_seeded'):
            call()
        assert session_bits(e) == before
    # the next step is the step a twin takes that saw none of this
    t = engines['seed0'][1]
    begin(t, c, G, 'fused', cost=True)
    t.gd_step_seeded(np.ones((B, H, N, 3), np.float32))
    s = np.full((B, H, N, 3), 0.25, np.float32)
    assert np.array_equal(e.gd_step_seeded(s), t.gd_step_seeded(s))
    # a wrong shape is the binding's to refuse
    with pytest.raises(ValueError):
        e.gd_grad_seeded(np.zeros((B, H, N + 1, 3), np.float32))


def test_no_session_and_a_multi_scene_session_take_no_seed(golden, G):
    e = new_engine(golden.weights_seed0)
    try:
        buf = np.zeros((4, 2, 20, 3), np.float32)
        p = buf.ctypes.data_as(f32p)
        assert e.lib.drp_gd_predict(e.h, p) == -2
        assert e.lib.drp_gd_grad_seeded(e.h, p, None, None) == -2
        assert e.lib.drp_gd_step_seeded(e.h, p, None) == -2
        c = case(20, 2)
        e.set_goal_scenes(np.stack([G, G]), [c['goal_coor'], c['goal_coor']])
        e.gd_begin_scenes(np.stack([c['s_cur'][:1], c['s_cur'][1:]]), np.stack([c['attr'][:1], c['attr'][1:]]),
                          np.stack([c['dens'][:1], c['dens'][1:]]), c['act_seqs'], 0.05, LO, HI)
        r, g, _ = e.gd_grad()
        for rc in (e.lib.drp_gd_predict(e.h, p), e.lib.drp_gd_grad_seeded(e.h, p, None, None), e.lib.drp_gd_step_seeded(e.h, p, None)):
            assert rc == -2
        assert 'scenes' in e.lib.drp_last_error(e.h).decode()
        r2, g2, _ = e.gd_grad()
        assert r2.tobytes() == r.tobytes() and g2.tobytes() == g.tobytes()
    finally:
        e.close()


@pytest.mark.parametrize('tape', TAPES)
def test_the_whole_path_runs_without_a_goal_ever_set(engines, tape):
    e, c = engines['seed0'][2], case(17, 3)
    e.set_engine(tape)
    e.gd_begin_cost(c['s_cur'], c['attr'], c['dens'], c['act_seqs'], 0.05, LO, HI)
    cost = costs.sum_costs(quadratic(c), costs.keep_out_cost([0.0, 0.0], 2.0, 0.1, M34, 24.0))
    first = None
    for it in range(8):
        pred = e.gd_predict()
        v, seed = cost(pred, None, True)
        first = v.sum() if first is None else first
        e.gd_step_seeded(seed)
    v, _ = cost(e.gd_predict(), None, False)
    print('[gd-seeded] %s: cost %.6e -> %.6e over 8 seeded steps' % (tape, first, v.sum()))
    assert v.sum() < first
    with pytest.raises(DrpError, match='goal not set'):
        e.gd_begin(c['s_cur'], c['attr'], c['dens'], c['act_seqs'], 0.05, LO, HI)


def test_a_cloud_call_between_predict_and_step_changes_nothing(engines, G):
    a, b, _ = engines['trained']
    c = case(20, 3)
    begin(a, c, G, 'fused', cost=True)
    begin(b, c, G, 'fused', cost=True)
    q = quadratic(c)
    for it in range(2):
        pa, pb = a.gd_predict(), b.gd_predict()
        assert pa.tobytes() == pb.tobytes()
        _, seed = q(pa, None, True)
        target = np.ascontiguousarray(c['targets'][-1][None, :12].repeat(4, 0))
        a.cloud_divergence(np.ascontiguousarray(pa[:, -1]), target, eps=float(1.0 / c['dens'][0]), iters=50, want_grad=True)
        assert a.gd_step_seeded(seed).tobytes() == b.gd_step_seeded(seed).tobytes()
    assert a.gd_predict().tobytes() == b.gd_predict().tobytes()


def test_built_in_sessions_the_trainer_and_the_dispatch_marks_are_undisturbed(engines, G, golden):
    a, b, _ = engines['seed0']
    c = case(20, 2)
    # a built-in GD session with seeded calls in between, against one without
    begin(a, c, G, 'fused')
    begin(b, c, G, 'fused')
    seed = np.full((4, 2, 20, 3), 1e-3, np.float32)
    for it in range(3):
        a.gd_predict()
        a.gd_grad_seeded(seed)
        assert a.gd_step().tobytes() == b.gd_step().tobytes()
        assert a.gd_actions().tobytes() == b.gd_actions().tobytes()
    # the dispatch marks: the seeded calls launch what gd_grad launches, no variant of their own
    a.dispatch_reset()
    a.gd_grad()
    built_in = set(a.last_dispatch())
    a.dispatch_reset()
    a.gd_predict()
    a.gd_grad_seeded(seed)
    a.gd_step_seeded(seed)
    assert set(a.last_dispatch()) <= built_in
    assert set(a.last_dispatch()) == built_in - {v for v in built_in if 'reward' in v}
    # an Adam trajectory of the trainer: three steps on a, with a cost session run on a between them, against b's three
    rng = np.random.default_rng(3)
    Bt, Nt = 2, 20
    s0, dens, attr = syn.make_pile(Nt, Bt, seed=9)
    states = np.stack([s0, s0 + 0.01 * rng.standard_normal(s0.shape).astype(np.float32)], 1)
    delta = 0.01 * rng.standard_normal((Bt, 1, Nt, 3)).astype(np.float32)
    attrs = np.stack([attr, attr], 1)
    nums = np.full((Bt,), Nt, np.int32)
    losses = []
    for e, disturb in ((a, True), (b, False)):
        e.load_weights(weights.blob_from_state_dict(golden.weights_seed0), 0.08)
        e.train_begin(1, 1e-3)
        out = []
        for it in range(3):
            out.append(e.train_step(states, delta, attrs, nums, dens)[0])
            if disturb:
                w = e.get_weights()
                begin(e, c, G, 'fused', cost=True)
                e.gd_step_seeded(seed)
                assert e.get_weights().tobytes() == w.tobytes()
        losses.append((out, e.get_weights().tobytes()))
        e.load_weights(weights.blob_from_state_dict(golden.weights_seed0), 0.08)
    assert losses[0] == losses[1]

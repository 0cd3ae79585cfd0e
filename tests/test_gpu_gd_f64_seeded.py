"""GPU: the float64 yardstick of planning on a caller's cost -- drp_gd_predict_f64, drp_gd_grad_f64_seeded -- and
Engine.gradient_probe_cost.

Tolerance against the float64 restatement (tests/_gd_seeded_ref.py, pinned by tests/test_gd_seeded_host.py): TOL = 1e-10 x the
largest magnitude of the compared array, the project's standing bound for float64 calls (tests/test_gpu_gd_f64.py: both sides
evaluate the same expressions in double on the same graph and differ in summation order only).  The probe is held to
ALL_STEP_BOUND of tests/test_gpu_gd_seeded.py."""
import numpy as np
import pytest

import _gd_seeded_ref as S
from dyn_res_pile_manip_amd import costs
from test_gpu_gd_seeded import ALL_STEP_BOUND, CAM, HI, LO, M34, SHAPES, G, case, engines, quadratic  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu
TOL = 1e-10


def args_of(c):
    return c['s_cur'], c['attr'], c['dens'], c['act_seqs']


def rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


_refs = {}


def reference(golden, wset, N, H):
    """the restatement's (values, pred, grad_act, grad_state) with quadratic_cost on every step, computed once"""
    if (wset, N, H) not in _refs:
        c = case(N, H)
        w = golden.weights_seed0 if wset == 'seed0' else golden.weights_trained
        out = S.gd_cost_and_grads64(w, c['s_cur'], c['dens'], c['attr'], c['act_seqs'], S.quadratic_torch(c['targets'], c['weights']),
                                    M34, 24.0)
        for v in out:
            v.setflags(write=False)
        _refs[(wset, N, H)] = out
    return _refs[(wset, N, H)]


@pytest.mark.parametrize('wset', ('seed0', 'trained'))
@pytest.mark.parametrize('N,H', SHAPES)
def test_matches_the_float64_restatement(engines, golden, wset, N, H):
    e, c = engines[wset][2], case(N, H)           # the context that never saw a goal
    v_ref, p_ref, ga_ref, gs_ref = reference(golden, wset, N, H)
    pred = e.gd_predict_f64(*args_of(c))
    assert pred.dtype == np.float64 and rel(pred, p_ref) <= TOL
    v, seed = quadratic(c)(pred, None, True)
    assert seed.dtype == np.float64 and rel(v, v_ref) <= TOL
    ga, gs = e.gd_grad_f64_seeded(*args_of(c), seed, want_state_grad=True)
    worst = max(rel(ga, ga_ref), rel(gs, gs_ref))
    print('[gd-f64-seeded] %s N=%d H=%d: worst error %.2e of the largest value' % (wset, N, H, worst))
    assert worst <= TOL
    assert np.array_equal(e.gd_grad_f64_seeded(*args_of(c), seed), ga)          # the state gradient is optional


@pytest.mark.parametrize('wset', ('seed0', 'trained'))
@pytest.mark.parametrize('N,H', SHAPES)
def test_the_rewards_own_seed_gives_the_rewards_own_gradient_in_float64(engines, G, wset, N, H):
    e, c = engines[wset][0], case(N, H)
    e.set_goal(G, c['goal_coor'])
    r, ga, gs = e.gd_grad_f64(*args_of(c), want_state_grad=True)
    seed = np.zeros_like(gs)
    seed[:, -1] = gs[:, -1]
    ga2, gs2 = e.gd_grad_f64_seeded(*args_of(c), seed, want_state_grad=True)
    assert np.array_equal(ga2, ga) and np.array_equal(gs2, gs)
    r3, ga3, gs3 = e.gd_grad_f64(*args_of(c), want_state_grad=True)            # and gd_grad_f64 keeps its bits behind it
    assert r3.tobytes() == r.tobytes() and ga3.tobytes() == ga.tobytes() and gs3.tobytes() == gs.tobytes()


def test_same_bits_run_to_run_and_under_a_one_row_cap(engines, G):
    e, c = engines['trained'][0], case(20, 3)
    e.set_goal(G, c['goal_coor'])
    pred = e.gd_predict_f64(*args_of(c))
    _, seed = quadratic(c)(pred, None, True)
    ga, gs = e.gd_grad_f64_seeded(*args_of(c), seed, want_state_grad=True)
    built_in = [x.tobytes() for x in e.gd_grad_f64(*args_of(c), want_state_grad=True)]
    assert e.gd_predict_f64(*args_of(c)).tobytes() == pred.tobytes()
    e.set_f64_cap(1)                              # one row per chunk: the seed is sliced row by row
    try:
        assert e.gd_predict_f64(*args_of(c)).tobytes() == pred.tobytes()
        ga2, gs2 = e.gd_grad_f64_seeded(*args_of(c), seed, want_state_grad=True)
        assert ga2.tobytes() == ga.tobytes() and gs2.tobytes() == gs.tobytes()
        assert [x.tobytes() for x in e.gd_grad_f64(*args_of(c), want_state_grad=True)] == built_in
    finally:
        e.set_f64_cap(0)
    ga3, gs3 = e.gd_grad_f64_seeded(*args_of(c), seed, want_state_grad=True)
    assert ga3.tobytes() == ga.tobytes() and gs3.tobytes() == gs.tobytes()


def test_the_float64_taps_and_a_session_keep_their_bits(engines, G):
    e, c = engines['seed0'][0], case(17, 2)
    sd = e.gen_s_delta(np.repeat(c['s_cur'], 2, 0), c['act_seqs'][:, 0])
    e.step_f64(np.repeat(c['attr'], 2, 0), np.repeat(c['s_cur'], 2, 0), sd, np.repeat(c['dens'], 2, 0))
    tap = e.f64_tap('particle_pred').tobytes()
    e.set_goal(G, c['goal_coor'])
    e.gd_begin(*args_of(c), 0.05, LO, HI)
    r, g, _ = e.gd_grad()
    pred = e.gd_predict_f64(*args_of(c))
    e.gd_grad_f64_seeded(*args_of(c), np.ones_like(pred))
    assert e.f64_tap('particle_pred').tobytes() == tap
    r2, g2, _ = e.gd_grad()                       # the one-shots ended no session
    assert r2.tobytes() == r.tobytes() and g2.tobytes() == g.tobytes()


def test_refusals_of_the_float64_pair(engines):
    e, c = engines['seed0'][2], case(17, 2)
    seed = np.zeros((4, 2, 17, 3), np.float64)
    from dyn_res_pile_manip_amd._lib import DrpError
    s = seed.copy()
    s[3, 0, 16, 2] = np.nan
    with pytest.raises(DrpError, match=r'drp error -1: .*row 3, step 0, particle 16'):
        e.gd_grad_f64_seeded(*args_of(c), s)
    with pytest.raises(ValueError):
        e.gd_grad_f64_seeded(*args_of(c), seed[:, :1])
    f = lambda a: a.ctypes.data_as(e.lib.drp_gd_predict_f64.argtypes[1])
    assert e.lib.drp_gd_predict_f64(e.h, f(c['s_cur']), f(c['attr']), f(c['dens']), 2, 17, f(c['act_seqs']), 4, 2, None) == -1
    assert e.lib.drp_gd_grad_f64_seeded(e.h, f(c['s_cur']), f(c['attr']), f(c['dens']), 2, 17, f(c['act_seqs']), 4, 2, None, None, None) == -1
    with pytest.raises(DrpError, match='goal not set'):       # gd_grad_f64 itself keeps requiring the goal
        e.gd_grad_f64(*args_of(c))


@pytest.mark.parametrize('tape', ('fused', 'mfma'))
@pytest.mark.parametrize('wset', ('seed0', 'trained'))
def test_gradient_probe_cost(engines, wset, tape):
    e = engines[wset][2]
    e.set_engine(tape)
    c = case(20, 3)
    p = e.gradient_probe_cost(quadratic(c), *args_of(c), LO, HI)
    print('[gd-f64-seeded] probe quadratic %s %s: %r' % (wset, tape, p))
    assert p['tape'] == tape and p['rel'] <= ALL_STEP_BOUND[(wset, tape)] and np.isfinite(p['seed_rel']) and p['seed_rel'] >= 0
    # the divergence tests' setting: 20 particles against a 12-point target, eps at one spacing, 50 sweeps
    div = costs.cloud_divergence_cost(e, c['targets'][-1][:12], None, 1.0, 50)
    ctx = {'dens': c['dens']}                           # one per start column
    p = e.gradient_probe_cost(div, *args_of(c), LO, HI, context=ctx)
    print('[gd-f64-seeded] probe divergence %s %s: %r' % (wset, tape, p))
    assert p['tape'] == tape and p['rel'] <= ALL_STEP_BOUND[(wset, tape)] and np.isfinite(p['seed_rel']) and p['seed_rel'] >= 0

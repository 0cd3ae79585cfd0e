"""CPU: the host side of planning on a caller's cost -- the float64 restatement with the loss as an argument
(tests/_gd_seeded_ref.py), costs.py, and what PlannerGD.trajectory_optimization_ptcl_cost decides before it touches a device.

Bounds.  The restatement with _f64_grad_ref.reward as its cost IS gd_loss_and_grads64's computation, so the two agree to 1e-12 of
each output's largest value (the same double operations; autograd may order a sum differently).  Central differences in push
space: tests/test_f64_grad_host.py's FD_BOUND and its derivation (h = 2^-14, the soft mask's third derivative) -- the quadratic
cost behind the rollout adds a polynomial, which tightens nothing and loosens nothing.  A cost's own gradient against central
differences of its own values in float64 at h = 1e-6: rounding 2^-53 |f| / h ~ 1e-10 |f| and truncation h^2 / 6 |f'''| ~ 1e-13 |f'''|,
held to 1e-6 of the gradient's length."""
import numpy as np
import pytest
import torch

import _f64_grad_ref as R
import _gd_seeded_ref as S
from dyn_res_pile_manip_amd import costs, synthetic as syn
from dyn_res_pile_manip_amd.planners import PlannerGD, world2cam_affine
from test_f64_grad_host import FD_BOUND, case_inputs

M34 = world2cam_affine(syn.demo_cam_extrinsics())
CAM = syn.demo_cam_params()


@pytest.fixture(scope='module')
def G():
    return syn.goal_field(syn.goal_distance_image(syn.goal_mask('I')))


@pytest.mark.parametrize('wset,case', [('seed0', 'h1'), ('seed0', 'h2'), ('trained', 'n20_h2')])
def test_with_the_reward_as_its_cost_the_restatement_is_gd_loss_and_grads64(golden, G, wset, case):
    w, c = case_inputs(golden, wset, case)
    r, ga, gs = R.gd_loss_and_grads64(w, c['s_cur'], c['dens'], c['attr'], c['act_seqs'], G, CAM, c['goal_coor'], M34, 24.0)
    G64, coor64, cam = R._d(G), R._d(c['goal_coor']), R._d(CAM).tolist()
    v, pred, ga2, gs2 = S.gd_cost_and_grads64(w, c['s_cur'], c['dens'], c['attr'], c['act_seqs'],
                                              lambda p: -R.reward(p[:, -1], G64, cam, coor64), M34, 24.0)
    for name, a, b in (('values', -v, r), ('grad_act', ga2, ga), ('grad_state', gs2, gs)):
        assert a.shape == b.shape and float(np.abs(a - b).max()) <= 1e-12 * float(np.abs(b).max()), name
    assert pred.shape == gs.shape
    # and a seed that is the reward's own final-step gradient gives the reward's gradients: the seam the device calls open
    seed = np.zeros_like(gs)
    seed[:, -1] = gs[:, -1]
    _, _, ga3, gs3 = S.gd_cost_and_grads64(w, c['s_cur'], c['dens'], c['attr'], c['act_seqs'], S.seed_cost(seed), M34, 24.0)
    assert float(np.abs(ga3 - ga).max()) <= 1e-12 * float(np.abs(ga).max())
    assert float(np.abs(gs3 - gs).max()) <= 1e-12 * float(np.abs(gs).max())


def test_the_restatement_agrees_with_its_central_differences_under_all_step_seeds(golden):
    c = S.make_case(20, 2)
    cost = S.quadratic_torch(c['targets'], c['weights'])

    def fn(a):
        v, _, ga, _, dec = S.gd_cost_and_grads64(golden.weights_trained, c['s_cur'], c['dens'], c['attr'], a, cost, M34, 24.0,
                                                 want_decisions=True)
        return -v, ga, dec          # fd_check's convention: rewards, and the gradient of loss = -sum(reward)
    res = R.fd_check(fn, c['act_seqs'], n_dir=8, max_redraw=2)
    gnorm = float(np.linalg.norm(fn(R.fd_point(c['act_seqs']))[1]))
    worst = max(abs(cd - an) for cd, an in res) / gnorm
    print('[gd-seeded-ref] central differences under all-step seeds: worst residual %.3e of |g| = %.3e' % (worst, gnorm))
    assert gnorm > 0 and worst < FD_BOUND


# ---- costs.py ------------------------------------------------------------------------------------------------------------------
class StubEngine:
    """cloud_divergence / cloud_divergence_f64 with a closed form in the device's place: sum_n |p_n - mean(q)|^2 / eps"""
    def __init__(self):
        self.calls = []

    def _call(self, name, dtype, p, q, n_p, n_q, eps, iters, want_grad):
        self.calls.append((name, np.asarray(p).dtype, np.asarray(eps).copy(), iters, n_q))
        p, q = np.asarray(p, np.float64), np.asarray(q, np.float64)
        m = np.stack([q[b, :(q.shape[1] if n_q is None else n_q[b])].mean(0) for b in range(q.shape[0])])
        d = p - m[:, None]
        out = {'divergence': (d * d).sum((1, 2)) / eps}
        if want_grad:
            out['grad'] = (2 * d / eps[:, None, None]).astype(dtype)
        return out

    def cloud_divergence(self, p, q, n_p=None, n_q=None, eps=None, iters=None, want_grad=False):
        return self._call('f32', np.float32, p, q, n_p, n_q, eps, iters, want_grad)

    def cloud_divergence_f64(self, p, q, n_p=None, n_q=None, eps=None, iters=None, want_grad=False):
        return self._call('f64', np.float64, p, q, n_p, n_q, eps, iters, want_grad)


def pred_of(B=4, H=3, N=7, seed=0):
    rng = np.random.default_rng(seed)
    p = rng.uniform(-0.2, 0.2, (B, H, N, 3))
    p[..., 2] += 0.75
    return p


def the_costs():
    rng = np.random.default_rng(1)
    tg = rng.uniform(-0.2, 0.2, (3, 7, 3))
    quad = costs.quadratic_cost(tg, [1.0, 0.5, 2.0])
    keep = costs.keep_out_cost([0.1, -0.2], 6.0, 0.3, M34, 24.0)
    keep_raw = costs.keep_out_cost([0.0, 0.0], 0.25, 2.0)
    div = costs.cloud_divergence_cost(StubEngine(), tg[-1, :5], None, 2.0, 50)
    tq = costs.torch_cost(lambda p, ctx: ((p - torch.from_numpy(tg)) ** 2 * torch.tensor([1.0, 0.5, 2.0]).reshape(1, 3, 1, 1) / 7).sum((1, 2, 3)))
    return {'quadratic': quad, 'keep_out': keep, 'keep_out_raw': keep_raw, 'cloud_divergence': div, 'torch': tq,
            'sum': costs.sum_costs(quad, keep, div)}


@pytest.mark.parametrize('name', ['quadratic', 'keep_out', 'keep_out_raw', 'cloud_divergence', 'torch', 'sum'])
def test_a_costs_gradient_is_the_gradient_of_its_values(name):
    cost = the_costs()[name]
    ctx = {'dens': np.array([4000.0, 5000.0])}
    p = pred_of()
    v, g = cost(p, ctx, True)
    assert v.shape == (4,) and g.shape == p.shape and v.dtype == np.float64 and g.dtype == np.float64
    v2, none = cost(p, ctx, False)
    assert none is None and np.array_equal(v2, v)
    if name.startswith('keep_out'):
        assert np.count_nonzero(g) > 0 and (name == 'keep_out' or np.count_nonzero(g) < g.size)    # inside and outside the disc
    rng = np.random.default_rng(2)
    gnorm = float(np.linalg.norm(g))
    h = 1e-6
    for _ in range(6):
        d = rng.standard_normal(p.shape)
        d /= np.linalg.norm(d)
        cd = (cost(p + h * d, ctx, False)[0].sum() - cost(p - h * d, ctx, False)[0].sum()) / (2 * h)
        assert abs(cd - float((g * d).sum())) <= 1e-6 * gnorm, (name, cd, float((g * d).sum()))
    # rows are independent: a row's value and gradient do not change when the other rows do
    q = p.copy()
    q[1:] += 0.01
    v3, g3 = cost(q, ctx, True)
    assert v3[0] == v[0] and np.array_equal(g3[0], g[0])
    # float32 in, float32 out
    v32, g32 = cost(p.astype(np.float32), ctx, True)
    assert v32.dtype == np.float32 and g32.dtype == np.float32
    np.testing.assert_allclose(v32, v, rtol=1e-4)


def test_torch_cost_of_the_quadratic_equals_the_numpy_one():
    c = the_costs()
    p = pred_of(seed=5)
    v, g = c['quadratic'](p, None, True)
    vt, gt = c['torch'](p, None, True)
    np.testing.assert_allclose(vt, v, rtol=1e-14)
    np.testing.assert_allclose(gt, g, rtol=1e-13, atol=1e-18)
    with pytest.raises(ValueError, match='one value per row'):
        costs.torch_cost(lambda p, ctx: p.sum())(p, None, True)


def test_cloud_divergence_cost_routes_dtype_eps_and_the_final_step():
    eng = StubEngine()
    cost = costs.cloud_divergence_cost(eng, np.zeros((5, 3), np.float32), 4, 2.0, 33)
    p = pred_of()
    v, g = cost(p.astype(np.float32), {'dens': np.array([4000.0, 5000.0])}, True)
    assert not g[:, :-1].any() and g[:, -1].any()
    name, dt, eps, iters, n_q = eng.calls[-1]
    assert (name, dt, iters) == ('f32', np.float32, 33) and list(n_q) == [4] * 4
    np.testing.assert_array_equal(eps, 2.0 / np.array([4000.0, 5000.0, 4000.0, 5000.0]))     # row = trajectory * nb + column
    cost(p, None, False)
    assert eng.calls[-1][0] == 'f64' and np.array_equal(eng.calls[-1][2], np.full(4, 2.0))
    cost(p[:1], {'dens': np.array([4000.0, 5000.0])}, False)                                   # the winner's re-rollout: column 0
    np.testing.assert_array_equal(eng.calls[-1][2], [2.0 / 4000.0])


def test_costs_refuse_what_they_cannot_read():
    with pytest.raises(ValueError):
        costs.quadratic_cost(np.zeros((2, 7, 3)))(pred_of(), None, True)
    with pytest.raises(ValueError):
        costs.keep_out_cost([0, 0], 0.0)
    with pytest.raises(ValueError):
        costs.sum_costs()
    with pytest.raises(ValueError):
        costs.quadratic_cost(np.zeros((3, 7, 3)))(np.zeros((4, 3, 7)), None, True)
    with pytest.raises(ValueError, match='values of shape'):
        costs.check_cost_output(np.zeros(3), None, (4, 3, 7, 3), False)
    with pytest.raises(ValueError, match='gradient of shape'):
        costs.check_cost_output(np.zeros(4), None, (4, 3, 7, 3), True)


# ---- the planner method, before any device -------------------------------------------------------------------------------------
def test_the_planner_method_refuses_before_it_binds_an_engine():
    config = syn.default_config()
    planner = PlannerGD(config, syn.SyntheticEnv(config))
    s = np.zeros((1, 7, 3), np.float32)
    lo, hi = syn.action_limits()
    kw = dict(n_sample=2, n_look_ahead=1, n_update_iter=2, action_lower_lim=lo, action_upper_lim=hi)
    args = (s, np.ones(1, np.float32), np.zeros((1, 7), np.float32))
    tail = (object(), np.zeros((1, 2, 4), np.float32), np.zeros(1))          # a model that is never reached
    cost = costs.quadratic_cost(np.zeros((1, 7, 3)))
    with pytest.raises(ValueError, match='comm'):
        planner.trajectory_optimization_ptcl_cost(*args, cost, *tail, comm=(0, 2, b'x'), **kw)
    with pytest.raises(TypeError, match='callable'):
        planner.trajectory_optimization_ptcl_cost(*args, None, *tail, **kw)
    with pytest.raises(ValueError, match='noise type'):
        planner.trajectory_optimization_ptcl_cost(*args, cost, *tail, noise_type='pink', **kw)
    with pytest.raises(AssertionError, match='one scene'):
        planner.trajectory_optimization_ptcl_cost(np.zeros((2, 1, 7, 3), np.float32), *args[1:], cost, *tail, **kw)
    config['mpc']['mpc_type'] = 'SHOOTING'
    with pytest.raises(ValueError, match='mpc_type'):
        planner.trajectory_optimization_ptcl_cost(*args, cost, *tail, **kw)
    with pytest.raises(NotImplementedError):                                  # and a model of another kind, as the built-in method
        config['mpc']['mpc_type'] = 'GD'
        planner.trajectory_optimization_ptcl_cost(*args, cost, *tail, **kw)

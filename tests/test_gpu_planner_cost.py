"""GPU: PlannerGD.trajectory_optimization_ptcl_cost -- the planners on a cost of the caller's.

With a cost that restates the built-in reward (tests/_f64_grad_ref.py's `reward`, the goal field and the goal pixels read from
`context`, through costs.torch_cost) the method is held against trajectory_optimization_ptcl_multi_traj on the same arguments at
the tolerances tests/test_gpu_planner.py holds reference-made dicts to: rewards and their means rtol 2e-5, their spread rtol
2e-4, pushes atol 2e-3."""
import copy

import numpy as np
import pytest
import torch

import _f64_grad_ref as R
from dyn_res_pile_manip_amd import costs, flex_rewards, synthetic as syn
from dyn_res_pile_manip_amd._lib import DrpError
from dyn_res_pile_manip_amd.gnn_dyn import PropNetDiffDenModel
from dyn_res_pile_manip_amd.planners import PlannerGD, world2cam_affine

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures('exact_goal_transform')]
M34 = world2cam_affine(syn.demo_cam_extrinsics())


@pytest.fixture(scope='module')
def stack(golden):
    config = syn.default_config()
    env = syn.SyntheticEnv(config)
    model = PropNetDiffDenModel(config, True)
    sd = {k[2:]: torch.from_numpy(golden.weights_seed0[k]) for k in golden.weights_seed0.files if k.startswith('w/')}
    model.load_state_dict(sd, strict=False)
    model.cuda().eval()
    yield env, model
    model.engine.close()


def planner_of(env, mpc_type):
    config = copy.deepcopy(syn.default_config())
    config['mpc']['mpc_type'] = mpc_type
    return PlannerGD(config, env)


def reward_as_a_cost():
    """the built-in reward of the final state, restated: context = {'field', 'goal_coor', 'cam'}"""
    def fn(pred, ctx):
        G = torch.from_numpy(np.asarray(ctx['field'], np.float64))
        coor = torch.from_numpy(np.asarray(ctx['goal_coor'], np.float64))
        return -R.reward(pred[:, -1].double(), G, ctx['cam'], coor).to(pred.dtype)
    return costs.torch_cost(fn)


@pytest.mark.parametrize('mpc_type', ['GD', 'MPPI', 'CEM'])
def test_the_built_in_reward_as_a_cost_plans_as_the_built_in_planner(stack, golden, mpc_type):
    env, model = stack
    g = golden.gd_planner
    s, dens, attr, act_seq = g['s_cur'], g['dens'], g['attr'], g['act_seq']
    N = s.shape[1]
    planner = planner_of(env, mpc_type)
    obs_goal = syn.goal_distance_image(syn.goal_mask('I'))
    coor = syn.goal_coor_strided(obs_goal, 5 * N)
    lo, hi = syn.action_limits()
    kw = dict(n_sample=act_seq.shape[1] if mpc_type == 'GD' else 64, n_look_ahead=1, n_update_iter=4, action_lower_lim=lo,
              action_upper_lim=hi, seed=77)
    want = planner.trajectory_optimization_ptcl_multi_traj(s, dens, attr, obs_goal, model, act_seq, np.zeros(1), use_gpu=True,
                                                           goal_coor=coor, **kw)
    ctx = {'field': flex_rewards.goal_field(obs_goal, model.engine), 'goal_coor': coor, 'cam': syn.demo_cam_params()}
    got = planner.trajectory_optimization_ptcl_cost(s, dens, attr, reward_as_a_cost(), model, act_seq, np.zeros(1), context=ctx, **kw)
    assert set(want) <= set(got) and got['iter_num'] == want['iter_num']
    for k in ('action_sequence', 'action_full', 'observation_sequence'):
        np.testing.assert_allclose(got[k], want[k], atol=2e-3, err_msg=k)
    for k in ('reward_full', 'reward', 'rew_mean'):
        np.testing.assert_allclose(got[k], want[k], rtol=2e-5, err_msg=k)
    np.testing.assert_allclose(got['rew_std'], want['rew_std'], rtol=2e-4)
    np.testing.assert_allclose(got['next_r'][-1], want['next_r'][-1], rtol=2e-5)
    if want['nominal_sequence'] is None:
        assert got['nominal_sequence'] is None
    else:
        np.testing.assert_allclose(got['nominal_sequence'], want['nominal_sequence'], atol=2e-3)


def shaped_cost(s):
    """keep the pile out of a disc beside it while tracking a target a little to its side: seeds on the only step"""
    target = (s[0] + np.array([0.02, 0.0, 0.0], np.float32))[None]
    return costs.sum_costs(costs.quadratic_cost(target), costs.keep_out_cost([0.5, 0.5], 3.0, 0.05, M34, 24.0))


@pytest.mark.parametrize('mpc_type', ['GD', 'MPPI'])
def test_a_shaped_cost_goes_down(stack, golden, mpc_type):
    env, model = stack
    g = golden.gd_planner
    s, dens, attr, act_seq = g['s_cur'], g['dens'], g['attr'], g['act_seq']
    lo, hi = syn.action_limits()
    res = planner_of(env, mpc_type).trajectory_optimization_ptcl_cost(
        s, dens, attr, shaped_cost(s), model, act_seq, np.zeros(1), n_sample=act_seq.shape[1] if mpc_type == 'GD' else 64,
        n_look_ahead=1, n_update_iter=8, action_lower_lim=lo, action_upper_lim=hi, seed=5)
    first, last = -res['rew_mean'][0, 0], -res['rew_mean'][0, -1]
    print('[planner-cost] %s: mean cost %.6e -> %.6e, the winner %.6e' % (mpc_type, first, last, -res['reward'][0]))
    # started at: the given candidates' mean cost.  GD moves every candidate, so the last iterate's mean is lower too; the
    # sampling planners' last mean is over fresh noisy samples, so there the winner speaks
    assert -res['reward'][0] < first
    if mpc_type == 'GD':
        assert last < first
    assert np.isnan(res['next_r'][:-1]).all() and res['next_r'][-1, 0] == res['reward'][0]


def test_refusals_surface(stack, golden):
    env, model = stack
    g = golden.gd_planner
    s, dens, attr, act_seq = g['s_cur'], g['dens'], g['attr'], g['act_seq']
    lo, hi = syn.action_limits()
    args = (model, act_seq, np.zeros(1))
    kw = dict(n_sample=act_seq.shape[1], n_look_ahead=1, n_update_iter=2, action_lower_lim=lo, action_upper_lim=hi, seed=5)
    planner = planner_of(env, 'GD')
    with pytest.raises(ValueError, match='comm'):
        planner.trajectory_optimization_ptcl_cost(s, dens, attr, shaped_cost(s), *args, comm=(0, 2, b''), **kw)
    with pytest.raises(ValueError, match='values of shape'):
        planner.trajectory_optimization_ptcl_cost(s, dens, attr, lambda p, c, w: (np.zeros(3), np.zeros_like(p)), *args, **kw)
    with pytest.raises(ValueError, match='gradient of shape'):
        planner.trajectory_optimization_ptcl_cost(s, dens, attr, lambda p, c, w: (np.zeros(p.shape[0]), np.zeros(p.shape[:3])), *args, **kw)

    def nan_grad(p, c, w):
        grad = np.zeros_like(p)
        grad[1, 0, 2, 0] = np.nan
        return np.zeros(p.shape[0], np.float32), grad
    with pytest.raises(DrpError, match='row 1, step 0, particle 2'):
        planner.trajectory_optimization_ptcl_cost(s, dens, attr, nan_grad, *args, **kw)

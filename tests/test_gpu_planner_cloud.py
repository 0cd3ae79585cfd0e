"""GPU: PlannerGD.trajectory_optimization_ptcl_cloud -- the built-in loops on a device-resident cloud goal -- against
trajectory_optimization_ptcl_cost with the goal's host twin (costs.cloud_chamfer_cost, costs.cloud_divergence_cost), same seed.

The sampling planners see the same draws, the same states and rewards with the same bits (tests/test_gpu_cloud_goal.py), so
MPPI and CEM are held to BITS: action_sequence, reward_full, rew_mean, rew_std, nominal_sequence.  GD is held to numbers equal
(the seam adds +0.0 seeds: a zero may change sign).  The Chamfer weight is 2.0 -- a power of two, for which the twin's
float64-scaled, once-rounded gradient is the kernel's --, the Sinkhorn twin has no weight (1.0).  20 particles, 8 samples, 3
iterations, a 12-point target.

The float64 yardstick of a cloud session's gradient is Engine.gradient_probe_cost on the twin: held to ALL_STEP_BOUND of
tests/test_gpu_gd_seeded.py (what tests/test_gpu_gd_f64_seeded.py holds the other costs' probes to), the figures printed,
seed_rel among them: a nearest neighbour that flips between the fp32 and the float64 prediction shows there."""
import copy

import numpy as np
import pytest
import torch

import _gd_seeded_ref as S
from dyn_res_pile_manip_amd import costs, synthetic as syn, weights
from dyn_res_pile_manip_amd.engine import Engine
from dyn_res_pile_manip_amd.gnn_dyn import PropNetDiffDenModel
from dyn_res_pile_manip_amd.planners import PlannerGD, world2cam_affine

pytestmark = pytest.mark.gpu
M34 = world2cam_affine(syn.demo_cam_extrinsics())
LO, HI = syn.action_limits()
N, M, NS, ITERS_PLAN, SWEEPS = 20, 12, 8, 3, 10
# tests/test_gpu_gd_seeded.py: 5 x the worst measured max |g32 - g64| / max |g64|, seed-0 weights (fused, mfma)
ALL_STEP_BOUND = {'fused': 4.8e-6, 'mfma': 1.03e-5}


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


def problem(mpc_type):
    s, dens, attr = syn.make_pile(N, 2, seed=31)
    dens = (dens * np.array([1.0, 1.5], np.float32)).astype(np.float32)
    traj = NS if mpc_type == 'GD' else 4
    act_seq = np.ascontiguousarray(syn.sample_pushes(traj, 2, seed=7).transpose(1, 0, 2)).astype(np.float32)     # [H, traj, 4]
    target = (syn.make_pile(M, 1, seed=77)[0][0] + np.array([0.02, -0.01, 0.0], np.float32)).astype(np.float32)
    return s, dens, attr, act_seq, target


@pytest.mark.parametrize('kind', ['chamfer', 'sinkhorn'])
@pytest.mark.parametrize('mpc_type', ['MPPI', 'CEM', 'GD'])
def test_the_cloud_planner_is_the_cost_planner_on_the_twin(stack, mpc_type, kind):
    env, model = stack
    s, dens, attr, act_seq, target = problem(mpc_type)
    planner = planner_of(env, mpc_type)
    kw = dict(n_sample=NS, n_look_ahead=2, n_update_iter=ITERS_PLAN, action_lower_lim=LO, action_upper_lim=HI, seed=77)
    w = 2.0 if kind == 'chamfer' else 1.0
    twin = (costs.cloud_chamfer_cost(model.engine, target, weight=w) if kind == 'chamfer'
            else costs.cloud_divergence_cost(model.engine, target, eps_scale=1.0, iters=SWEEPS))
    want = planner.trajectory_optimization_ptcl_cost(s, dens, attr, twin, model, act_seq, np.zeros(2), context={'dens': dens}, **kw)
    got = planner.trajectory_optimization_ptcl_cloud(s, dens, attr, target, model, act_seq, np.zeros(2), kind=kind, weight=w,
                                                     eps_scale=1.0, iters=SWEEPS, **kw)
    assert set(want) == set(got) and got['iter_num'] == want['iter_num']
    assert np.all(np.isfinite(got['rew_mean'])) and (got['rew_mean'] < 0).all()
    keys = ('action_sequence', 'reward_full', 'rew_mean', 'rew_std', 'nominal_sequence', 'action_full', 'reward', 'next_r',
            'observation_sequence')
    for k in keys:
        if want[k] is None:
            assert got[k] is None, k
        elif mpc_type == 'GD':
            np.testing.assert_array_equal(got[k], want[k], err_msg=k)           # numbers equal (NaN in next_r: equal too)
        else:
            assert np.asarray(got[k]).dtype == np.asarray(want[k]).dtype and np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes(), k
    if mpc_type != 'GD':
        assert not np.array_equal(got['nominal_sequence'], act_seq[:, 0])       # the updates moved it


def test_refusals(stack):
    env, model = stack
    s, dens, attr, act_seq, target = problem('MPPI')
    planner = planner_of(env, 'MPPI')
    kw = dict(n_sample=NS, n_look_ahead=2, n_update_iter=2, action_lower_lim=LO, action_upper_lim=HI, seed=5)
    with pytest.raises(ValueError, match='comm'):
        planner.trajectory_optimization_ptcl_cloud(s, dens, attr, target, model, act_seq, np.zeros(2), comm=(0, 2, b''), **kw)
    with pytest.raises(ValueError, match='per scene'):
        planner.trajectory_optimization_ptcl_cloud(s, dens, attr, np.stack([target, target]), model, act_seq, np.zeros(2), **kw)
    with pytest.raises(ValueError, match='unknown cloud goal kind'):
        planner.trajectory_optimization_ptcl_cloud(s, dens, attr, target, model, act_seq, np.zeros(2), kind='emd', **kw)


@pytest.mark.parametrize('tape', ['fused', 'mfma'])
def test_gradient_probe_on_the_chamfer_twin(golden, tape):
    e = Engine(0)
    try:
        e.load_weights(weights.blob_from_state_dict(golden.weights_seed0), 0.08)
        e.set_camera(M34, 24.0, syn.demo_cam_params())
        e.set_engine(tape)
        c = S.make_case(20, 3)
        cost = costs.cloud_chamfer_cost(e, c['targets'][-1][:12], weight=2.0)
        p = e.gradient_probe_cost(cost, c['s_cur'], c['attr'], c['dens'], c['act_seqs'], LO, HI)
        print('[planner-cloud] probe chamfer twin %s: rel %.3e (bound %.2e), seed_rel %.3e, reward_rel %.3e'
              % (tape, p['rel'], ALL_STEP_BOUND[tape], p['seed_rel'], p['reward_rel']))
        assert p['tape'] == tape and np.isfinite(p['seed_rel']) and p['seed_rel'] >= 0
        assert p['rel'] <= ALL_STEP_BOUND[tape]
    finally:
        e.close()

"""GPU, scope row f1: the reverse-mode kernels and the gradient-descent planner (the
reference's live mpc_type 'GD') against gradients and a full planner run
captured from the reference (tests/golden/grad.npz, gd_planner.npz)."""
import numpy as np
import pytest
import torch

from dyn_res_pile_manip_amd import synthetic as syn, weights
from dyn_res_pile_manip_amd.gnn_dyn import PropNetDiffDenModel
from dyn_res_pile_manip_amd.planners import PlannerGD, world2cam_affine

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures('exact_goal_transform')]
# max|gradient - reference's autograd| / max|reference's|: 5 x the worst OBSERVED (round 6) -- d loss / d state
# 1.6e-6, d loss / d push 5.5e-7 on the seed-0 weights, 7.7e-7 on the stress weights; rounds 2 - 5 asserted 1e-3 / 2e-3
GRAD_STATE_BOUND = 8e-6
GRAD_BOUND = 3e-6
GRAD_BOUND_STRESS = 4e-6


@pytest.fixture(scope='module')
def ctx(golden):
    from dyn_res_pile_manip_amd.engine import Engine
    eng = Engine(0)
    eng.load_weights(weights.blob_from_state_dict(golden.weights_seed0), 0.08)
    eng.set_camera(world2cam_affine(syn.demo_cam_extrinsics()), 24.0, syn.demo_cam_params())
    yield eng
    eng.close()


@pytest.mark.parametrize('case', ['h1', 'h1_n100', 'h2'])
def test_gradients_match_the_reference(ctx, golden, case):
    g = golden.grad
    obs_goal = syn.goal_distance_image(syn.goal_mask('I'))
    ctx.set_goal(syn.goal_field(obs_goal), g[case + '/goal_coor'])
    lo, hi = syn.action_limits()
    ctx.gd_begin(g[case + '/s_cur'], g[case + '/attr'], g[case + '/dens'], g[case + '/act_seqs'], 0.05, lo, hi)
    r, ga, gs = ctx.gd_grad(want_state_grad=True)
    np.testing.assert_allclose(r, g[case + '/reward'][:, 0], rtol=2e-5)
    ref_gs, ref_ga = g[case + '/grad_state_pred'], g[case + '/grad_act']
    # d loss / d predicted state: bilinear-sample and chamfer arg-min gradients through the projection
    # (the reference's retained gradient of its in-place-filled state_pred tensor only shows the final
    # step's slice: earlier slices were read through an older version of the tensor)
    assert gs.shape == ref_gs.shape
    err_s = float(np.abs(gs[:, -1] - ref_gs[:, -1]).max() / np.abs(ref_gs).max())
    # d loss / d push through predictor, 3 propagation steps, particle encoder and gen_s_delta
    err = float(np.abs(ga - ref_ga).max() / np.abs(ref_ga).max())
    print('[grad-err] seed0 %s: d/d state %.3e, d/d push %.3e (abs %.3e)' % (case, err_s, err, np.abs(ga - ref_ga).max()))
    assert err_s < GRAD_STATE_BOUND
    assert err < GRAD_BOUND
    assert np.abs(ga - ref_ga).max() < 1e-4
    # rows whose push misses the pile have exactly zero gradient in both
    np.testing.assert_array_equal(np.abs(ga).sum((1, 2)) == 0, np.abs(ref_ga).sum((1, 2)) == 0)


@pytest.mark.parametrize('case', ['seed1_attr_h1', 'big_h1', 'big_attr_h2'])
def test_gradients_under_other_weights_match_the_reference(golden, case):
    """Beyond the seed-0 weights (tests/golden/grad_stress.npz): a second seed with per-particle attributes in two
    batch columns, and first encoder layers x 300 (hidden activations ~1e2; the tape's ReLU masks come from the
    split-fp16 forward pass under its range shift), horizons 1 and 2 -- small batches (the launch-per-stage
    kernels) and the same cases replicated to a chip-filling batch (kmb_step_bwd)."""
    from dyn_res_pile_manip_amd.engine import Engine
    from test_oracle_golden import stress_weights
    g = golden.grad_stress
    eng = Engine(0)
    eng.load_weights(weights.blob_from_state_dict(stress_weights(g, case)), 0.08)
    eng.set_camera(world2cam_affine(syn.demo_cam_extrinsics()), 24.0, syn.demo_cam_params())
    obs_goal = syn.goal_distance_image(syn.goal_mask('I'))
    eng.set_goal(syn.goal_field(obs_goal), g[case + '/goal_coor'])
    lo, hi = syn.action_limits()
    ref_ga = g[case + '/grad_act']
    N = g[case + '/s_cur'].shape[1]
    for reps in (1, -(-1100 // (ref_ga.shape[0] * ((N + 31) // 32)))):
        acts = np.tile(g[case + '/act_seqs'], (reps, 1, 1))
        eng.gd_begin(g[case + '/s_cur'], g[case + '/attr'], g[case + '/dens'], acts, 0.05, lo, hi)
        r, ga, _ = eng.gd_grad()
        want = np.tile(ref_ga, (reps, 1, 1))
        np.testing.assert_allclose(r, np.tile(g[case + '/reward'][:, 0], reps), rtol=2e-5)
        err = float(np.abs(ga - want).max() / np.abs(ref_ga).max())
        print('[grad-err] stress %s reps=%d: %.3e' % (case, reps, err))
        assert err < GRAD_BOUND_STRESS, (reps, err)
        assert np.abs(ga).sum((1, 2)).min() > 0
    eng.close()


def test_adam_iterations_and_planner_dict_match_the_reference(golden):
    """The reference's own GD planner run (3 Adam iterations, 10 trajectories x 3 columns, N = 40),
    called exactly as env/flex_env.py:1048-1065 calls it."""
    config = syn.default_config()
    config['mpc']['mpc_type'] = 'GD'
    env = syn.SyntheticEnv(config)
    model = PropNetDiffDenModel(config, True)
    model.load_state_dict({k[2:]: torch.from_numpy(golden.weights_seed0[k]) for k in golden.weights_seed0.files
                           if k.startswith('w/')}, strict=False)
    planner = PlannerGD(config, env)
    g = golden.gd_planner
    obs_goal = syn.goal_distance_image(syn.goal_mask('I'))
    lo, hi = syn.action_limits()
    res = planner.trajectory_optimization_ptcl_multi_traj(
        g['s_cur'], g['dens'], g['attr'], obs_goal, model, g['act_seq'], np.zeros(1), n_sample=10, n_look_ahead=1,
        n_update_iter=3, action_lower_lim=lo, action_upper_lim=hi, use_gpu=True, time_lim=1e9)
    model.engine.close()
    # goal pixels are subsampled by farthest-point sampling from index 0 (planners.py:621): deterministic
    np.testing.assert_allclose(res['rew_mean'], g['out/rew_mean'], rtol=1e-4)
    np.testing.assert_allclose(res['rew_std'], g['out/rew_std'], rtol=2e-3)
    np.testing.assert_allclose(res['action_full'], g['out/action_full'], atol=2e-3)
    np.testing.assert_allclose(res['reward_full'], g['out/reward_full'], rtol=1e-4)
    np.testing.assert_allclose(res['action_sequence'], g['out/action_sequence'], atol=2e-3)
    np.testing.assert_allclose(res['observation_sequence'], g['out/observation_sequence'], atol=5e-6)
    np.testing.assert_allclose(res['reward'], g['out/reward'], rtol=1e-4)
    np.testing.assert_allclose(res['next_r'], g['out/next_r'], rtol=1e-4)
    assert res['iter_num'] == int(g['out/iter_num'])


def test_binding_time_limit_gives_the_reference_iteration_count(golden):
    """Rows a14 / a15: with time_lim = 50 ms and N = 40 (15 ms per iteration in the reference's model,
    planners.py:25-28) the reference runs int(50 / 15) = 3 of the 10 allowed iterations (planners.py:679-682);
    gd_loop = 2 only sizes rew_mean / rew_std.  Same iteration count, same Adam trajectory, same dict."""
    config = syn.default_config()
    config['mpc']['mpc_type'] = 'GD'
    env = syn.SyntheticEnv(config)
    model = PropNetDiffDenModel(config, True)
    model.load_state_dict({k[2:]: torch.from_numpy(golden.weights_seed0[k]) for k in golden.weights_seed0.files
                           if k.startswith('w/')}, strict=False)
    planner = PlannerGD(config, env)
    g = golden.gd_planner_tl
    obs_goal = syn.goal_distance_image(syn.goal_mask('I'))
    lo, hi = syn.action_limits()
    res = planner.trajectory_optimization_ptcl_multi_traj(
        g['s_cur'], g['dens'], g['attr'], obs_goal, model, g['act_seq'], np.zeros(1), n_sample=10, n_look_ahead=1,
        n_update_iter=int(g['n_update_iter']), action_lower_lim=lo, action_upper_lim=hi, use_gpu=True,
        gd_loop=int(g['gd_loop']), time_lim=float(g['time_lim']))
    assert res['iter_num'] == int(g['out/iter_num']) == 2
    assert res['rew_mean'].shape == g['out/rew_mean'].shape == (1, 20)
    np.testing.assert_allclose(res['rew_mean'], g['out/rew_mean'], rtol=1e-4)
    np.testing.assert_allclose(res['rew_std'], g['out/rew_std'], rtol=2e-3)
    np.testing.assert_allclose(res['action_full'], g['out/action_full'], atol=2e-3)
    np.testing.assert_allclose(res['reward_full'], g['out/reward_full'], rtol=1e-4)
    np.testing.assert_allclose(res['action_sequence'], g['out/action_sequence'], atol=2e-3)
    np.testing.assert_allclose(res['observation_sequence'], g['out/observation_sequence'], atol=5e-6)
    np.testing.assert_allclose(res['reward'], g['out/reward'], rtol=1e-4)
    np.testing.assert_allclose(res['next_r'], g['out/next_r'], rtol=1e-4)
    # the wall clock plays no part: a second call gives the same bits
    res2 = planner.trajectory_optimization_ptcl_multi_traj(
        g['s_cur'], g['dens'], g['attr'], obs_goal, model, g['act_seq'], np.zeros(1), n_sample=10, n_look_ahead=1,
        n_update_iter=int(g['n_update_iter']), action_lower_lim=lo, action_upper_lim=hi, use_gpu=True,
        gd_loop=int(g['gd_loop']), time_lim=float(g['time_lim']))
    np.testing.assert_array_equal(res['action_full'], res2['action_full'])
    assert res2['iter_num'] == 2
    # a budget below one iteration: the reference fails at its return statement; here a clear error
    with pytest.raises(ValueError):
        planner.trajectory_optimization_ptcl_multi_traj(
            g['s_cur'], g['dens'], g['attr'], obs_goal, model, g['act_seq'], np.zeros(1), n_sample=10, n_look_ahead=1,
            n_update_iter=10, action_lower_lim=lo, action_upper_lim=hi, use_gpu=True, time_lim=10.0)
    model.engine.close()


def test_gradients_are_reproducible_and_both_list_paths_agree(ctx, golden, monkeypatch):
    """No atomics in the backward pass: two evaluations give bit-identical gradients, and the
    reversed neighbour lists built in LDS or in global memory (samples beyond 3072 particles,
    forced here with DRP_REV_GLOBAL) give the same bits too."""
    from dyn_res_pile_manip_amd.engine import Engine
    obs_goal = syn.goal_distance_image(syn.goal_mask('I'))
    lo, hi = syn.action_limits()
    monkeypatch.setenv('DRP_REV_GLOBAL', '1')
    other = Engine(0)
    monkeypatch.delenv('DRP_REV_GLOBAL')
    other.load_weights(weights.blob_from_state_dict(golden.weights_seed0), 0.08)
    other.set_camera(world2cam_affine(syn.demo_cam_extrinsics()), 24.0, syn.demo_cam_params())
    for N, B, H in ((120, 6, 1), (300, 3, 2), (3200, 2, 1)):
        s0, dens, attr = syn.make_pile(N, 1, seed=N)
        gc = syn.goal_coor_strided(obs_goal, min(5 * N, 2000))
        acts = np.stack([syn.nominal_pushes(H, seed=50 + i) for i in range(B)]).astype(np.float32)
        acts[:, 0] = [-3.5, 0.3, 2.5, -0.2]           # through the pile: every row has a gradient
        acts[:, 0, 1] += 0.1 * np.arange(B)
        res = []
        for eng in (ctx, other):
            eng.set_goal(syn.goal_field(obs_goal), gc)
            eng.gd_begin(s0, attr, dens, acts, 0.05, lo, hi)
            r0, g0, _ = eng.gd_grad()
            r1, g1, _ = eng.gd_grad()
            np.testing.assert_array_equal(g0, g1)
            np.testing.assert_array_equal(r0, r1)
            assert np.isfinite(g0).all() and np.abs(g0).max() > 0
            res.append(g0)
        np.testing.assert_array_equal(res[0], res[1])
    other.close()


@pytest.mark.parametrize('case', ['h1', 'h2'])
def test_large_batches_take_the_matrix_core_node_kernels(ctx, golden, case):
    """With >= 1024 tiles of 32 rows the node-level backward stages run on the fp32 matrix cores
    (k_backward_mfma.h) instead of the chunked row kernels: the reference's case replicated to
    that size must give the reference's gradients in every replica."""
    g = golden.grad
    B0 = g[case + '/act_seqs'].shape[0]
    N = g[case + '/s_cur'].shape[1]
    reps = -(-1100 // (B0 * ((N + 31) // 32)))
    obs_goal = syn.goal_distance_image(syn.goal_mask('I'))
    ctx.set_goal(syn.goal_field(obs_goal), g[case + '/goal_coor'])
    lo, hi = syn.action_limits()
    acts = np.tile(g[case + '/act_seqs'], (reps, 1, 1))           # row = sample * n_batch + batch
    assert acts.shape[0] * ((N + 31) // 32) >= 1024
    ctx.gd_begin(g[case + '/s_cur'], g[case + '/attr'], g[case + '/dens'], acts, 0.05, lo, hi)
    r, ga, _ = ctx.gd_grad()
    ref_ga = np.tile(g[case + '/grad_act'], (reps, 1, 1))
    np.testing.assert_allclose(r, np.tile(g[case + '/reward'][:, 0], reps), rtol=2e-5)
    assert np.abs(ga - ref_ga).max() < 2e-3 * np.abs(ref_ga).max()
    assert np.abs(ga - ref_ga).max() < 1e-4
    # replicas are independent samples: identical bits
    np.testing.assert_array_equal(ga[:B0], ga[-B0:])


@pytest.mark.parametrize('N,B', [(12, 1500), (40, 300), (100, 64), (5, 260)])
def test_fused_backward_equals_the_stage_kernels_for_small_piles_and_batches(monkeypatch, N, B):
    """kmb_step_bwd (a workgroup owns whole samples; everything between the reward's gradient and the impulses in one
    launch) runs for every tile count and for small batches of small samples since late round 2; the stage kernels
    (DRP_NO_BWD_FUSED=1) are the cross-check: the same gradients to rounding (the two sum a row's edges in different
    groupings), rewards bit for bit."""
    from dyn_res_pile_manip_amd.engine import Engine
    from dyn_res_pile_manip_amd import weights
    from dyn_res_pile_manip_amd.planners import world2cam_affine
    s0, dens, attr = syn.make_pile(N, 1, seed=N)
    acts = syn.sample_pushes(B, 1, seed=B)
    obs_goal = syn.goal_distance_image(syn.goal_mask('I'))
    lo, hi = syn.action_limits()
    res = {}
    for stage in (False, True):
        if stage:
            monkeypatch.setenv('DRP_NO_BWD_FUSED', '1')
        else:
            monkeypatch.delenv('DRP_NO_BWD_FUSED', raising=False)
        eng = Engine(0)
        eng.load_weights(weights.blob_from_state_dict(weights.random_state_dict(seed=0)), 0.08)
        eng.set_camera(world2cam_affine(syn.demo_cam_extrinsics()), 24.0, syn.demo_cam_params())
        eng.set_goal(syn.goal_field(obs_goal), syn.goal_coor_strided(obs_goal, 5 * N))
        eng.gd_begin(s0, attr, dens, acts, 0.05, lo, hi)
        res[stage] = eng.gd_grad()
        eng.close()
    np.testing.assert_array_equal(res[False][0], res[True][0])
    scale = np.abs(res[True][1]).max()
    assert scale > 0 and np.isfinite(res[False][1]).all()
    assert np.abs(res[False][1] - res[True][1]).max() < 2e-5 * scale


@pytest.mark.parametrize('N,B,H', [(12, 1500, 1), (20, 1500, 1), (50, 300, 1), (100, 750, 1), (100, 7, 2), (64, 300, 2),
                                   (256, 40, 1), (5, 260, 2), (33, 257, 1)])
def test_rows_kept_in_registers_against_the_rows_through_memory(monkeypatch, N, B, H):
    """kmb_rows_bwd (piles of up to 256 particles: a wave keeps g_eff, g_cnode and its own g_agg rows in registers through
    all phases, the group's g_agg rows in LDS, the 64 x 64 layers on the six-product bf16 split) against kmb_step_bwd
    (DRP_NO_BWD_ROWS=1: every row through memory per phase, fp32 MFMA): the same masked sums in the same order, the
    layers to fp32 rounding -- rewards bit for bit, push and state gradients to 5e-5 of their scale per row (seen: 1e-6, 8e-6 at 100 particles;
    a ReLU kink of a recomputed hidden unit aside, below); horizon 2 also
    covers the g_agg rows the relation encoder's backward reads from memory."""
    from dyn_res_pile_manip_amd.engine import Engine
    from dyn_res_pile_manip_amd import weights
    from dyn_res_pile_manip_amd.planners import world2cam_affine
    s0, dens, attr = syn.make_pile(N, 1, seed=N)
    acts = syn.sample_pushes(B, H, seed=B)
    obs_goal = syn.goal_distance_image(syn.goal_mask('I'))
    lo, hi = syn.action_limits()
    res = {}
    for rows in (True, False):
        if rows:
            monkeypatch.delenv('DRP_NO_BWD_ROWS', raising=False)
        else:
            monkeypatch.setenv('DRP_NO_BWD_ROWS', '1')
        eng = Engine(0)
        eng.load_weights(weights.blob_from_state_dict(weights.random_state_dict(seed=0)), 0.08)
        eng.set_camera(world2cam_affine(syn.demo_cam_extrinsics()), 24.0, syn.demo_cam_params())
        eng.set_goal(syn.goal_field(obs_goal), syn.goal_coor_strided(obs_goal, 5 * N))
        eng.gd_begin(s0, attr, dens, acts, 0.05, lo, hi)
        res[rows] = eng.gd_grad(want_state_grad=True)
        eng.close()
    np.testing.assert_array_equal(res[True][0], res[False][0])
    for a, b in zip(res[True][1:], res[False][1:]):
        scale = np.abs(b).max()
        assert scale > 0 and np.isfinite(a).all()
        per_row = np.abs(a - b).reshape(B, -1).max(1) / scale
        print('N=%d B=%d H=%d: max deviation %.2e of the scale, %d of %d rows above 5e-5' % (N, B, H, per_row.max(), (per_row > 5e-5).sum(), B))
        # Both kernels recompute the hidden layers of the predictor and the particle encoder for their ReLU masks, one on fp32
        # matrix instructions, the other on the six-product bf16 split: a hidden unit within rounding of zero can fall on
        # different sides (seen: one row of 40 at 256 particles, 1.2e-3 of the scale; the REFERENCE's own sign for that unit is
        # a third opinion).  Such a row is allowed -- one per thousand, and no further off than a single unit's share.
        assert (per_row > 5e-5).sum() <= 1 + B // 1000 and per_row.max() < 5e-3


@pytest.mark.parametrize('N,B', [(20, 1500), (100, 300), (128, 40), (7, 33)])
def test_reversed_lists_from_the_lists_own_launch(monkeypatch, N, B):
    """Horizon 1, samples of one graph chunk (up to 128 particles): k_graph_rev builds the reversed lists behind the
    neighbour lists in the same launch, and the optimiser step rides on the last kb_sdelta launch; with
    DRP_NO_GRAPH_REV=1 kb_reverse_lists runs as a launch of its own.  Same lists: the same rewards, pushes after three
    iterations and gradients, bit for bit."""
    from dyn_res_pile_manip_amd.engine import Engine
    from dyn_res_pile_manip_amd import weights
    from dyn_res_pile_manip_amd.planners import world2cam_affine
    s0, dens, attr = syn.make_pile(N, 1, seed=N)
    acts = syn.sample_pushes(B, 1, seed=B)
    obs_goal = syn.goal_distance_image(syn.goal_mask('I'))
    lo, hi = syn.action_limits()
    res = {}
    for own in (False, True):
        if own:
            monkeypatch.setenv('DRP_NO_GRAPH_REV', '1')
        else:
            monkeypatch.delenv('DRP_NO_GRAPH_REV', raising=False)
        eng = Engine(0)
        eng.load_weights(weights.blob_from_state_dict(weights.random_state_dict(seed=0)), 0.08)
        eng.set_camera(world2cam_affine(syn.demo_cam_extrinsics()), 24.0, syn.demo_cam_params())
        eng.set_goal(syn.goal_field(obs_goal), syn.goal_coor_strided(obs_goal, 5 * N))
        eng.gd_begin(s0, attr, dens, acts, 0.05, lo, hi)
        out = list(eng.gd_grad(want_state_grad=True))
        for _ in range(3):
            out.append(eng.gd_step())
        out.append(eng.gd_actions())
        out.append(eng.debug_fetch('rev_off', (B, N + 1), np.int32))
        res[own] = out
        eng.close()
    assert np.abs(res[True][1]).max() > 0 and not np.array_equal(res[True][-2], acts)
    for a, b in zip(res[False], res[True]):
        np.testing.assert_array_equal(a, b)


def test_pipelined_iterations_equal_the_blocking_ones(ctx, golden):
    """drp_gd_step_async / drp_gd_wait (iteration i + 1 enqueued before the host waits for iteration i) against
    drp_gd_step + drp_gd_get: the same rewards and pushes, bit for bit, in every iteration; a slot that has not been
    waited for is refused."""
    from dyn_res_pile_manip_amd import _lib
    g = golden.grad
    obs_goal = syn.goal_distance_image(syn.goal_mask('I'))
    ctx.set_goal(syn.goal_field(obs_goal), g['h1/goal_coor'])
    lo, hi = syn.action_limits()
    args = (g['h1/s_cur'], g['h1/attr'], g['h1/dens'], g['h1/act_seqs'], 0.05, lo, hi)
    ctx.gd_begin(*args)
    want = []
    for _ in range(5):
        r = ctx.gd_step()
        want.append((r, ctx.gd_actions()))
    ctx.gd_begin(*args)
    ctx.gd_step_async(0)
    with pytest.raises(_lib.DrpError):
        ctx.gd_step_async(0)
    for i in range(5):
        if i + 1 < 5:
            ctx.gd_step_async((i + 1) & 1)
        r, a = ctx.gd_wait(i & 1)
        np.testing.assert_array_equal(r, want[i][0])
        np.testing.assert_array_equal(a, want[i][1])
    with pytest.raises(_lib.DrpError):
        ctx.gd_wait(0)
    # all five enqueued before the first wait (the planner keeps three ahead): the iterations' own kernels write the
    # eight pinned slots, no copy sits between two iterations on the stream
    ctx.gd_begin(*args)
    for i in range(5):
        ctx.gd_step_async(3 + i)
    with pytest.raises(_lib.DrpError):
        ctx.gd_step_async(8)
    for i in range(5):
        r, a = ctx.gd_wait(3 + i)
        np.testing.assert_array_equal(r, want[i][0])
        np.testing.assert_array_equal(a, want[i][1])


@pytest.mark.parametrize('N', [20, 70])
def test_a_blocking_gradient_between_an_async_step_and_its_wait(ctx, N):
    """A pass's outputs are its arguments (csrc/capi_gd.h: GdPass): drp_gd_grad issued while an iteration's slot is still
    pending is a gradients-only pass -- no optimiser step, no store to the slot.  Horizon 2 (the t > 0 branch and the Adam
    step on the t == 0 launch both run), one tile of 32 rows and three with the last ragged: step, gradient, wait against
    step, wait, gradient, bit for bit."""
    B, H = 4, 2
    s0, dens, attr = syn.make_pile(N, 1, seed=N)
    obs_goal = syn.goal_distance_image(syn.goal_mask('I'))
    ctx.set_goal(syn.goal_field(obs_goal), syn.goal_coor_strided(obs_goal, 5 * N))
    lo, hi = syn.action_limits()
    acts = np.stack([syn.nominal_pushes(H, seed=50 + i) for i in range(B)]).astype(np.float32)
    acts[:, 0] = [-3.5, 0.3, 2.5, -0.2]           # through the pile: every row has a gradient
    acts[:, 0, 1] += 0.1 * np.arange(B)
    args = (s0, attr, dens, acts, 0.05, lo, hi)
    ctx.gd_begin(*args)
    ctx.gd_step_async(0)
    grad_a = ctx.gd_grad(want_state_grad=True)
    wait_a = ctx.gd_wait(0)
    after_a = ctx.gd_actions()
    ctx.gd_begin(*args)
    ctx.gd_step_async(0)
    wait_b = ctx.gd_wait(0)
    grad_b = ctx.gd_grad(want_state_grad=True)
    after_b = ctx.gd_actions()
    for a, b in zip(wait_a + grad_a, wait_b + grad_b):
        np.testing.assert_array_equal(a, b)
    assert np.isfinite(grad_a[1]).all() and (np.abs(grad_a[1]).sum((1, 2)) > 0).all()
    assert not np.array_equal(wait_a[1], acts)                      # the step moved the pushes ...
    np.testing.assert_array_equal(after_a, wait_a[1])               # ... and the gradient pass did not
    np.testing.assert_array_equal(after_b, wait_b[1])


@pytest.mark.parametrize('case', ['h1', 'h2'])
def test_the_stage_kernels_against_the_reference(monkeypatch, golden, case):
    """The planner's reverse-mode node stages a launch per stage (kmb_predict, kmb_node_step, kb_edge_terms, kmb_node_encode),
    which the golden shapes reach only with the one-launch kernels off (DRP_NO_BWD_FUSED=1 DRP_NO_BWD_ROWS=1): the reference's
    autograd gradients, and the dispatch says it was them."""
    from dyn_res_pile_manip_amd.engine import Engine
    for k in ('DRP_NO_BWD_ROWS', 'DRP_NO_BWD_FUSED'):
        monkeypatch.setenv(k, '1')
    g = golden.grad
    eng = Engine(0)
    eng.load_weights(weights.blob_from_state_dict(golden.weights_seed0), 0.08)
    eng.set_camera(world2cam_affine(syn.demo_cam_extrinsics()), 24.0, syn.demo_cam_params())
    obs_goal = syn.goal_distance_image(syn.goal_mask('I'))
    eng.set_goal(syn.goal_field(obs_goal), g[case + '/goal_coor'])
    lo, hi = syn.action_limits()
    eng.gd_begin(g[case + '/s_cur'], g[case + '/attr'], g[case + '/dens'], g[case + '/act_seqs'], 0.05, lo, hi)
    eng.dispatch_reset()
    r, ga, _ = eng.gd_grad()
    ran = eng.last_dispatch()
    eng.close()
    assert 'bwd:stages kmb_*' in ran and 'bwd:kmb_rows_bwd' not in ran and 'bwd:kmb_step_bwd' not in ran, ran
    np.testing.assert_allclose(r, g[case + '/reward'][:, 0], rtol=2e-5)
    ref_ga = g[case + '/grad_act']
    assert np.abs(ga - ref_ga).max() < 2e-3 * np.abs(ref_ga).max()


# ---- a tape forward's engine and lists are run_step's arguments: the context's selection and step workspace stay as they were ----
ENGINE_NAMES = ['valu', 'mfma', 'split', 'fused', 'lite']


@pytest.fixture(scope='module')
def untaped(golden):
    """a context that never ran a tape, and the step inputs (3 samples) per particle count"""
    from dyn_res_pile_manip_amd.engine import Engine
    eng = Engine(0)
    eng.load_weights(weights.blob_from_state_dict(golden.weights_seed0), 0.08)
    eng.set_camera(world2cam_affine(syn.demo_cam_extrinsics()), 24.0, syn.demo_cam_params())
    inputs, steps = {}, {}

    def step(name, N):
        if N not in inputs:
            s0, dens, attr = syn.make_pile(N, 3, seed=N)
            inputs[N] = (attr, s0, eng.gen_s_delta(s0, syn.sample_pushes(3, 1, seed=N)[:, 0]), dens)
        if (name, N) not in steps:
            eng.set_engine(name)
            steps[name, N] = eng.step(*inputs[N])
        return inputs[N], steps[name, N]
    yield step
    eng.close()


def _step_as_on_the_untaped_context(eng, untaped, name, N):
    from dyn_res_pile_manip_amd import _lib
    inputs, want = untaped(name, N)
    assert eng.engine_id == _lib.ENGINES[name]
    got = eng.step(*inputs)
    assert np.abs(got - inputs[1]).max() > 0
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize('N', [20, 130])
@pytest.mark.parametrize('name', ENGINE_NAMES)
def test_a_tape_forward_leaves_the_selected_engine_and_the_step_workspace_alone(ctx, untaped, name, N):
    """gd_grad writes its tape on the fused or the fp32 matrix engine whatever is selected, its impulses and lists into the
    tape's slices (N = 20: km_prop<tape> per step and k_graph_rev; N = 130: km_prop3<tape> and the strip graph).  A step on
    the same context afterwards runs the selected engine in the context's own workspace: the bits of a context that never
    ran a tape."""
    s0, dens, attr = syn.make_pile(N, 3, seed=N + 1)
    obs_goal = syn.goal_distance_image(syn.goal_mask('I'))
    lo, hi = syn.action_limits()
    ctx.set_goal(syn.goal_field(obs_goal), syn.goal_coor_strided(obs_goal, 5 * N))
    ctx.set_engine(name)
    try:
        ctx.gd_begin(s0, attr, dens, syn.sample_pushes(6, 2, seed=N), 0.05, lo, hi)
        r, ga = ctx.gd_grad()[:2]
        assert np.isfinite(r).all() and np.abs(ga).max() > 0
        _step_as_on_the_untaped_context(ctx, untaped, name, N)
    finally:
        ctx.set_engine('fused')


def test_a_training_tape_leaves_the_selected_engine_and_the_step_workspace_alone(golden, untaped):
    from dyn_res_pile_manip_amd.engine import Engine
    g = golden.train
    batch = [g['b2_r5/' + k] for k in ('states', 'states_delta', 'attrs', 'particle_nums', 'particle_dens')]
    eng = Engine(0)
    try:
        eng.load_weights(weights.blob_from_state_dict(golden.weights_seed0), 0.08)
        eng.set_camera(world2cam_affine(syn.demo_cam_extrinsics()), 24.0, syn.demo_cam_params())
        eng.set_engine('split')
        eng.train_begin(batch[0].shape[1] - 1, 1e-3, 0.9)
        loss, grad = eng.train_step(*batch, mode='grad', want_grad=True)
        assert np.isfinite(loss) and np.abs(grad).max() > 0
        _step_as_on_the_untaped_context(eng, untaped, 'split', 20)
    finally:
        eng.close()

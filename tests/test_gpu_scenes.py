"""GPU: multi-scene sessions (include/drp.h: drp_set_goal_scenes ... drp_gd_begin_scenes).  The yardstick is the single-scene
path, which the existing fixtures pin to the reference: everything a scene gets out of an S-scene session -- rewards, draws,
nominals, statistics, gradients, pushes, the planner's dict -- must be the bits of a single-scene session on that scene alone.

Shapes: S = 3 scenes x nb = 2 columns; N = 20 (one-launch rollout) and 65 (step-by-step pipeline); H = 3; 48 samples / 6
trajectories per scene; three different 720 x 720 goals with m = (5N, 3N, 1) goal pixels, the table's padding filled with NaN."""
import copy

import numpy as np
import pytest

from dyn_res_pile_manip_amd import _lib, synthetic as syn, weights
from dyn_res_pile_manip_amd.engine import interleave_scenes, split_scenes
from dyn_res_pile_manip_amd.planners import world2cam_affine
from oracle import propnet_sparse as osp

pytestmark = pytest.mark.gpu

S, NB, H, NS, TRAJ = 3, 2, 3, 48, 6
SEEDS = (11, 2 ** 40 + 22, 33)
MP = dict(sigma=0.6, beta_filter=0.7, reward_weight=20.0)
CASES = [(20, 'seed0', 'fused'), (65, 'seed0', 'fused'), (20, 'trained', 'fused'), (65, 'trained', 'fused'), (20, 'seed0', 'mfma')]


def goal_images():
    m = np.zeros((syn.SCREEN, syn.SCREEN), np.uint8)
    yy, xx = np.mgrid[0:syn.SCREEN, 0:syn.SCREEN]
    m[(yy - 250) ** 2 + (xx - 430) ** 2 < 60 ** 2] = 1          # a disc off the centre
    return np.stack([syn.goal_distance_image(syn.goal_mask('I')), syn.goal_distance_image(syn.goal_mask('disc')),
                     syn.goal_distance_image(m)])


@pytest.fixture(scope='module')
def eng():
    from dyn_res_pile_manip_amd.engine import Engine
    e = Engine(0)
    e.set_camera(world2cam_affine(syn.demo_cam_extrinsics()), 24.0, syn.demo_cam_params())
    e.images = goal_images()
    e.loaded = None
    e.goal_cache = {}
    yield e
    e.close()


def prepare(eng, golden, N, wset='seed0', engine='fused'):
    """weights, engine, the three goals with m = (5N, 3N, 1) as single goals AND as the table (NaN padding), three piles"""
    if eng.loaded != wset:
        eng.load_weights(weights.blob_from_state_dict(golden.weights_seed0 if wset == 'seed0' else golden.weights_trained), 0.08)
        eng.loaded = wset
    eng.set_engine(engine)
    if N not in eng.goal_cache:
        eng.goal_cache[N] = [eng.set_goal_image(eng.images[k], mk, want=True) for k, mk in enumerate((5 * N, 3 * N, 1))]
    goals = eng.goal_cache[N]
    m = np.array([g[1].shape[0] for g in goals], np.int32)
    assert tuple(m) == (5 * N, 3 * N, 1)
    coor = np.full((S, 5 * N, 2), np.nan, np.float32)
    for k, g in enumerate(goals):
        coor[k, :m[k]] = g[1]
    eng.set_goal_scenes(np.stack([g[0] for g in goals]), coor, m)
    piles = [syn.make_pile(N, NB, seed=7 + k) for k in range(S)]
    s0 = np.stack([p[0] for p in piles])
    dens = np.stack([p[1] for p in piles]) * np.array([[1.0], [0.9], [1.1]], np.float32)
    attr = np.stack([p[2] for p in piles])
    return goals, s0, attr, dens


def single_goal(eng, goals, k):
    eng.set_goal(goals[k][0], goals[k][1])


# ---- 1. the goal table --------------------------------------------------------------------------------------------
def test_goal_image_scenes_slots_are_the_single_scene_bits(eng, golden):
    N = 20
    prepare(eng, golden, N)
    singles = [eng.set_goal_image(eng.images[k], 5 * N, want=True) for k in range(S)]
    m = eng.set_goal_image_scenes(eng.images, 5 * N)
    fields, coors = eng.set_goal_image_scenes(eng.images, 5 * N, want=True)
    np.testing.assert_array_equal(m, [c.shape[0] for _, c in singles])
    for k in range(S):
        np.testing.assert_array_equal(fields[k], singles[k][0])
        np.testing.assert_array_equal(coors[k], singles[k][1])
    # and the device's table holds them: rewards through the table are the single goal's
    st = syn.make_pile(N, 4, seed=3)[0]
    for k in range(S):
        eng.set_goal(*singles[k])
        np.testing.assert_array_equal(eng.reward_scenes(st, np.full(4, k)), eng.reward(st))


def test_installing_a_table_leaves_the_single_goal_alone(eng, golden):
    N = 20
    goals, _, _, _ = prepare(eng, golden, N)
    st = syn.make_pile(N, 4, seed=4)[0]
    eng.set_goal_image(eng.images[1], 3 * N)
    before = eng.reward(st)
    eng.set_goal_image_scenes(eng.images[::-1].copy(), 5 * N)
    np.testing.assert_array_equal(eng.reward(st), before)
    eng.set_goal_scenes(np.stack([g[0] for g in goals]), [g[1] for g in goals])
    np.testing.assert_array_equal(eng.reward(st), before)
    # and the reverse: a new single goal leaves the table alone
    r_tab = eng.reward_scenes(st, [0, 1, 2, 0])
    single_goal(eng, goals, 2)
    np.testing.assert_array_equal(eng.reward_scenes(st, [0, 1, 2, 0]), r_tab)


# ---- 2. the reward -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', [20, 65])
def test_reward_scenes_rows_are_the_single_goal_bits(eng, golden, N):
    goals, s0, attr, dens = prepare(eng, golden, N)
    states = np.concatenate([eng.rollout(s0[k], attr[k], dens[k], syn.sample_pushes(8, H, seed=k))[0][:, -1] for k in range(S)])
    scene = np.random.default_rng(5).permutation(np.repeat(np.arange(S), 8)).astype(np.int32)
    for normalize in (True, False):
        out = eng.reward_scenes(states, scene, normalize=normalize)
        assert np.isfinite(out).all()                     # the NaN padding behind m[s] is never read
        for k in range(S):
            rows = np.nonzero(scene == k)[0]
            single_goal(eng, goals, k)
            np.testing.assert_array_equal(out[rows], eng.reward(states[rows], normalize=normalize))
            ref = osp.reward(states[rows], goals[k][0], syn.demo_cam_params(), goals[k][1], normalize=normalize)
            np.testing.assert_allclose(out[rows], ref, rtol=1e-5)
    # three different goals: the rows of one state differ by scene
    r3 = eng.reward_scenes(np.repeat(states[:1], S, 0), np.arange(S))
    assert len(set(r3.tolist())) == S


# ---- 3. MPPI -----------------------------------------------------------------------------------------------------
def nominals():
    return np.stack([syn.nominal_pushes(H, seed=k) for k in range(S)])


def run_single(eng, goals, s0, attr, dens, k, update, noise=None, n_iter=3, noise_type='normal'):
    lo, hi = syn.action_limits()
    single_goal(eng, goals, k)
    eng.mpc_begin(s0[k], attr[k], dens[k], nominals()[k], NS, act_lo=lo, act_hi=hi, seed=SEEDS[k], noise_type=noise_type, **MP)
    out = []
    for it in range(n_iter):
        eng.mpc_sample(it, None if noise is None else noise[it, k])
        eng.mpc_rollout(False)
        update(eng)
        got = eng.mpc_get(actions=True, rewards=True, nominal=True)
        out.append((got['actions'], got['rewards'], got['nominal'], eng.mpc_stats()))
    return out


def run_multi(eng, s0, attr, dens, update, noise=None, n_iter=3, noise_type='normal'):
    lo, hi = syn.action_limits()
    eng.mpc_begin_scenes(s0, attr, dens, nominals(), NS, act_lo=lo, act_hi=hi, seeds=SEEDS, noise_type=noise_type, **MP)
    out = []
    for it in range(n_iter):
        eng.mpc_sample(it, None if noise is None else noise[it])
        eng.mpc_rollout(False)
        update(eng)
        got = eng.mpc_get(actions=True, rewards=True, nominal=True)
        out.append((split_scenes(got['actions'], S, NB), split_scenes(got['rewards'], S, NB), got['nominal'], eng.mpc_stats_scenes()))
    return out


def assert_scenes_equal(multi, singles):
    for it, (a, r, nom, stats) in enumerate(multi):
        for k in range(S):
            sa, sr, snom, sstats = singles[k][it]
            np.testing.assert_array_equal(a[k], sa, err_msg='actions it %d scene %d' % (it, k))
            np.testing.assert_array_equal(r[k], sr, err_msg='rewards it %d scene %d' % (it, k))
            np.testing.assert_array_equal(nom[k], snom, err_msg='nominal it %d scene %d' % (it, k))
            assert stats[k] == sstats, (it, k, stats[k], sstats)


UPDATES = {'softmax': lambda e: e.mpc_update_device(), 'elite': lambda e: e.mpc_update_elite_device(5)}


@pytest.mark.parametrize('N,wset,engine', CASES)
@pytest.mark.parametrize('update', ['softmax', 'elite'])
def test_mppi_session_scenes_are_single_sessions(eng, golden, N, wset, engine, update):
    goals, s0, attr, dens = prepare(eng, golden, N, wset, engine)
    multi = run_multi(eng, s0, attr, dens, UPDATES[update])
    singles = [run_single(eng, goals, s0, attr, dens, k, UPDATES[update]) for k in range(S)]
    assert_scenes_equal(multi, singles)
    # the scenes are different problems: their draws and nominals differ
    assert not np.array_equal(multi[0][0][0], multi[0][0][1]) and not np.array_equal(multi[-1][2][0], multi[-1][2][1])
    # two runs of the session are bit-equal
    again = run_multi(eng, s0, attr, dens, UPDATES[update])
    for (a, r, nom, st), (a2, r2, nom2, st2) in zip(multi, again):
        np.testing.assert_array_equal(a, a2)
        np.testing.assert_array_equal(r, r2)
        np.testing.assert_array_equal(nom, nom2)
        assert st == st2


@pytest.mark.parametrize('noise_type', ['normal', 'uniform'])
def test_mppi_session_with_host_noise(eng, golden, noise_type):
    N = 20
    goals, s0, attr, dens = prepare(eng, golden, N)
    rng = np.random.default_rng(9)
    noise = (rng.normal(size=(3, S, NS, H, 4)) if noise_type == 'normal' else rng.uniform(-1, 1, (3, S, NS, H, 4))).astype(np.float32)
    multi = run_multi(eng, s0, attr, dens, UPDATES['softmax'], noise=noise, noise_type=noise_type)
    singles = [run_single(eng, goals, s0, attr, dens, k, UPDATES['softmax'], noise=noise, noise_type=noise_type) for k in range(S)]
    assert_scenes_equal(multi, singles)


def test_mppi_all_step_rewards_and_async_fetch(eng, golden):
    """reward_all_steps reads the row's scene at every step; fetch_async / wait carry the session's rows"""
    N = 20
    goals, s0, attr, dens = prepare(eng, golden, N)
    lo, hi = syn.action_limits()
    eng.mpc_begin_scenes(s0, attr, dens, nominals(), NS, act_lo=lo, act_hi=hi, seeds=SEEDS, **MP)
    eng.mpc_sample(0)
    eng.mpc_rollout(True)
    eng.mpc_fetch_async(0)
    got = eng.mpc_get(actions=True, rewards=True, rewards_all=True)
    w = eng.mpc_wait(0)
    np.testing.assert_array_equal(w['actions'], got['actions'])
    np.testing.assert_array_equal(w['rewards'], got['rewards'])
    ra = split_scenes(got['rewards_all'], S, NB)
    for k in range(S):
        single_goal(eng, goals, k)
        eng.mpc_begin(s0[k], attr[k], dens[k], nominals()[k], NS, act_lo=lo, act_hi=hi, seed=SEEDS[k], **MP)
        eng.mpc_sample(0)
        eng.mpc_rollout(True)
        np.testing.assert_array_equal(ra[k], eng.mpc_get(rewards_all=True)['rewards_all'])


# ---- 4. GD -------------------------------------------------------------------------------------------------------
def gd_candidates():
    return np.stack([np.repeat(syn.sample_pushes(TRAJ, H, seed=20 + k), NB, axis=0) for k in range(S)])      # [S, TRAJ * NB, H, 4]


@pytest.mark.parametrize('N,wset,engine', CASES)
def test_gd_session_scenes_are_single_sessions(eng, golden, N, wset, engine):
    goals, s0, attr, dens = prepare(eng, golden, N, wset, engine)
    lo, hi = syn.action_limits()
    cand = gd_candidates()
    eng.dispatch_reset()
    eng.gd_begin_scenes(s0, attr, dens, interleave_scenes(cand, NB), 0.05, lo, hi)
    r, g, gs = eng.gd_grad(want_state_grad=True)
    assert ('k_aggregate_tape' in eng.last_dispatch()) == (engine == 'mfma')          # the tape the case asks for
    r, g, gs = split_scenes(r, S, NB), split_scenes(g, S, NB), split_scenes(gs, S, NB)
    rs = []
    for _ in range(4):
        rs.append(split_scenes(eng.gd_step(), S, NB))
    acts = split_scenes(eng.gd_actions(), S, NB)
    # the pipelined loop of the same problem
    eng.gd_begin_scenes(s0, attr, dens, interleave_scenes(cand, NB), 0.05, lo, hi)
    for q in range(4):
        eng.gd_step_async(q)
    waited = [eng.gd_wait(q) for q in range(4)]
    for q in range(4):
        np.testing.assert_array_equal(split_scenes(waited[q][0], S, NB), rs[q])
    np.testing.assert_array_equal(split_scenes(waited[3][1], S, NB), acts)
    for k in range(S):
        single_goal(eng, goals, k)
        eng.gd_begin(s0[k], attr[k], dens[k], cand[k], 0.05, lo, hi)
        r1, g1, gs1 = eng.gd_grad(want_state_grad=True)
        np.testing.assert_array_equal(r[k], r1)
        np.testing.assert_array_equal(g[k], g1)
        np.testing.assert_array_equal(gs[k], gs1)
        for q in range(4):
            np.testing.assert_array_equal(rs[q][k], eng.gd_step(), err_msg='step %d scene %d' % (q, k))
        np.testing.assert_array_equal(acts[k], eng.gd_actions())
    assert np.abs(g).max() > 0 and not np.array_equal(r[0], r[1])


# ---- 5. the planner ----------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def stack(golden):
    import torch
    from dyn_res_pile_manip_amd.gnn_dyn import PropNetDiffDenModel
    config = syn.default_config()
    env = syn.SyntheticEnv(config)
    model = PropNetDiffDenModel(config, True)
    sd = {k[2:]: torch.from_numpy(golden.weights_seed0[k]) for k in golden.weights_seed0.files if k.startswith('w/')}
    model.load_state_dict(sd, strict=False)
    model.cuda().eval()
    yield env, model
    model.engine.close()


@pytest.mark.parametrize('mpc_type', ['GD', 'MPPI', 'CEM'])
def test_planner_multi_scene_returns_the_single_scene_dicts(stack, mpc_type):
    from dyn_res_pile_manip_amd.planners import PlannerGD
    env, model = stack
    N = 20
    config = copy.deepcopy(syn.default_config())
    config['mpc']['mpc_type'] = mpc_type
    config['mpc']['mppi']['reward_weight'] = 20.0
    planner = PlannerGD(config, env)
    piles = [syn.make_pile(N, NB, seed=7 + k) for k in range(S)]
    s0, dens, attr = (np.stack([p[q] for p in piles]) for q in range(3))
    images = goal_images()
    act_seq = np.stack([syn.sample_pushes(TRAJ, H, seed=20 + k).transpose(1, 0, 2) for k in range(S)])     # [S, H, TRAJ, 4]
    lo, hi = syn.action_limits()
    kw = dict(n_sample=TRAJ if mpc_type == 'GD' else NS, n_look_ahead=H, n_update_iter=3, action_lower_lim=lo,
              action_upper_lim=hi, use_gpu=True, time_lim=1e9)
    multi = planner.trajectory_optimization_ptcl_multi_scene(s0, dens, attr, images, model, act_seq, np.zeros(H), seeds=SEEDS, **kw)
    assert len(multi) == S
    for k in range(S):
        one = planner.trajectory_optimization_ptcl_multi_traj(s0[k], dens[k], attr[k], images[k], model, act_seq[k], np.zeros(H),
                                                              seed=SEEDS[k], **kw)
        assert set(multi[k].keys()) == set(one.keys())
        for key in one:
            if key == 'times':
                continue
            if one[key] is None:
                assert multi[k][key] is None, key
            else:
                np.testing.assert_array_equal(multi[k][key], one[key], err_msg='%s scene %d' % (key, k))
    assert not np.array_equal(multi[0]['action_sequence'], multi[1]['action_sequence'])
    # a second call re-uses the installed table
    again = planner.trajectory_optimization_ptcl_multi_scene(s0, dens, attr, images, model, act_seq, np.zeros(H), seeds=SEEDS, **kw)
    assert again[0]['times']['goal_cached'] and not multi[0]['times']['goal_cached']
    np.testing.assert_array_equal(again[2]['action_sequence'], multi[2]['action_sequence'])
    for bad in (dict(comm=(0, 1, None)), dict(wallclock_limit=True), dict(distractor_df_fn=lambda *a: None)):
        with pytest.raises(NotImplementedError):
            planner.trajectory_optimization_ptcl_multi_scene(s0, dens, attr, images, model, act_seq, np.zeros(H), seeds=SEEDS,
                                                             **dict(kw, **bad))


# ---- 6. S = 1 and isolation --------------------------------------------------------------------------------------
def test_one_scene_session_is_mpc_begin(eng, golden):
    N = 20
    goals, s0, attr, dens = prepare(eng, golden, N)
    lo, hi = syn.action_limits()
    eng.set_goal_scenes(goals[1][0][None], [goals[1][1]])
    eng.mpc_begin_scenes(s0[1:2], attr[1:2], dens[1:2], nominals()[1:2], NS, act_lo=lo, act_hi=hi, seeds=SEEDS[1:2], **MP)
    one = []
    for it in range(2):
        eng.mpc_sample(it)
        eng.mpc_rollout(False)
        eng.mpc_update_device()
        got = eng.mpc_get(actions=True, rewards=True, nominal=True)
        one.append((got['actions'], got['rewards'], got['nominal'][0], eng.mpc_stats(), eng.mpc_stats_scenes()))
    ref = run_single(eng, goals, s0, attr, dens, 1, UPDATES['softmax'], n_iter=2)
    for (a, r, nom, st, sts), (ra, rr, rnom, rst) in zip(one, ref):
        np.testing.assert_array_equal(a, ra)
        np.testing.assert_array_equal(r, rr)
        np.testing.assert_array_equal(nom, rnom)
        assert st == rst and sts == [rst]
    assert eng.mpc_stats_scenes() == [eng.mpc_stats()]              # the getter serves a single-scene session too


@pytest.mark.parametrize('N', [20, 65])
def test_a_scene_session_leaves_the_other_paths_their_bits(eng, golden, N):
    goals, s0, attr, dens = prepare(eng, golden, N)
    lo, hi = syn.action_limits()
    cand = gd_candidates()

    def others():
        mp = run_single(eng, goals, s0, attr, dens, 0, UPDATES['softmax'], n_iter=2)
        eng.gd_begin(s0[0], attr[0], dens[0], cand[0], 0.05, lo, hi)
        gd = eng.gd_grad()[:2]
        acts = syn.sample_pushes(NB, 1, seed=1)[:, 0]
        step = eng.step(attr[0], s0[0], eng.gen_s_delta(s0[0], acts), dens[0])
        return mp, gd, step

    before = others()
    run_multi(eng, s0, attr, dens, UPDATES['elite'], n_iter=2)
    eng.gd_begin_scenes(s0, attr, dens, interleave_scenes(cand, NB), 0.05, lo, hi)
    eng.gd_step()
    after = others()
    for (a, r, nom, st), (a2, r2, nom2, st2) in zip(before[0], after[0]):
        np.testing.assert_array_equal(a, a2)
        np.testing.assert_array_equal(r, r2)
        np.testing.assert_array_equal(nom, nom2)
        assert st == st2
    np.testing.assert_array_equal(before[1][0], after[1][0])
    np.testing.assert_array_equal(before[1][1], after[1][1])
    np.testing.assert_array_equal(before[2], after[2])

    # the rollout of a scene session is dispatched as the one of a plain session of S * nb columns
    acts = interleave_scenes(np.stack([np.repeat(syn.sample_pushes(NS, H, seed=k), NB, axis=0) for k in range(S)]), NB)
    eng.mpc_begin_scenes(s0, attr, dens, nominals(), NS, act_lo=lo, act_hi=hi, seeds=SEEDS, **MP)
    eng.mpc_set_actions(acts)
    for _ in range(8):              # (the plans read a degree statistic of the last lists of this shape, refreshed every eighth launch)
        eng.mpc_rollout(False)
    eng.dispatch_reset()
    eng.mpc_rollout(False)
    marks = eng.last_dispatch()
    states = eng.mpc_get(states=True)['states']
    single_goal(eng, goals, 0)
    eng.mpc_begin(s0.reshape(S * NB, N, 3), attr.reshape(S * NB, N), dens.reshape(S * NB), nominals()[0], NS, act_lo=lo, act_hi=hi, **MP)
    eng.mpc_set_actions(acts)
    eng.dispatch_reset()
    eng.mpc_rollout(False)
    assert eng.last_dispatch() == marks
    np.testing.assert_array_equal(eng.mpc_get(states=True)['states'], states)


# ---- 7. refusals -------------------------------------------------------------------------------------------------
def refused(eng, code_word, call):
    with pytest.raises(_lib.DrpError) as e:
        call()
    msg = str(e.value)
    assert code_word in msg, msg
    assert msg.split(': ', 1)[1].strip(), msg                    # drp_last_error says why
    return msg


def test_refusals_leave_the_context_usable(eng, golden):
    from dyn_res_pile_manip_amd.engine import Engine
    N = 20
    goals, s0, attr, dens = prepare(eng, golden, N)
    lo, hi = syn.action_limits()
    fields = np.stack([g[0] for g in goals])
    st = syn.make_pile(N, 3, seed=4)[0]
    good = eng.reward_scenes(st, [0, 1, 2])
    EINVAL, ESTATE = 'drp error -1', 'drp error -2'
    # S = 0 and S = 65, m[s] = 0 and m[s] > m_max: refused, and the installed table is the one it was
    h, w = fields.shape[1:]
    refused(eng, EINVAL, lambda: eng.set_goal_scenes(np.zeros((0, h, w), np.float32), np.zeros((0, 4, 2), np.float32), np.zeros(0, np.int32)))
    refused(eng, EINVAL, lambda: eng.set_goal_scenes(np.zeros((65, 8, 8), np.float32), np.zeros((65, 4, 2), np.float32), np.ones(65, np.int32)))
    refused(eng, EINVAL, lambda: eng.set_goal_image_scenes(np.zeros((0, h, w), np.float32), 5 * N))
    refused(eng, EINVAL, lambda: eng.set_goal_image_scenes(np.ones((65, 8, 8), np.float32), 5 * N))
    coor = np.zeros((S, 4, 2), np.float32)
    assert 'scene 1' in refused(eng, EINVAL, lambda: eng.set_goal_scenes(fields, coor, [4, 0, 4]))
    assert 'scene 2' in refused(eng, EINVAL, lambda: eng.set_goal_scenes(fields, coor, [4, 4, 5]))
    # an image without goal pixels in slot 1
    bad = eng.images.copy()
    bad[1] = 10.0
    assert 'scene 1' in refused(eng, EINVAL, lambda: eng.set_goal_image_scenes(bad, 5 * N))
    np.testing.assert_array_equal(eng.reward_scenes(st, [0, 1, 2]), good)
    # a scene index out of range
    refused(eng, EINVAL, lambda: eng.reward_scenes(st, [0, 3, 1]))
    refused(eng, EINVAL, lambda: eng.reward_scenes(st, [0, -1, 1]))
    # a table of S' != S scenes
    refused(eng, EINVAL, lambda: eng.mpc_begin_scenes(s0[:2], attr[:2], dens[:2], nominals()[:2], NS, act_lo=lo, act_hi=hi, seeds=SEEDS[:2], **MP))
    cand = gd_candidates()
    refused(eng, EINVAL, lambda: eng.gd_begin_scenes(s0[:2], attr[:2], dens[:2], interleave_scenes(cand[:2], NB), 0.05, lo, hi))
    # B no multiple of S * nb
    refused(eng, EINVAL, lambda: eng.gd_begin_scenes(s0, attr, dens, interleave_scenes(cand, NB)[:-NB], 0.05, lo, hi))
    # the host-transport forms in a session of S > 1 scenes
    eng.mpc_begin_scenes(s0, attr, dens, nominals(), NS, act_lo=lo, act_hi=hi, seeds=SEEDS, **MP)
    eng.mpc_sample(0)
    eng.mpc_rollout(False)
    refused(eng, ESTATE, lambda: eng.mpc_partials())
    refused(eng, ESTATE, lambda: eng.mpc_update(np.zeros((1, 6 + 4 * H))))
    refused(eng, ESTATE, lambda: eng.mpc_elite(5))
    refused(eng, ESTATE, lambda: eng.mpc_update_elite(np.zeros((1, 5, 2 + 4 * H)), 5))
    eng.mpc_update_device()                                      # the session itself goes on
    assert np.isfinite(eng.mpc_get(nominal=True)['nominal']).all()
    np.testing.assert_array_equal(eng.reward_scenes(st, [0, 1, 2]), good)
    # a context without a table
    e2 = Engine(0)
    try:
        e2.load_weights(weights.blob_from_state_dict(golden.weights_seed0), 0.08)
        e2.set_camera(world2cam_affine(syn.demo_cam_extrinsics()), 24.0, syn.demo_cam_params())
        e2.set_goal(*goals[0])
        refused(e2, ESTATE, lambda: e2.reward_scenes(st, [0, 0, 0]))
        refused(e2, ESTATE, lambda: e2.mpc_begin_scenes(s0, attr, dens, nominals(), NS, act_lo=lo, act_hi=hi, seeds=SEEDS, **MP))
        refused(e2, ESTATE, lambda: e2.gd_begin_scenes(s0, attr, dens, interleave_scenes(cand, NB), 0.05, lo, hi))
        assert np.isfinite(e2.reward(st)).all()
    finally:
        e2.close()

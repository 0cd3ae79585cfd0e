"""GPU: the sampling planners on a cost of the caller's -- drp_mpc_begin_cost, drp_mpc_set_rewards.

A goal session and a cost session with the same parameters and Philox key, 64 samples x 20 particles x H = 3 (nb = 1): the
draws and the states are held to bits, and with the goal session's rewards handed to the cost session the softmax and the
elite updates are held to bits too (nominal doubles and statistics) -- the update kernels are the same launches on the same
slot."""
import numpy as np
import pytest

from dyn_res_pile_manip_amd import synthetic as syn, weights
from dyn_res_pile_manip_amd._lib import DrpError
from dyn_res_pile_manip_amd.engine import Engine
from dyn_res_pile_manip_amd.planners import world2cam_affine

pytestmark = pytest.mark.gpu
M34 = world2cam_affine(syn.demo_cam_extrinsics())
CAM = syn.demo_cam_params()
LO, HI = syn.action_limits()
NS, N, H = 64, 20, 3


@pytest.fixture(scope='module')
def pair(golden):
    """(a context with a goal, one that never sees one), and the problem"""
    s0, dens, attr = syn.make_pile(N, 1, seed=4)
    G = syn.goal_field(syn.goal_distance_image(syn.goal_mask('I')))
    coor = syn.goal_coor_strided(syn.goal_distance_image(syn.goal_mask('I')), 5 * N)
    es = []
    for goal in (True, False):
        e = Engine(0)
        e.load_weights(weights.blob_from_state_dict(golden.weights_seed0), 0.08)
        e.set_camera(M34, 24.0, CAM)
        if goal:
            e.set_goal(G, coor)
        es.append(e)
    yield es[0], es[1], (s0, attr, dens)
    for e in es:
        e.close()


def begin(e, prob, cost):
    nominal = syn.nominal_pushes(H, 0).astype(np.float64)
    (e.mpc_begin_cost if cost else e.mpc_begin)(*prob, nominal, NS, 0.6, 0.7, 10.0, LO, HI, seed=1234)


def iteration(g, c, it):
    """sample and roll out in both; the cost session gets the goal session's rewards -> (them, the states)"""
    for e in (g, c):
        e.mpc_sample(it)
        e.mpc_rollout()
    a, b = g.mpc_get(actions=True, rewards=True, states=True), c.mpc_get(actions=True, states=True)
    assert a['actions'].tobytes() == b['actions'].tobytes() and a['states'].tobytes() == b['states'].tobytes()
    c.mpc_set_rewards(a['rewards'])
    assert c.mpc_get(rewards=True)['rewards'].tobytes() == a['rewards'].tobytes()
    return a['rewards'], a['states']


def same_update(g, c):
    assert g.mpc_get(nominal=True)['nominal'].tobytes() == c.mpc_get(nominal=True)['nominal'].tobytes()
    bits = lambda e: np.array([[float(v) for v in d.values()] for d in e.mpc_stats_scenes()]).tobytes()
    assert bits(g) == bits(c)


def test_softmax_update_on_handed_in_rewards_keeps_its_bits(pair):
    g, c, prob = pair
    begin(g, prob, False)
    begin(c, prob, True)
    for it in range(2):
        iteration(g, c, it)
        g.mpc_update_device()
        c.mpc_update_device()
        same_update(g, c)
    assert not np.array_equal(g.mpc_get(nominal=True)['nominal'], syn.nominal_pushes(H, 0))


@pytest.mark.parametrize('k', [1, 8])
def test_elite_update_on_handed_in_rewards_keeps_its_bits(pair, k):
    g, c, prob = pair
    begin(g, prob, False)
    begin(c, prob, True)
    for it in range(2):
        iteration(g, c, it)
        g.mpc_update_elite_device(k)
        c.mpc_update_elite_device(k)
        same_update(g, c)


def test_nothing_reads_the_rewards_before_they_are_in(pair):
    g, c, prob = pair
    begin(c, prob, True)
    c.mpc_sample(0)
    c.mpc_rollout()
    nominal = c.mpc_get(nominal=True)['nominal']
    rec = np.zeros((1, 6 + 4 * H))
    for call in (c.mpc_update_device, lambda: c.mpc_update_elite_device(4), c.mpc_partials, lambda: c.mpc_update(rec),
                 lambda: c.mpc_elite(4), lambda: c.mpc_update_elite(np.zeros((1, 4, 2 + 4 * H)), 4), lambda: c.mpc_fetch_async(0)):
        with pytest.raises(DrpError, match=r'drp error -2: .*drp_mpc_begin_cost.*drp_mpc_set_rewards'):
            call()
    assert c.mpc_get(nominal=True)['nominal'].tobytes() == nominal.tobytes()
    with pytest.raises(DrpError, match=r'drp error -1: .*reward_all_steps'):
        c.mpc_rollout(reward_all_steps=True)
    assert c.lib.drp_mpc_set_rewards(c.h, None) == -1
    with pytest.raises(ValueError):
        c.mpc_set_rewards(np.zeros(NS + 1, np.float32))
    # NaN rewards are the update kernels' to handle; the next rollout wants rewards again
    r = np.zeros(NS, np.float32)
    r[5] = np.nan
    c.mpc_set_rewards(r)
    c.mpc_update_device()
    c.mpc_sample(1)
    c.mpc_rollout()
    with pytest.raises(DrpError, match='drp_mpc_set_rewards'):
        c.mpc_update_device()


def test_set_rewards_replaces_a_goal_sessions_rewards(pair):
    g, c, prob = pair
    begin(g, prob, False)
    begin(c, prob, True)
    rewards, _ = iteration(g, c, 0)
    mine = -np.arange(NS, dtype=np.float32) / NS
    g.mpc_set_rewards(mine)
    c.mpc_set_rewards(mine)
    assert g.mpc_get(rewards=True)['rewards'].tobytes() == mine.tobytes()
    g.mpc_update_device()
    c.mpc_update_device()
    same_update(g, c)
    assert g.mpc_stats_scenes()[0]['argmax'] == 0            # the best sample is now the first


def test_a_goal_session_cannot_begin_without_a_goal_but_a_cost_session_can(pair):
    g, c, prob = pair
    with pytest.raises(DrpError, match='goal not set'):
        begin(c, prob, False)
    begin(c, prob, True)

"""What planning on a caller's cost costs (Engine.gd_predict, gd_step_seeded, mpc_set_rewards) beside the built-in iterations.

  python tools/cost_timing.py [iterations per block [blocks]]        -> stdout (kept as profiles/cost_timing.txt)

On ONE context, in interleaved blocks (every call below is complete on the device when it returns, so a host clock around a
block of calls is the device's time plus the host's), the median of the blocks with their spread.

GD, 1 500 rows x {20, 50, 100} particles, H in {1, 3}, per iteration:

  gd_step      the built-in iteration (reward on the device), the rewards fetched
  seeded       gd_step_seeded alone, the seed computed once beforehand: one upload of the seed and kb_seed_stage in kb_reward's place
  predict      gd_predict alone: the forward with tape and the states' download
  composed     gd_predict -> costs.quadratic_cost on the host -> gd_step_seeded: what a Python cost pays, transfers included

MPPI, 1 024 samples x 300 particles x H = 10, per iteration:

  built-in     mpc_sample -> mpc_rollout (reward on the device) -> mpc_update_device -> mpc_get(actions, rewards)
  cost         mpc_sample -> mpc_rollout (no reward) -> mpc_get(actions, states) -> a numpy reward -> mpc_set_rewards ->
               mpc_update_device

  python tools/cost_timing.py --built-in-only [iterations [blocks]]   gd_step and the built-in MPPI iteration alone.  Run from
                                                                      the root of another checkout (the package is imported
                                                                      from the working directory) it times that checkout's
                                                                      build, whatever entry points it has: an interleaved A/B
                                                                      of two commits"""
import sys
import time

sys.path.insert(0, '.')
import numpy as np

from dyn_res_pile_manip_amd import synthetic as syn, weights
from dyn_res_pile_manip_amd.engine import Engine
from dyn_res_pile_manip_amd.planners import world2cam_affine

BUILT_IN_ONLY = '--built-in-only' in sys.argv
if not BUILT_IN_ONLY:
    from dyn_res_pile_manip_amd import costs
argv = [a for a in sys.argv[1:] if a != '--built-in-only']
ITERS = int(argv[0]) if len(argv) > 0 else 10
BLOCKS = int(argv[1]) if len(argv) > 1 else 7
LO, HI = syn.action_limits()

eng = Engine(0)
eng.load_weights(weights.blob_from_state_dict(weights.random_state_dict(0)), 0.08)
eng.set_camera(world2cam_affine(syn.demo_cam_extrinsics()), 24.0, syn.demo_cam_params())
obs_goal = syn.goal_distance_image(syn.goal_mask('I'))
G = syn.goal_field(obs_goal)


def blocks(calls, head):
    for k in calls:                                                 # warm-up: every shape and path once, then again
        calls[k](), calls[k]()
    took = dict((k, []) for k in calls)
    for rep in range(BLOCKS):                                       # interleaved blocks; the median of each
        for k in calls:
            eng.sync()
            t0 = time.perf_counter()
            for _ in range(ITERS):
                calls[k]()
            eng.sync()
            took[k].append((time.perf_counter() - t0) / ITERS * 1e3)
    med = dict((k, float(np.median(v))) for k, v in took.items())
    for k in calls:
        print('%s %-9s %.3f ms (blocks %.3f .. %.3f)' % (head, k, med[k], min(took[k]), max(took[k])), flush=True)
    return med


ROWS = 1500
for N in (20, 50, 100):
    for H in (1, 3):
        s0, dens, attr = syn.make_pile(N, 1, seed=N)
        acts = syn.sample_pushes(ROWS, H, seed=N)
        eng.set_goal(G, syn.goal_coor_strided(obs_goal, 5 * N))
        # lr 0: the pushes stay where they are, every block times the same problem
        eng.gd_begin(s0, attr, dens, acts, 0.0, LO, HI)
        calls = {'gd_step': eng.gd_step}
        if not BUILT_IN_ONLY:
            targets = np.stack([s0[0] + 0.01 * (t + 1) for t in range(H)]).astype(np.float32)
            cost = costs.quadratic_cost(targets)
            seed = cost(eng.gd_predict(), None, True)[1]
            calls['seeded'] = lambda: eng.gd_step_seeded(seed)
            calls['predict'] = eng.gd_predict
            calls['composed'] = lambda: eng.gd_step_seeded(cost(eng.gd_predict(), None, True)[1])
            t0 = time.perf_counter()
            pred = eng.gd_predict()
            for _ in range(20):
                cost(pred, None, True)
            host_cost = (time.perf_counter() - t0) / 20 * 1e3
        head = 'GD rows=%d N=%d H=%d:' % (ROWS, N, H)
        med = blocks(calls, head)
        if not BUILT_IN_ONLY:
            print('%s seeded / gd_step %.3f, composed / gd_step %.3f, (predict + seeded) / gd_step %.3f; quadratic_cost on the host %.3f ms'
                  % (head, med['seeded'] / med['gd_step'], med['composed'] / med['gd_step'],
                     (med['predict'] + med['seeded']) / med['gd_step'], host_cost), flush=True)

NS, N, H = 1024, 300, 10
s0, dens, attr = syn.make_pile(N, 1, seed=3)
nominal = syn.nominal_pushes(H, 0).astype(np.float64)
eng.set_goal(G, syn.goal_coor_strided(obs_goal, 5 * N))
mp = dict(n_sample=NS, sigma=0.6, beta_filter=0.7, reward_weight=10.0, act_lo=LO, act_hi=HI, seed=11)
it = [0]


def built_in():
    if sess[0] != 'goal':
        eng.mpc_begin(s0, attr, dens, nominal, **mp)
        sess[0] = 'goal'
    it[0] += 1
    eng.mpc_sample(it[0])
    eng.mpc_rollout(False)
    eng.mpc_update_device()
    eng.mpc_get(actions=True, rewards=True)


def on_a_cost():
    if sess[0] != 'cost':
        eng.mpc_begin_cost(s0, attr, dens, nominal, **mp)
        sess[0] = 'cost'
    it[0] += 1
    eng.mpc_sample(it[0])
    eng.mpc_rollout(False)
    got = eng.mpc_get(actions=True, states=True)
    d = got['states'][:, -1] - target
    eng.mpc_set_rewards(-(d * d).sum((1, 2)) / N)
    eng.mpc_update_device()


sess = [None]
target = (s0[0] + 0.02).astype(np.float32)[None]
calls = {'built-in': built_in}
if not BUILT_IN_ONLY:
    calls['cost'] = on_a_cost
head = 'MPPI samples=%d N=%d H=%d:' % (NS, N, H)
med = blocks(calls, head)
if not BUILT_IN_ONLY:
    print('%s cost / built-in %.3f (the states\' download: %.1f MB per iteration)'
          % (head, med['cost'] / med['built-in'], NS * H * N * 3 * 4 / 1e6), flush=True)
eng.close()

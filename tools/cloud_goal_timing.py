"""What planning to a device-resident cloud goal costs (Engine.set_goal_cloud, mpc_begin_cloud, gd_begin_cloud) beside the
built-in image goal and beside the same cost through the caller's-cost seam.

  python tools/cloud_goal_timing.py [iterations per block [blocks]]        -> stdout (kept in profiles/cloud_goal_timing.txt)

On ONE context, in interleaved blocks (every call below is complete on the device when it returns, so a host clock around a
block of calls is the device's time plus the host's), the median of the blocks with their spread.  The target has as many
points as the pile.

MPPI, 1 024 samples x {20, 100, 300} particles x H = 10, per iteration (mpc_sample -> mpc_rollout -> mpc_update_device ->
mpc_get(actions, rewards)):

  image        the built-in image goal
  chamfer      the cloud session, Chamfer
  sinkhorn     the cloud session, Sinkhorn divergence at iters 50
  host-ch      the seam: rollout without reward -> mpc_get(actions, states) -> costs.cloud_chamfer_cost -> mpc_set_rewards -> update
  host-sk      the same with costs.cloud_divergence_cost at iters 50: what a user had before

GD, 1 500 rows x {20, 100} particles x H = 3, per iteration: gd_step (image, chamfer, sinkhorn) against gd_predict -> the cost
on the host -> gd_step_seeded (host-ch, host-sk).

Behind each shape: the reward kernels' device time alone (the 'reward' / 'bwd_reward' probe classes: events around the launches)
and the once-per-session target self problem (the 'loss' class around the session's begin).

  DRP_LIB=<another build's libdrp.so> python tools/cloud_goal_timing.py --built-in-only [iterations [blocks]]
       the image-goal iterations alone, on a library that need not have the cloud entry points (the parent commit's build):
       an interleaved A/B of two builds is this line and the same line without DRP_LIB run in turns.  Run from the root of
       another checkout (the package is imported from the working directory) it times that checkout with its own binding"""
import sys
import time

sys.path.insert(0, '.')
import numpy as np

from dyn_res_pile_manip_amd import _lib as L

BUILT_IN_ONLY = '--built-in-only' in sys.argv
if BUILT_IN_ONLY:
    for name in ('drp_set_goal_cloud', 'drp_mpc_begin_cloud', 'drp_gd_begin_cloud', 'drp_cloud_goal_eval'):
        L.SIGNATURES.pop(name, None)            # the other build may not export them, and nothing below calls them

from dyn_res_pile_manip_amd import costs, synthetic as syn, weights
from dyn_res_pile_manip_amd.engine import Engine
from dyn_res_pile_manip_amd.planners import world2cam_affine

argv = [a for a in sys.argv[1:] if a != '--built-in-only']
ITERS = int(argv[0]) if len(argv) > 0 else 5
BLOCKS = int(argv[1]) if len(argv) > 1 else 5
SWEEPS = 50
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
        print('%s %-9s %8.3f ms (blocks %.3f .. %.3f)' % (head, k, med[k], min(took[k]), max(took[k])), flush=True)
    return med


def probed(cls, call, n=3):
    """device time of the class's launches inside one call: the median of n"""
    out = []
    for _ in range(n):
        eng.probe_begin(cls)
        call()
        out.append(eng.probe_read()[0])
    eng.probe_begin(None)
    return float(np.median(out))


def target_of(s0):
    return (s0[0] + np.array([0.02, -0.01, 0.0], np.float32)).astype(np.float32)


def ratios(head, med):
    if BUILT_IN_ONLY:
        return
    print('%s chamfer / image %.3f, sinkhorn / image %.3f, host-ch / chamfer %.3f, host-sk / sinkhorn %.3f'
          % (head, med['chamfer'] / med['image'], med['sinkhorn'] / med['image'], med['host-ch'] / med['chamfer'],
             med['host-sk'] / med['sinkhorn']), flush=True)
    for kind, host in (('chamfer', 'host-ch'), ('sinkhorn', 'host-sk')):
        if not med[kind] < med[host]:
            print('%s NOTE: the %s session is NOT faster than the host path' % (head, kind), flush=True)


# ---- MPPI ----------------------------------------------------------------------------------------------------------------------
NS, H = 1024, 10
for N in (20, 100, 300):
    s0, dens, attr = syn.make_pile(N, 1, seed=3)
    target = target_of(s0)
    nominal = syn.nominal_pushes(H, 0).astype(np.float64)
    eng.set_goal(G, syn.goal_coor_strided(obs_goal, 5 * N))
    mp = dict(n_sample=NS, sigma=0.6, beta_filter=0.7, reward_weight=10.0, act_lo=LO, act_hi=HI, seed=11)
    sess, it = [None], [0]
    ctx = {'dens': dens}
    twins = {} if BUILT_IN_ONLY else {'host-ch': costs.cloud_chamfer_cost(eng, target),
                                      'host-sk': costs.cloud_divergence_cost(eng, target, eps_scale=1.0, iters=SWEEPS)}

    def on_device(name):
        def run():
            if sess[0] != name:
                if name == 'image':
                    eng.mpc_begin(s0, attr, dens, nominal, **mp)
                else:
                    eng.set_goal_cloud(target, kind=name, iters=SWEEPS)
                    eng.mpc_begin_cloud(s0, attr, dens, nominal, **mp)
                sess[0] = name
            it[0] += 1
            eng.mpc_sample(it[0])
            eng.mpc_rollout(False)
            eng.mpc_update_device()
            eng.mpc_get(actions=True, rewards=True)
        return run

    def on_host(name):
        def run():
            if sess[0] != 'cost':
                eng.mpc_begin_cost(s0, attr, dens, nominal, **mp)
                sess[0] = 'cost'
            it[0] += 1
            eng.mpc_sample(it[0])
            eng.mpc_rollout(False)
            got = eng.mpc_get(actions=True, states=True)
            values, _ = twins[name](got['states'], ctx, False)
            eng.mpc_set_rewards(-np.asarray(values, np.float32))
            eng.mpc_update_device()
        return run

    calls = {'image': on_device('image')}
    if not BUILT_IN_ONLY:
        calls.update({'chamfer': on_device('chamfer'), 'sinkhorn': on_device('sinkhorn'), 'host-ch': on_host('host-ch'),
                      'host-sk': on_host('host-sk')})
    head = 'MPPI samples=%d N=%d H=%d:' % (NS, N, H)
    med = blocks(calls, head)
    ratios(head, med)
    if not BUILT_IN_ONLY:
        for kind in ('image', 'chamfer', 'sinkhorn'):
            calls[kind]()
            print('%s %-9s reward kernels alone %.3f ms' % (head, kind, probed('reward', lambda: eng.mpc_rollout(False))), flush=True)

        def begin_sinkhorn():
            eng.mpc_begin_cloud(s0, attr, dens, nominal, **mp)
        print('%s sinkhorn  target self problem, once per session %.3f ms' % (head, probed('loss', begin_sinkhorn)), flush=True)

# ---- GD --------------------------------------------------------------------------------------------------------------------------
ROWS, H = 1500, 3
for N in (20, 100):
    s0, dens, attr = syn.make_pile(N, 1, seed=N)
    target = target_of(s0)
    acts = syn.sample_pushes(ROWS, H, seed=N)
    eng.set_goal(G, syn.goal_coor_strided(obs_goal, 5 * N))
    sess = [None]
    ctx = {'dens': dens}
    twins = {} if BUILT_IN_ONLY else {'host-ch': costs.cloud_chamfer_cost(eng, target),
                                      'host-sk': costs.cloud_divergence_cost(eng, target, eps_scale=1.0, iters=SWEEPS)}

    def on_device(name):
        def run():
            if sess[0] != name:
                # lr 0: the pushes stay where they are, every block times the same problem
                if name == 'image':
                    eng.gd_begin(s0, attr, dens, acts, 0.0, LO, HI)
                else:
                    eng.set_goal_cloud(target, kind=name, iters=SWEEPS)
                    eng.gd_begin_cloud(s0, attr, dens, acts, 0.0, LO, HI)
                sess[0] = name
            eng.gd_step()
        return run

    def on_host(name):
        def run():
            if sess[0] != 'cost':
                eng.gd_begin_cost(s0, attr, dens, acts, 0.0, LO, HI)
                sess[0] = 'cost'
            eng.gd_step_seeded(twins[name](eng.gd_predict(), ctx, True)[1])
        return run

    calls = {'image': on_device('image')}
    if not BUILT_IN_ONLY:
        calls.update({'chamfer': on_device('chamfer'), 'sinkhorn': on_device('sinkhorn'), 'host-ch': on_host('host-ch'),
                      'host-sk': on_host('host-sk')})
    head = 'GD rows=%d N=%d H=%d:' % (ROWS, N, H)
    med = blocks(calls, head)
    ratios(head, med)
    if not BUILT_IN_ONLY:
        for kind in ('image', 'chamfer', 'sinkhorn'):
            calls[kind]()
            print('%s %-9s reward kernels alone %.3f ms' % (head, kind, probed('bwd_reward', eng.gd_step)), flush=True)

        def begin_sinkhorn():
            eng.gd_begin_cloud(s0, attr, dens, acts, 0.0, LO, HI)
        print('%s sinkhorn  target self problem, once per session %.3f ms' % (head, probed('loss', begin_sinkhorn)), flush=True)
eng.close()

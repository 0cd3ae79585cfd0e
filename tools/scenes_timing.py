"""One S-scene session against S single-scene iterations run back to back (include/drp.h: drp_mpc_begin_scenes,
drp_gd_begin_scenes), on ONE context, interleaved, the order alternating from round to round:

  MPPI  1024 samples per scene x {20, 50, 100, 300} particles x 10 steps, nb = 1: sample, rollout, final reward, device update
  GD    1500 rows per scene x the same particle counts, horizon 1 (the demo shape): forward with tape, reward + backward, Adam

for S in {1, 2, 4, 8}.  The baseline is the existing single-scene API on the same build and box: a window of S x ITERS
iterations of one single-scene session, against ITERS iterations of the S-scene session -- the same number of scene-iterations
in both windows, each ended by one device synchronise.  The baseline window leaves out what a real queue of scenes pays on top
(a session begin and a goal install per scene), so it is the queue at its best.  Before the timing, scene 0 of the S-scene
session is checked to be bit-equal to its single-scene session at the timed size.  Run it on one box and keep the output:

    python tools/scenes_timing.py | tee profiles/scenes_timing.txt
"""
import sys
import time

sys.path.insert(0, '.')
import numpy as np

from dyn_res_pile_manip_amd import synthetic as syn, weights
from dyn_res_pile_manip_amd.engine import Engine, interleave_scenes, split_scenes
from dyn_res_pile_manip_amd.planners import world2cam_affine

NS, H, ROWS, ROUNDS, WARM = 1024, 10, 1500, 6, 3
SCENES = (1, 2, 4, 8)
SIZES = (20, 50, 100, 300)
ITERS = {20: 40, 50: 40, 100: 20, 300: 10}
MP = dict(sigma=0.3 * 24 / 12.0, beta_filter=0.7, reward_weight=0.1)


def problem(eng, images, S, N):
    """S piles and the goal table of S goals (the two synthetic goals in turn); scene 0's goal as the single goal"""
    piles = [syn.make_pile(N, 1, seed=k) for k in range(S)]
    s0, dens, attr = (np.stack([p[q] for p in piles]) for q in range(3))
    eng.set_goal_image_scenes(np.stack([images[k % 2] for k in range(S)]), 5 * N)
    eng.set_goal_image(images[0], 5 * N)
    return s0, attr, dens


def mppi_begin(eng, prob, S):
    s0, attr, dens = prob
    lo, hi = syn.action_limits()
    if S == 0:
        eng.mpc_begin(s0[0], attr[0], dens[0], syn.nominal_pushes(H, seed=0), NS, act_lo=lo, act_hi=hi, seed=100, **MP)
    else:
        eng.mpc_begin_scenes(s0, attr, dens, np.stack([syn.nominal_pushes(H, seed=k) for k in range(S)]), NS, act_lo=lo, act_hi=hi,
                             seeds=[100 + k for k in range(S)], **MP)


def mppi_iter(eng, it):
    eng.mpc_sample(it)
    eng.mpc_rollout(False)
    eng.mpc_update_device()


def gd_begin(eng, prob, S):
    s0, attr, dens = prob
    lo, hi = syn.action_limits()
    if S == 0:
        eng.gd_begin(s0[0], attr[0], dens[0], syn.sample_pushes(ROWS, 1, seed=0), 0.05, lo, hi)
    else:
        eng.gd_begin_scenes(s0, attr, dens, interleave_scenes(np.stack([syn.sample_pushes(ROWS, 1, seed=k) for k in range(S)]), 1),
                            0.05, lo, hi)


def window(eng, step, n):
    t0 = time.perf_counter()
    for it in range(n):
        step(it)
    eng.sync()
    return (time.perf_counter() - t0) * 1e3


def same_bits(eng, prob, S):
    mppi_begin(eng, prob, S)
    mppi_iter(eng, 0)
    multi = eng.mpc_get(rewards=True, nominal=True)
    mppi_begin(eng, prob, 0)
    mppi_iter(eng, 0)
    one = eng.mpc_get(rewards=True, nominal=True)
    return (np.array_equal(split_scenes(multi['rewards'], S, 1)[0], one['rewards']) and
            np.array_equal(multi['nominal'][0], one['nominal']))


def measure(eng, prob, S, N, begin, step):
    """-> (ms per scene-iteration as S single sessions, as one session), medians over the rounds, and both lists"""
    n = ITERS[N]
    ms = {'queue': [], 'session': []}
    for mode in ('queue', 'session'):
        begin(eng, prob, 0 if mode == 'queue' else S)
        window(eng, step, WARM)
    for r in range(ROUNDS):
        for mode in (('queue', 'session') if r % 2 == 0 else ('session', 'queue')):
            begin(eng, prob, 0 if mode == 'queue' else S)
            window(eng, step, 1)
            ms[mode].append(window(eng, step, n * S if mode == 'queue' else n) / (n * S))
    return ms


def main():
    eng = Engine(0)
    eng.set_camera(world2cam_affine(syn.demo_cam_extrinsics()), 24.0, syn.demo_cam_params())
    print('device', eng.device_info())
    eng.load_weights(weights.blob_from_state_dict(weights.random_state_dict(seed=0)), 0.08)
    images = [syn.goal_distance_image(syn.goal_mask(k)) for k in ('I', 'disc')]
    print('ms per scene-iteration (window / (iterations x S)); queue = S single-scene iterations back to back, session = one '
          'S-scene iteration; median [min .. max] over %d interleaved rounds' % ROUNDS)
    def gd_iter(it):
        eng._ck(eng.lib.drp_gd_step(eng.h, None))          # enqueued: no host wait inside the window

    for name, begin, step in (('MPPI %d samples per scene x H %d' % (NS, H), mppi_begin, lambda it: mppi_iter(eng, it)),
                              ('GD %d rows per scene x H 1' % ROWS, gd_begin, gd_iter)):
        print(name)
        for N in SIZES:
            for S in SCENES:
                prob = problem(eng, images, S, N)
                bits = same_bits(eng, prob, S) if begin is mppi_begin else None
                ms = measure(eng, prob, S, N, begin, step)
                q, s = np.median(ms['queue']), np.median(ms['session'])
                print('  N %3d  S %d  queue %.4f [%.4f .. %.4f]  session %.4f [%.4f .. %.4f]  session / queue %.3f%s'
                      % (N, S, q, min(ms['queue']), max(ms['queue']), s, min(ms['session']), max(ms['session']), s / q,
                         '' if bits is None else ('  scene 0 bit-equal' if bits else '  SCENE 0 DIFFERS')))
    eng.close()


if __name__ == '__main__':
    main()

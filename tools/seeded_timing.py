"""What training on a caller's loss costs (Engine.train_predict, train_step_seeded, train_step_custom) beside the built-in update.

  python tools/seeded_timing.py [iterations per block [blocks]]        -> stdout (kept as profiles/seeded_timing.txt)

At 4 x 5 x 100 and 4 x 5 x 300 (batch x n_rollout x particles, the reference's training shape), with data impulses and with
pushes, on ONE context, in interleaved blocks (every call is complete on the device when it returns -- the trainer's one wait --
so a host clock around a block of calls is the device's time plus the host's):

  update      train_step / train_step_actions(mode='update'): the built-in MSE step
  predict     train_predict alone
  seeded      train_step_seeded(mode='update') alone, the seed computed once beforehand
  custom      train_step_custom(losses.mse_loss, mode='update'): predict + the host loss + seeded

The median of the blocks with their spread; `seeded / update` is what the seam itself costs (one upload of the seed, kt_seed_given
in kt_mse_grad's place), `custom / update` the whole price of a Python loss (one forward more, and the loss on the host).

  python tools/seeded_timing.py --update-only [iterations [blocks]]    the built-in update alone.  Run from the root of another
                                                                       checkout (the package is imported from the working
                                                                       directory) it times that checkout's build, whatever
                                                                       entry points it has: an interleaved A/B of two commits"""
import sys
import time

sys.path.insert(0, '.')
import numpy as np

from dyn_res_pile_manip_amd import synthetic as syn, weights
from dyn_res_pile_manip_amd.engine import Engine
from dyn_res_pile_manip_amd.planners import world2cam_affine

UPDATE_ONLY = '--update-only' in sys.argv
if not UPDATE_ONLY:
    from dyn_res_pile_manip_amd import losses
argv = [a for a in sys.argv[1:] if a != '--update-only']
ITERS = int(argv[0]) if len(argv) > 0 else 40
BLOCKS = int(argv[1]) if len(argv) > 1 else 7
H = 5

eng = Engine(0)
eng.load_weights(weights.blob_from_state_dict(weights.random_state_dict(0)), 0.08)
eng.set_camera(world2cam_affine(syn.demo_cam_extrinsics()), 24.0, syn.demo_cam_params())


def make_batch(nums, rng):
    B, N = len(nums), max(nums)
    states = np.zeros((B, H + 1, N, 3), np.float32)
    sdelta = np.zeros((B, H, N, 3), np.float32)
    actions = np.zeros((B, H, 4), np.float32)
    dens = np.zeros((B,), np.float32)
    for b, n in enumerate(nums):
        s, d, _ = syn.make_pile(n, 1, seed=b)
        dens[b] = d[0]
        for t in range(H + 1):
            states[b, t, :n] = s[0] + 0.003 * t * rng.standard_normal((n, 3)).astype(np.float32)
        sdelta[b, :, :n] = 0.004 * rng.standard_normal((H, n, 3)).astype(np.float32)
        for t in range(H):
            actions[b, t] = syn.pushes_through(states[b, t, :n][None], seed=b * 10 + t)[0]
    return states, sdelta, actions, np.zeros((B, H + 1, N), np.float32), np.asarray(nums, np.int32), dens


for nums in ([100, 80, 50, 90], [300, 240, 150, 280]):
    states, sdelta, actions, attrs, pn, dens = make_batch(nums, np.random.default_rng(0))
    eng.train_begin(H, 1e-5, 0.9)
    for by_actions in (False, True):
        kw = {'actions': actions} if by_actions else {'states_delta': sdelta}
        context = [states, sdelta, attrs, pn, dens]
        if by_actions:
            def update():
                eng.train_step_actions(states, actions, attrs, pn, dens, mode='update')
        else:
            def update():
                eng.train_step(states, sdelta, attrs, pn, dens, mode='update')
        calls = {'update': update}
        if not UPDATE_ONLY:
            seed = losses.mse_loss(eng.train_predict(states, attrs, pn, dens, **kw), context)[1]
            calls['predict'] = lambda: eng.train_predict(states, attrs, pn, dens, **kw)
            calls['seeded'] = lambda: eng.train_step_seeded(states, attrs, pn, dens, seed, mode='update', **kw)
            calls['custom'] = lambda: eng.train_step_custom(losses.mse_loss, states, attrs, pn, dens, mode='update', context=context, **kw)
            t0 = time.perf_counter()
            for _ in range(200):
                losses.mse_loss(states[:, 1:], context)
            host_loss = (time.perf_counter() - t0) / 200 * 1e3
        for k in calls:                                             # warm-up: every shape and path once, then again
            calls[k](), calls[k]()
        took = dict((k, []) for k in calls)
        for rep in range(BLOCKS):                                   # interleaved blocks; the median of each
            for k in calls:
                eng.sync()
                t0 = time.perf_counter()
                for _ in range(ITERS):
                    calls[k]()
                eng.sync()
                took[k].append((time.perf_counter() - t0) / ITERS * 1e3)
        med = dict((k, float(np.median(v))) for k, v in took.items())
        head = 'B=4 n_rollout=%d N=%d impulses=%s:' % (H, max(nums), 'actions' if by_actions else 'data')
        for k in calls:
            print('%s %-8s %.3f ms (blocks %.3f .. %.3f)' % (head, k, med[k], min(took[k]), max(took[k])), flush=True)
        if not UPDATE_ONLY:
            print('%s seeded / update %.3f, custom / update %.3f, (predict + seeded) / update %.3f; mse_loss on the host %.3f ms'
                  % (head, med['seeded'] / med['update'], med['custom'] / med['update'],
                     (med['predict'] + med['seeded']) / med['update'], host_loss), flush=True)
eng.close()

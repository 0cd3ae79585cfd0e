"""Time one training iteration (train/train_gnn_dyn.py:159-210; batch_size 4, n_rollout 5 as
config/train/gnn_dyn.yaml) on the device, next to the dense torch-autograd oracle on the host.

  python tools/train_timing.py [shape index [iterations]]
  python tools/train_timing.py --loss chamfer    a Chamfer update (train_step_untracked) against an MSE update of the same shape,
                                                 interleaved on one context: B = 4 and 32, N = M = 300, n_rollout = 5
  python tools/train_timing.py --impulses actions [iterations]
                                                 an update through the push (train_step_actions: random pushes that cross the
                                                 pile) against an update on data impulses, interleaved on one context, at the
                                                 reference's batch (4 x <= 300 particles, n_rollout = 5); `--impulses data` is
                                                 the default run"""
import sys
import time

sys.path.insert(0, '.')
import numpy as np

from dyn_res_pile_manip_amd import synthetic as syn, weights
from dyn_res_pile_manip_amd.engine import Engine
from oracle import propnet_dense as od

eng = Engine(0)
sd = weights.random_state_dict(0)
eng.load_weights(weights.blob_from_state_dict(sd), 0.08)
W = {k: np.asarray(v) for k, v in sd.items()}
rng = np.random.default_rng(0)
SHAPES = ((4, [300, 240, 150, 280]), (4, [1000, 800, 900, 600]), (32, [300] * 32))
CHAMFER = '--loss' in sys.argv and sys.argv[sys.argv.index('--loss') + 1] == 'chamfer'
if CHAMFER:
    sys.argv = sys.argv[:1]
    SHAPES = ((4, [300] * 4), (32, [300] * 32))
ACTIONS = False
if '--impulses' in sys.argv:
    at = sys.argv.index('--impulses')
    if sys.argv[at + 1] not in ('data', 'actions'):
        raise SystemExit('--impulses data | actions')
    ACTIONS = sys.argv[at + 1] == 'actions'
    del sys.argv[at:at + 2]
if ACTIONS:
    from dyn_res_pile_manip_amd.planners import world2cam_affine
    eng.set_camera(world2cam_affine(syn.demo_cam_extrinsics()), 24.0, syn.demo_cam_params())
    SHAPES = SHAPES[:1]
    sys.argv.insert(1, '0')
if len(sys.argv) > 1:                      # one shape only (profiling): its index
    SHAPES = (SHAPES[int(sys.argv[1])],)
ITERS = int(sys.argv[2]) if len(sys.argv) > 2 else 10
for B, nums in SHAPES:
    N, H = max(nums), 5
    states = np.zeros((B, H + 1, N, 3), np.float32)
    sdelta = np.zeros((B, H, N, 3), np.float32)
    attrs = np.zeros((B, H + 1, N), np.float32)
    dens = np.zeros((B,), np.float32)
    for b, n in enumerate(nums):
        s, d, _ = syn.make_pile(n, 1, seed=b)
        dens[b] = d[0]
        for t in range(H + 1):
            states[b, t, :n] = s[0] + 0.003 * t * rng.standard_normal((n, 3)).astype(np.float32)
        sdelta[b, :, :n] = 0.004 * rng.standard_normal((H, n, 3)).astype(np.float32)
    pn = np.asarray(nums, np.int32)
    eng.train_begin(H, 1e-3, 0.9)
    if CHAMFER:
        # the next states with their rows shuffled: M = N, every row a target
        targets = np.stack([np.stack([states[b, t + 1][rng.permutation(N)] for t in range(H)]) for b in range(B)])
        tn = np.full((B, H), N, np.int32)
        steps = {'mse': lambda: eng.train_step(states, sdelta, attrs, pn, dens, mode='update'),
                 'chamfer': lambda: eng.train_step_untracked(states, sdelta, attrs, pn, dens, targets, tn, mode='update')}
        for k in steps:
            steps[k](), steps[k]()
        took = {'mse': [], 'chamfer': []}
        for rep in range(6):                                        # interleaved blocks; the median of each
            for k in ('mse', 'chamfer'):
                eng.sync()
                t0 = time.perf_counter()
                for _ in range(ITERS):
                    steps[k]()
                eng.sync()
                took[k].append((time.perf_counter() - t0) / ITERS * 1e3)
        print('B=%d N=M=%d n_rollout=%d: update with the MSE loss %.3f ms (blocks %.3f .. %.3f), with the Chamfer loss %.3f ms '
              '(%.3f .. %.3f)' % (B, N, H, np.median(took['mse']), min(took['mse']), max(took['mse']),
                                  np.median(took['chamfer']), min(took['chamfer']), max(took['chamfer'])), flush=True)
        continue
    if ACTIONS:
        acts = np.stack([np.stack([syn.pushes_through(states[b, t, :n][None], seed=10 * b + t)[0] for t in range(H)])
                         for b, n in enumerate(nums)])
        steps = {'data': lambda: eng.train_step(states, sdelta, attrs, pn, dens, mode='update'),
                 'actions': lambda: eng.train_step_actions(states, acts, attrs, pn, dens, mode='update')}
        for k in steps:
            steps[k](), steps[k]()
        took = {'data': [], 'actions': []}
        for rep in range(6):                                        # interleaved blocks; the median of each
            for k in ('data', 'actions'):
                eng.sync()
                t0 = time.perf_counter()
                for _ in range(ITERS):
                    loss, _ = steps[k]()
                    assert np.isfinite(loss), (k, loss)
                eng.sync()
                took[k].append((time.perf_counter() - t0) / ITERS * 1e3)
        print('B=%d N<=%d n_rollout=%d: update on data impulses %.3f ms (blocks %.3f .. %.3f), through the push %.3f ms '
              '(%.3f .. %.3f)' % (B, N, H, np.median(took['data']), min(took['data']), max(took['data']),
                                  np.median(took['actions']), min(took['actions']), max(took['actions'])), flush=True)
        continue
    for _ in range(2):
        eng.train_step(states, sdelta, attrs, pn, dens, mode='update')
    eng.sync()
    t0 = time.perf_counter()
    for _ in range(ITERS):
        loss, _ = eng.train_step(states, sdelta, attrs, pn, dens, mode='update')
    eng.sync()
    ms = (time.perf_counter() - t0) / ITERS * 1e3
    for _ in range(2):
        eng.train_step(states, sdelta, attrs, pn, dens, mode='eval')
    eng.sync()
    t0 = time.perf_counter()
    for _ in range(10):
        eng.train_step(states, sdelta, attrs, pn, dens, mode='eval')
    eng.sync()
    ms_eval = (time.perf_counter() - t0) / 10 * 1e3
    line = 'B=%d N<=%d n_rollout=%d: %.2f ms per training iteration (upload, 5 steps forward, backward, weight gradients, Adam, re-pack); %.2f ms forward-only' % (B, N, H, ms, ms_eval)
    if B * N <= 1200 and len(sys.argv) <= 1:
        t0 = time.perf_counter()
        od.train_loss_and_grads(W, states, sdelta, attrs, pn, dens)
        line += '; dense torch autograd on the host: %.0f ms' % ((time.perf_counter() - t0) * 1e3)
    print(line, flush=True)

"""What accumulating gradients and the clipped optimiser step cost (Engine.train_accumulate, train_apply) beside the built-in update.

  python tools/accum_timing.py [iterations per block [blocks]]        -> stdout (kept as profiles/accum_timing.txt)

At 4 x 5 x 100 and 4 x 5 x 300 (batch x n_rollout x particles, the reference's training shape), data impulses, on ONE context, in
interleaved blocks (every trainer call is complete on the device when it returns, and a block ends in a sync, so a host clock
around a block is the device's time plus the host's), for K = 1 and K = 4 batches per optimiser step:

  update xK     K calls of train_step(mode='update'): K built-in steps
  group of K    K times (train_step(mode='grad'), train_accumulate(B)), then train_apply(1 / (K B), max_norm=1.0): ONE step on the
                gradient of the K batches' mean loss
  apply         train_apply alone (the norm's two launches, the scaled Adam launch, the re-pack and the wait), a gradient pass and
                its accumulation having gone before, outside the clock

The median of the blocks with their spread.  `group / update` is what the seam costs per batch: the grad passes are the update's
own minus k_adam and the re-pack, which the group pays once.

  python tools/accum_timing.py --update-only [iterations [blocks]]    the built-in update alone.  Run from the root of another
                                                                      checkout (the package is imported from the working
                                                                      directory) it times that checkout's build, whatever
                                                                      entry points it has: an interleaved A/B of two commits"""
import sys
import time

sys.path.insert(0, '.')
import numpy as np

from dyn_res_pile_manip_amd import synthetic as syn, weights
from dyn_res_pile_manip_amd.engine import Engine

UPDATE_ONLY = '--update-only' in sys.argv
argv = [a for a in sys.argv[1:] if a != '--update-only']
ITERS = int(argv[0]) if len(argv) > 0 else 40
BLOCKS = int(argv[1]) if len(argv) > 1 else 7
H = 5

eng = Engine(0)
eng.load_weights(weights.blob_from_state_dict(weights.random_state_dict(0)), 0.08)


def make_batch(nums, rng):
    B, N = len(nums), max(nums)
    states = np.zeros((B, H + 1, N, 3), np.float32)
    sdelta = np.zeros((B, H, N, 3), np.float32)
    dens = np.zeros((B,), np.float32)
    for b, n in enumerate(nums):
        s, d, _ = syn.make_pile(n, 1, seed=b)
        dens[b] = d[0]
        for t in range(H + 1):
            states[b, t, :n] = s[0] + 0.003 * t * rng.standard_normal((n, 3)).astype(np.float32)
        sdelta[b, :, :n] = 0.004 * rng.standard_normal((H, n, 3)).astype(np.float32)
    return states, sdelta, np.zeros((B, H + 1, N), np.float32), np.asarray(nums, np.int32), dens


def timed(call, per=1):
    eng.sync()
    t0 = time.perf_counter()
    for _ in range(ITERS):
        call()
    eng.sync()
    return (time.perf_counter() - t0) / (ITERS * per) * 1e3


for nums in ([100, 80, 50, 90], [300, 240, 150, 280]):
    batch = make_batch(nums, np.random.default_rng(0))
    B = len(nums)
    eng.train_begin(H, 1e-5, 0.9)
    head = 'B=4 n_rollout=%d N=%d:' % (H, max(nums))

    def update():
        eng.train_step(*batch, mode='update')

    if UPDATE_ONLY:
        update(), update()
        took = [timed(update) for _ in range(BLOCKS)]
        print('%s update   %.3f ms (blocks %.3f .. %.3f)' % (head, float(np.median(took)), min(took), max(took)), flush=True)
        continue

    def group(K):
        for _ in range(K):
            eng.train_step(*batch, mode='grad')
            eng.train_accumulate(B)
        return eng.train_apply(1.0 / (K * B), max_norm=1.0)

    def apply_alone():
        """-> the milliseconds of one train_apply, its gradient pass and accumulation outside the clock"""
        eng.train_step(*batch, mode='grad')
        eng.train_accumulate(B)
        eng.sync()
        t0 = time.perf_counter()
        eng.train_apply(1.0 / B, max_norm=1.0)
        return (time.perf_counter() - t0) * 1e3

    for K in (1, 4):
        calls = {'update x%d' % K: lambda: [update() for _ in range(K)], 'group of %d' % K: lambda: group(K)}
        for k in calls:                                             # warm-up: every path once, then again
            calls[k](), calls[k]()
        took = dict((k, []) for k in calls)
        took['apply'] = []
        for rep in range(BLOCKS):                                   # interleaved blocks; the median of each
            for k in calls:
                took[k].append(timed(calls[k]))
            took['apply'].append(float(np.median([apply_alone() for _ in range(ITERS)])))
        med = dict((k, float(np.median(v))) for k, v in took.items())
        for k in took:
            print('%s K=%d %-11s %.3f ms (blocks %.3f .. %.3f)' % (head, K, k, med[k], min(took[k]), max(took[k])), flush=True)
        out = group(K)
        print('%s K=%d group / update %.3f per optimiser step, %.3f ms per batch against %.3f; last GradNorm %.6f Clip %.4f'
              % (head, K, med['group of %d' % K] / med['update x%d' % K], med['group of %d' % K] / K, med['update x%d' % K] / K,
                 out['norm'], out['clip']), flush=True)
eng.close()

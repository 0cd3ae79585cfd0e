"""Soak of the trainer: thousands of update iterations over batches of every size the one-launch backward pass and the stage
kernels take (1 ... 8 samples of 10 ... 300 particles, rollouts of 1 ... 5 steps), contexts created and destroyed in between.
Every loss finite, the loss of a fixed held-out batch not above where it started, free device memory flat from context to context.

  python tools/train_soak.py [--impulses data | actions]     actions: the same batches through train_step_actions, every step's
                                                             impulse from a random push that crosses the recorded pile"""
import sys
import time
sys.path.insert(0, '.')
import numpy as np
import torch
from dyn_res_pile_manip_amd import synthetic as syn, weights
from dyn_res_pile_manip_amd.engine import Engine

ACTIONS = '--impulses' in sys.argv and sys.argv[sys.argv.index('--impulses') + 1] == 'actions'


def through_the_push(batch, seed):
    """a push_batch with pushes across every step's recorded pile in place of its impulses"""
    states, _, attrs, nums, dens = batch
    acts = np.stack([np.stack([syn.pushes_through(states[b, t, :n][None], seed=seed * 64 + b * 8 + t)[0]
                               for t in range(states.shape[1] - 1)]) for b, n in enumerate(nums)])
    return (states, acts, attrs, nums, dens)


free0 = torch.cuda.mem_get_info()[0]
t0 = time.time()
total = 0
for rep in range(8):
    eng = Engine(0)
    eng.load_weights(weights.blob_from_state_dict(weights.random_state_dict(rep)), 0.08)
    H = [5, 3, 1, 5][rep % 4]
    rng = np.random.default_rng(rep)
    batches = []
    for k in range(24):
        B = int(rng.choice([1, 2, 4, 8]))
        batches.append(syn.push_batch(100 * rep + k, B, H))
    held = syn.push_batch(9999, 4, H)
    step = eng.train_step
    if ACTIONS:
        from dyn_res_pile_manip_amd.planners import world2cam_affine
        eng.set_camera(world2cam_affine(syn.demo_cam_extrinsics()), 24.0, syn.demo_cam_params())
        batches = [through_the_push(b, 100 * rep + k) for k, b in enumerate(batches)]
        held = through_the_push(held, 9999)
        step = eng.train_step_actions
    eng.train_begin(H, 1e-3, 0.9)
    first, _ = step(*held, mode='eval')
    for it in range(750):
        loss, _ = step(*batches[it % len(batches)], mode='update')
        assert np.isfinite(loss), (rep, it, loss)
        total += 1
    last, _ = step(*held, mode='eval')
    ran = eng.last_dispatch()
    print('H=%d: held-out loss %.4e -> %.4e; variants seen: %s' % (H, first, last, [v for v in ran if v.startswith('train:')]), flush=True)
    assert np.isfinite(last) and last < 1.2 * first          # (750 iterations at 1e-3: the five-step loss has barely begun to fall)
    eng.close()
    torch.cuda.synchronize()
    print('   free HBM %.1f MB' % (torch.cuda.mem_get_info()[0] / 1e6), flush=True)
torch.cuda.synchronize()
free1 = torch.cuda.mem_get_info()[0]
print('%d update iterations in %.1f s; free HBM before %.1f MB after %.1f MB' % (total, time.time() - t0, free0 / 1e6, free1 / 1e6))
# the first contexts leave the HIP runtime's own pools behind (kernel scratch, staging): flat from then on

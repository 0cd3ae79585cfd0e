"""Time the trainer's gradient probe (Engine.train_gradient_probe: one fp32 gradient pass and one float64 pass on the device) with
the Chamfer loss against the same probe with the MSE, on the fixture batch b4_r3 (tests/golden/train.npz: 4 samples of at most
64 particles, 3 rollout steps), interleaved on one context.

  python tools/probe_timing.py [iterations]

The targets are the batch's next states with the correspondence dropped (dataset_gnn_dyn.drop_correspondence) and a 1e-3 jitter,
as the tests make them.  A diagnostic call: the figure goes to DESIGN.md 8, nothing is asserted."""
import os
import sys
import time

sys.path.insert(0, '.')
import numpy as np

from dyn_res_pile_manip_amd import weights
from dyn_res_pile_manip_amd.dataset_gnn_dyn import drop_correspondence
from dyn_res_pile_manip_amd.engine import Engine

ITERS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
g = np.load(os.path.join('tests', 'golden', 'train.npz'), allow_pickle=False)
states, sdelta, attrs, nums, dens = [g['b4_r3/' + k] for k in ('states', 'states_delta', 'attrs', 'particle_nums', 'particle_dens')]
B, T1, N, _ = states.shape
H = T1 - 1
rng = np.random.default_rng(0)
clouds = []
for b in range(B):
    n = int(nums[b])
    sample = (states[b, :, :n], np.zeros((H, n, 3), np.float32), np.zeros((T1, n), np.float32), n, 1.0, None)
    clouds.append([(c + 1e-3 * rng.standard_normal(c.shape)).astype(np.float32) for c in drop_correspondence(sample, rng)[6]])
M = max(c.shape[0] for cs in clouds for c in cs)
targets = np.zeros((B, H, M, 3), np.float32)
tnums = np.zeros((B, H), np.int32)
for b, cs in enumerate(clouds):
    for t, c in enumerate(cs):
        targets[b, t, :c.shape[0]] = c
        tnums[b, t] = c.shape[0]

eng = Engine(0)
eng.load_weights(weights.blob_from_state_dict(weights.random_state_dict(0)), 0.08)
eng.train_begin(H, 1e-3, 0.9)
probes = {'mse': lambda: eng.train_gradient_probe(states, sdelta, attrs, nums, dens),
          'chamfer': lambda: eng.train_gradient_probe(states, sdelta, attrs, nums, dens, targets=targets, target_nums=tnums)}
last = {}
for k in probes:
    probes[k](), probes[k]()
took = {'mse': [], 'chamfer': []}
for rep in range(6):                                        # interleaved blocks; the median of each
    for k in ('mse', 'chamfer'):
        eng.sync()
        t0 = time.perf_counter()
        for _ in range(ITERS):
            last[k] = probes[k]()
        eng.sync()
        took[k].append((time.perf_counter() - t0) / ITERS * 1e3)
print('b4_r3 (B=%d N=%d M=%d n_rollout=%d): gradient probe with the MSE %.3f ms (blocks %.3f .. %.3f), with the Chamfer loss %.3f ms '
      '(%.3f .. %.3f); worst rel %.2e / %.2e, min_margin %.3e'
      % (B, N, M, H, np.median(took['mse']), min(took['mse']), max(took['mse']), np.median(took['chamfer']), min(took['chamfer']),
         max(took['chamfer']), last['mse']['rel'], last['chamfer']['rel'], last['chamfer']['min_margin']), flush=True)
eng.close()

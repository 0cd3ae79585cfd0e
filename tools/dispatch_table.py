#!/usr/bin/env python
"""Which kernel variants serve which call: a fixed grid of shapes through the Engine API (dispatch_reset, the call,
last_dispatch), one line per call:

    <engine> <entry> B=<B> N=<N> nb=<n_batch> H=<H> -> <sorted variant names, ' | ' between them>

    python tools/dispatch_table.py > tests/dispatch_table.txt        (on a GPU)

tests/dispatch_table.txt is this tool's output on the commit named in its first line; tests/test_gpu_dispatch_table.py holds the
built library to it line for line, tests/test_dispatch_plan.py holds csrc/dispatch.h's plan functions to it without a GPU.

The grid: the designed forward shapes, the gradient and the training shapes of tests/test_gpu_fuzz_oracle.py, and a shape just
inside and just outside every threshold of the dispatch policy.  One kind of case is left out (`async_pair`): where a workgroup of
the whole-sample kernels gets 65 ... 128 rows, paired or unpaired tiles follow a mean in-degree the device writes behind earlier
launches, and the name is not a function of the shape.  Every case runs on a fresh context, so nothing of an earlier case (the
in-degree word, cached argument blocks) reaches it."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dyn_res_pile_manip_amd import synthetic as syn, weights, _lib  # noqa: E402
from dyn_res_pile_manip_amd.engine import Engine  # noqa: E402
from oracle import propnet_sparse as osp  # noqa: E402

def fuzz_shapes():
    """DESIGNED / GD_SHAPES / TRAIN_SHAPES of tests/test_gpu_fuzz_oracle.py, read from its text (importing it needs pytest's fixtures)."""
    import ast
    src = open(os.path.join(ROOT, 'tests', 'test_gpu_fuzz_oracle.py')).read()
    out = {}
    for node in ast.parse(src).body:
        if isinstance(node, ast.Assign) and getattr(node.targets[0], 'id', '') in ('DESIGNED', 'GD_SHAPES', 'TRAIN_SHAPES'):
            out[node.targets[0].id] = ast.literal_eval(node.value)
    return out['DESIGNED'], out['GD_SHAPES'], out['TRAIN_SHAPES']


def async_pair(B, N, nb, n_cu):
    """Does a workgroup of a whole-sample launch of this batch get 65 ... 128 rows?  (samples per workgroup: the batch over the
    CUs; a cached pile size goes out in blocks of n_cu x (288 or 256 rows / N) samples, whole multiples of nb, and a last shorter one)"""
    spws = [(B + n_cu - 1) // n_cu]
    if N <= 128 or 225 <= N <= 256:
        spw_cap = max(1, (288 if N <= 64 else 256) // N)
        chunk = n_cu * spw_cap // nb * nb
        if 0 < chunk < B:
            spws = [spw_cap] + ([(B % chunk + n_cu - 1) // n_cu] if B % chunk else [])
    return any(65 <= s * N <= 128 for s in spws)


def forward_grid(n_cu):
    designed, _, _ = fuzz_shapes()
    grid = [(B // nb * nb, N, nb, H) for B, N, nb, H, _, _, _ in designed]     # the test's batch: whole multiples of n_batch
    few, full = n_cu - n_cu // 5, n_cu
    # particle counts on both sides of 64 (one-launch rollout, pairing), 128 (cache, plain / strip build), 225 and 256 (cache,
    # whole samples), 400 (cells), 800 (wide strips); a handful of samples, half a chip, a chip and four chips of them
    for N in (63, 64, 65, 128, 129, 200, 201, 224, 225, 256, 257, 399, 400, 799, 800):
        for B in (4, n_cu // 2, full, 4 * full):
            if B * N <= 300000:
                grid.append((B, N, 1, 1))
    # n_cu - n_cu / 5 samples of piles above 256 particles: whole samples or tiles dealt over the chip
    grid += [(few - 1, 300, 1, 1), (few, 300, 1, 1)]
    # rows per workgroup: 256 / 288 (a cached launch's cap), 704 (the one-launch rollout's), on both sides
    grid += [(8 * full, 32, 1, 1), (9 * full, 32, 1, 1), (10 * full, 32, 1, 1), (11 * full, 64, 1, 1), (12 * full, 64, 1, 1),
             (22 * full, 32, 2, 1), (23 * full, 32, 1, 1), (4 * full, 64, 1, 2), (4 * full + 1, 64, 1, 1), (2 * full, 128, 2, 1),
             (2 * full + 2, 128, 2, 1)]
    # n_cu / 2 workgroups: four threads per receiver in the plain build, several workgroups per sample in the aggregate
    grid += [(n_cu // 2 - 1, 64, 1, 1), (n_cu // 2 + 1, 64, 1, 1), (n_cu // 4, 200, 1, 1), (n_cu // 4 + 1, 200, 1, 1), (n_cu // 2 - 1, 201, 1, 1)]
    seen, out = set(), []
    for g in grid:
        if g not in seen and not async_pair(g[0], g[1], g[2], n_cu):
            seen.add(g)
            out.append(g)
    return out


# where the engine matters: graph builds, the aggregate's variants, the encoders
OTHER_ENGINE_GRID = [(6, 40, 2, 2), (4, 300, 1, 2), (3, 700, 1, 1), (130, 64, 1, 1), (127, 64, 1, 1), (128, 64, 1, 1), (4, 400, 1, 1),
                     (2, 800, 1, 1), (300, 150, 2, 1)]


class Runner(object):
    def __init__(self):
        self.sd = weights.random_state_dict(seed=0)
        self.blob = weights.blob_from_state_dict(self.sd)
        self.M34 = osp.world2cam_affine(syn.demo_cam_extrinsics(), 24)
        self.obs_goal = syn.goal_distance_image(syn.goal_mask('I'))
        self.G = syn.goal_field(self.obs_goal)
        self.lines = []

    def fresh(self, engine, N):
        e = Engine(0)
        e.load_weights(self.blob, 0.08)
        e.set_camera(self.M34, 24.0, syn.demo_cam_params())
        e.set_goal(self.G, syn.goal_coor_strided(self.obs_goal, min(5 * N, 400)))
        e.set_engine(_lib.ENGINES[engine])
        e.dispatch_reset()
        return e

    def emit(self, e, engine, entry, B, N, nb, H):
        self.lines.append('%s %s B=%d N=%d nb=%d H=%d -> %s' % (engine, entry, B, N, nb, H, ' | '.join(sorted(e.last_dispatch()))))
        e.dispatch_reset()

    def forward(self, engine, B, N, nb, H, entries):
        s0, dens, attr = syn.make_pile(N, nb, seed=B * 7919 + N * 31 + H)
        acts = np.stack([syn.sample_pushes(B, 1, seed=t)[:, 0] for t in range(H)], 1)
        lo, hi = syn.action_limits()
        for entry in entries:
            e = self.fresh(engine, N)
            if entry == 'rollout':
                e.rollout(s0, attr, dens, acts, want_states=False, want_reward=True)
            elif entry == 'step':
                s1 = np.tile(s0, (B // nb, 1, 1))
                e.step(np.tile(attr, (B // nb, 1)), s1, np.zeros_like(s1), np.tile(dens, B // nb))
            elif entry == 'mppi':
                e.mpc_begin(s0, attr, dens, syn.nominal_pushes(H, seed=1), B // nb, 0.6, 0.7, 0.1, lo, hi, seed=5)
                e.dispatch_reset()
                e.mpc_sample(1)
                e.mpc_rollout(False)
                e.mpc_update_device()
            e.sync()
            self.emit(e, engine, entry, B, N, nb, H)
            e.close()

    def gd(self, engine, B, N, nb, H):
        s0, dens, attr = syn.make_pile(N, nb, seed=B * 13 + N)
        acts = np.stack([syn.sample_pushes(B, 1, seed=t)[:, 0] for t in range(H)], 1)
        lo, hi = syn.action_limits()
        e = self.fresh(engine, N)
        e.gd_begin(s0, attr, dens, acts, 0.05, lo, hi)
        e.dispatch_reset()
        e.gd_step()
        self.emit(e, engine, 'gd', B, N, nb, H)
        e.close()

    def train(self, engine, nums, T):
        eps = [syn.push_episode(n, T, 500 + i) for i, n in enumerate(nums)]
        B, N = len(nums), max(nums)
        states = np.zeros((B, T + 1, N, 3), np.float32)
        sdelta = np.zeros((B, T, N, 3), np.float32)
        attrs = np.zeros((B, T + 1, N), np.float32)
        for j, ep in enumerate(eps):
            states[j, :, :ep[3]], sdelta[j, :, :ep[3]] = ep[0], ep[1]
        e = self.fresh(engine, N)
        e.train_begin(T, 1e-3, 0.9)
        e.dispatch_reset()
        e.train_step(states, sdelta, attrs, np.asarray(nums, np.int32), np.array([ep[4] for ep in eps], np.float32), mode='grad')
        self.emit(e, engine, 'train', B, N, 1, T)
        e.close()


def main():
    r = Runner()
    e = Engine(0)
    info = e.device_info()
    e.close()
    n_cu = info['n_cu']
    try:
        commit = subprocess.check_output(['git', 'rev-parse', 'HEAD'], cwd=ROOT, stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        commit = os.environ.get('DRP_TABLE_COMMIT', 'unknown')
    commit = os.environ.get('DRP_TABLE_COMMIT', commit)
    print('# commit %s  device "%s"  n_cu %d' % (commit, info['name'], n_cu))
    _, gd_shapes, train_shapes = fuzz_shapes()
    for B, N, nb, H in forward_grid(n_cu):
        r.forward('fused', B, N, nb, H, ('rollout', 'step') + (('mppi',) if B * N * H <= 150000 else ()))
    for engine in ('valu', 'mfma', 'split'):
        for B, N, nb, H in OTHER_ENGINE_GRID:
            r.forward(engine, B, N, nb, H, ('rollout',))
    for B, N, nb, H, _, engine in gd_shapes:
        B = B // nb * nb
        if engine != 'fused' or not async_pair(B, N, nb, n_cu):
            r.gd(engine, B, N, nb, H)
    # the backward pass's thresholds: rows kernel up to 256 particles, whole samples from n_cu - n_cu / 5
    for B, N in ((4, 256), (4, 257), (n_cu - n_cu // 5 - 1, 260), (n_cu - n_cu // 5, 260), (n_cu, 41), (n_cu, 40)):
        r.gd('fused', B, N, 1, 1)
    for nums, T, engine in train_shapes:
        r.train(engine, nums, T)
    # the trainer's node stages: one launch up to n_cu / 4 tiles of 32 rows
    for nums in ([256] * (n_cu // 32), [256] * (n_cu // 32 + 1)):
        r.train('fused', nums, 1)
    # the tape in more than one km_prop3 launch: 40 particles are cached on the tape, seven samples to a workgroup and launch --
    # one block of whole multiples of the 30 batch columns and a tail of one multiple; a block and seven samples for the trainer
    r.gd('fused', n_cu * 7 // 30 * 30 + 30, 40, 30, 2)
    r.train('fused', [40] * (n_cu * 7 + 7), 1)
    sys.stdout.write('\n'.join(r.lines) + '\n')


if __name__ == '__main__':
    main()

"""Child process of tests/test_gpu_ctx_lifecycle.py: contexts are created, used on every surface that allocates, and
destroyed; the device's free memory after each destroy goes out as one JSON line.

    python tests/_ctx_lifecycle_child.py EPISODE_DIR
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'golden'))

import torch  # noqa: E402

import _rgr_ref  # noqa: E402
import _rgr_train_ref  # noqa: E402
import make_golden_gnn_dataset as mk  # noqa: E402
from dyn_res_pile_manip_amd import _lib, res_regressor as rr, synthetic as syn, weights  # noqa: E402
from dyn_res_pile_manip_amd.dataset_gnn_dyn import ParticleDataset  # noqa: E402
from dyn_res_pile_manip_amd.engine import Engine  # noqa: E402
from dyn_res_pile_manip_amd.planners import world2cam_affine  # noqa: E402

BLOB = weights.blob_from_state_dict(weights.random_state_dict(seed=0))
RGR_BLOB = rr.blob_from_state_dict(_rgr_train_ref.fixture_state_dict(11, 1), 1)
LO, HI = syn.action_limits()
DRP_EINVAL = -1                     # include/drp.h


def free_bytes():
    torch.cuda.synchronize()
    return int(torch.cuda.mem_get_info(0)[0])


def planner_setup(eng):
    eng.load_weights(BLOB, 0.08)
    eng.set_camera(world2cam_affine(syn.demo_cam_extrinsics()), 24.0, syn.demo_cam_params())
    eng.set_goal_image(syn.goal_distance_image(syn.goal_mask('I')), 200, fps_init=0, mode='cv5', want=False)


def rollout(eng, B, N, family):
    """a rollout of the recorded shape B x N x 1 step (tests/dispatch_table.txt) on the kernel family it is recorded with"""
    s0, dens, attr = syn.make_pile(N, 1, seed=N)
    eng.dispatch_reset()
    eng.rollout(s0, attr, dens, syn.sample_pushes(B, 1, seed=0), want_states=True, want_reward=True)
    launched = eng.last_dispatch()
    assert any(v.startswith(family + '<') for v in launched), (B, N, launched)


def gd_session(eng, wait):
    N = 20
    s0, dens, attr = syn.make_pile(N, 4, seed=N)
    acts = np.repeat(np.stack([syn.nominal_pushes(2, seed=i) for i in range(3)]), 4, axis=0).astype(np.float32)
    eng.gd_begin(s0, attr, dens, acts, 0.05, LO, HI)
    eng.gd_step_async(0)
    eng.gd_step_async(1)
    if wait:
        for slot in (0, 1):
            r, a = eng.gd_wait(slot)
            assert np.isfinite(r).all() and np.isfinite(a).all()


def exercise(eng, episodes):
    planner_setup(eng)
    rollout(eng, 128, 64, 'km_rollout')
    rollout(eng, 256, 280, 'km_prop3')

    # the sampling planner, both pinned slots in flight at once
    s0, dens, attr = syn.make_pile(40, 1, seed=0)
    eng.mpc_begin(s0, attr, dens, syn.nominal_pushes(2, seed=0), n_sample=8, sigma=0.6, beta_filter=0.7, reward_weight=0.1,
                  act_lo=LO, act_hi=HI, seed=1)
    for it in (0, 1):
        eng.mpc_sample(it)
        eng.mpc_rollout(False)
        eng.mpc_update_device()
        eng.mpc_fetch_async(it)
    for it in (0, 1):
        eng.mpc_wait(it)

    gd_session(eng, wait=True)

    # one optimiser step of the dynamics model
    B, T, N = 2, 2, 48
    rng = np.random.default_rng(0)
    states = np.zeros((B, T + 1, N, 3), np.float32)
    for b in range(B):
        s, _, _ = syn.make_pile(N, 1, seed=3 + b, kind='blob')
        states[b, :] = s[0] * 0.3 + [0, 0, 0.52]
    sdelta = (0.004 * rng.standard_normal((B, T, N, 3))).astype(np.float32)
    eng.train_begin(T, 1e-3, 0.9)
    loss, _ = eng.train_step(states, sdelta, np.zeros((B, T + 1, N), np.float32), np.full(B, N, np.int32),
                             np.array([300.0, 350.0], np.float32), mode='update')
    assert np.isfinite(loss)

    # the resolution regressor: load, forward, one training step, the two timing entry points, the weights back
    x = _rgr_ref.rand_input(5000, 2)
    eng.rgr_load(RGR_BLOB, 1)
    assert np.isfinite(eng.rgr_forward(x)).all()
    eng.rgr_train_begin(1e-4, 0.9, 0.0)
    eng.rgr_train_step(x, y=np.array([40.0, 90.0], np.float32), conf=np.ones(2, np.float32), mode='update')
    assert eng.rgr_time(2, iters=3).shape == (3,)
    assert eng.rgr_train_time(2, iters=2).shape == (2, 3)
    assert eng.rgr_get_weights().shape == RGR_BLOB.shape

    # one training batch of the dynamics model from recorded episodes
    ds = ParticleDataset(episodes, mk.CONFIG, 'train', (syn.demo_cam_params(), syn.demo_cam_extrinsics()), engine=eng)
    ds.run([ds.load(0)], [(1000.0, 17)])

    eng.probe_begin('prop')
    rollout(eng, 256, 280, 'km_prop3')
    ms, launches = eng.probe_read()[:2]
    assert launches >= 1 and ms > 0.0
    eng.probe_begin('')


def main():
    episodes = sys.argv[1]
    syn.write_episodes(episodes, n_episode=mk.EPISODES['n_episode'], n_timestep=mk.EPISODES['n_timestep'], seed=mk.EPISODES['seed'])
    out = {'start': free_bytes(), 'cycles': []}
    for _ in range(3):
        eng = Engine(0)
        exercise(eng, episodes)
        eng.close()
        out['cycles'].append(free_bytes())

    eng = Engine(0)                     # destroyed straight after a refused call
    try:
        eng.load_weights(BLOB[:-1], 0.08)
        raise AssertionError('a short blob was accepted')
    except _lib.DrpError as e:
        assert 'drp error %d:' % DRP_EINVAL in str(e), str(e)
    eng.close()
    out['after_refusal'] = free_bytes()

    eng = Engine(0)                     # destroyed with iterations in flight in both slots
    planner_setup(eng)
    gd_session(eng, wait=False)
    eng.close()
    out['after_pending'] = free_bytes()
    print('LIFECYCLE ' + json.dumps(out), flush=True)


if __name__ == '__main__':
    main()

"""Randomised check of the trainer's gradients through the push (drp_train_step_actions) against the float64 call on the device
(drp_train_grad_f64_actions, through Engine.train_gradient_probe): random batch sizes, particle counts with and without padding,
rollouts of 1-4 steps, both tapes, pushes that cross the pile.  Bounds: the loss within 1e-4, every one of the 18 tensors within
2e-4 of its largest gradient (tests/test_gpu_train_actions.py).  Nothing here picks seeds by their margins: a row within fp32
drift of the hard mask's edges or of the soft mask's kink takes another branch in float64, so a case beyond the bound is counted
and reported, and only more than one in eight fails the run.

  python tools/fuzz_train_actions.py [cases]"""
import sys
sys.path.insert(0, '.')
import numpy as np
from dyn_res_pile_manip_amd import synthetic as syn, weights
from dyn_res_pile_manip_amd.engine import Engine
from dyn_res_pile_manip_amd.planners import world2cam_affine

LOSS_REL, GRAD_REL = 1e-4, 2e-4
n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 24
rng = np.random.default_rng(2)
worst, bad = 0.0, 0
for case in range(n_cases):
    B = int(rng.choice([1, 2, 3, 5]))
    N = int(rng.choice([5, 11, 24, 33, 70, 150, 300]))
    H = int(rng.choice([1, 2, 3, 4]))
    nums = rng.integers(max(1, N // 3), N + 1, B)
    nums[int(rng.integers(B))] = N                      # the padded width is some sample's count, as collate_fn makes it
    tape = str(rng.choice(['fused', 'mfma']))
    states = np.zeros((B, H + 1, N, 3), np.float32)
    acts = np.zeros((B, H, 4), np.float32)
    dens = np.zeros((B,), np.float32)
    for b, n in enumerate(nums):
        s, d, _ = syn.make_pile(int(n), 1, seed=1000 + 10 * case + b, kind=str(rng.choice(['uniform', 'blob'])))
        dens[b] = d[0] * rng.uniform(0.6, 1.4)
        for t in range(H + 1):
            states[b, t, :n] = s[0] + 0.004 * t * rng.standard_normal((n, 3)).astype(np.float32)
        for t in range(H):
            acts[b, t] = syn.pushes_through(states[b, t, :n][None], seed=100 * case + 10 * b + t)[0]
    attrs = np.zeros((B, H + 1, N), np.float32)
    eng = Engine(0)
    eng.load_weights(weights.blob_from_state_dict(weights.random_state_dict(case)), 0.08)
    eng.set_camera(world2cam_affine(syn.demo_cam_extrinsics()), 24.0, syn.demo_cam_params())
    eng.set_engine(tape)
    eng.train_begin(H, 1e-3, 0.9)
    pr = eng.train_gradient_probe(states, None, attrs, nums.astype(np.int32), dens, actions=acts)
    eng.close()
    e = max(t['max_abs_err'] / max(t['max_abs_ref'], 1e-8) for t in pr['tensors'].values())
    el = pr['loss_diff'] / pr['loss64']
    ok = all(t['max_abs_err'] < GRAD_REL * t['max_abs_ref'] + 1e-9 for t in pr['tensors'].values()) and el < LOSS_REL
    print('case %d (B=%d N=%d counts %s H=%d %s): gradient error %.2e, loss error %.2e%s'
          % (case, B, N, [int(n) for n in nums], H, tape, e, el, '' if ok else '  [beyond the bound, counted]'), flush=True)
    assert np.isfinite(e) and np.isfinite(el), case
    if not ok:
        bad += 1
        continue
    worst = max(worst, e)
assert bad <= max(1, n_cases // 8), bad
print('%d cases, %d beyond the bound (a row at the edge of a mask); worst gradient error within it %.2e of the largest entry of a tensor'
      % (n_cases, bad, worst))

"""Randomised cross-check of the engines on odd shapes (N = 1 ... 700 incl. non-multiples of 32, several
batch columns, horizons, attribute patterns, sparse and clumped piles): the fused engine against the
fp32 MFMA engine and the VALU engine, and small cases against the numpy oracle."""
import sys
sys.path.insert(0, '.')
import numpy as np
from dyn_res_pile_manip_amd import synthetic as syn, weights, _lib
from dyn_res_pile_manip_amd.engine import Engine
from dyn_res_pile_manip_amd.planners import world2cam_affine
from oracle import propnet_sparse as osp

eng = Engine(0)
sd = weights.random_state_dict(3)
eng.load_weights(weights.blob_from_state_dict(sd), 0.08)
eng.set_camera(world2cam_affine(syn.demo_cam_extrinsics()), 24.0, syn.demo_cam_params())
W = osp.weights_np({k: np.asarray(v) for k, v in sd.items()})
rng = np.random.default_rng(0)
worst, worst_at = 0.0, None
flipped, rows_later = 0, 0
n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 60
for case in range(n_cases):
    N = int(rng.choice([1, 2, 3, 9, 10, 11, 31, 32, 33, 63, 64, 65, 100, 257, 300, 511, 700]))
    nb = int(rng.choice([1, 1, 2, 3]))
    ns = int(rng.choice([1, 2, 5, 16, 16, 300, 517]))   # >= 256 rows: the fused engine runs km_prop3 (three steps per launch)
    if ns >= 256 and N > 300:
        N = int(rng.choice([300, 300, 450]))             # 450: the two-dimensional cell graph under km_prop3
    H = int(rng.choice([1, 2, 4]))
    kind = str(rng.choice(['uniform', 'blob']))
    s0, dens, attr = syn.make_pile(N, nb, seed=case, kind=kind)
    scale = float(rng.choice([1.0, 0.3, 3.0]))          # clumped (everything within the radius) or sparse (isolated particles)
    s0[..., :2] *= scale
    mode = int(rng.integers(0, 4))
    if mode == 1:
        attr = np.full_like(attr, 0.25)
    elif mode == 2:
        attr = rng.uniform(-1, 1, attr.shape).astype(np.float32)
    elif mode == 3 and nb > 1:
        # some columns with uniform attributes, some without: km_prop3's tiles span samples, so a tile can hold
        # receivers with and without the self-edge shortcut
        attr = attr.copy()
        attr[1::2] = rng.uniform(-1, 1, attr[1::2].shape).astype(np.float32)
    dens = (dens * rng.uniform(0.3, 2.0, dens.shape)).astype(np.float32)
    acts = syn.sample_pushes(ns * nb, H, seed=case)
    outs = {}
    for name in ('valu', 'mfma', 'fused', 'lite'):
        eng.set_engine(_lib.ENGINES[name])
        outs[name], _ = eng.rollout(s0, attr, dens, acts)
        assert np.isfinite(outs[name]).all(), (case, name)
    prev = np.tile(s0, (ns, 1, 1))
    for t in range(H):
        disp = max(np.abs(outs['mfma'][:, t] - prev).max(), 1e-7)
        for name in ('valu', 'fused', 'lite'):
            # lite: the opt-in reduced products (include/drp.h), held to 1e-2 of the displacement here -- its own accuracy is the
            # probe's and tests/test_gpu_lite.py's business; this run looks for rows that break, not for rounding
            tol = 1e-2 if name == 'lite' else 1e-4
            per_row = np.abs(outs[name][:, t] - outs['mfma'][:, t]).reshape(ns * nb, -1).max(1) / disp
            if t == 0:
                e = per_row.max()
                if e > worst and name != 'lite':
                    worst, worst_at = e, (case, name, t, N, nb, ns, H, kind, scale, mode, float(disp))
                assert e < tol, (case, name, t, N, nb, ns, H, kind, scale, mode, e)
            else:
                # later steps start from states that differ in the last bits; a receiver whose 10th and 11th
                # nearest senders are almost equidistant may then pick the other one (rows of dense piles):
                # most rows must still agree
                if name != 'lite':
                    flipped += int((per_row > 1e-4 * (t + 1)).sum())
                    rows_later += per_row.size
        prev = outs['mfma'][:, t]
    if N <= 100 and ns * nb <= 6:
        # teacher-forced one-step check against the numpy oracle
        B = ns * nb
        s_in = np.tile(s0, (ns, 1, 1))
        a_in = np.tile(attr, (ns, 1))
        d_in = np.tile(dens, ns)
        sdl = eng.gen_s_delta(s_in, acts[:, 0])
        ref = osp.predict_one_step(W, a_in, s_in, sdl, d_in)
        disp = max(np.abs(ref - s_in).max(), 1e-7)
        e = np.abs(outs['fused'][:, 0] - ref).max() / disp
        assert e < 1e-4, (case, 'oracle', N, e)
assert flipped <= 0.03 * max(rows_later, 1), (flipped, rows_later)
print('rows whose neighbour choice diverged after the first step: %d of %d' % (flipped, rows_later))
print('%d cases ok; worst relative displacement error per step %.2e at (case, engine, step, N, nb, ns, H, kind, scale, attr mode, displacement) = %s' % (n_cases, worst, worst_at))

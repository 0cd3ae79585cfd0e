"""Fixture of the untracked data path (row x4 / u1): the reference's own depth2fgpcd -> fps_rad -> recenter (utils.py:491-506,
438-449, 468-477, called as dataset/dataset_gnn_dyn.py:97-101 calls them) on EVERY frame of windows of the episodes
make_golden_gnn_dataset.py writes, with the intermediates.

    python tests/golden/make_golden_gnn_frames.py /path/to/reference     -> tests/golden/gnn_frames.npz

The reference's utils is imported with make_golden_gnn_dataset's stubs; fps_rad is wrapped as there to record the start it
draws and the indices it chooses.  Per case the draws on numpy's global generator are DepthDataset's: np.random.seed(seed),
particle_den = uniform(15, 6500), then fps_rad's own randint(n_fg_t) for the frames t = 0..T-1 in order.  Frame 0 is sampled at
radius 1/sqrt(den), the frames after it at 1/sqrt(den * target_den_scale).  The episodes are not stored: the tests write them
again (EPISODES).  Arrays only; per case k: c<k>_den, c<k>_n_fg [T], c<k>_init [T], c<k>_counts [T], and the frames' chosen
indices (int32) and recentered float64 points one after the other in c<k>_chosen [sum counts], c<k>_recenter [sum counts, 3]."""
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden_gnn_dataset as mk  # noqa: E402
from dyn_res_pile_manip_amd import synthetic  # noqa: E402
from dyn_res_pile_manip_amd.dataset_gnn_dyn import PARTICLE_DEN_MAX, PARTICLE_DEN_MIN, DepthDataset, read_depth  # noqa: E402

EPISODES = mk.EPISODES
CONFIG = mk.CONFIG
# (numpy seed, phase, idx, target_den_scale): the seeds' first uniform(15, 6500) draws span 82 .. 6286
CASES = [(9, 'train', 0, 1.0), (7, 'train', 3, 1.0), (19, 'valid', 1, 2.0), (5, 'valid', 0, 1.0), (0, 'train', 1, 1.0),
         (4, 'valid', 3, 1.0)]


def main(ref_root, out=os.path.join(mk.ROOT, 'tests', 'golden', 'gnn_frames.npz')):
    mk._stubs()
    sys.path.insert(0, ref_root)
    import utils as U
    rec = {}
    randint0 = np.random.randint

    def fps_rad(pcd, radius):
        def randint(n):
            v = randint0(n)
            rec['init'] = v
            return v
        np.random.randint = randint
        try:
            pts = U.fps_rad(pcd, radius)
        finally:
            np.random.randint = randint0
        where = {pcd[i].tobytes(): i for i in range(pcd.shape[0])}
        return pts, np.array([where[p.tobytes()] for p in pts], np.int32)

    cam = (synthetic.demo_cam_params(), synthetic.demo_cam_extrinsics())
    res = {'cases': np.array([[s, 0 if ph == 'train' else 1, i] for s, ph, i, _ in CASES], np.int64),
           'scales': np.array([c[3] for c in CASES], np.float64),
           'episodes': np.array([EPISODES['n_episode'], EPISODES['n_timestep'], EPISODES['seed']], np.int64)}
    with tempfile.TemporaryDirectory() as d:
        synthetic.write_episodes(d, **EPISODES)
        for k, (seed, phase, idx, scale) in enumerate(CASES):
            ds = DepthDataset(d, CONFIG, phase, cam)                       # locate() only: which files a window reads
            ep, t0 = ds.locate(idx)
            T = ds.n_his + ds.n_roll
            np.random.seed(seed)
            den = np.random.uniform(PARTICLE_DEN_MIN, PARTICLE_DEN_MAX)
            n_fg, init, counts, chosen, recentered = [], [], [], [], []
            for t in range(T):
                particle_r = 1 / np.sqrt(den if t == 0 else den * scale)
                depth = read_depth(os.path.join(d, '%d' % ep, '%d_depth.png' % (t0 + t))) / (ds.global_scale * 1000.0)   # :97
                pcd = U.depth2fgpcd(depth, (depth < 0.599 / 0.8), ds.cam_params)                                        # :98
                pts, ch = fps_rad(pcd, particle_r)                                                                        # :99
                rc = U.recenter(pcd, pts, r=min(0.02, 0.5 * particle_r))                                                 # :101
                n_fg.append(pcd.shape[0])
                init.append(rec['init'])
                counts.append(len(ch))
                chosen.append(ch)
                recentered.append(np.asarray(rc, np.float64))
            print('case %d: seed %d %s[%d] scale %g den %.1f n_fg %s counts %s' % (k, seed, phase, idx, scale, den, n_fg, counts))
            p = 'c%d_' % k
            res[p + 'den'] = np.float64(den)
            res[p + 'n_fg'] = np.array(n_fg, np.int64)
            res[p + 'init'] = np.array(init, np.int64)
            res[p + 'counts'] = np.array(counts, np.int64)
            res[p + 'chosen'] = np.concatenate(chosen)
            res[p + 'recenter'] = np.concatenate(recentered)
    mk.save_npz(out, res)
    print('wrote', out, os.path.getsize(out), 'bytes')


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else '../reference')

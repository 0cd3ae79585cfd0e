"""Fixture of the GNN dataset (row x4): the reference's own ParticleDataset.__getitem__ (dataset/dataset_gnn_dyn.py) on
episodes written by synthetic.write_episodes, with its intermediates.

    python tests/golden/make_golden_gnn_dataset.py /path/to/reference     -> tests/golden/gnn_dataset.npz

The reference module is imported with stubs for what it cannot import here: cv2.imread (through PIL: uint16 for
IMREAD_ANYDEPTH, BGR otherwise), env.flex_env.FlexEnv and dgl.geometry (unused by the dataset), open3d (unused).  Its
fps_rad, recenter and KDTree are wrapped to record n_fg, the sampler's start, the chosen indices, the recentered points and
the nearest indices.  The episodes are not stored: the tests write them again with the same call (EPISODES below)."""
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from dyn_res_pile_manip_amd import synthetic  # noqa: E402
from dyn_res_pile_manip_amd.dataset_gnn_dyn import read_color, read_depth  # noqa: E402

EPISODES = dict(n_episode=4, n_timestep=6, seed=0)
CONFIG = {'dataset': {'global_scale': 24, 'n_episode': 4, 'n_timestep': 6},
          'train': {'train_valid_ratio': 0.5, 'n_history': 1, 'n_rollout': 5}}
# (numpy seed, phase, idx): the seeds' first uniform(15, 6500) draws span the range
CASES = [(9, 'train', 0), (7, 'train', 3), (19, 'valid', 1), (12, 'train', 1), (5, 'valid', 0), (1, 'train', 2),
         (18, 'valid', 3), (4, 'train', 0)]


def _stubs():
    cv2 = types.ModuleType('cv2')
    cv2.IMREAD_ANYDEPTH = 2
    cv2.imread = lambda path, flag=None: read_depth(path) if flag == 2 else read_color(path)
    sys.modules['cv2'] = cv2
    env = types.ModuleType('env')
    fe = types.ModuleType('env.flex_env')
    fe.FlexEnv = type('FlexEnv', (), {})
    env.flex_env = fe
    sys.modules['env'] = env
    sys.modules['env.flex_env'] = fe
    dgl = types.ModuleType('dgl')
    geo = types.ModuleType('dgl.geometry')
    geo.farthest_point_sampler = None
    dgl.geometry = geo
    sys.modules['dgl'] = dgl
    sys.modules['dgl.geometry'] = geo
    sys.modules['open3d'] = types.ModuleType('open3d')


def save_npz(path, arrays):
    """np.savez_compressed with fixed zip timestamps: the file is byte-identical on regeneration"""
    import io
    import zipfile
    with zipfile.ZipFile(path, 'w', compression=zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            zi = zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(zi, buf.getvalue())


def main(ref_root, out=os.path.join(ROOT, 'tests', 'golden', 'gnn_dataset.npz')):
    _stubs()
    sys.path.insert(0, ref_root)
    import dataset.dataset_gnn_dyn as D
    rec = {}
    fps_rad0, recenter0, KDTree0 = D.fps_rad, D.recenter, D.KDTree
    randint0 = np.random.randint

    def fps_rad(pcd, radius):
        rec['n_fg'] = pcd.shape[0]
        def randint(n):
            v = randint0(n)
            rec['init'] = v
            return v
        np.random.randint = randint
        try:
            pts = fps_rad0(pcd, radius)
        finally:
            np.random.randint = randint0
        where = {pcd[i].tobytes(): i for i in range(pcd.shape[0])}
        rec['chosen'] = np.array([where[p.tobytes()] for p in pts], np.int32)
        return pts

    def recenter(pcd, sampled, r=0.02):
        out = recenter0(pcd, sampled, r)
        rec['recenter'] = out.copy()
        return out

    class KDTree(KDTree0):
        def query(self, x, k=1):
            d, i = KDTree0.query(self, x, k=k)
            rec['nearest'] = np.asarray(i, np.int32)
            return d, i

    D.fps_rad, D.recenter, D.KDTree = fps_rad, recenter, KDTree
    cam = (synthetic.demo_cam_params(), synthetic.demo_cam_extrinsics())
    res = {'cases': np.array([[s, 0 if ph == 'train' else 1, i] for s, ph, i in CASES], np.int64),
           'episodes': np.array([EPISODES['n_episode'], EPISODES['n_timestep'], EPISODES['seed']], np.int64)}
    with tempfile.TemporaryDirectory() as d:
        synthetic.write_episodes(d, **EPISODES)
        for k, (seed, phase, idx) in enumerate(CASES):
            ds = D.ParticleDataset(d, CONFIG, phase, cam)
            np.random.seed(seed)
            states, sdelta, attrs, n, den, _ = ds[idx]
            print('case %d: seed %d %s[%d] den %.1f n_fg %d particles %d' % (k, seed, phase, idx, den, rec['n_fg'], n))
            p = 'c%d_' % k
            res[p + 'n_fg'] = np.int64(rec['n_fg'])
            res[p + 'init'] = np.int64(rec['init'])
            res[p + 'chosen'] = rec['chosen']
            res[p + 'recenter'] = rec['recenter']
            res[p + 'nearest'] = rec['nearest']
            res[p + 'states'] = states.numpy()
            res[p + 'states_delta'] = sdelta.numpy()
            res[p + 'particle_num'] = np.int64(n)
            res[p + 'particle_den'] = np.float64(den)
    save_npz(out, res)
    print('wrote', out, os.path.getsize(out), 'bytes')


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else '../reference')

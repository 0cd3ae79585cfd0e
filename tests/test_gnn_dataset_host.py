"""CPU: the GNN dataset's host side (row x4) -- the float64 restatement (tests/_gnn_dataset_ref.py) against the reference's
own __getitem__ (tests/golden/gnn_dataset.npz), the phase split and index mapping, the host foreground count, the push
frames, and the refusals that need no GPU."""
import copy
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))


@pytest.fixture(scope='module')
def episodes(tmp_path_factory):
    import make_golden_gnn_dataset as mk
    from dyn_res_pile_manip_amd import synthetic
    d = str(tmp_path_factory.mktemp('gnn_episodes_host'))
    synthetic.write_episodes(d, **mk.EPISODES)
    return d


def _ds(d, phase='train', **over):
    import make_golden_gnn_dataset as mk
    from dyn_res_pile_manip_amd import synthetic
    from dyn_res_pile_manip_amd.dataset_gnn_dyn import ParticleDataset
    cfg = copy.deepcopy(mk.CONFIG)
    for k, v in over.items():
        cfg['train' if k == 'train_valid_ratio' else 'dataset'][k] = v
    return ParticleDataset(d, cfg, phase, (synthetic.demo_cam_params(), synthetic.demo_cam_extrinsics()))


def test_restatement_matches_reference(golden, episodes):
    import _gnn_dataset_ref as R
    g = golden.gnn_dataset
    for k, (seed, ph, idx) in enumerate(g['cases']):
        ds = _ds(episodes, 'train' if ph == 0 else 'valid')
        p = 'c%d_' % k
        np.random.seed(int(seed))
        sample = ds.load(int(idx))
        den, init = ds.draw(sample)                        # the reference's draws, in its order
        assert den == float(g[p + 'particle_den']) and init == int(g[p + 'init'])
        assert sample['n_fg'] == int(g[p + 'n_fg'])        # host count = the reference's cloud size
        r = R.sample(ds, int(idx), den, init)
        assert r['n_fg'] == int(g[p + 'n_fg'])
        np.testing.assert_array_equal(r['chosen'], g[p + 'chosen'])
        assert r['particle_num'] == int(g[p + 'particle_num'])
        np.testing.assert_array_equal(r['recenter'], g[p + 'recenter'])
        np.testing.assert_array_equal(r['nearest'], g[p + 'nearest'])
        np.testing.assert_array_equal(r['states'], g[p + 'states'])
        np.testing.assert_array_equal(r['states_delta'], g[p + 'states_delta'])


def test_phase_split_and_index_mapping(episodes):
    tr, va = _ds(episodes, 'train'), _ds(episodes, 'valid')
    # n_episode 4, ratio 0.5, 7 frames, n_his + n_roll = 6: two windows per episode
    assert len(tr) == 4 and len(va) == 4
    assert [tr.locate(i) for i in range(4)] == [(0, 0), (0, 1), (1, 0), (1, 1)]
    assert [va.locate(i) for i in range(4)] == [(2, 0), (2, 1), (3, 0), (3, 1)]
    assert len(_ds(episodes, 'train', train_valid_ratio=0.9)) == 6
    with pytest.raises(AssertionError):
        _ds(episodes, 'test')
    with pytest.raises(IndexError):
        tr.locate(4)


def test_read_particles_and_push_frame_follow_the_reference(episodes):
    from dyn_res_pile_manip_amd import synthetic
    from dyn_res_pile_manip_amd.dataset_gnn_dyn import push_frame
    ds = _ds(episodes)
    ext, gs = synthetic.demo_cam_extrinsics(), 24
    path = os.path.join(episodes, '0', '3_particles.npy')
    raw = np.load(path).reshape(-1, 4)
    raw[:, 3] = 1.0
    opencv_T_opengl = np.array([[1, 0, 0, 0], [0, -1, 0, 0], [0, 0, -1, 0], [0, 0, 0, 1]])
    opencv_T_world = np.matmul(np.linalg.inv(ext), opencv_T_opengl)
    ref = np.matmul(np.linalg.inv(opencv_T_world), raw.T).T[:, :3] / gs       # dataset_gnn_dyn.py:69-78
    np.testing.assert_array_equal(ds.read_particles(path), ref)
    for act in ([3.0, -1.0, -0.5, 2.0], [-4.0, 4.0, 1.0, 1.0]):
        s, e = np.array(act[:2]), np.array(act[2:])
        def o2c(p):
            return np.matmul(np.linalg.inv(opencv_T_world), np.concatenate([p, np.ones((1, 1))], 1).T).T[:, :3] / gs
        s_cam, e_cam = o2c(np.array([[s[0], 0.0, -s[1]]]))[0], o2c(np.array([[e[0], 0.0, -e[1]]]))[0]
        d = e_cam - s_cam
        pf = push_frame(np.array(act), ext, gs)
        np.testing.assert_array_equal(pf, np.concatenate([s_cam, e_cam, d / np.linalg.norm(d), [np.linalg.norm(d)]]))
        assert abs(pf[8]) < 1e-6
    assert np.isnan(push_frame(np.array([1.0, 1.0, 1.0, 1.0]), ext, gs)[6:9]).all()   # the reference exits there


def test_host_foreground_count(episodes):
    from dyn_res_pile_manip_amd.dataset_gnn_dyn import count_fg, read_depth
    d = read_depth(os.path.join(episodes, '1', '0_depth.png'))
    assert d.dtype == np.uint16 and d.shape == (720, 720)
    depth = d / (24 * 1000.0)
    assert count_fg(d, 24) == int(np.logical_and(depth < 0.599 / 0.8, depth > 0).sum())
    edge = np.array([[0, 17970, 17971, 17969, 65535]], np.uint16)   # 0.599/0.8 * 24000 = 17970.000...
    e = edge / 24000.0
    assert count_fg(edge, 24) == int(((e < 0.599 / 0.8) & (e > 0)).sum())


def test_loader_refuses_bad_configs_without_gpu(episodes):
    from dyn_res_pile_manip_amd.dataset_gnn_dyn import DeviceLoader
    ds = _ds(episodes)
    for kw in ({'batch_size': 0}, {'batch_size': 4, 'chunk': 0}, {'batch_size': 4, 'chunk': 2000},
               {'batch_size': 4, 'threads': 17}, {'batch_size': 4, 'threads': 0}):
        with pytest.raises(ValueError):
            DeviceLoader(ds, **kw)
    with pytest.raises(ValueError):
        ds.get_batch([])
    with pytest.raises(ValueError):
        ds.get_batch([0] * 1025)
    assert len(DeviceLoader(ds, 3)) == 2 and len(DeviceLoader(ds, 3, drop_last=True)) == 1


def test_episode_writer_layout(episodes):
    import pickle
    from PIL import Image
    ep = os.path.join(episodes, '2')
    names = sorted(os.listdir(ep))
    assert 'actions.p' in names and len(names) == 1 + 3 * 7
    with open(os.path.join(ep, 'actions.p'), 'rb') as f:
        acts = pickle.load(f)
    assert acts.shape == (6, 4) and acts.dtype == np.float64
    p = np.load(os.path.join(ep, '0_particles.npy'))
    assert p.dtype == np.float32 and p.shape[1] == 4 and (p[:, 3] == 1).all()
    with Image.open(os.path.join(ep, '0_color.png')) as im:
        assert im.mode == 'RGB' and im.size == (720, 720)

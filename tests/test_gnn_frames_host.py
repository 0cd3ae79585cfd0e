"""CPU: untracked samples straight from depth frames (row x4 / u1), the host side -- the float64 restatement
(tests/_gnn_dataset_ref.py) against the reference's own chain on every frame (tests/golden/gnn_frames.npz,
tests/golden/make_golden_gnn_frames.py), DepthDataset on episodes without particle and colour files, its draw order, the
depth_only refusals and the --data depth flag logic."""
import copy
import os
import shutil
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))


@pytest.fixture(scope='module')
def episodes(tmp_path_factory):
    """(the fixture's episodes as written, a copy that holds only the depth PNGs and actions.p)"""
    import make_golden_gnn_frames as mk
    from dyn_res_pile_manip_amd import synthetic
    full = str(tmp_path_factory.mktemp('gnn_frames_host'))
    synthetic.write_episodes(full, **mk.EPISODES)
    bare = str(tmp_path_factory.mktemp('gnn_frames_host_bare'))
    for ep in os.listdir(full):
        os.makedirs(os.path.join(bare, ep))
        for f in os.listdir(os.path.join(full, ep)):
            if not (f.endswith('_particles.npy') or f.endswith('_color.png')):
                shutil.copy(os.path.join(full, ep, f), os.path.join(bare, ep, f))
    return full, bare


def _cam():
    from dyn_res_pile_manip_amd import synthetic
    return (synthetic.demo_cam_params(), synthetic.demo_cam_extrinsics())


def _ds(d, phase='train', cls=None, **kw):
    import make_golden_gnn_frames as mk
    from dyn_res_pile_manip_amd.dataset_gnn_dyn import DepthDataset
    return (cls or DepthDataset)(d, copy.deepcopy(mk.CONFIG), phase, _cam(), **kw)


class NumpyEngine(object):
    """Engine.ptcl_dataset_frames by the numpy restatement: what the device call must give, for the host-side tests"""

    def ptcl_dataset_frames(self, depth, global_scale, cam_params, radius, init_idx, n_fg, episode=None):
        import _gnn_dataset_ref as R
        B, T = depth.shape[:2]
        clouds = [[None] * T for _ in range(B)]
        for b in range(B):
            for t in range(T):
                pcd = R.depth_cloud(depth[b, t], global_scale, cam_params)
                assert pcd.shape[0] == n_fg[b][t]
                ch = R.fps_rad_idx(pcd, radius[b][t], init_idx[b][t])
                clouds[b][t] = R.recenter(pcd, pcd[ch], min(0.02, 0.5 * radius[b][t])).astype(np.float32)
        counts = np.array([[len(c) for c in row] for row in clouds], np.int32)
        out = np.zeros((B, T, counts.max(), 3), np.float32)
        for b in range(B):
            for t in range(T):
                out[b, t, :counts[b, t]] = clouds[b][t]
        return out, counts


def test_restatement_matches_reference_on_every_frame(golden, episodes):
    import _gnn_dataset_ref as R
    g = golden.gnn_frames
    assert len(g['cases']) == 6 and (g['scales'] != 1.0).sum() == 1
    dens = [float(g['c%d_den' % k]) for k in range(6)]
    assert min(dens) < 83 and max(dens) > 6286                              # the densities span 82 .. 6286
    for k, (seed, ph, idx) in enumerate(g['cases']):
        ds = _ds(episodes[1], 'train' if ph == 0 else 'valid', target_den_scale=float(g['scales'][k]))
        p = 'c%d_' % k
        np.random.seed(int(seed))
        sample = ds.load(int(idx))
        den, init = ds.draw(sample)                                         # DepthDataset's draws = the generator's
        assert den == float(g[p + 'den'])
        np.testing.assert_array_equal(init, g[p + 'init'])
        np.testing.assert_array_equal(sample['n_fg'], g[p + 'n_fg'])
        radius = ds.radii(den, len(init))
        assert radius[0] == 1 / np.sqrt(den) and radius[1] == 1 / np.sqrt(den * float(g['scales'][k]))
        ends = np.cumsum(g[p + 'counts'])
        for t in range(len(init)):
            pcd = R.depth_cloud(sample['depth'][t], ds.global_scale, ds.cam_params)
            assert pcd.shape[0] == int(g[p + 'n_fg'][t])
            ch = R.fps_rad_idx(pcd, radius[t], init[t])
            lo, hi = int(ends[t] - g[p + 'counts'][t]), int(ends[t])
            np.testing.assert_array_equal(ch, g[p + 'chosen'][lo:hi])
            np.testing.assert_array_equal(R.recenter(pcd, pcd[ch], min(0.02, 0.5 * radius[t])), g[p + 'recenter'][lo:hi])


def test_load_needs_only_depth_and_actions(episodes):
    full, bare = episodes
    names = sorted(os.listdir(os.path.join(bare, '0')))
    assert len(names) == 1 + 7 and not [n for n in names if 'particles' in n or 'color' in n]
    ds, ref = _ds(bare), _ds(full)
    assert len(ds) == 4 and [ds.locate(i) for i in range(4)] == [(0, 0), (0, 1), (1, 0), (1, 1)]
    assert len(_ds(bare, 'valid')) == 4 and _ds(bare, 'valid').locate(3) == (3, 1)
    s = ds.load(3)
    assert s['episode'] == 1 and s['depth'].shape == (6, 720, 720) and s['depth'].dtype == np.uint16
    assert len(s['n_fg']) == 6 and s['actions'].shape == (5, 4) and s['color'] is None
    np.testing.assert_array_equal(s['depth'], ref.load(3)['depth'])
    from dyn_res_pile_manip_amd.dataset_gnn_dyn import ParticleDataset
    tracked = _ds(full, cls=ParticleDataset).load(3)
    np.testing.assert_array_equal(s['depth'][0], tracked['depth'])          # frame 0 is ParticleDataset's depth image
    np.testing.assert_array_equal(s['actions'], tracked['actions'])
    assert s['n_fg'][0] == tracked['n_fg']
    with pytest.raises(FileNotFoundError):
        _ds(bare, cls=ParticleDataset).load(3)                               # the tracked path does need the particle files
    with pytest.raises(ValueError):
        _ds(bare, target_den_scale=0.0)


def test_draw_order_and_first_sample_agrees_with_particle_dataset(episodes, monkeypatch):
    from dyn_res_pile_manip_amd.dataset_gnn_dyn import ParticleDataset
    full, bare = episodes
    ds = _ds(bare)
    s = ds.load(0)
    calls = []
    uniform0, randint0 = np.random.uniform, np.random.randint
    monkeypatch.setattr(np.random, 'uniform', lambda *a: calls.append(('uniform',) + a) or uniform0(*a))
    monkeypatch.setattr(np.random, 'randint', lambda *a: calls.append(('randint',) + a) or randint0(*a))
    np.random.seed(3)
    den, init = ds.draw(s)
    assert calls == [('uniform', 15, 6500)] + [('randint', n) for n in s['n_fg']]     # den, then the frames in order
    assert len(init) == 6 and all(0 <= i < n for i, n in zip(init, s['n_fg']))
    monkeypatch.undo()
    np.random.seed(3)
    den_p, init_p = ParticleDataset.draw(_ds(full, cls=ParticleDataset).load(0))
    assert (den, init[0]) == (den_p, init_p)
    np.random.seed(3)
    assert np.random.uniform(15, 6500) == den and [np.random.randint(n) for n in s['n_fg']] == init
    # a frame without foreground draws nothing (the device refuses it)
    np.random.seed(3)
    _, init_e = ds.draw(dict(s, n_fg=[s['n_fg'][0], 0] + s['n_fg'][2:]))
    assert init_e[1] == 0 and init_e[0] == init[0]


def test_samples_and_batches_have_collate_untracked_layout(episodes):
    from dyn_res_pile_manip_amd.dataset_gnn_dyn import DeviceLoader
    from dyn_res_pile_manip_amd.train_gnn_dyn import collate_untracked
    ds = _ds(episodes[1], engine=NumpyEngine())
    np.random.seed(9)                                                       # den 82: a handful of particles per frame
    item = ds[0]
    states, sdelta, attrs, n, den, color, targets = item
    T = 6
    assert states.shape == (T, n, 3) and states.dtype == np.float32 and states[0].any() and not states[1:].any()
    assert sdelta.shape == (T - 1, n, 3) and not sdelta.any() and attrs.shape == (T, n) and not attrs.any()
    assert color is None and len(targets) == T - 1 and all(t.ndim == 2 and t.shape[1] == 3 for t in targets)
    np.random.seed(9)
    assert den == np.random.uniform(15, 6500)
    np.random.seed(9)
    batch = ds.get_batch([0])
    assert batch.depth_only is True and len(batch) == 8
    ref = collate_untracked([item], actions=ds.load(0)['actions'][None])
    for a, b in zip(batch, ref):
        assert (a is None and b is None) or (np.asarray(a).dtype == np.asarray(b).dtype and np.array_equal(a, b))
    np.testing.assert_array_equal(batch.actions, ref.actions)
    assert batch.actions.shape == (1, T - 1, 4) and batch.actions.dtype == np.float32
    np.testing.assert_array_equal(batch[7][0], [len(t) for t in targets])
    assert DeviceLoader(ds, 2).chunk == 16                                  # the smaller default chunk of T-image samples
    with pytest.raises(ValueError):
        ds.get_batch([])
    with pytest.raises(ValueError):
        ds.get_batch([0] * 171)                                             # 171 x 6 frames > 1024 images


def test_depth_only_batches_are_refused_without_chamfer_and_actions():
    from dyn_res_pile_manip_amd import train_gnn_dyn as TG
    z = np.zeros
    batch = TG.PaddedBatch((z((1, 3, 4, 3), np.float32), z((1, 2, 4, 3), np.float32), z((1, 3, 4), np.float32),
                            np.array([4], np.int32), np.array([100.0], np.float32), None, z((1, 2, 5, 3), np.float32),
                            np.array([[5, 5]], np.int32)))
    batch.actions = z((1, 2, 4), np.float32)
    batch.depth_only = True
    for loss, impulses in (('mse', 'data'), ('mse', 'actions'), ('chamfer', 'data')):
        with pytest.raises(ValueError, match='depth-only'):
            TG.run_batch(None, None, batch, 'train', 2, loss=loss, impulses=impulses)
        with pytest.raises(ValueError, match='depth-only'):
            TG.run_batch(None, None, batch, 'valid', 2, loss=loss, impulses=impulses)
        with pytest.raises(ValueError, match='depth-only'):
            TG.probe_batch(None, batch, impulses=impulses, loss=loss)
    with pytest.raises(ValueError, match='depth-only'):
        TG.run_batch(None, None, batch)                                     # the defaults are 'mse' / 'data'
    TG.check_depth_only(batch, 'chamfer', 'actions')
    batch.depth_only = False
    TG.check_depth_only(batch, 'mse', 'data')                               # an ordinary batch is not concerned
    assert TG.PaddedBatch(()).depth_only is False


def test_data_depth_flag_logic(tmp_path):
    from dyn_res_pile_manip_amd import train_gnn_dyn as TG
    R = TG.resolve_data_options
    assert R('particles', None, None) == ('mse', 'data')
    assert R('particles', 'chamfer', None) == ('chamfer', 'data')
    assert R('particles', 'mse', 'actions') == ('mse', 'actions')
    assert R('depth', None, None) == ('chamfer', 'actions')
    assert R('depth', 'chamfer', None) == R('depth', None, 'actions') == R('depth', 'chamfer', 'actions') == ('chamfer', 'actions')
    for loss, impulses in (('mse', None), (None, 'data'), ('mse', 'data'), ('chamfer', 'data'), ('mse', 'actions')):
        with pytest.raises(ValueError, match='contradicts'):
            R('depth', loss, impulses)
    with pytest.raises(ValueError):
        R('rgb', None, None)
    # main() refuses before it touches the disk or a device; the command line refuses with argparse's exit
    cfg = TG.default_config()
    with pytest.raises(ValueError, match='contradicts'):
        TG.main(cfg, data_root=str(tmp_path), train_dir=str(tmp_path / 'run'), data='depth', loss='mse')
    with pytest.raises(ValueError, match='contradicts'):
        TG.main(cfg, data_root=str(tmp_path), train_dir=str(tmp_path / 'run'), data='depth', impulses='data')
    with pytest.raises(ValueError):                                         # grad_probe_every pairs with MSE: depth implies Chamfer
        TG.main(cfg, data_root=str(tmp_path), train_dir=str(tmp_path / 'run'), data='depth', grad_probe_every=1)
    assert not (tmp_path / 'run').exists()
    for argv in (['--data', 'depth', '--loss', 'mse'], ['--data', 'depth', '--impulses', 'data'], ['--data', 'video']):
        with pytest.raises(SystemExit) as ei:
            TG._cli(argv)
        assert ei.value.code == 2


def test_the_dataset_calls_host_arithmetic_passes_its_check_program(tmp_path):
    """csrc/ptcl_dataset_host.h (arena layout, per-image checks) is plain C++: tools/ptcl_dataset_host_check.cpp built for the host"""
    import subprocess
    import __graft_entry__ as g
    exe = str(tmp_path / 'ptcl_dataset_host_check')
    subprocess.check_call([g.HIPCC, '-x', 'c++', '-std=c++17', '-O1', os.path.join(ROOT, 'tools', 'ptcl_dataset_host_check.cpp'), '-o', exe])
    assert 'all checks passed' in subprocess.check_output([exe]).decode()

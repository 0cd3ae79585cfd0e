"""GPU: untracked samples straight from recorded depth frames (row x4 / u1, drp_ptcl_dataset_frames) against the reference's
own depth2fgpcd -> fps_rad -> recenter on every frame (tests/golden/gnn_frames.npz, tests/golden/make_golden_gnn_frames.py),
against drp_ptcl_dataset_batch on frame 0, composition over frames, samples and chunks, small crafted images against the numpy
restatement (tests/_gnn_dataset_ref.py), the sampler's properties, refusals, isolation, and main(data='depth') end to end.

Every comparison is exact: the chain is float64 in the reference's evaluation order with one final rounding to float32."""
import copy
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

pytestmark = pytest.mark.gpu
SMALL_CAM = [30.0, 28.0, 16.0, 20.0]      # intrinsics for the crafted 40 x 33 images: neighbouring pixels lie ~ 0.02 apart


@pytest.fixture(scope='module')
def eng():
    import __graft_entry__ as g
    g.build()
    from dyn_res_pile_manip_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope='module')
def tracked_episodes(tmp_path_factory):
    """the fixture's episodes as written, particle files included (the existing path needs them)"""
    import make_golden_gnn_frames as mk
    from dyn_res_pile_manip_amd import synthetic
    d = str(tmp_path_factory.mktemp('gnn_frames_tracked'))
    synthetic.write_episodes(d, **mk.EPISODES)
    return d


@pytest.fixture(scope='module')
def episodes(tracked_episodes, tmp_path_factory):
    """the same episodes without any particle or colour file: depth PNGs and actions.p alone"""
    import shutil
    d = str(tmp_path_factory.mktemp('gnn_frames'))
    for ep in os.listdir(tracked_episodes):
        os.makedirs(os.path.join(d, ep))
        for f in os.listdir(os.path.join(tracked_episodes, ep)):
            if not (f.endswith('_particles.npy') or f.endswith('_color.png')):
                shutil.copy(os.path.join(tracked_episodes, ep, f), os.path.join(d, ep, f))
    return d


def _cam():
    from dyn_res_pile_manip_amd import synthetic
    return (synthetic.demo_cam_params(), synthetic.demo_cam_extrinsics())


def _ds(d, eng, phase='train', ratio=None, cls=None, **kw):
    import make_golden_gnn_frames as mk
    from dyn_res_pile_manip_amd.dataset_gnn_dyn import DepthDataset
    cfg = copy.deepcopy(mk.CONFIG)
    if ratio is not None:
        cfg['train']['train_valid_ratio'] = ratio
    return (cls or DepthDataset)(d, cfg, phase, _cam(), engine=eng, **kw)


def _bits(a, b):
    """same dtype, shape and bytes (so that -0.0 and +0.0 differ)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    assert a.tobytes() == b.tobytes(), np.argwhere(a != b)[:5]


def _check_against_numpy(eng, depth, gs, cam, radius, init):
    """one frames call against the restatement, frame by frame: counts, picks, float64 recentered points, float32 clouds"""
    import _gnn_dataset_ref as R
    depth, radius, init = np.asarray(depth), np.asarray(radius, np.float64), np.asarray(init)
    B, T = depth.shape[:2]
    n_fg = np.array([[R.depth_cloud(depth[b, t], gs, cam).shape[0] for t in range(T)] for b in range(B)])
    clouds, counts = eng.ptcl_dataset_frames(depth, gs, cam, radius, init, n_fg)
    np.testing.assert_array_equal(eng.ptcl_dataset_frames_tap('nfg'), n_fg)
    chosen, rec = eng.ptcl_dataset_frames_tap('chosen'), eng.ptcl_dataset_frames_tap('recenter')
    want_counts = np.zeros((B, T), np.int32)
    for b in range(B):
        for t in range(T):
            pcd = R.depth_cloud(depth[b, t], gs, cam)
            ch = R.fps_rad_idx(pcd, radius[b, t], int(init[b, t]))
            want_counts[b, t] = n = len(ch)
            assert counts[b, t] == n, (b, t, counts[b, t], n)
            np.testing.assert_array_equal(chosen[b, t, :n], ch)
            want = R.recenter(pcd, pcd[ch], min(0.02, 0.5 * radius[b, t]))
            _bits(rec[b, t, :n], want)
            _bits(clouds[b, t, :n], want.astype(np.float32))
            _bits(clouds[b, t, n:], np.zeros((clouds.shape[2] - n, 3), np.float32))
    assert clouds.shape == (B, T, want_counts.max(), 3) and counts.dtype == np.int32
    return clouds, counts


# ---- 1: against the reference ----------------------------------------------------------------------------------------------
def test_matches_reference_fixture_on_every_frame(golden, episodes, eng):
    g = golden.gnn_frames
    for k, (seed, ph, idx) in enumerate(g['cases']):
        ds = _ds(episodes, eng, 'train' if ph == 0 else 'valid', target_den_scale=float(g['scales'][k]))
        p = 'c%d_' % k
        np.random.seed(int(seed))
        s = ds.load(int(idx))
        den, init = ds.draw(s)
        assert den == float(g[p + 'den'])                                  # the same draws, exactly
        np.testing.assert_array_equal(init, g[p + 'init'])
        clouds, counts = ds.run([s], [(den, init)])
        np.testing.assert_array_equal(counts[0], g[p + 'counts'])
        np.testing.assert_array_equal(eng.ptcl_dataset_frames_tap('nfg')[0], g[p + 'n_fg'])
        chosen, rec = eng.ptcl_dataset_frames_tap('chosen')[0], eng.ptcl_dataset_frames_tap('recenter')[0]
        assert clouds.shape == (1, len(init), int(g[p + 'counts'].max()), 3)
        ends = np.cumsum(g[p + 'counts'])
        for t in range(len(init)):
            n = int(g[p + 'counts'][t])
            lo, hi = int(ends[t]) - n, int(ends[t])
            np.testing.assert_array_equal(chosen[t, :n], g[p + 'chosen'][lo:hi])
            _bits(rec[t, :n], g[p + 'recenter'][lo:hi])
            _bits(clouds[0, t, :n], g[p + 'recenter'][lo:hi].astype(np.float32))
            _bits(clouds[0, t, n:], np.zeros((clouds.shape[2] - n, 3), np.float32))


# ---- 2: against the existing path ------------------------------------------------------------------------------------------
def test_frame_zero_equals_ptcl_dataset_batch(tracked_episodes, eng):
    from dyn_res_pile_manip_amd.dataset_gnn_dyn import ParticleDataset
    pds = _ds(tracked_episodes, eng, ratio=1.0, cls=ParticleDataset)
    dds = _ds(tracked_episodes, eng, ratio=1.0)
    for seed, idx in ((9, 0), (11, 3)):
        np.random.seed(seed)
        ps = pds.load(idx)
        den_p, init_p = pds.draw(ps)
        _, _, n = pds.run([ps], [(den_p, init_p)])
        n = int(n[0])
        chosen_p = eng.ptcl_dataset_tap('chosen')[0, :n].copy()
        rec_p = eng.ptcl_dataset_tap('recenter')[0, :n].copy()
        np.random.seed(seed)
        s = dds.load(idx)
        den, init = dds.draw(s)
        assert (den, init[0]) == (den_p, init_p)
        clouds, counts = dds.run([s], [(den, init)])
        assert counts[0, 0] == n
        _bits(eng.ptcl_dataset_frames_tap('chosen')[0, 0, :n], chosen_p)
        _bits(eng.ptcl_dataset_frames_tap('recenter')[0, 0, :n], rec_p)
        _bits(clouds[0, 0, :n], rec_p.astype(np.float32))


# ---- 3: composition --------------------------------------------------------------------------------------------------------
def _four(ds):
    samples = [ds.load(i) for i in range(4)]
    dens = (300.0, 2100.0, 82.0, 4700.0)
    draws = [(den, [(7919 * (b + 1) * (t + 3)) % n for t, n in enumerate(s['n_fg'])]) for b, (den, s) in enumerate(zip(dens, samples))]
    return samples, draws


def test_frames_samples_permutations_and_repeats_compose(episodes, eng):
    ds = _ds(episodes, eng, ratio=1.0, target_den_scale=1.5)
    samples, draws = _four(ds)
    clouds, counts = ds.run(samples, draws)
    B, T = counts.shape
    assert (B, T) == (4, 6) and len(set(counts.ravel().tolist())) > 8          # ragged [B][T] counts
    chosen, rec = eng.ptcl_dataset_frames_tap('chosen'), eng.ptcl_dataset_frames_tap('recenter')

    def same(b, t, cl, cn, ch, rc, bb=0, tt=0):
        n = int(counts[b, t])
        assert cn[bb, tt] == n
        _bits(cl[bb, tt, :n], clouds[b, t, :n])
        assert not cl[bb, tt, n:].any() and not np.signbit(cl[bb, tt, n:]).any()
        _bits(ch[bb, tt, :n], chosen[b, t, :n])
        _bits(rc[bb, tt, :n], rec[b, t, :n])

    taps = lambda: (eng.ptcl_dataset_frames_tap('chosen'), eng.ptcl_dataset_frames_tap('recenter'))
    # two runs give the same bits
    again = ds.run(samples, draws)
    _bits(again[0], clouds)
    _bits(again[1], counts)
    # every frame of the T = 6 call equals a T = 1 call on that frame alone (two samples: twelve calls)
    for b in (1, 2):
        s, (den, init) = samples[b], draws[b]
        radius = ds.radii(den, T)
        for t in range(T):
            cl, cn = eng.ptcl_dataset_frames(s['depth'][None, t:t + 1], ds.global_scale, ds.cam_params, [[radius[t]]], [[init[t]]],
                                             [[s['n_fg'][t]]])
            same(b, t, cl, cn, *taps())
    # a batch equals its samples one by one
    for b in range(B):
        cl, cn = ds.run([samples[b]], [draws[b]])
        ch, rc = taps()
        for t in range(T):
            same(b, t, cl, cn, ch, rc, 0, t)
    # permuting the samples only permutes the result
    perm = [2, 0, 3, 1]
    cl, cn = ds.run([samples[i] for i in perm], [draws[i] for i in perm])
    ch, rc = taps()
    assert cl.shape == clouds.shape
    for j, b in enumerate(perm):
        for t in range(T):
            same(b, t, cl, cn, ch, rc, j, t)


def test_loader_chunk_sizes_give_the_same_batches(episodes, eng):
    import torch
    from dyn_res_pile_manip_amd.dataset_gnn_dyn import DeviceLoader
    ds = _ds(episodes, eng, ratio=1.0)
    assert len(ds) == 8
    runs = []
    for chunk in (1, 3, 16):
        torch.manual_seed(5)
        np.random.seed(5)
        runs.append(list(DeviceLoader(ds, 3, shuffle=True, chunk=chunk, threads=4)))
    assert [len(r) for r in runs] == [3, 3, 3] and [len(b[3]) for b in runs[0]] == [3, 3, 2]
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert len(a) == len(b) == 8 and a.depth_only is True and b.depth_only is True
            for x, y in zip(a, b):
                if x is not None:
                    _bits(x, y)
            _bits(a.actions, b.actions)
            np.testing.assert_array_equal(a.offsets, b.offsets)
    # the order is torch's DataLoader over the indices, the draws one numpy stream in sample order: get_batch on the same order
    torch.manual_seed(5)
    np.random.seed(5)
    order = DeviceLoader(ds, 3, shuffle=True).index_batches()
    first = ds.get_batch(order[0])
    for x, y in zip(first, runs[0][0]):
        if x is not None:
            _bits(x, y)
    b0 = runs[0][0]
    assert b0[0].shape[1] == 6 and b0[0][:, 0].any() and not b0[0][:, 1:].any() and not b0[1].any() and not b0[2].any()
    assert b0[6].shape[:2] == (3, 5) and b0[7].shape == (3, 5) and b0.actions.shape == (3, 5, 4)


# ---- 4: small crafted images against the numpy restatement -----------------------------------------------------------------
def _crafted(n_fg, seed, h=40, w=33):
    """a uint16 depth image with exactly n_fg foreground pixels at random places (h * w = 1320: no multiple of the 1024-pixel
    tile); the rest is 0 or beyond the depth threshold"""
    rng = np.random.default_rng(seed)
    img = np.where(rng.random(h * w) < 0.5, 0, rng.integers(17971, 30000, h * w)).astype(np.uint16)
    img[rng.permutation(h * w)[:n_fg]] = rng.integers(12000, 17000, n_fg)
    return img.reshape(h, w)


def test_crafted_images_against_the_restatement(eng):
    # one foreground pixel | the sampler's thread stride 1023, 1024, 1025 | every pixel | frames of very different n_fg and
    # radii in one sample | a radius that covers the whole cloud (the last frame of sample 1)
    n_fg = [[1, 1023, 1024, 1025], [1320, 50, 700, 400]]
    depth = np.stack([np.stack([_crafted(n, 10 * b + t) for t, n in enumerate(row)]) for b, row in enumerate(n_fg)])
    radius = [[0.05, 0.11, 0.07, 0.25], [0.04, 0.3, 0.013, 10.0]]
    init = [[0, 1022, 1023, 1024], [1319, 49, 0, 123]]
    clouds, counts = _check_against_numpy(eng, depth, 24, SMALL_CAM, radius, init)
    assert counts[0, 0] == 1 and counts[1, 3] == 1 and counts.max() > 300 and len(set(counts.ravel().tolist())) >= 6
    import _gnn_dataset_ref as R
    # the single pixel is its own recentered point
    _bits(clouds[0, 0, 0], R.depth_cloud(depth[0, 0], 24, SMALL_CAM)[0].astype(np.float32))
    # B * T = 1, on each kind of frame
    for b, t in ((0, 0), (0, 3), (1, 0)):
        cl, cn = _check_against_numpy(eng, depth[b:b + 1, t:t + 1], 24, SMALL_CAM, [[radius[b][t]]], [[init[b][t]]])
        n = int(counts[b, t])
        assert cn[0, 0] == n
        _bits(cl[0, 0], clouds[b, t, :cl.shape[2]])
    # T = 1 with many samples, and a wide image whose rows are no multiple of anything
    wide = np.stack([_crafted(n, 50 + i, h=7, w=211)[None] for i, n in enumerate((3, 900, 1477, 64, 1))])
    _check_against_numpy(eng, wide, 24, [90.0, 90.0, 100.0, 3.0], [[0.03], [0.05], [0.02], [0.2], [1.0]], [[2], [0], [1476], [63], [0]])


# ---- 5: properties ---------------------------------------------------------------------------------------------------------
def test_every_point_is_covered_and_recentering_stays_in_its_ball(episodes, eng):
    import _gnn_dataset_ref as R
    ds = _ds(episodes, eng, 'valid', target_den_scale=0.5)
    samples = [ds.load(0), ds.load(3)]
    draws = [(430.0, [n // 2 for n in samples[0]['n_fg']]), (950.0, [n - 1 for n in samples[1]['n_fg']])]   # no fixture's densities
    clouds, counts = ds.run(samples, draws)
    chosen, rec = eng.ptcl_dataset_frames_tap('chosen'), eng.ptcl_dataset_frames_tap('recenter')
    for b, (s, (den, init)) in enumerate(zip(samples, draws)):
        radius = ds.radii(den, len(init))
        assert radius[1] == 1 / np.sqrt(den * 0.5) > radius[0]
        for t in range(len(init)):
            n = int(counts[b, t])
            pcd = R.depth_cloud(s['depth'][t], ds.global_scale, ds.cam_params)
            ch = chosen[b, t, :n]
            assert ch[0] == init[t] and len(set(ch.tolist())) == n and ch.min() >= 0 and ch.max() < pcd.shape[0]
            dist = np.full((pcd.shape[0],), np.inf)
            for c in ch:
                dist = np.minimum(dist, np.linalg.norm(pcd - pcd[c], axis=1))
            assert dist.max() <= radius[t]                                  # the sampler's loop exit, in float64
            r = min(0.02, 0.5 * radius[t])
            assert np.linalg.norm(rec[b, t, :n] - pcd[ch], axis=1).max() <= r
            assert np.isfinite(clouds[b, t]).all()


# ---- 6: refusals -----------------------------------------------------------------------------------------------------------
def test_refusals_name_episode_and_frame_and_leave_the_context_usable(eng):
    from dyn_res_pile_manip_amd import _lib
    n_fg = np.array([[500, 300, 640], [64, 900, 1100]])
    depth = np.stack([np.stack([_crafted(n, 100 + 10 * b + t) for t, n in enumerate(row)]) for b, row in enumerate(n_fg)])
    radius = np.array([[0.05, 0.07, 0.04], [0.1, 0.03, 0.06]])
    init = np.array([[3, 299, 0], [63, 10, 555]])
    episode = [41, 57]
    call = lambda **kw: eng.ptcl_dataset_frames(**dict(dict(depth=depth, global_scale=24, cam_params=SMALL_CAM, radius=radius,
                                                            init_idx=init, n_fg=n_fg, episode=episode), **kw))
    good = call()
    wb, wt = np.unravel_index(good[1].argmax(), good[1].shape)          # the frame that needs the most slots

    def at(a, b, t, v):
        a = np.array(a)
        a[b, t] = v
        return a
    zeroed = depth.copy()
    zeroed[1, 1] = 0
    cases = {
        'an all-zero frame in the middle of a window': (dict(depth=zeroed, n_fg=at(n_fg, 1, 1, 0), init_idx=at(init, 1, 1, 0)), 57, 1),
        'a wrong host count for one frame': (dict(n_fg=at(n_fg, 0, 2, 639)), 41, 2),
        'a start equal to n_fg': (dict(init_idx=at(init, 1, 0, 64)), 57, 0),
        'n_cap one too small': (dict(n_cap=int(good[1].max()) - 1), episode[wb], int(wt)),
        'a zero radius': (dict(radius=at(radius, 0, 1, 0.0)), 41, 1),
        'a non-finite radius': (dict(radius=at(radius, 1, 2, np.inf)), 57, 2),
    }
    for name, (kw, ep, frame) in cases.items():
        with pytest.raises(_lib.DrpError) as ei:
            call(**kw)
        msg = str(ei.value)
        assert 'drp error %d:' % -1 in msg and 'episode %d frame %d' % (ep, frame) in msg, (name, msg)
        again = call()
        _bits(again[0], good[0])
        _bits(again[1], good[1])
    # a radius of 1e-4 on one small cloud of 5600 points reaches the cap of 4096 particles
    big = np.stack([_crafted(700, 1, h=80, w=70), _crafted(5600, 2, h=80, w=70)])[None]
    with pytest.raises(_lib.DrpError) as ei:
        eng.ptcl_dataset_frames(big, 24, SMALL_CAM, [[0.05, 1e-4]], [[0, 0]], [[700, 5600]], episode=[7])
    assert 'drp error -1:' in str(ei.value) and 'episode 7 frame 1' in str(ei.value) and 'cap of 4096' in str(ei.value)
    _bits(call()[0], good[0])
    # B * T = 1025 images, and a null argument: nothing to name there
    with pytest.raises(_lib.DrpError, match='drp error -1:.*1..1024 images'):
        eng.ptcl_dataset_frames(np.zeros((205, 5, 4, 4), np.uint16), 24, SMALL_CAM, np.ones((205, 5)), np.zeros((205, 5)), np.ones((205, 5)))
    U16, I32, F32, F64 = [ctypes.POINTER(t) for t in (ctypes.c_uint16, ctypes.c_int32, ctypes.c_float, ctypes.c_double)]
    cam = np.array(SMALL_CAM)
    init32, nfg32 = np.ascontiguousarray(init, np.int32), np.ascontiguousarray(n_fg, np.int32)
    out, cnt, nmax = np.empty((2 * 3 * 4096 * 3,), np.float32), np.empty((6,), np.int32), ctypes.c_int()
    args = [depth.ctypes.data_as(U16), cam.ctypes.data_as(F64), radius.ctypes.data_as(F64), init32.ctypes.data_as(I32),
            nfg32.ctypes.data_as(I32), out.ctypes.data_as(F32), cnt.ctypes.data_as(I32), ctypes.byref(nmax)]
    for drop in range(len(args)):
        a = [None if i == drop else v for i, v in enumerate(args)]
        rc = eng.lib.drp_ptcl_dataset_frames(eng.h, 2, 3, a[0], 40, 33, 24.0, a[1], a[2], a[3], a[4], None, 4096, a[5], a[6], a[7])
        assert rc == -1 and 'null argument' in eng.lib.drp_last_error(eng.h).decode()
    for bad in (dict(B=0), dict(T=0), dict(h=0), dict(n_cap=0), dict(gs=0.0)):
        p = dict(dict(B=2, T=3, h=40, n_cap=4096, gs=24.0), **bad)
        assert eng.lib.drp_ptcl_dataset_frames(eng.h, p['B'], p['T'], args[0], p['h'], 33, p['gs'], args[1], args[2], args[3], args[4],
                                               None, p['n_cap'], args[5], args[6], args[7]) == -1, bad
    with pytest.raises(ValueError):
        eng.ptcl_dataset_frames(depth, 24, SMALL_CAM, radius[:, :2], init, n_fg)
    again = call()
    _bits(again[0], good[0])
    _bits(again[1], good[1])


def _at(a, idx, v):
    a = np.array(a)
    a[idx] = v
    return a


def _refused_then_good(call, good, cases):
    """every input of `cases` carries two faults: (overrides, what the message says, what it does not say); after each refusal a
    good call gives the bits of the good call made before it"""
    from dyn_res_pile_manip_amd import _lib
    for kw, says, silent in cases:
        with pytest.raises(_lib.DrpError) as ei:
            call(**kw)
        msg = str(ei.value)
        assert 'drp error -1:' in msg and all(s in msg for s in says) and silent not in msg, (kw, msg)
        for x, y in zip(call(), good):
            _bits(x, y)


def test_batch_call_names_the_first_of_two_faults(eng):
    # B = 2, T = 2: five particles per frame, T_cam identity, unit in-plane pushes
    n_fg = [500, 640]
    rng = np.random.default_rng(3)
    push = np.zeros((2, 1, 10))
    push[..., 6] = push[..., 9] = 1.0
    base = dict(depth=np.stack([_crafted(n, 200 + b) for b, n in enumerate(n_fg)]), global_scale=24, cam_params=SMALL_CAM,
                T_cam=np.eye(4), particles=[rng.normal(size=(2, 5, 4)).astype(np.float32) for _ in range(2)], radius=[0.05, 0.07],
                init_idx=[3, 639], n_fg=n_fg, push=push, episode=[41, 57])
    call = lambda **kw: eng.ptcl_dataset_batch(**dict(base, **kw))
    good = call()
    assert good[0].shape[:2] == (2, 2) and good[2].min() > 1
    _refused_then_good(call, good, [
        # within a sample: the radius before the pushes
        (dict(radius=_at(base['radius'], 0, np.inf), push=_at(push, (0, 0, 9), 0.0)), ('bad fps radius', 'episode 41:'), 'push'),
        # across samples: sample 0's last check before sample 1's first
        (dict(push=_at(push, (0, 0, 8), 0.5), init_idx=_at(base['init_idx'], 1, -1)), ('leaves the table plane', 'episode 41:'),
         'sampler start'),
        # behind the counts wait: the host's count before the start
        (dict(n_fg=_at(n_fg, 1, 639), init_idx=_at(base['init_idx'], 1, 640)), ('foreground pixels on the host', 'episode 57:'),
         'sampler start'),
    ])


def test_frames_call_names_the_first_of_two_faults(eng):
    n_fg = np.array([[500, 300, 640], [64, 900, 1100]])             # B = 2, T = 3
    base = dict(depth=np.stack([np.stack([_crafted(n, 100 + 10 * b + t) for t, n in enumerate(row)]) for b, row in enumerate(n_fg)]),
                global_scale=24, cam_params=SMALL_CAM, radius=np.array([[0.05, 0.07, 0.04], [0.1, 0.03, 0.06]]),
                init_idx=np.array([[3, 299, 0], [63, 10, 555]]), n_fg=n_fg, episode=[41, 57])
    call = lambda **kw: eng.ptcl_dataset_frames(**dict(base, **kw))
    good = call()
    _refused_then_good(call, good, [
        # within an image: the start before the radius
        (dict(init_idx=_at(base['init_idx'], (0, 1), -1), radius=_at(base['radius'], (0, 1), 0.0)),
         ('sampler start', 'episode 41 frame 1:'), 'radius'),
        # across images in (b, t) order: the last check of (0, 2) before the radius of (1, 0)
        (dict(radius=_at(base['radius'], (1, 0), np.nan), n_fg=_at(n_fg, (0, 2), 40 * 33 + 1)),
         ('host foreground count', 'episode 41 frame 2:'), 'radius'),
    ])


# ---- 7: isolation ----------------------------------------------------------------------------------------------------------
def test_isolation_from_training_extraction_and_the_batch_call(tracked_episodes, episodes, eng):
    from dyn_res_pile_manip_amd import _lib, synthetic as syn, weights
    from dyn_res_pile_manip_amd.dataset_gnn_dyn import ParticleDataset
    eng.load_weights(weights.blob_from_state_dict(weights.random_state_dict(seed=0)), 0.08)
    eng.train_begin(5, 1e-3, 0.9)
    batch = syn.push_batch(0)
    depth_raw = np.ascontiguousarray(syn.render_depth(800, seed=3)[..., -1])
    pds = _ds(tracked_episodes, eng, ratio=1.0, cls=ParticleDataset)
    ps = [pds.load(0), pds.load(2)]
    pdraws = [(1000.0, 17), (240.0, 5)]
    dds = _ds(episodes, eng, ratio=1.0)
    samples, draws = _four(dds)

    def tracked_run():
        """the batch call's outputs and its taps (slots beyond a sample's count are never written: left out)"""
        out = list(pds.run(ps, pdraws))
        counts = out[2]
        out.append(eng.ptcl_dataset_tap('nfg'))
        for name in ('chosen', 'recenter', 'nearest'):
            tap = eng.ptcl_dataset_tap(name)
            out += [tap[b, :int(n)].copy() for b, n in enumerate(counts)]
        return out

    def probe():
        loss, _ = eng.train_step(*batch, mode='eval')
        ptcl, r, _ = eng.obs2ptcl(depth_raw, 24.0, syn.demo_cam_params(), 50, 2, init_idx=[0, 5])
        return [np.float64(loss), ptcl, r] + tracked_run()
    before = probe()
    eng.dispatch_reset()
    eng.train_step(*batch, mode='eval')
    marks = eng.last_dispatch()
    with pytest.raises(_lib.DrpError, match='not populated'):
        eng.ptcl_dataset_frames_tap('nfg')                                  # the buffers hold the batch call's bytes
    clouds, counts = dds.run(samples[:2], draws[:2])
    assert eng.last_dispatch() == marks
    # a pd_* tap never returns frames data: refused while the buffers hold the frames call's bytes
    for name in ('nfg', 'chosen', 'recenter', 'nearest'):
        with pytest.raises(_lib.DrpError, match='not populated'):
            eng.ptcl_dataset_tap(name)
    assert eng.ptcl_dataset_frames_tap('nfg').shape == (2, 6)
    t_frames = eng.ptcl_dataset_time()
    assert set(t_frames) == {'upload', 'compaction', 'fps_rad', 'recenter', 'track_pack', 'download'}
    assert all(v >= 0 for v in t_frames.values())
    after = probe()
    for x, y in zip(before, after):
        _bits(x, y)
    with pytest.raises(_lib.DrpError, match='not populated'):
        eng.ptcl_dataset_frames_tap('chosen')
    # a refused frames call leaves the next batch call its bits
    with pytest.raises(_lib.DrpError):
        dds.run(samples[:1], [(draws[0][0], [samples[0]['n_fg'][0]] + draws[0][1][1:])])
    for x, y in zip(before[3:], tracked_run()):
        _bits(x, y)


def test_a_running_gd_session_keeps_its_bits(episodes):
    from oracle import propnet_sparse as osp
    from dyn_res_pile_manip_amd import synthetic as syn, weights
    from dyn_res_pile_manip_amd.engine import Engine
    sd = weights.random_state_dict(seed=0)
    M34 = osp.world2cam_affine(syn.demo_cam_extrinsics(), 24)
    runs = []
    for disturb in (False, True):
        e = Engine(0)
        e.load_weights(weights.blob_from_state_dict(sd), 0.08)
        e.set_camera(M34, 24.0, syn.demo_cam_params())
        e.set_goal_image(syn.goal_distance_image(syn.goal_mask('I')), 5 * 64, fps_init=0, mode='cv5')
        s0, dens, attr = syn.make_pile(64, 1, seed=0)
        lo, hi = syn.action_limits()
        e.gd_begin(s0, attr, dens, syn.sample_pushes(4, 3, seed=0), 0.05, lo, hi)
        out = [e.gd_step()]
        marks = e.last_dispatch()
        if disturb:
            ds = _ds(episodes, e)
            s = ds.load(1)
            ds.run([s], [(700.0, [n // 3 for n in s['n_fg']])])
            assert e.last_dispatch() == marks
        out.append(e.gd_step())
        out.append(e.gd_actions())
        runs.append(out)
        e.close()
    for a, b in zip(runs[0], runs[1]):
        for x, y in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
            _bits(np.asarray(x), np.asarray(y))


# ---- 8: end to end ---------------------------------------------------------------------------------------------------------
def test_main_on_depth_only_episodes(episodes, eng, tmp_path):
    import torch
    from dyn_res_pile_manip_amd import train_gnn_dyn as TG
    from dyn_res_pile_manip_amd.gnn_dyn import PropNetDiffDenModel
    assert not [f for f in os.listdir(os.path.join(episodes, '0')) if 'particles' in f or 'color' in f]
    cfg = TG.default_config()
    cfg['dataset'].update(n_episode=4, n_timestep=6)
    cfg['train'].update(n_rollout=2, batch_size=4, train_valid_ratio=0.5, lr=2e-4, ckp_per_iter=2, log_per_iter=1)
    out = str(tmp_path / 'run')
    with pytest.raises(ValueError, match='contradicts'):
        TG.main(cfg, data_root=episodes, train_dir=out, engine=eng, data='depth', loss='mse')
    result, d = TG.main(cfg, data_root=episodes, train_dir=out, threads=4, n_epoch=1, engine=eng, data='depth', probe_every=2)
    assert d == out
    for f in ('config.yaml', 'log.txt', 'net_best.pth', 'net_epoch_0_iter_0.pth', 'net_epoch_0_iter_2.pth'):
        assert os.path.exists(os.path.join(out, f)), f
    rmse = [r for (_, ph, r) in result['history'] if ph in ('train', 'valid')]
    assert len(rmse) == 2 and np.isfinite(rmse).all() and np.isfinite(result['best_valid_loss'])   # 10 windows: 3 iterations each
    probes = [r for (_, ph, r) in result['history'] if ph == 'grad_probe']
    assert len(probes) == 2 and np.isfinite(probes).all()
    with open(os.path.join(out, 'log.txt')) as f:
        log = f.read()
    assert log.count('min_margin') == 2 and log.count('train [0][') == 3
    model = PropNetDiffDenModel(cfg, engine=eng)
    model.load_state_dict(torch.load(os.path.join(out, 'net_best.pth')))


def test_adam_updates_lower_the_loss_on_a_fixed_depth_batch(episodes):
    """the step count and learning rate of test_gpu_train_untracked.py's fixed-batch test: 6 epochs of 4 updates at lr 2e-4"""
    import dyn_res_pile_manip_amd.planners as osp
    from dyn_res_pile_manip_amd import synthetic as syn, train_gnn_dyn as TG, weights
    from dyn_res_pile_manip_amd.dataset_gnn_dyn import DepthDataset
    from dyn_res_pile_manip_amd.engine import Engine
    from dyn_res_pile_manip_amd.gnn_dyn import PropNetDiffDenModel
    cfg = TG.default_config()
    cfg['dataset'].update(n_episode=4, n_timestep=6)
    cfg['train'].update(n_rollout=3, train_valid_ratio=0.5, lr=2e-4, adam_beta1=0.9)
    model = PropNetDiffDenModel(cfg, engine=Engine(0))
    model.load_state_dict(weights.random_state_dict(seed=0, predictor_scale=1.0))
    ds = DepthDataset(episodes, cfg, 'train', _cam(), engine=model.engine)
    model.engine.set_camera(osp.world2cam_affine(np.asarray(_cam()[1], dtype=np.float64)), 24.0, _cam()[0])
    np.random.seed(2)
    data = ds.get_batch([0, 2, 5, 7])
    assert data.depth_only and data[0].shape[1] == 4 and data[6].shape[:2] == (4, 3)
    opt = TG.DeviceAdam(model, 2e-4, betas=(0.9, 0.999), n_rollout=3)
    with pytest.raises(ValueError, match='depth-only'):
        TG.run_batch(model, opt, data, 'train', 3, loss='chamfer')           # zero impulses are never trained on
    with pytest.raises(ValueError, match='depth-only'):
        TG.run_batch(model, opt, data, 'train', 3, impulses='actions')
    kw = dict(n_rollout=3, loss='chamfer', impulses='actions')
    before = TG.run_batch(model, opt, data, 'valid', **kw)
    w0 = model.engine.get_weights().copy()
    losses = [TG.run_batch(model, opt, data, 'train', **kw) for _ in range(24)]
    after = TG.run_batch(model, opt, data, 'valid', **kw)
    print('[gnn-frames] eval loss %.6e -> %.6e after 24 updates' % (before, after))
    assert np.isfinite(losses).all() and after < before
    assert np.abs(model.engine.get_weights() - w0).max() > 1e-4
    pr = TG.probe_batch(model, data, impulses='actions', loss='chamfer')
    assert np.isfinite(pr['rel']) and np.isfinite(pr['min_margin'])
    model.engine.close()

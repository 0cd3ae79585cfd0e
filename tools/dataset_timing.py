"""Cost of the GNN data path (row x4, drp_ptcl_dataset_batch) on synthetic episodes.

  python tools/dataset_timing.py [--episodes 4] [--threads 8] [--reps 5]

Reports (medians of --reps):
  - per-stage device time of one call (upload | compaction | fps_rad | recenter | track + pack | download, HIP events) at
    B = 4 / 64 / 256, particle_den drawn as the reference draws it (uniform 15 .. 6500);
  - host decoding per sample (depth PNG, particle files, actions.p, push frames) on one thread and on --threads;
  - DeviceLoader's samples/s at batch 4, chunk 64, against what the device trainer consumes (UPDATE steps at batch 4).

  python tools/dataset_timing.py --frames [--episodes 4] [--threads 8] [--reps 5]

The untracked path from depth frames alone (drp_ptcl_dataset_frames, DepthDataset; T = 6 frames per sample):
  - per-stage device time of one call (the fifth stage is the pack alone) at B = 4 / 16 / 64 samples = 24 / 96 / 384 images;
  - host decoding per sample (T depth PNGs, actions.p) on one thread and on --threads;
  - DeviceLoader's samples/s at batch 4, chunk 16, against what a Chamfer + actions UPDATE step consumes on the same batches
    (tools/train_timing.py times that step on synthetic piles).
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


STAGES = ('upload', 'compaction', 'fps_rad', 'recenter', 'track_pack', 'download')


def tracked_step(eng, cam, cfg, T):
    eng.train_begin(5, 1e-3, 0.9)
    return lambda b: eng.train_step(*b[:5], mode='update')


def depth_step(eng, cam, cfg, T):
    from dyn_res_pile_manip_amd.planners import world2cam_affine
    eng.set_camera(world2cam_affine(np.asarray(cam[1], dtype=np.float64)), float(cfg['dataset']['global_scale']), cam[0])
    eng.train_begin(T - 1, 1e-3, 0.9)
    return lambda b: eng.train_step_actions(b[0], b.actions, b[2], b[3], b[4], b[6], b[7], mode='update')


# per mode: the dataset class, the batch sizes, the fifth stage's label, the files a sample does not have, the trainer step; then
# what its printed lines say differently (T: frames per sample)
MODES = {
    False: dict(cls='ParticleDataset', sizes=(4, 64, 256), label='track_pack', strip=(), step=tracked_step, trainer='trainer',
                of_T='', per='sample', x_T='', decode_n=48, pngs='', rate='%.0f'),
    True: dict(cls='DepthDataset', sizes=(4, 16, 64), label='pack', strip=('_particles.npy', '_color.png'), step=depth_step,
               trainer='Chamfer + actions trainer', of_T=' of %(T)d frames', per='frame', x_T=' x T=%(T)d', decode_n=32,
               pngs=' (%(T)d PNGs)', rate='%.1f'),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--episodes', type=int, default=4)
    ap.add_argument('--threads', type=int, default=8)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--frames', action='store_true', help='time drp_ptcl_dataset_frames / DepthDataset instead')
    a = ap.parse_args()
    m = MODES[a.frames]
    import __graft_entry__ as g
    g.build()
    from concurrent.futures import ThreadPoolExecutor
    import torch
    from dyn_res_pile_manip_amd import dataset_gnn_dyn, synthetic, weights
    from dyn_res_pile_manip_amd.engine import Engine
    from dyn_res_pile_manip_amd.train_gnn_dyn import default_config
    eng = Engine(0)
    print('device: %s' % eng.device_info()['name'])
    cfg = default_config()
    cfg['dataset'].update(n_episode=a.episodes, n_timestep=10)
    cfg['train']['train_valid_ratio'] = 1.0
    with tempfile.TemporaryDirectory() as d:
        t0 = time.perf_counter()
        synthetic.write_episodes(d, a.episodes, 10, seed=0)
        for ep in os.listdir(d):                       # --frames: what a recorded robot episode holds, depth PNGs and actions.p
            for f in os.listdir(os.path.join(d, ep)):
                if m['strip'] and f.endswith(m['strip']):
                    os.remove(os.path.join(d, ep, f))
        cam = (synthetic.demo_cam_params(), synthetic.demo_cam_extrinsics())
        ds = getattr(dataset_gnn_dyn, m['cls'])(d, cfg, 'train', cam, engine=eng)
        T = ds.n_his + ds.n_roll
        fill = lambda text: text % {'T': T}
        print('%d episodes, %d samples%s (written in %.1f s)' % (a.episodes, len(ds), fill(m['of_T']), time.perf_counter() - t0))
        samples = [ds.load(i) for i in range(len(ds))]
        fg = np.concatenate([np.atleast_1d(s['n_fg']) for s in samples])
        print('foreground points per %s: %d .. %d' % (m['per'], fg.min(), fg.max()))
        np.random.seed(0)
        for B in m['sizes']:
            rows, walls, nmax = [], [], []
            for r in range(a.reps + 1):
                batch = [samples[(r * B + j) % len(samples)] for j in range(B)]
                draws = [ds.draw(s) for s in batch]
                t0 = time.perf_counter()
                cnt = ds.run(batch, draws)[-1]
                wall = time.perf_counter() - t0
                if r == 0:
                    continue                       # first call: allocations
                rows.append([eng.ptcl_dataset_time()[k] for k in STAGES])
                walls.append(wall * 1e3)
                nmax.append(int(cnt.max()))
            med = np.median(np.array(rows), axis=0)
            print('B=%3d%s device ms: %s | sum %.2f | call wall %.2f ms | max particles %d' % (
                B, fill(m['x_T']), ' '.join('%s %.3f' % (k if k != 'track_pack' else m['label'], v) for k, v in zip(STAGES, med)),
                med.sum(), np.median(walls), max(nmax)))
        for threads in (1, a.threads):
            n = m['decode_n']
            with ThreadPoolExecutor(max_workers=threads) as pool:
                t0 = time.perf_counter()
                list(pool.map(ds.load, [i % len(ds) for i in range(n)]))
                dt = time.perf_counter() - t0
            print('host decode: %.2f ms per sample%s on %d thread(s)' % (dt / n * 1e3, fill(m['pngs']), threads))
        np.random.seed(0)
        torch.manual_seed(0)
        loader = dataset_gnn_dyn.DeviceLoader(ds, 4, shuffle=True, threads=a.threads)
        t0 = time.perf_counter()
        batches = list(loader)
        dt = time.perf_counter() - t0
        print(('DeviceLoader batch 4, chunk %%d, %%d threads: %s samples/s' % m['rate']) % (loader.chunk, a.threads, len(ds) / dt))
        eng.load_weights(weights.blob_from_state_dict(weights.random_state_dict(seed=0, predictor_scale=1.0)), 0.08)
        step = m['step'](eng, cam, cfg, T)
        for b in batches[:2]:
            step(b)
        t0 = time.perf_counter()
        k = 0
        for _ in range(5):
            for b in batches:
                step(b)
                k += 1
        dt = time.perf_counter() - t0
        print('%s at batch 4: %.2f ms per step = %.0f samples/s' % (m['trainer'], dt / k * 1e3, 4 * k / dt))
    eng.close()


if __name__ == '__main__':
    main()

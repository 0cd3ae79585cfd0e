"""What the float64 yardstick costs: device time of Engine.step_f64 by HIP events, its share of the fp64 matrix peak counted
on algorithmic FLOPs, and what load_weights(probe=True) adds to a plain load_weights.  Writes profiles/f64_timing.txt.

    python tools/f64_timing.py [--reps 15] [--out profiles/f64_timing.txt]

Each figure is the median of `reps` runs after three warm-up runs; the events bracket the whole call on the default
stream's timeline (uploads, the fp32 graph build, the float64 kernels, the download), the context's own stream being
waited for inside the call.  No pass mark: the numbers say what the probe costs."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from dyn_res_pile_manip_amd import synthetic as syn, weights
from dyn_res_pile_manip_amd.engine import Engine
from oracle.propnet_sparse import world2cam_affine

PEAK_FP64_MATRIX_TFLOPS = 78.6          # MI355X, dense fp64 matrix peak at 2.4 GHz


def flops(eng, a, s, sd, d):
    """algorithmic FLOPs of one step: 2 x in x out per row of every layer, relation layers per list entry"""
    _, cnt = eng.build_graph(s, sd)
    rows, edges = a.size, int(cnt.sum())
    node = 2 * (5 * 64 + 64 * 64) + 3 * 2 * 129 * 64 + 2 * (64 * 64 + 64 * 3)
    edge = 2 * (6 * 64 + 2 * 64 * 64) + 3 * (2 * 193 * 64 + 64)
    return rows * node + edges * edge, edges


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'f64_timing.txt'))
    args = ap.parse_args()
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'weights_seed0.npz'))
    blob = weights.blob_from_state_dict(g)
    eng = Engine(0)
    eng.load_weights(blob, 0.08)
    eng.set_camera(world2cam_affine(syn.demo_cam_extrinsics(), 24), 24.0, syn.demo_cam_params())
    lines = ['float64 one-step evaluation and accuracy probe: what they cost',
             'device: %s; clocks as the machine had them (not pinned); median of %d runs after 3 warm-up runs' %
             (eng.device_info()['name'], args.reps), '']
    for B, N in ((8, 64), (64, 300), (1024, 300)):
        s0, dens, attr = syn.make_pile(N, 1, seed=0)
        s = np.repeat(s0, B, axis=0)
        a, d = np.repeat(attr, B, axis=0), np.repeat(dens, B)
        sd = eng.gen_s_delta(s, syn.sample_pushes(B, 1, seed=0)[:, 0])
        fl, edges = flops(eng, a, s, sd, d)
        ms, wall = [], []
        for r in range(args.reps + 3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            eng.step_f64(a, s, sd, d)
            e1.record()
            e1.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
            ms.append(e0.elapsed_time(e1))
        m, wl = float(np.median(ms[3:])), float(np.median(wall[3:]))
        lines.append('step_f64 %4d x %3d (%8d list entries): %9.3f ms by events (%9.3f ms wall, min %.3f, max %.3f); %.2f GFLOP '
                     '-> %.3f TFLOP/s = %.2f %% of the %.1f TFLOP/s fp64 matrix peak (the call includes its host copies)'
                     % (B, N, edges, m, wl, min(ms[3:]), max(ms[3:]), fl / 1e9, fl / m / 1e9, 100.0 * fl / m / 1e9 / PEAK_FP64_MATRIX_TFLOPS,
                        PEAK_FP64_MATRIX_TFLOPS))
    # load_weights with and without the probe, interleaved
    plain, probed = [], []
    for r in range(args.reps + 3):
        for store, kw in ((plain, {}), (probed, {'probe': True})):
            t0 = time.perf_counter()
            eng.load_weights(blob, 0.08, **kw)
            store.append((time.perf_counter() - t0) * 1e3)
    p0, p1 = float(np.median(plain[3:])), float(np.median(probed[3:]))
    lines += ['', 'load_weights, interleaved, wall: plain %.3f ms, probe=True %.3f ms -> the probe adds %.3f ms (8 x 64 batch: its pile, '
              'gen_s_delta, one step on the engine, one in float64, the reduction)' % (p0, p1, p1 - p0)]
    eng.close()
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()

"""Timing of the resolution regressor on the device (model/res_regressor.py; include/drp.h drp_rgr_*), medians:

  forward at B = 1, 4, 16, 64  device time of the kernels (HIP events, drp_rgr_time) and the whole call (input upload included)
  parts at B = 1 and 16        the convolutions, FC1 alone (and its share of the measured 6.3 TB/s HBM copy rate), FC2..head
  infer_param                  720 x 720 masks -> particle count, per distance transform (one call: upload, stack, forward)

  python tools/rgr_timing.py [--iters N] [--out profiles/rgr_timing.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBPS = 6.3                           # float4 copy, MI355X
FC1_BYTES = 4096 * 25088 * 4


def wall_ms(fn, iters):
    fn()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from dyn_res_pile_manip_amd import res_regressor as rr, synthetic as syn
    from dyn_res_pile_manip_amd.engine import Engine

    eng = Engine(0)
    lines = ['device: %s' % eng.device_info()['name']]
    eng.rgr_load(rr.blob_from_state_dict(rr.random_state_dict(0, 1), 1), 1)
    rng = np.random.Generator(np.random.PCG64(1))
    x = rng.random((64, 6, 224, 224), dtype=np.float32)
    lines.append('forward (ms, median of %d)        device   call' % args.iters)
    for B in (1, 4, 16, 64):
        eng.rgr_forward(x[:B])
        dev = float(np.median(eng.rgr_time(B, args.iters)))
        call = wall_ms(lambda: eng.rgr_forward(x[:B]), max(5, args.iters // 5))
        lines.append('  B=%-2d                            %7.3f  %7.3f' % (B, dev, call))
    for B in (1, 16):
        conv = float(np.median(eng.rgr_time(B, args.iters, parts=1)))
        fc1 = float(np.median(eng.rgr_time(B, args.iters, parts=2)))
        tail = float(np.median(eng.rgr_time(B, args.iters, parts=4)))
        tb = FC1_BYTES / (fc1 * 1e-3) / 1e12
        lines.append('  B=%-2d parts: convolutions %.3f ms, FC1 %.3f ms (%.2f TB/s = %.2f of %.1f TB/s), FC2..head %.3f ms'
                     % (B, conv, fc1, tb, tb / HBM_TBPS, HBM_TBPS, tail))
    obs = syn.render_depth(n_granules=1500, seed=0)
    init, goal = rr.masks_from_obs(obs, syn.goal_distance_image(syn.goal_mask('I')), syn.GLOBAL_SCALE)
    for mode in ('cv5', 'exact'):
        ms = wall_ms(lambda: eng.rgr_infer(init, goal, mode), max(5, args.iters // 5))
        lines.append('infer_param 720x720 %-5s  %.3f ms  (output %.3f)' % (mode, ms, float(eng.rgr_infer(init, goal, mode)[0])))
    eng.close()
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()

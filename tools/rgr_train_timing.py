"""Timing of the resolution regressor's training step on the device (include/drp.h drp_rgr_train_*), medians:

  UPDATE step at B = 16    device time split into forward | loss + FC backward with FC1's fused Adam step | conv backward
                           + Adam over the other parameters (HIP events, drp_rgr_train_time), and the whole call
  FC1's update pass        the fused wgrad + L1 + Adam kernel alone is not separable by events; its floor is the bytes it
                           must move (W, m, v read and written: 6 x 411 MB) at the 6.3 TB/s HBM copy rate, reported as the
                           FC phase's achieved fraction of that (an upper bound on the time the pass itself took)
  torch reference          torch-ROCm autograd + torch.optim.Adam of the same model (the reference's nn.Sequential, built
                           here from torch.nn) at the same batch on the same GPU, fp32

  python tools/rgr_train_timing.py [--iters N] [--B 16] [--out profiles/rgr_train_timing.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBPS = 6.3                           # float4 copy, MI355X
FC1_UPDATE_BYTES = 6 * 4096 * 25088 * 4


def torch_reference_ms(sd, x, y, conf, iters):
    import torch
    import torch.nn as nn
    dev = torch.device('cuda:0')
    layers = []
    for i, (co, ci) in enumerate(((64, 6), (128, 64), (256, 128), (512, 256), (512, 512))):
        layers += [nn.Conv2d(ci, co, 4, 2, 1), nn.LeakyReLU(0.2)]
    layers.append(nn.Flatten())
    for fo, fi in ((4096, 25088), (1024, 4096), (256, 1024), (64, 256)):
        layers += [nn.Linear(fi, fo), nn.LeakyReLU(0.2)]
    layers.append(nn.Linear(64, 1))
    model = nn.Sequential(*layers)
    model.load_state_dict({k[len('model.'):]: torch.from_numpy(v) for k, v in sd.items()})
    model = model.to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=1e-5, betas=(0.9, 0.999))
    xt, yt, ct = (torch.from_numpy(a).to(dev) for a in (x, y.reshape(-1, 1), conf.reshape(-1, 1)))
    mse = nn.MSELoss(reduction='none')

    def step():
        out = model(xt)
        loss_mse = (mse(out, yt) * ct).mean()
        reg, n = 0.0, 0
        for ii, W in enumerate(list(model.parameters())):
            if ii % 2 == 0:
                reg = reg + W.norm(1)
                n += W.numel()
        loss = loss_mse + (reg / n) * 2e-4
        opt.zero_grad()
        loss.backward()
        opt.step()
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--B', type=int, default=16)
    ap.add_argument('--no-torch', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from dyn_res_pile_manip_amd import res_regressor as rr
    from dyn_res_pile_manip_amd.engine import Engine

    B = args.B
    sd = rr.random_state_dict(0, 1)
    rng = np.random.Generator(np.random.PCG64(1))
    x = rng.random((B, 6, 224, 224), dtype=np.float32)
    y = rng.uniform(20, 130, B).astype(np.float32)
    conf = rng.uniform(0.1, 1.0, B).astype(np.float32)
    tline = None
    if not args.no_torch:               # first, while torch is the only one holding the device
        try:
            tms = torch_reference_ms(sd, x, y, conf, args.iters)
            tline = 'torch-ROCm autograd + torch.optim.Adam, same model, B=%d: %.3f ms per step' % (B, tms)
        except Exception as e:                                    # noqa: BLE001 (a measurement tool: report, go on)
            tline = 'torch reference failed: %r' % (e,)
    eng = Engine(0)
    lines = ['device: %s' % eng.device_info()['name']]
    eng.rgr_load(rr.blob_from_state_dict(sd, 1), 1)
    eng.rgr_train_begin(1e-5, 0.9, 2e-4)
    eng.rgr_train_step(x, y=y, conf=conf, mode='update')
    ms = np.median(eng.rgr_train_time(B, args.iters), axis=0)
    t0 = time.perf_counter()
    n_call = max(3, args.iters // 4)
    for _ in range(n_call):
        eng.rgr_train_step(x, y=y, conf=conf, mode='update')
    call = (time.perf_counter() - t0) * 1e3 / n_call
    fwd, fc, conv = (float(v) for v in ms)
    floor = FC1_UPDATE_BYTES / (HBM_TBPS * 1e12) * 1e3
    lines.append('UPDATE step, B=%d (ms, median of %d): device %.3f = forward %.3f + loss/FC backward/FC1 Adam %.3f + conv '
                 'backward/other Adam %.3f; whole call %.3f (input upload and loss copy included)'
                 % (B, args.iters, fwd + fc + conv, fwd, fc, conv, call))
    lines.append('FC1 update pass floor: %.1f MB at %.1f TB/s = %.3f ms; the whole FC phase reaches %.2f of it'
                 % (FC1_UPDATE_BYTES / 1e6, HBM_TBPS, floor, floor / fc))
    eng.close()
    if tline:
        lines.append(tline)
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()

"""The bits and the refusals of the two dataset calls on a fixed, seeded list of small cases: one SHA-256 per output, and for a
refused call its code and full message.

  python tools/dataset_bits.py > bits.txt        (from the repository root, on the device)

Run at two commits on one machine, the two outputs are compared line by line: a refactor of the calls' host side
(csrc/capi_ptcl_dataset.h, Engine.ptcl_dataset_batch / _frames and their taps) moves no line.  Only public methods of Engine are
called, so the script runs unchanged at either commit.  Crafted 40 x 33 images (tests/test_gpu_gnn_frames.py: _crafted, SMALL_CAM),
all on ONE context in this order, so that every call but the first follows a call of some kind:
  good calls   batch at (B, T) = (1, 2), (1, 3), (3, 2), (3, 3) with unequal particle counts per sample; frames at (B, T) =
               (1, 1), (2, 3), (3, 1); a batch call, a frames call and a batch call again; every output and every tap each time
  refusals     every per-image refusal of either call, before the launch and behind the counts wait, n_cap one too small among
               them, and inputs with two faults (the first in image order, then in the call's fixed order, is named); behind each
               the outputs and taps of a good call"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from dyn_res_pile_manip_amd import _lib
from dyn_res_pile_manip_amd.engine import Engine

SMALL_CAM = [30.0, 28.0, 16.0, 20.0]
GS = 24
H, W = 40, 33
T_CAM = np.array([[0.96, -0.28, 0.0, 0.3], [0.28, 0.96, 0.0, -0.2], [0.0, 0.0, 1.0, 14.0], [0.0, 0.0, 0.0, 1.0]])


def crafted(n_fg, seed, h=H, w=W):
    """tests/test_gpu_gnn_frames.py: _crafted -- exactly n_fg foreground pixels at random places"""
    rng = np.random.default_rng(seed)
    img = np.where(rng.random(h * w) < 0.5, 0, rng.integers(17971, 30000, h * w)).astype(np.uint16)
    img[rng.permutation(h * w)[:n_fg]] = rng.integers(12000, 17000, n_fg)
    return img.reshape(h, w)


def show(label, value):
    a = np.ascontiguousarray(value)
    print('%s %s %s %s' % (hashlib.sha256(a.tobytes()).hexdigest(), label, a.dtype, list(a.shape)))


def at(a, idx, v):
    a = np.array(a)
    a[idx] = v
    return a


def batch_args(B, T, seed):
    """a batch call's arguments: B images, sample b with 5 + 3 b particles per frame, in-plane pushes"""
    rng = np.random.default_rng(seed)
    n_fg = [int(n) for n in rng.integers(200, 1200, B)]
    push = np.zeros((B, T - 1, 10))
    push[..., :6] = rng.normal(size=(B, T - 1, 6))
    d = rng.normal(size=(B, T - 1, 2))
    push[..., 6:8] = d / np.linalg.norm(d, axis=-1, keepdims=True)
    push[..., 9] = rng.uniform(0.1, 0.5, (B, T - 1))
    return dict(depth=np.stack([crafted(n, seed * 100 + b) for b, n in enumerate(n_fg)]), global_scale=GS, cam_params=SMALL_CAM,
                T_cam=T_CAM, particles=[(rng.normal(size=(T, 5 + 3 * b, 4)) * 8).astype(np.float32) for b in range(B)],
                radius=rng.uniform(0.03, 0.12, B), init_idx=[int(rng.integers(n)) for n in n_fg], n_fg=n_fg, push=push,
                episode=[40 + 7 * b for b in range(B)])


def frames_args(B, T, seed):
    rng = np.random.default_rng(seed)
    n_fg = rng.integers(60, 1300, (B, T))
    return dict(depth=np.stack([np.stack([crafted(n, seed * 100 + 10 * b + t) for t, n in enumerate(row)]) for b, row in enumerate(n_fg)]),
                global_scale=GS, cam_params=SMALL_CAM, radius=rng.uniform(0.03, 0.12, (B, T)), init_idx=rng.integers(n_fg), n_fg=n_fg,
                episode=[50 + 9 * b for b in range(B)])


def run(eng, kind, tag, args):
    """one call: its outputs and taps, or its refusal"""
    call, tap, taps = ((eng.ptcl_dataset_batch, eng.ptcl_dataset_tap, ('nfg', 'chosen', 'recenter', 'nearest')) if kind == 'batch'
                       else (eng.ptcl_dataset_frames, eng.ptcl_dataset_frames_tap, ('nfg', 'chosen', 'recenter')))
    try:
        out = call(**args)
    except _lib.DrpError as e:
        print('REFUSED %s %s: %s' % (kind, tag, e))
        return None
    for k, v in enumerate(out):
        show('%s %s out%d' % (kind, tag, k), v)
    counts = out[-1]
    for name in taps:
        t = tap(name)
        if name != 'nfg':                              # slots beyond an image's count are never written
            t = np.concatenate([row[:n] for row, n in zip(t.reshape((counts.size,) + t.shape[counts.ndim:]), counts.ravel())])
        show('%s %s tap %s' % (kind, tag, name), t)
    other = eng.ptcl_dataset_frames_tap if kind == 'batch' else eng.ptcl_dataset_tap
    try:
        other('nfg')
        print('%s %s: the other call\'s tap answered' % (kind, tag))
    except _lib.DrpError as e:
        print('REFUSED %s %s other tap: %s' % (kind, tag, e))
    return out


def main():
    eng = Engine(0)
    for B, T in ((1, 2), (1, 3), (3, 2), (3, 3)):
        run(eng, 'batch', 'B=%d T=%d' % (B, T), batch_args(B, T, 10 * B + T))
    for B, T in ((1, 1), (2, 3), (3, 1)):
        run(eng, 'frames', 'B=%d T=%d' % (B, T), frames_args(B, T, 10 * B + T))
    bg, fg = batch_args(2, 2, 7), frames_args(2, 3, 8)
    good = {'batch': bg, 'frames': fg}
    for kind in ('batch', 'frames', 'batch', 'frames'):
        out = run(eng, kind, 'alternating', good[kind])
        good[kind + '_counts'] = out[-1]

    zero_b, zero_f = bg['depth'].copy(), fg['depth'].copy()
    zero_b[1] = 0
    zero_f[1, 1] = 0
    big = np.stack([crafted(700, 1, h=80, w=70), crafted(5600, 2, h=80, w=70)])
    push = bg['push']
    refusals = [
        ('batch', 'no particles', dict(particles=[bg['particles'][0], bg['particles'][1][:, :0]])),
        ('batch', 'init -1', dict(init_idx=at(bg['init_idx'], 1, -1))),
        ('batch', 'radius 0', dict(radius=at(bg['radius'], 0, 0.0))),
        ('batch', 'radius inf', dict(radius=at(bg['radius'], 1, np.inf))),
        ('batch', 'radius nan', dict(radius=at(bg['radius'], 1, np.nan))),
        ('batch', 'push length 0', dict(push=at(push, (1, 0, 9), 0.0))),
        ('batch', 'push length inf', dict(push=at(push, (0, 0, 9), np.inf))),
        ('batch', 'push off the plane', dict(push=at(push, (1, 0, 8), 0.5))),
        ('batch', 'n_fg above h w', dict(n_fg=at(bg['n_fg'], 1, H * W + 1))),
        ('batch', 'n_fg -1', dict(n_fg=at(bg['n_fg'], 0, -1))),
        ('batch', 'no foreground', dict(depth=zero_b, n_fg=at(bg['n_fg'], 1, 0), init_idx=at(bg['init_idx'], 1, 0))),
        ('batch', 'wrong host count', dict(n_fg=at(bg['n_fg'], 0, bg['n_fg'][0] - 1), init_idx=at(bg['init_idx'], 0, 0))),
        ('batch', 'start equal to n_fg', dict(init_idx=at(bg['init_idx'], 1, bg['n_fg'][1]))),
        ('batch', 'cap reached', dict(depth=big, radius=[0.05, 1e-4], init_idx=[0, 0], n_fg=[700, 5600])),
        ('batch', 'n_cap one too small', dict(n_cap=int(good['batch_counts'].max()) - 1)),
        ('batch', 'two faults: radius, push length', dict(radius=at(bg['radius'], 0, np.inf), push=at(push, (0, 0, 9), 0.0))),
        ('batch', 'two faults: push plane of 0, init of 1', dict(push=at(push, (0, 0, 8), 0.5), init_idx=at(bg['init_idx'], 1, -1))),
        ('batch', 'two faults: host count, start', dict(n_fg=at(bg['n_fg'], 1, bg['n_fg'][1] - 1), init_idx=at(bg['init_idx'], 1, bg['n_fg'][1]))),
        ('batch', 'two faults: n_ptcl of 1, n_fg of 0', dict(particles=[bg['particles'][0], bg['particles'][1][:, :0]], n_fg=at(bg['n_fg'], 0, -1))),
        ('frames', 'init -1', dict(init_idx=at(fg['init_idx'], (1, 2), -1))),
        ('frames', 'radius 0', dict(radius=at(fg['radius'], (0, 1), 0.0))),
        ('frames', 'radius inf', dict(radius=at(fg['radius'], (1, 2), np.inf))),
        ('frames', 'radius nan', dict(radius=at(fg['radius'], (1, 0), np.nan))),
        ('frames', 'n_fg above h w', dict(n_fg=at(fg['n_fg'], (0, 2), H * W + 1))),
        ('frames', 'n_fg -1', dict(n_fg=at(fg['n_fg'], (1, 1), -1))),
        ('frames', 'no foreground', dict(depth=zero_f, n_fg=at(fg['n_fg'], (1, 1), 0), init_idx=at(fg['init_idx'], (1, 1), 0))),
        ('frames', 'wrong host count', dict(n_fg=at(fg['n_fg'], (0, 2), fg['n_fg'][0, 2] - 1), init_idx=at(fg['init_idx'], (0, 2), 0))),
        ('frames', 'start equal to n_fg', dict(init_idx=at(fg['init_idx'], (1, 0), fg['n_fg'][1, 0]))),
        ('frames', 'cap reached', dict(depth=big[None], radius=[[0.05, 1e-4]], init_idx=[[0, 0]], n_fg=[[700, 5600]], episode=[7])),
        ('frames', 'n_cap one too small', dict(n_cap=int(good['frames_counts'].max()) - 1)),
        ('frames', 'two faults: init and radius of one image', dict(init_idx=at(fg['init_idx'], (0, 1), -1), radius=at(fg['radius'], (0, 1), 0.0))),
        ('frames', 'two faults: radius of (1, 0), n_fg of (0, 2)', dict(radius=at(fg['radius'], (1, 0), np.inf), n_fg=at(fg['n_fg'], (0, 2), H * W + 1))),
        ('frames', 'two faults: host count of (1, 1), empty (1, 2)', dict(depth=at(fg['depth'], (1, 2), 0), n_fg=at(at(fg['n_fg'], (1, 2), 0), (1, 1), fg['n_fg'][1, 1] - 1),
                                                                        init_idx=at(at(fg['init_idx'], (1, 2), 0), (1, 1), 0))),
    ]
    for kind, tag, kw in refusals:
        if run(eng, kind, tag, dict(good[kind], **kw)) is not None:
            print('NOT REFUSED %s %s' % (kind, tag))
        run(eng, kind, 'after ' + tag, good[kind])
    eng.close()


if __name__ == '__main__':
    main()

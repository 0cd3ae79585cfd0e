"""The bits of the cloud losses and of both trainers on a fixed, seeded list of small cases: one SHA-256 per output, nothing else.

  python tools/loss_bits.py > bits.txt        (from the repository root, on the device)

Run at two commits on one machine, the two outputs are compared line by line: a refactor of the loss kernels' arguments, of the
one-shots' staging or of the trainers' entry points moves no line.  Only public methods of Engine are called, so the script runs
unchanged at either commit.  The cases:
  one-shots   cloud_chamfer, cloud_chamfer_f64, cloud_match, every optional output, on one context in this order of (B, N, M):
              (3, 70, 130), (2, 5, 3), (1, 65, 64), (1, 1, 1), (1, 64, 64)
  fp32        the fixture batch b2_r5 (data impulses) and the push batches tiny and mask (tests/_train_actions_ref.py), every loss
              kind their entry points take; mode='grad' (loss, blob, matches), then two mode='update' steps and get_weights();
              on the selected tape and with the `mfma` engine selected
  float64     train_grad_f64 / _actions / _untracked on the same batches: loss, terms, blob, margin"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import numpy as np

import _train_actions_ref as A
import _untracked_ref as U
from dyn_res_pile_manip_amd import weights
from dyn_res_pile_manip_amd.engine import Engine

ONE_SHOTS = (((70, 130, 70, 130), 3), ((5, 3, 5, 3), 2), ((65, 60, 65, 64), 1), ((1, 1, 1, 1), 1), ((64, 64, 64, 64), 1))
MIX = 0.3


class Golden(object):
    def __getattr__(self, name):
        return np.load(os.path.join(ROOT, 'tests', 'golden', name + '.npz'), allow_pickle=False)


def show(label, value):
    a = np.ascontiguousarray(value)
    print('%s %s %s %s' % (hashlib.sha256(a.tobytes()).hexdigest(), label, a.dtype, list(a.shape)))


def one_shots():
    eng = Engine(0)
    for shape, B in ONE_SHOTS:
        case = U.chamfer_case(shape, B)
        for name, out in (('cloud_chamfer', eng.cloud_chamfer(*case, want_grad=True, want_nn=True)),
                          ('cloud_chamfer_f64', eng.cloud_chamfer_f64(*case, want_grad=True, want_nn=True)),
                          ('cloud_match', eng.cloud_match(*case, want_grad=True, want_match=True, want_dual=True))):
            for k in sorted(out):
                show('%s B=%d N=%d M=%d %s' % (name, B, shape[2], shape[3], k), out[k])
    eng.close()


def fp32_steps(golden, name, five, by_actions, targets, tnums):
    """label -> a step at the given mode, for every loss kind the batch's entry points take"""
    states, imp, attrs, nums, dens = five
    imp_kw = {'actions': imp} if by_actions else {'states_delta': imp}
    steps = {}
    if by_actions:
        steps['train_step_actions mse'] = lambda e, mode: e.train_step_actions(*five, mode=mode, want_grad=True)
        steps['train_step_actions chamfer'] = lambda e, mode: e.train_step_actions(*five, targets=targets, target_nums=tnums,
                                                                                    mode=mode, want_grad=True)
    else:
        steps['train_step mse'] = lambda e, mode: e.train_step(*five, mode=mode, want_grad=True)
        steps['train_step_untracked chamfer'] = lambda e, mode: e.train_step_untracked(*five, targets, tnums, mode=mode,
                                                                                        want_grad=True)
    for kind in ('chamfer', 'match', 'chamfer+match'):
        steps['train_step_loss ' + kind] = (lambda e, mode, kind=kind: e.train_step_loss(
            states, attrs, nums, dens, targets, tnums, loss=kind, match_weight=MIX, mode=mode, want_grad=True, want_match=True,
            **imp_kw))
    return steps


def trainers(golden):
    blob = weights.blob_from_state_dict(golden.weights_seed0)
    batches = [('b2_r5', False, U.untracked_batch(golden, 'b2_r5'))]
    for name in ('tiny', 'mask'):
        five = A.batch(golden, name)
        batches.append((name, True, five + list(U.make_targets(five[0], five[3], 500))))
    for name, by_actions, seven in batches:
        five, (targets, tnums) = seven[:5], seven[5:]
        H = five[0].shape[1] - 1
        for engine in ('selected', 'mfma'):
            for label, step in sorted(fp32_steps(golden, name, five, by_actions, targets, tnums).items()):
                eng = Engine(0)                 # a fresh context per trajectory: Adam's state starts at zero
                eng.load_weights(blob, 0.08)
                eng.set_camera(*A.camera_args())
                if engine == 'mfma':
                    eng.set_engine('mfma')
                eng.train_begin(H, 1e-3, 0.9)
                tag = '%s %s %s' % (name, engine, label)
                out = step(eng, 'grad')
                show(tag + ' grad loss', np.float64(out[0]))
                show(tag + ' grad blob', out[1])
                if len(out) > 2 and out[2] is not None:
                    show(tag + ' grad match', out[2])
                for it in range(2):
                    show(tag + ' update %d loss' % it, np.float64(step(eng, 'update')[0]))
                show(tag + ' weights', eng.get_weights())
                eng.close()
        eng = Engine(0)
        eng.load_weights(blob, 0.08)
        eng.set_camera(*A.camera_args())
        states, imp, attrs, nums, dens = five
        if by_actions:
            calls = (('train_grad_f64_actions', eng.train_grad_f64_actions(*five)),
                     ('train_grad_f64_untracked', eng.train_grad_f64_untracked(states, None, attrs, nums, dens, targets, tnums, actions=imp)))
        else:
            calls = (('train_grad_f64', eng.train_grad_f64(*five)),
                     ('train_grad_f64_untracked', eng.train_grad_f64_untracked(*five, targets, tnums)))
        for label, out in calls:
            for k, v in zip(('loss', 'terms', 'blob', 'margin'), out):
                show('%s %s %s' % (name, label, k), np.float64(v) if k == 'loss' else v)
        eng.close()


if __name__ == '__main__':
    one_shots()
    trainers(Golden())

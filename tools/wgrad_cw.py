#!/usr/bin/env python
"""The trainer's weight-gradient sums against their float64 reconstruction: the worst |gradient - float64 sum| / bound per
state-dict tensor and case (tests/_wgrad_ref.py has the bound, tests/test_gpu_wgrad_cw.py asserts <= 1 on the same cases).

  python tools/wgrad_cw.py > profiles/wgrad_cw.txt

One line per case and tensor; the cases are the test's (tests/_wgrad_cases.py): six hand-made batches and the four fixture cases,
both tapes, both sum kernels (DRP_NO_WGRAD_MFMA=1 is set here before the context of a `valu` case is made), then the sibling
calls -- through the push, against untracked clouds, the accumulate path, an update pass.  Last, for scale, the norm-wise
distance of the whole gradient from float64 on the fixture cases (Engine.train_gradient_probe)."""
import os
import sys

sys.path.insert(0, '.')
sys.path.insert(0, 'tests')
import numpy as np

import _wgrad_cases as C
from dyn_res_pile_manip_amd import weights
from dyn_res_pile_manip_amd.engine import Engine


class Golden(object):
    def __getattr__(self, name):
        return np.load(os.path.join('tests', 'golden', name + '.npz'), allow_pickle=False)


def main():
    golden = Golden()
    cases = [('n%s H=%d' % ('_'.join(map(str, nums)), H), C.hand_made(list(nums), H), golden.weights_seed0) for nums, H in C.HAND]
    cases += [('%s %s' % (name, wset), C.fixture_batch(golden, name), C.weights_of(golden, wset)) for name, wset in C.FIXTURES]
    worst = {}
    for sums in ('mfma', 'valu'):
        if sums == 'valu':
            os.environ['DRP_NO_WGRAD_MFMA'] = '1'
        else:
            os.environ.pop('DRP_NO_WGRAD_MFMA', None)
        for tape in ('fused', 'mfma'):
            for label, batch, w in cases:
                B, T1, N, _ = batch[0].shape
                e = Engine(0)
                try:
                    e.load_weights(weights.blob_from_state_dict(w), 0.08)
                    e.set_engine(tape)
                    e.train_begin(T1 - 1, 1e-3, 0.9)
                    loss, grad = e.train_step(*batch, mode='grad', want_grad=True)
                    ratios = C.measure(e, grad, B, N, T1 - 1, sums == 'mfma', '%s %s/%s' % (label, tape, sums))
                finally:
                    e.close()
                for key, r in ratios.items():
                    worst[(sums, key)] = max(worst.get((sums, key), 0.0), r)
    # the sibling calls (default tape and sum kernel): the push, the Chamfer loss, the accumulate path, an update pass
    os.environ.pop('DRP_NO_WGRAD_MFMA', None)
    e = Engine(0)
    try:
        e.load_weights(weights.blob_from_state_dict(golden.weights_trained), 0.08)
        e.set_camera(*C.camera_args())
        sib = [C.pass_actions(e, golden), C.pass_untracked(e, golden)]
    finally:
        e.close()
    e = Engine(0)
    try:
        e.load_weights(weights.blob_from_state_dict(golden.weights_seed0), 0.08)
        sib += list(C.pass_accumulate_and_update(e, golden))
    finally:
        e.close()
    for ratios in sib:
        for key, r in ratios.items():
            worst[('mfma', key)] = max(worst[('mfma', key)], r)
    print()
    print('worst over all cases, per tensor and sum kernel (1.0 = the bound):')
    for key, _ in weights.STATE_DICT_KEYS:
        print('  %-45s mfma %.4f   valu %.4f' % (key[len('model.'):], worst[('mfma', key)], worst[('valu', key)]))
    print('  %-45s mfma %.4f   valu %.4f' % ('all', max(v for (s, _), v in worst.items() if s == 'mfma'),
                                             max(v for (s, _), v in worst.items() if s == 'valu')))
    # beside it, the norm-wise distance of the whole pass from float64 (Engine.train_gradient_probe): what the rows add
    print()
    print('norm-wise, the whole pass against drp_train_grad_f64: worst tensor\'s max |g32 - g64| / max |g64|, and |loss32 - loss64|')
    for name, wset in C.FIXTURES:
        batch = C.fixture_batch(golden, name)
        e = Engine(0)
        try:
            e.load_weights(weights.blob_from_state_dict(C.weights_of(golden, wset)), 0.08)
            for tape in ('fused', 'mfma'):
                e.set_engine(tape)
                e.train_begin(batch[0].shape[1] - 1, 1e-3, 0.9)
                p = e.train_gradient_probe(*batch)
                print('  %s %-7s %-5s %.3e (%s)   loss %.3e' % (name, wset, p['tape'], p['rel'], p['worst'][len('model.'):], p['loss_diff']))
        finally:
            e.close()


if __name__ == '__main__':
    main()

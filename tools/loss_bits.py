"""The bits of the cloud losses and of both trainers on a fixed, seeded list of small cases: one SHA-256 per output, nothing else.

  python tools/loss_bits.py > bits.txt        (from the repository root, on the device)

Run at two commits on one machine, the two outputs are compared line by line: a refactor of the loss kernels' arguments, of the
one-shots' staging or of the trainers' entry points moves no line.  Only public methods of Engine are called, so the script runs
unchanged at either commit.  The cases:
  one-shots   cloud_chamfer, cloud_chamfer_f64, cloud_match, cloud_match_f64 (its own matching, and match_in = cloud_match's),
              cloud_transport, cloud_divergence and cloud_divergence_f64 (balanced, and with reach / mass_q / want_transported),
              every optional output, on one context in this order of (B, N, M): (3, 70, 130), (2, 5, 3), (1, 65, 64), (1, 1, 1),
              (1, 64, 64); eps is a per-sample array where B > 1 and a number where B = 1.  Behind them the Sinkhorn calls alone
              where kt_parts (csrc/k_sinkhorn.h) changes regime: (1, 257, 300) -- one lane an output one way, two the other --,
              (1, 16, 16) -- 16 outputs x 64 parts, exactly 1024 items -- and (1, 1024, 1024) at iters = 2
  fp32        the fixture batch b2_r5 (data impulses) and the push batches tiny and mask (tests/_train_actions_ref.py), every loss
              kind their entry points take -- train_step_transport, train_step_divergence (balanced and with a reach, want_err),
              train_predict + train_step_seeded and train_step_custom(losses.mse_loss) among them; mode='grad' (loss, blob, the
              call's other outputs), then two mode='update' steps and get_weights(); on the selected tape and with the `mfma`
              engine selected
  float64     train_grad_f64 / _actions / _untracked, train_grad_f64_divergence (both ways), train_grad_f64_match (its own
              matching, and match_in = the fp32 side's), train_predict_f64 and train_grad_f64_seeded on the same batches: every
              output; on b2_r5 once more, behind the probes, under a set_f64_cap that cuts the batch into chunks of one sample
              (then set_f64_cap(0)): the loss launches at a sample offset
  probes      train_gradient_probe with no targets, targets, eps / iters, eps / iters / reach, loss='match', 'chamfer+match', and
              train_gradient_probe_custom, on the same batches: every scalar of the dict by repr in sorted key order, the
              per-tensor table hashed"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import numpy as np

import _train_actions_ref as A
import _untracked_ref as U
from dyn_res_pile_manip_amd import losses, weights
from dyn_res_pile_manip_amd.engine import Engine

ONE_SHOTS = (((70, 130, 70, 130), 3), ((5, 3, 5, 3), 2), ((65, 60, 65, 64), 1), ((1, 1, 1, 1), 1), ((64, 64, 64, 64), 1))
PARTS_SHOTS = (((257, 300, 257, 300), 1, None), ((16, 16, 16, 16), 1, None), ((1024, 1024, 1024, 1024), 1, 2))     # iters: None = ITERS
MIX = 0.3
EPS = 4e-4                  # the one-shots' regularisation strength: the clouds' squared spacing (tests/_untracked_ref.chamfer_case)
ITERS = 50
REACH_PER_EPS = 4.0         # reach = 4 eps, one-shots and trainers alike: two spacings


class Golden(object):
    def __getattr__(self, name):
        return np.load(os.path.join(ROOT, 'tests', 'golden', name + '.npz'), allow_pickle=False)


def show(label, value):
    a = np.ascontiguousarray(value)
    print('%s %s %s %s' % (hashlib.sha256(a.tobytes()).hexdigest(), label, a.dtype, list(a.shape)))


def sinkhorn_shots(eng, case, shape, B, iters):
    """the five Sinkhorn one-shots on one case, every optional output"""
    p, q, n_p, n_q = case
    eps = EPS * (1.0 + 0.5 * np.arange(B)) if B > 1 else EPS
    mass_q = np.clip(n_q / n_p.astype(np.float64), 0.125, 8.0)
    want = {'want_grad': True, 'want_dual': True, 'want_col_err': True}
    div = dict(want, want_self_err=True)
    reach = dict(div, reach=REACH_PER_EPS * np.asarray(eps), mass_q=mass_q if B > 1 else float(mass_q[0]), want_transported=True)
    for name, out in (('cloud_transport', eng.cloud_transport(*case, eps=eps, iters=iters, **want)),
                      ('cloud_divergence', eng.cloud_divergence(*case, eps=eps, iters=iters, **div)),
                      ('cloud_divergence reach', eng.cloud_divergence(*case, eps=eps, iters=iters, **reach)),
                      ('cloud_divergence_f64', eng.cloud_divergence_f64(*case, eps=eps, iters=iters, **div)),
                      ('cloud_divergence_f64 reach', eng.cloud_divergence_f64(*case, eps=eps, iters=iters, **reach))):
        for k in sorted(out):
            show('%s B=%d N=%d M=%d iters=%d %s' % (name, B, shape[2], shape[3], iters, k), out[k])


def one_shots():
    eng = Engine(0)
    for shape, B in ONE_SHOTS:
        case = U.chamfer_case(shape, B)
        for name, out in (('cloud_chamfer', eng.cloud_chamfer(*case, want_grad=True, want_nn=True)),
                          ('cloud_chamfer_f64', eng.cloud_chamfer_f64(*case, want_grad=True, want_nn=True)),
                          ('cloud_match', eng.cloud_match(*case, want_grad=True, want_match=True, want_dual=True))):
            for k in sorted(out):
                show('%s B=%d N=%d M=%d %s' % (name, B, shape[2], shape[3], k), out[k])
        pairs = eng.cloud_match(*case, want_match=True)['match_pq']
        sinkhorn_shots(eng, case, shape, B, ITERS)
        for name, out in (('cloud_match_f64', eng.cloud_match_f64(*case, want_grad=True, want_match=True, want_dual=True)),
                          ('cloud_match_f64 match_in', eng.cloud_match_f64(*case, match_in=pairs, want_grad=True, want_match=True,
                                                                           want_dual=True))):
            for k in sorted(out):
                show('%s B=%d N=%d M=%d %s' % (name, B, shape[2], shape[3], k), out[k])
    for shape, B, iters in PARTS_SHOTS:
        sinkhorn_shots(eng, U.chamfer_case(shape, B), shape, B, iters or ITERS)
    eng.close()


def sinkhorn_args(five, tnums):
    """the trainers' eps [B], reach [B] and mass_q [n_rollout, B] of a batch, as train_gnn_dyn forms them at scale 1 and reach 4"""
    dens, nums = np.asarray(five[4], np.float64).reshape(-1), np.asarray(five[3], np.float64).reshape(-1, 1)
    eps = 1.0 / dens
    return eps, REACH_PER_EPS * eps, np.ascontiguousarray(np.clip(np.asarray(tnums, np.float64) / nums, 0.125, 8.0).T)


def one_sample_cap(states):
    """a float64 cap that holds one sample of the batch and not two (the arithmetic of tests/test_gpu_train_f64.py's _lib_cap_for,
    from include/drp.h's figures: tape 24 KB per particle and step, reverse pass and operands 52 KB per particle, 307 KB of
    accumulators per sample)"""
    _, T1, N, _ = states.shape
    return int(((24 * 1024 * (T1 - 1) + 52 * 1024) * N + 307 * 1024) * 1.5)


def fp32_steps(golden, name, five, by_actions, targets, tnums):
    """label -> a step at the given mode, for every loss kind the batch's entry points take: (loss, blob, further outputs)"""
    states, imp, attrs, nums, dens = five
    imp_kw = {'actions': imp} if by_actions else {'states_delta': imp}
    eps, reach, mass_q = sinkhorn_args(five, tnums)
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
    six = (states, attrs, nums, dens, targets, tnums)
    steps['train_step_transport'] = lambda e, mode: e.train_step_transport(*six, eps, ITERS, mode=mode, want_grad=True,
                                                                           want_col_err=True, **imp_kw)
    steps['train_step_divergence'] = lambda e, mode: e.train_step_divergence(*six, eps, ITERS, mode=mode, want_grad=True,
                                                                             want_err=True, **imp_kw)
    steps['train_step_divergence reach'] = lambda e, mode: e.train_step_divergence(
        *six, eps, ITERS, mode=mode, want_grad=True, want_err=True, reach=reach, mass_q=mass_q, **imp_kw)
    steps['train_step_divergence reach scalar'] = lambda e, mode: e.train_step_divergence(
        *six, float(eps[0]), ITERS, mode=mode, want_grad=True, reach=float(reach[0]), **imp_kw)
    steps['train_step_custom mse_loss'] = lambda e, mode: e.train_step_custom(losses.mse_loss, states, attrs, nums, dens, mode=mode,
                                                                              want_grad=True, context=five, **imp_kw)

    def seeded(e, mode):
        pred = e.train_predict(states, attrs, nums, dens, **imp_kw)
        value, seed = losses.mse_loss(pred, five)
        return value, e.train_step_seeded(states, attrs, nums, dens, seed, mode=mode, want_grad=True, **imp_kw), pred
    steps['train_predict train_step_seeded'] = seeded
    return steps


def show_probe(tag, pr):
    """a probe's dict: every scalar by repr in sorted key order, the per-tensor table hashed"""
    for k in sorted(pr):
        if k != 'tensors':
            print('%s %s = %r' % (tag, k, pr[k]))
    show(tag + ' tensors', np.array([[pr['tensors'][key][f] for f in ('max_abs_err', 'max_abs_ref', 'rel')]
                                     for key in sorted(pr['tensors'])], np.float64))


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
                for k in range(3, len(out)):
                    show(tag + ' grad out %d' % k, out[k])
                for it in range(2):
                    show(tag + ' update %d loss' % it, np.float64(step(eng, 'update')[0]))
                show(tag + ' weights', eng.get_weights())
                eng.close()
        eng = Engine(0)
        eng.load_weights(blob, 0.08)
        eng.set_camera(*A.camera_args())
        states, imp, attrs, nums, dens = five
        # the yardsticks of the targeted losses and of a caller's loss: states_delta positionally (None beside actions)
        sd, act = (None, imp) if by_actions else (imp, None)
        imp_kw = {'actions': imp} if by_actions else {'states_delta': imp}
        seven64 = (states, sd, attrs, nums, dens, targets, tnums)
        eps, reach, mass_q = sinkhorn_args(five, tnums)
        eng.train_begin(H, 1e-3, 0.9)
        match32 = eng.train_step_loss(states, attrs, nums, dens, targets, tnums, loss='match', mode='grad', want_match=True,
                                      **imp_kw)[2]

        def float64_calls(tag):
            """every float64 trainer call of the batch, every output"""
            if by_actions:
                calls = (('train_grad_f64_actions', eng.train_grad_f64_actions(*five)),
                         ('train_grad_f64_untracked', eng.train_grad_f64_untracked(states, None, attrs, nums, dens, targets, tnums,
                                                                                   actions=imp)))
            else:
                calls = (('train_grad_f64', eng.train_grad_f64(*five)),
                         ('train_grad_f64_untracked', eng.train_grad_f64_untracked(*five, targets, tnums)))
            for label, out in calls:
                for k, v in zip(('loss', 'terms', 'blob', 'margin'), out):
                    show('%s %s %s' % (tag, label, k), np.float64(v) if k == 'loss' else v)
            pred64 = eng.train_predict_f64(states, attrs, nums, dens, **imp_kw)
            calls = (('train_grad_f64_divergence', eng.train_grad_f64_divergence(*seven64, eps, ITERS, actions=act, want_state=True,
                                                                                 want_err=True)),
                     ('train_grad_f64_divergence reach', eng.train_grad_f64_divergence(*seven64, eps, ITERS, actions=act, want_state=True,
                                                                                       want_err=True, reach=reach, mass_q=mass_q)),
                     ('train_grad_f64_divergence reach scalar', eng.train_grad_f64_divergence(*seven64, float(eps[0]), ITERS, actions=act,
                                                                                              reach=float(reach[0]))),
                     ('train_grad_f64_match', eng.train_grad_f64_match(*seven64, actions=act, want_state=True, want_info=True)),
                     ('train_grad_f64_match mix', eng.train_grad_f64_match(*seven64, 'chamfer+match', MIX, actions=act, want_info=True)),
                     ('train_grad_f64_match match_in', eng.train_grad_f64_match(*seven64, actions=act, match_in=match32, want_info=True)),
                     ('train_predict_f64', (pred64,)),
                     ('train_grad_f64_seeded', eng.train_grad_f64_seeded(states, attrs, nums, dens, losses.mse_loss(pred64, five)[1],
                                                                         want_state=True, **imp_kw)))
            for label, out in calls:
                for k, v in enumerate(out):
                    for key, item in (sorted(v.items()) if isinstance(v, dict) else (('', v),)):
                        if item is not None:
                            show('%s %s out %d %s' % (tag, label, k, key), item)
        float64_calls(name)
        probes = (('mse', {}), ('chamfer', {'targets': targets, 'target_nums': tnums}),
                  ('sinkhorn', {'targets': targets, 'target_nums': tnums, 'eps': eps, 'iters': ITERS}),
                  ('sinkhorn reach', {'targets': targets, 'target_nums': tnums, 'eps': eps, 'iters': ITERS, 'reach': reach,
                                      'mass_q': mass_q}),
                  ('match', {'targets': targets, 'target_nums': tnums, 'loss': 'match'}),
                  ('chamfer+match', {'targets': targets, 'target_nums': tnums, 'loss': 'chamfer+match', 'match_weight': MIX}))
        for label, kw in probes:
            show_probe('%s train_gradient_probe %s' % (name, label), eng.train_gradient_probe(states, sd, attrs, nums, dens, actions=act,
                                                                                              **kw))
        show_probe('%s train_gradient_probe_custom' % name, eng.train_gradient_probe_custom(losses.mse_loss, states, attrs, nums, dens,
                                                                                             context=five, **imp_kw))
        if name == 'b2_r5':
            # the same calls in chunks of one sample: every float64 loss launch at a sample offset b0 > 0
            eng.set_f64_cap(one_sample_cap(states))
            try:
                float64_calls(name + ' one-sample chunks')
            finally:
                eng.set_f64_cap(0)
        eng.close()


if __name__ == '__main__':
    one_shots()
    trainers(Golden())

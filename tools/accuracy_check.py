"""Arithmetic accuracy of the engines on the golden one-step case: the final particle effect
(64 features after three propagation steps, before the predictor) against the reference's."""
import sys
sys.path.insert(0, '.')
import numpy as np
from dyn_res_pile_manip_amd import weights, _lib
from dyn_res_pile_manip_amd.engine import Engine
g = np.load('tests/golden/one_step.npz')
w = np.load('tests/golden/weights_seed0.npz')
eng = Engine(0)
eng.load_weights(weights.blob_from_state_dict(w), 0.08)
for case in ('n64', 'n8'):
    a, s, sd, d = [g[case + '/' + k] for k in ('attr', 's_cur', 's_delta', 'dens')]
    ref = g[case + '/particle_effect_2'].reshape(a.shape[0], a.shape[1], 64)
    for name in ('valu', 'mfma', 'split', 'fused', 'lite'):
        eng.set_engine(_lib.ENGINES[name])
        eng.step(a, s, sd, d)
        eff = eng.debug_fetch('effect', ref.shape)
        print('%-4s %-5s final effect: max |err| / max |ref| = %.2e' % (case, name, np.abs(eff - ref).max() / np.abs(ref).max()))

# the float64 yardstick: every engine's one-step error against the device's float64 evaluation of the same step
# (Engine.accuracy_probe), as a share of the largest displacement, on the seed-0 and on the trained weights
t = np.load('tests/golden/trained.npz')
legs = [('seed-0', w, [(g, c + '/') for c in ('n8', 'n64')]),
        ('trained', np.load('tests/golden/weights_trained.npz'), [(t, 'one_step/%s/' % c) for c in ('n20', 'n50', 'n100', 'n300')])]
for label, wts, cases in legs:
    eng.load_weights(weights.blob_from_state_dict(wts), 0.08)
    for src, p in cases:
        a, s, sd, d = [src[p + k] for k in ('attr', 's_cur', 's_delta', 'dens')]
        for name in ('valu', 'mfma', 'split', 'fused', 'lite'):
            r = eng.accuracy_probe(a, s, sd, d, engine=_lib.ENGINES[name])
            print('%-7s %-14s %-5s against float64: max |err| %.3e, largest displacement %.3e, ratio %.3e (particle %d)'
                  % (label, p, name, r['abs'], r['disp'], r['disp_rel'], r['worst']))

# --grad: the quantity the live planner consumes.  The gradient of the GD planner's loss on each tape (the fused engine's
# split-fp16 one, the fp32 matrix engine's) against the device's float64 evaluation of the same iteration
# (Engine.gradient_probe), per weight set, on the gradient cases of the golden files
if '--grad' in sys.argv:
    from dyn_res_pile_manip_amd import synthetic as syn
    from dyn_res_pile_manip_amd.planners import world2cam_affine
    eng.set_camera(world2cam_affine(syn.demo_cam_extrinsics()), 24.0, syn.demo_cam_params())
    G = syn.goal_field(syn.goal_distance_image(syn.goal_mask('I')))
    lo, hi = syn.action_limits()
    gr = np.load('tests/golden/grad.npz')
    legs = [('seed-0', w, [(gr, c + '/') for c in ('h1', 'h2', 'h1_n100')]),
            ('trained', np.load('tests/golden/weights_trained.npz'), [(t, 'grad/n%d_h%d/' % (n, h)) for n in (20, 50, 100) for h in (1, 2)])]
    for label, wts, cases in legs:
        eng.load_weights(weights.blob_from_state_dict(wts), 0.08)
        for src, p in cases:
            eng.set_goal(G, src[p + 'goal_coor'])
            for name in ('fused', 'mfma'):
                eng.set_engine(_lib.ENGINES[name])
                r = eng.gradient_probe(src[p + 's_cur'], src[p + 'attr'], src[p + 'dens'], src[p + 'act_seqs'], lo, hi)
                print('%-7s %-14s %-5s tape against float64: max |g32 - g64| %.3e, max |g64| %.3e, ratio %.3e (component %d), reward %.3e'
                      % (label, p, r['tape'], r['abs'], r['scale'], r['rel'], r['worst'], r['reward_rel']))
    eng.set_engine(_lib.ENGINES['fused'])

# --train-grad: the quantity the trainer consumes.  Every parameter's gradient of train.npz's batches on each tape against the
# device's float64 evaluation of the same loop body (Engine.train_gradient_probe), per weight set
if '--train-grad' in sys.argv:
    tr = np.load('tests/golden/train.npz')
    for label, wts in (('seed-0', np.load('tests/golden/weights_seed0.npz')), ('trained', np.load('tests/golden/weights_trained.npz'))):
        eng.load_weights(weights.blob_from_state_dict(wts), 0.08)
        for case in ('b4_r3', 'b2_r5'):
            batch = [tr[case + '/' + k] for k in ('states', 'states_delta', 'attrs', 'particle_nums', 'particle_dens')]
            for name in ('fused', 'mfma'):
                eng.set_engine(_lib.ENGINES[name])
                eng.train_begin(batch[0].shape[1] - 1, 1e-3, 0.9)
                r = eng.train_gradient_probe(*batch)
                print('%-7s %-6s %-5s tape against float64: worst tensor %s, max |g32 - g64| / max |g64| %.3e, loss difference %.3e'
                      % (label, case, r['tape'], r['worst'], r['rel'], r['loss_diff']))
    eng.set_engine(_lib.ENGINES['fused'])

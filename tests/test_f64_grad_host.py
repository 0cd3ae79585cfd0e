"""CPU: the float64 restatement of one GD-planner iteration (tests/_f64_grad_ref.py), the reference of the device's
drp_gd_grad_f64 (tests/test_gpu_gd_f64.py), pinned to the reference's own fp32 autograd on every gradient case of the golden
files, and checked against its own central differences.

Bounds (the project's rule for gradient bounds: 5 x the worst measured ratio to max |g_ref|).  Measured here, the
restatement against the fixture, max |g64 - g_ref| / max |g_ref|:

    seed-0 (grad.npz)          h1 4.4e-7   h2 5.9e-7   h1_n100 9.2e-7                     d / d state: 2.1e-6, 5.7e-7, 1.9e-6
    stress (grad_stress.npz)   seed1_attr_h1 8.6e-7   big_h1 3.0e-7   big_attr_h2 1.3e-6
    trained (trained.npz)      n20 1.1e-6, 1.5e-6   n50 9.8e-7, 1.1e-6   n100 1.0e-6, 3.7e-6   (h1, h2)

all of the order of fp32 autograd's own rounding (the fixture is the rounded side).  The state gradient is compared on the final
step's slice: the reference's retained gradient of its in-place-filled tensor shows no other (tests/test_gpu_gd.py)."""
import numpy as np
import pytest

import _f64_grad_ref as R
from dyn_res_pile_manip_amd import synthetic as syn
from dyn_res_pile_manip_amd.planners import world2cam_affine

GRAD_BOUND = {'seed0': 5e-6, 'stress': 7e-6, 'trained': 2e-5}      # 5 x 9.2e-7, 1.3e-6, 3.7e-6
GRAD_STATE_BOUND = 1.1e-5                                             # 5 x 2.1e-6
# Central differences at h = 2^-14: the truncation term is h^2 / 6 |f'''|; every derivative of the soft mask
# exp(-pen / 0.01) costs a factor of at most 1 / 0.01, so |f'''| <= 1e4 |f'| and the residual stays below
# 2^-28 / 6 x 1e4 = 6.2e-6 of the gradient's length (rounded up); the evaluations' own rounding (1e-16 / h) is far below
FD_BOUND = 1e-5

CASES = ([('seed0', c) for c in ('h1', 'h2', 'h1_n100')] + [('stress', c) for c in ('seed1_attr_h1', 'big_h1', 'big_attr_h2')] +
         [('trained', 'n%d_h%d' % (n, h)) for n in (20, 50, 100) for h in (1, 2)])


def case_inputs(golden, wset, case):
    """-> (weights, dict of the case's arrays) of a gradient case of grad.npz / grad_stress.npz / trained.npz"""
    if wset == 'seed0':
        g, p, w = golden.grad, case + '/', golden.weights_seed0
    elif wset == 'stress':
        from test_oracle_golden import stress_weights
        g, p = golden.grad_stress, case + '/'
        w = stress_weights(g, case)
    else:
        g, p, w = golden.trained, 'grad/' + case + '/', golden.weights_trained
    return w, dict((k, g[p + k]) for k in ('s_cur', 'dens', 'attr', 'act_seqs', 'goal_coor', 'reward', 'grad_act')
                   + (('grad_state_pred',) if p + 'grad_state_pred' in g.files else ()))


@pytest.fixture(scope='module')
def scene():
    return {'G': syn.goal_field(syn.goal_distance_image(syn.goal_mask('I'))), 'cam': syn.demo_cam_params(),
            'm34': world2cam_affine(syn.demo_cam_extrinsics())}


def restated(scene, w, c, acts=None, **kw):
    return R.gd_loss_and_grads64(w, c['s_cur'], c['dens'], c['attr'], c['act_seqs'] if acts is None else acts, scene['G'],
                                 scene['cam'], c['goal_coor'], scene['m34'], 24.0, **kw)


@pytest.mark.parametrize('wset,case', CASES)
def test_restatement_matches_the_references_autograd(golden, scene, wset, case):
    w, c = case_inputs(golden, wset, case)
    r, ga, gs = restated(scene, w, c)
    ref_r = c['reward'].reshape(len(r), -1)[:, 0]
    np.testing.assert_allclose(r, ref_r, rtol=2e-5)
    err = float(np.abs(ga - c['grad_act']).max() / np.abs(c['grad_act']).max())
    line = '[f64-ref] %s %s: d/d push %.3e' % (wset, case, err)
    assert ga.dtype == np.float64 and gs.dtype == np.float64
    if 'grad_state_pred' in c:
        ref = c['grad_state_pred']
        err_s = float(np.abs(gs[:, -1] - ref[:, -1]).max() / np.abs(ref).max())
        line += ', d/d state %.3e' % err_s
        print(line)
        assert err_s < GRAD_STATE_BOUND
    else:
        print(line)
    assert err < GRAD_BOUND[wset]
    assert err < 1e-3           # above this the restatement would be wrong, not loose


@pytest.mark.parametrize('wset,case', [('trained', 'n20_h1'), ('seed0', 'h2')])
def test_restatement_agrees_with_its_central_differences(golden, scene, wset, case):
    """8 directions in push space at h = 2^-14, none of which flips a neighbour list, the hard mask, the bilinear cell or the
    arg-min between -h and +h (at most 2 redrawn).  The residuals are recorded in _f64_grad_ref.FD_RESIDUAL: the device's own
    directional derivative is held to 10 x them."""
    w, c = case_inputs(golden, wset, case)

    def fn(a):
        r, ga, _, dec = restated(scene, w, c, acts=a, want_decisions=True)
        return r, ga, dec
    res = R.fd_check(fn, c['act_seqs'], n_dir=8, max_redraw=2)
    gnorm = float(np.linalg.norm(fn(R.fd_point(c['act_seqs']))[1]))
    worst = max(abs(cd - an) for cd, an in res) / gnorm
    print('[f64-ref] %s %s: central differences, worst residual %.3e of |g| = %.3e' % (wset, case, worst, gnorm))
    assert worst < FD_BOUND
    assert worst <= R.FD_RESIDUAL[case] * 1.0000001, 'the recorded residual is no longer the worst: record %.3e' % worst

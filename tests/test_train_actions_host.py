"""CPU: the float64 reference of training through the push (tests/_train_actions_ref.py: train_actions64) and the preconditions
of every comparison tests/test_gpu_train_actions.py makes.

(a) train_actions64 against its own central differences: a dozen weight entries, and one coordinate of a predicted state that a
    later step's push moves (the `nudge` pattern of tests/_untracked_ref.py) -- the push's position share is in that derivative.
(b) The preconditions, for every case of the GPU tests, at every step, on every real row of the float64 run: |u|, |u - L| and
    ||v| - w| above PUSH_MARGIN_MIN (the hard mask and the soft mask's kink cannot flip under fp32 drift), and every Chamfer
    arg-min margin above tests/_untracked_ref.py's MARGIN_MIN.
(c) The dataset's push_frame and the planner's frame from the engine's camera constants agree for the fixture camera; a loader
    batch's `actions` are the pickled pushes (its GPU half is in the GPU tests: the loader runs on the device).
(d) tests/golden/train_actions.npz (the reference's model and gen_s_delta in fp32 autograd) against train_actions64.
"""
import numpy as np
import pytest
import torch

import _f64_grad_ref as R
import _train_actions_ref as A
import _untracked_ref as U
from dyn_res_pile_manip_amd import synthetic as syn
from dyn_res_pile_manip_amd import weights

FD_H = 2.0 ** -20          # tests/test_f64_train_host.py derives both
FD_BOUND = 1e-5


@pytest.mark.parametrize('wset', ['seed0', 'trained'])
@pytest.mark.parametrize('name', ['b3_n24', 'b4_r3', 'b2_r5', 'n300', 'tiny', 'mask', 'golden'])
def test_push_margins_of_every_gpu_case(golden, name, wset):
    _, _, _, _, info = A.reference(golden, name, wset)
    print('[train-actions] %s %s: push margin %.3e' % (name, wset, info['push_margin']))
    assert info['push_margin'] > A.PUSH_MARGIN_MIN


@pytest.mark.parametrize('name,wset', A.TRAIN_CASES)
def test_chamfer_margins_of_every_gpu_case(golden, name, wset):
    _, _, _, _, info = A.reference(golden, name, wset, 'chamfer')
    print('[train-actions] %s %s chamfer: push margin %.3e, arg-min margin %.3e' % (name, wset, info['push_margin'], info['margin']))
    assert info['push_margin'] > A.PUSH_MARGIN_MIN and info['margin'] > U.MARGIN_MIN


@pytest.mark.parametrize('wset', ['seed0', 'trained'])
def test_the_mask_case_puts_zero_rows_into_real_rows_graphs(golden, wset):
    """sample 1 of the mask case lies around the camera-frame origin: at every step its zero rows are senders of real rows, no
    sender of a real row is within PUSH_MARGIN_MIN of the radius or of a tie at the top-10 cut (fp32 drift cannot change a
    graph), and the loop that gives the zero rows gen_s_delta's impulse (what an unmasked kernel computes) is outside the GPU
    tests' gradient bound on some tensor"""
    b = A.batch(golden, 'mask')
    nums = b[3]
    _, _, ref_blob, _, info = A.reference(golden, 'mask', wset)
    _, _, bad_blob, _, bad = A.reference(golden, 'mask', wset, masked=False)
    assert (b[0][1, :, 17:] == 0).all() and np.abs(b[0][1, :, :17, 2]).max() < 0.02
    for t in range(b[1].shape[1]):
        s_cur = b[0][:, 0].astype(np.float64) if t == 0 else info['preds'][:, t - 1]
        radius, gap = A.graph_margin(s_cur + info['sdelta'][:, t], nums)
        edges = int(info['graphs'][t][1, :17, 17:].sum())
        print('[train-actions] mask %s step %d: %d edges from zero rows to real rows, radius margin %.3e, cut gap %.3e'
              % (wset, t, edges, radius, gap))
        assert edges > 0 and radius > A.PUSH_MARGIN_MIN and gap > A.PUSH_MARGIN_MIN
    assert max(np.abs(bad['sdelta'][j, :, n:]).max() for j, n in enumerate(nums) if n < 24) > 0.05
    off, worst = 0, 0.0
    for key, shape in weights.STATE_DICT_KEYS:
        n = int(np.prod(shape))
        ref = np.abs(ref_blob[off:off + n]).max()
        worst = max(worst, np.abs(bad_blob[off:off + n] - ref_blob[off:off + n]).max() / max(ref, 1e-8))
        off += n
    print('[train-actions] mask %s: the unmasked loop is off by %.3e of a tensor\'s largest gradient' % (wset, worst))
    assert worst > 100 * A.GRAD_REL


def test_adam_trajectory_stays_inside_the_margin(golden):
    lr, beta1 = [float(v) for v in golden.train['b4_r3/lr_beta1']]
    _, _, _, margin = A.adam_trajectory64(golden, 'b3_n24', lr, beta1)
    assert margin > A.PUSH_MARGIN_MIN


def test_padded_rows_get_zero_and_real_rows_gen_s_delta(golden):
    b = A.batch(golden, 'mask')
    _, _, _, _, info = A.reference(golden, 'mask', 'seed0')
    nums = b[3]
    for j, n in enumerate(nums):
        assert (info['sdelta'][j, :, n:] == 0).all()
    sd0 = R.gen_s_delta(torch.from_numpy(b[0][:1, 0].astype(np.float64)), torch.from_numpy(b[1][:1, 0].astype(np.float64)),
                        torch.from_numpy(A.M34), A.GS)[0].numpy()
    np.testing.assert_array_equal(info['sdelta'][0, 0], sd0)
    # the push over the camera-frame origin WOULD move a zero row: the mask is not vacuous on this case
    z = R.gen_s_delta(torch.zeros((1, 1, 3), dtype=torch.float64), torch.from_numpy(b[1][:1, 0].astype(np.float64)),
                      torch.from_numpy(A.M34), A.GS)
    assert float(z.abs().max()) > 0.05


def test_reference_agrees_with_its_central_differences(golden):
    b = A.batch(golden, 'golden')
    W0 = dict((k, v.numpy().copy()) for k, v in R.weights64(golden.weights_seed0).items())
    loss, _, grads, gs, info0 = A.train_actions64(W0, *b, keep64=True)
    nums = b[3]
    keys = [p for p in A.PARAMS if p.endswith('.weight')]
    keys += [A.PARAMS[3], A.PARAMS[9], A.PARAMS[13]]                # three biases
    worst = 0.0

    def same_graphs(info):
        for a, c in zip(info['graphs'], info0['graphs']):
            for j, n in enumerate(nums):
                assert np.array_equal(a[j, :n], c[j, :n]), 'a neighbour list flips at h = %g' % FD_H
    for key in keys:
        flat = int(np.argmax(np.abs(grads[key])))
        vals = []
        for sgn in (1.0, -1.0):
            W = dict((k, v.copy()) for k, v in W0.items())
            W[key].reshape(-1)[flat] += sgn * FD_H
            l, _, _, _, info = A.train_actions64(W, *b, keep64=True)
            same_graphs(info)
            vals.append(l)
        cd = (vals[0] - vals[1]) / (2 * FD_H)
        res = abs(cd - grads[key].reshape(-1)[flat]) / np.abs(grads[key]).max()
        worst = max(worst, res)
        assert res < FD_BOUND, (key, flat, cd, grads[key].reshape(-1)[flat])
    print('[train-actions] central differences on %d weight entries, worst residual %.3e' % (len(keys), worst))
    # one coordinate of a predicted state: the row of step 0 whose impulse at step 1 is the largest (the push's share is in it)
    j = 0
    i = int(np.argmax(np.abs(info0['sdelta'][j, 1]).max(-1)))
    assert np.abs(info0['sdelta'][j, 1, i]).max() > 1e-3
    for k in range(3):
        vals = []
        for sgn in (1.0, -1.0):
            l, _, _, _, info = A.train_actions64(W0, *b, keep64=True, nudge=(0, j, i, k, sgn * FD_H))
            same_graphs(info)
            vals.append(l)
        cd = (vals[0] - vals[1]) / (2 * FD_H)
        res = abs(cd - gs[j, 0, i, k]) / np.abs(gs[j, 0]).max()
        print('[train-actions] d loss / d s_pred_0[%d, %d, %d]: autograd %.6e, central difference %.6e' % (j, i, k, gs[j, 0, i, k], cd))
        assert res < FD_BOUND


def test_push_share_is_not_negligible_on_the_trained_cases(golden):
    """without the push's position share every gradient tensor is another number on the trained weights (measured: 0.14 to 1.0
    of a tensor's largest gradient on b3_n24): a backward pass that drops the share cannot hide inside GRAD_REL there.  On the
    seed-0 weights, whose predictor is scaled by 0.02, the share is 2e-4 to 4e-4 -- those cases hold the forward pass and the
    mask, the trained ones the share."""
    import _f64_train_ref as T
    b = A.batch(golden, 'b3_n24')
    _, _, grads, _, info = A.train_actions64(golden.weights_trained, *b)
    # the same impulses fed as data: the loop of tests/_f64_train_ref.py, whose gradient lacks the share
    _, _, g2, _ = T.train_loss_and_grads64(golden.weights_trained, b[0], info['sdelta'].astype(np.float32), b[2], b[3], b[4])
    rels = [float(np.abs(grads[k] - g2[k]).max() / np.abs(grads[k]).max()) for k in A.PARAMS]
    print('[train-actions] gradient without the push share, per tensor: %s' % ' '.join('%.1e' % r for r in rels))
    assert min(rels) > 100 * A.GRAD_REL


def test_dataset_frame_and_planner_frame_agree():
    from dyn_res_pile_manip_amd.dataset_gnn_dyn import push_frame
    rng = np.random.default_rng(5)
    for _ in range(8):
        act = rng.uniform(-4, 4, 4)
        f = push_frame(act, syn.demo_cam_extrinsics(), A.GS)
        sc, ec, dirn, length = A._frame(torch.from_numpy(act[None]))
        np.testing.assert_allclose(f[0:3], sc[0].numpy(), rtol=0, atol=1e-12)
        np.testing.assert_allclose(f[3:6], ec[0].numpy(), rtol=0, atol=1e-12)
        np.testing.assert_allclose(f[6:9], dirn[0].numpy(), rtol=0, atol=1e-12)
        assert abs(f[9] - float(length[0])) < 1e-12
    # the engine's camera constants are the fp32 cast of the same matrix
    from dyn_res_pile_manip_amd.planners import world2cam_affine
    np.testing.assert_array_equal(world2cam_affine(syn.demo_cam_extrinsics()), A.M34.astype(np.float32))


def test_reference_fixture(golden):
    """tests/golden/train_actions.npz: the reference's model and PlannerGD.gen_s_delta on s_cur[b, :n], fp32 autograd -- within
    the distance the reference's own fp32 autograd keeps from float64 on train.npz (test_f64_train_host.py: below 1e-6 of a
    tensor's largest gradient; asserted at that test's 1e-4 sanity bound, a wrong restatement is off by its own size)"""
    g = golden.train_actions
    b = A.batch(golden, 'golden')
    for k, a in zip(('states', 'actions', 'attrs', 'particle_nums', 'particle_dens'), b):
        np.testing.assert_array_equal(g[k], a)
    assert g['states'].shape == (2, 4, 16, 3) and list(g['particle_nums']) == [16, 11]
    loss, _, blob, _, _ = A.reference(golden, 'golden', 'seed0')
    _, _, grads, _, _ = A.train_actions64(golden.weights_seed0, *b)
    assert abs(loss - float(g['loss'])) < 1e-5 * loss
    worst = 0.0
    assert len([k for k in g.files if k.startswith('grad/')]) == 18
    for k in A.PARAMS:
        ref = g['grad/' + k].astype(np.float64)
        err = float(np.abs(grads[k] - ref).max() / np.abs(grads[k]).max())
        print('[train-actions] reference fp32 autograd, %-45s %.3e' % (k, err))
        worst = max(worst, err)
    assert worst < 1e-4

"""CPU: the host side of training on a caller's loss (drp_train_predict / drp_train_step_seeded and their float64 pair).

(a) tests/_seeded_ref.py -- the float64 loop with the loss as an argument, the reference of tests/test_gpu_train_seeded.py -- fed
    the MSE reproduces tests/_f64_train_ref.py: loss, terms, every parameter gradient and the state gradient within 1e-12 of each
    tensor's largest entry (the same graph and the same expressions: only autograd's accumulation order can differ), and its seed
    is the MSE's own 2 d / (3 n_b H B).
(b) losses.mse_loss and losses.pseudo_huber_loss return the gradient of their own value (central differences in float64), and
    losses.torch_loss of the same expressions returns the same value and gradient, for float32 and float64 input; padded rows
    come back exactly 0.
(c) the trainer's option checks: a callable loss, --loss-fn, custom_probe_every.
(d) the staged batch's layout with and without the seed block: today's calls' layouts are unchanged."""
import os
import subprocess

import numpy as np
import pytest

import _f64_train_ref as T
import _seeded_ref as S
from dyn_res_pile_manip_amd import losses, train_gnn_dyn as TG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12
BATCH_KEYS = ('states', 'states_delta', 'attrs', 'particle_nums', 'particle_dens')
CASES = [(b, w) for b in ('b4_r3', 'b2_r5') for w in ('seed0', 'trained')]


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300))


# ---- (a) the restatement --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,wset', CASES)
def test_restatement_with_the_mse_is_the_training_restatement(golden, name, wset):
    batch = [golden.train[name + '/' + k] for k in BATCH_KEYS]
    W = golden.weights_seed0 if wset == 'seed0' else golden.weights_trained
    loss, terms, grads, gs = T.train_loss_and_grads64(W, *batch)
    closs, cgrads, cgs, pred, seed = S.train_loss_and_grads64_custom(W, batch, S.mse_torch)
    import torch
    cterms = S.mse_terms_torch(torch.from_numpy(pred), batch).numpy()
    figures = {'loss': abs(closs - loss) / abs(loss), 'terms': rel(cterms, terms), 'grad_state': rel(cgs, gs)}
    for k in T.PARAMS:
        figures[k] = rel(cgrads[k], grads[k])
    worst = max(figures, key=lambda k: figures[k])
    print('[seeded-ref] %s %s: worst %s %.2e of the tensor\'s largest entry' % (name, wset, worst, figures[worst]))
    for k, v in figures.items():
        assert v <= TOL, (k, v)
    # the seed is the loss term's own derivative, with no share of the later steps: the MSE's, restated
    nums = np.asarray(batch[3])
    B, H = pred.shape[:2]
    want = np.zeros_like(pred)
    for b in range(B):
        n = int(nums[b])
        want[b, :, :n] = 2.0 * (pred[b, :, :n] - batch[0][b, 1:, :n].astype(np.float64)) / (3.0 * n * H * B)
    err = rel(seed, want)
    print('[seeded-ref] %s %s: seed against 2 d / (3 n H B): %.2e' % (name, wset, err))
    assert err <= TOL
    np.testing.assert_array_equal(seed[:, -1], cgs[:, -1])            # the last step has no later one: seed and total agree there
    assert np.abs(seed[:, 0] - cgs[:, 0]).max() > 0                    # ... and every earlier step does
    for b in range(B):
        assert not seed[b, :, int(nums[b]):].any()


# ---- (b) the example losses and the adapter ---------------------------------------------------------------------------------
# Central differences at h = 2^-20 in one coordinate of the prediction, in float64, as tests/test_f64_train_host.py takes its own.
# Truncation h^2 / 6 |f'''|: the MSE is a quadratic (none); pseudo-Huber's third derivative in d is at most 0.86 / delta^2 =
# 0.86 x 400 = 344 at the densities below, so 2^-40 / 6 x 344 = 5.2e-11 times the term's weight w = 1 / (3 n H B), against a
# largest gradient of the order of |d| w = 0.05 w: 1e-9 of it.  Rounding: two evaluations of a value of at most 1e-2 (some 60 terms
# of 2^-53 relative each) divided by 2 h: 1e-2 x 60 x 1.1e-16 / 1.9e-6 = 3.5e-11 absolute, against gradients of 0.05 / 60 = 8e-4:
# 4e-8.  Bound: 1e-6 of the largest gradient.
FD_H = 2.0 ** -20
FD_BOUND = 1e-6


def small_batch(dtype=np.float64):
    """2 samples x 2 steps x 5 rows, the second sample with one padded row; displacements of the order of one sampling spacing
    (delta = 0.05 at density 400), so that pseudo-Huber is read on both sides of its bend -> (pred, context)"""
    rng = np.random.default_rng(7)
    B, H, N = 2, 2, 5
    nums = np.array([5, 4], np.int32)
    dens = np.array([400.0, 380.0], np.float32)
    states = rng.standard_normal((B, H + 1, N, 3)).astype(np.float32) * 0.2
    pred = states[:, 1:].astype(np.float64) + 0.05 * rng.standard_normal((B, H, N, 3))
    for b in range(B):
        states[b, :, nums[b]:] = 0.0
        pred[b, :, nums[b]:] = 123.0                    # what the forward leaves on a padded row is not the loss's to read
    context = [states, None, np.zeros((B, H + 1, N), np.float32), nums, dens]
    return pred.astype(dtype), context


@pytest.mark.parametrize('fn', [losses.mse_loss, losses.pseudo_huber_loss], ids=['mse', 'pseudo_huber'])
def test_example_losses_return_the_gradient_of_their_value(fn):
    pred, context = small_batch()
    value, grad = fn(pred, context)
    assert grad.dtype == np.float64 and grad.shape == pred.shape and isinstance(value, float)
    nums = context[3]
    worst = 0.0
    for b in range(pred.shape[0]):
        assert (grad[b, :, nums[b]:] == 0.0).all()                      # padded rows: exactly 0
        for idx in np.ndindex(pred.shape[1], int(nums[b]), 3):
            vals = []
            for sgn in (1.0, -1.0):
                p = pred.copy()
                p[(b,) + idx] += sgn * FD_H
                vals.append(fn(p, context)[0])
            cd = (vals[0] - vals[1]) / (2 * FD_H)
            worst = max(worst, abs(cd - grad[(b,) + idx]) / np.abs(grad).max())
    print('[seeded-losses] %s: central differences on every real coordinate, worst residual %.3e of the largest gradient'
          % (fn.__name__, worst))
    assert worst < FD_BOUND
    moved = pred.copy()
    moved[1, :, nums[1]:] = -7.0                                        # the padding is not read
    v2, g2 = fn(moved, context)
    assert v2 == value
    np.testing.assert_array_equal(g2, grad)


# float64: both sides evaluate the same expressions in double, in different orders: 1e-12.  float32: every value passes a handful
# of roundings of 2^-24 = 6e-8 relative (the difference, the square, the quotient by delta^2 on one side and the product with the
# density on the other, the root, the divisions) and d itself carries up to one rounding of a coordinate of 0.6, 3.6e-8 absolute
# against displacements of 0.05 -- 7e-7 of the largest; the sum of 54 terms adds under 54 x 6e-8.  Bound: 1e-5.
@pytest.mark.parametrize('dtype,tol', [(np.float64, 1e-12), (np.float32, 1e-5)], ids=['f64', 'f32'])
@pytest.mark.parametrize('fn,fn_torch', [(losses.mse_loss, S.mse_torch), (losses.pseudo_huber_loss, S.pseudo_huber_torch)],
                         ids=['mse', 'pseudo_huber'])
def test_torch_loss_of_the_same_expression_agrees(fn, fn_torch, dtype, tol):
    pred, context = small_batch(dtype)
    value, grad = fn(pred, context)
    tvalue, tgrad = losses.torch_loss(fn_torch)(pred, context)
    assert grad.dtype == dtype and tgrad.dtype == dtype and tgrad.shape == pred.shape
    figures = (abs(tvalue - value) / abs(value), rel(tgrad, grad))
    print('[seeded-losses] %s %s: torch_loss against numpy: value %.2e, gradient %.2e' % ((fn.__name__, np.dtype(dtype).name) + figures))
    assert figures[0] <= tol and figures[1] <= tol
    nums = context[3]
    for b in range(pred.shape[0]):
        assert (tgrad[b, :, nums[b]:] == 0.0).all() and (grad[b, :, nums[b]:] == 0.0).all()


def test_torch_loss_refuses_what_is_no_scalar():
    pred, context = small_batch()
    with pytest.raises(ValueError, match='scalar'):
        losses.torch_loss(lambda p, c: p.sum(0))(pred, context)


# ---- (c) the option checks ----------------------------------------------------------------------------------------------------
OLDER = ('grad_probe_every', 'probe_every', 'sinkhorn_probe_every', 'match_probe_every', 'sinkhorn_reach_probe_every')


def test_a_callable_loss_is_accepted_and_strings_are_what_they_were():
    TG.check_loss(losses.mse_loss)
    TG.check_probe_options(losses.mse_loss, 0, 0)
    TG.check_custom_probe_option(losses.mse_loss, 3)
    TG.check_custom_probe_option('mse', 0, grad_probe_every=2)
    assert TG.resolve_data_options('particles', losses.mse_loss, None) == (losses.mse_loss, 'data')
    assert TG.resolve_data_options('depth', losses.mse_loss, None) == (losses.mse_loss, 'actions')
    with pytest.raises(ValueError, match='loss must be one of'):
        TG.check_loss('huber')
    assert TG.LOSSES == ('mse', 'chamfer')


def test_custom_probe_every_needs_a_callable_loss_and_stands_alone():
    with pytest.raises(ValueError, match='custom_probe_every needs a callable loss'):
        TG.check_custom_probe_option('mse', 2)
    with pytest.raises(ValueError, match='non-negative integer'):
        TG.check_custom_probe_option(losses.mse_loss, -1)
    for name in OLDER:
        with pytest.raises(ValueError, match='give custom_probe_every alone'):
            TG.check_custom_probe_option('mse', 2, **{name: 2})
    with pytest.raises(ValueError, match='custom_probe_every needs a callable loss'):
        TG.train({'train': {'n_rollout': 1, 'n_history': 1}}, None, {}, custom_probe_every=2)


@pytest.mark.parametrize('name', OLDER)
def test_the_older_probe_options_refuse_a_callable_loss_by_name(name):
    with pytest.raises(ValueError, match='%s probes the built-in losses: a callable loss \\(pseudo_huber_loss\\)' % name):
        TG.train({'train': {'n_rollout': 1, 'n_history': 1}}, None, {}, loss=losses.pseudo_huber_loss, **{name: 2})
    with pytest.raises(ValueError, match=name + ' probes the built-in losses'):
        TG.check_custom_probe_option(losses.pseudo_huber_loss, 0, **{name: 1})


def test_the_command_line_takes_loss_fn_or_loss(capsys):
    assert TG.load_loss_fn('dyn_res_pile_manip_amd.losses:pseudo_huber_loss') is losses.pseudo_huber_loss
    with pytest.raises(ValueError, match='not callable'):
        TG.load_loss_fn('dyn_res_pile_manip_amd.train_gnn_dyn:LOSSES')
    with pytest.raises(ValueError, match='package.module:attribute'):
        TG.load_loss_fn('dyn_res_pile_manip_amd.losses')
    for argv, word in ((['--loss', 'mse', '--loss-fn', 'dyn_res_pile_manip_amd.losses:mse_loss'], 'not both'),
                       (['--loss-fn', 'dyn_res_pile_manip_amd.train_gnn_dyn:LOSSES'], 'not callable'),
                       (['--custom-probe-every', '2'], 'needs a callable loss'),
                       (['--loss-fn', 'dyn_res_pile_manip_amd.losses:mse_loss', '--probe-every', '2'], 'probe_every probes the built-in')):
        with pytest.raises(SystemExit):
            TG._cli(argv)
        assert word in capsys.readouterr().err


def test_a_depth_only_batch_takes_a_callable_loss_through_the_push_alone():
    data = TG.PaddedBatch((None,) * 6)
    data.depth_only = True
    TG.check_depth_only(data, losses.mse_loss, 'actions')
    with pytest.raises(ValueError, match='depth-only'):
        TG.check_depth_only(data, losses.mse_loss, 'data')


# ---- (d) the layout ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def host_check(tmp_path_factory):
    import __graft_entry__ as g
    exe = str(tmp_path_factory.mktemp('host_check') / 'train_host_check')
    subprocess.check_call([g.HIPCC, '-x', 'c++', '-std=c++17', '-O1', os.path.join(ROOT, 'tools', 'train_host_check.cpp'), '-o', exe])
    return exe


def layout(exe, B, H, N, M, actions, eps, reach, seed):
    out = subprocess.check_output([exe, 'layout'] + [str(int(v)) for v in (B, H, N, M, actions, eps, reach, seed)]).decode().split()
    return dict(zip(('states', 'sdelta', 'attrs', 'dens', 'nums', 'targets', 'tnums', 'bytes', 'eps', 'rho', 'mass_q', 'seed'),
                    [int(v) for v in out]))


def up(v):
    return (v + 15) // 16 * 16


@pytest.mark.parametrize('B,H,N,M,actions,eps,reach', [(4, 5, 300, 0, 0, 0, 0), (3, 3, 23, 17, 1, 0, 0), (2, 1, 7, 5, 0, 1, 0),
                                                        (2, 5, 11, 9, 1, 1, 1), (1, 1, 1, 0, 0, 0, 0)])
def test_the_seed_block_lies_behind_a_batch_that_did_not_move(host_check, B, H, N, M, actions, eps, reach):
    plain = layout(host_check, B, H, N, M, actions, eps, reach, 0)
    # today's layout, summed by hand from its description: states | impulses | attributes | densities | counts [| targets | counts]
    # [| eps [| rho | mass_q]], every block on 16 bytes
    at = {'states': 0}
    at['sdelta'] = up(B * (H + 1) * N * 3 * 4)
    at['attrs'] = up(at['sdelta'] + (B * H * 4 if actions else B * H * N * 3) * 4)
    at['dens'] = up(at['attrs'] + B * (H + 1) * N * 4)
    at['nums'] = up(at['dens'] + B * 4)
    end = up(at['nums'] + B * 4)
    at['targets'] = at['tnums'] = at['eps'] = at['rho'] = at['mass_q'] = 0
    if M > 0:
        at['targets'] = end
        at['tnums'] = up(end + B * H * M * 3 * 4)
        end = up(at['tnums'] + B * H * 4)
    if eps:
        at['eps'] = end
        end = up(end + B * 8)
    if eps and reach:
        at['rho'] = end
        at['mass_q'] = up(end + B * 8)
        end = up(at['mass_q'] + H * B * 8)
    at['bytes'], at['seed'] = end, 0
    assert plain == at
    seeded = layout(host_check, B, H, N, M, actions, eps, reach, 1)
    assert seeded['seed'] == plain['bytes'] and seeded['bytes'] == up(plain['bytes'] + B * H * N * 3 * 4)
    for k in plain:
        if k not in ('seed', 'bytes'):
            assert seeded[k] == plain[k], k


def test_the_host_check_program_covers_the_seed_and_passes(host_check):
    src = open(os.path.join(ROOT, 'tools', 'train_host_check.cpp')).read()
    assert 'stage_seed(' in src and 'first_bad_seed(' in src
    assert 'all checks passed' in subprocess.check_output([host_check]).decode()

"""CPU: the float64 restatement of the training loop body (tests/_f64_train_ref.py), the reference of the device's
drp_train_grad_f64 (tests/test_gpu_train_f64.py), pinned two ways.

(a) To the reference's own model run in double (tests/golden/train_f64.npz, written by make_golden_train_f64.py, which also
asserts that every step's adjacency of the double positions is that of their fp32 roundings): loss, loss terms and every
parameter's gradient within 1e-10 x the largest magnitude of the compared tensor, the bound the float64 calls are held to --
both sides evaluate the same expressions in double on the same graph and differ in summation order only.

(b) To its own central differences on a dozen weight entries spread over all nine layers.

Also printed: how far the reference's fp32 autograd gradients of train.npz lie from float64 (measured: at most
6.3e-7 of a tensor's largest gradient on b4_r3, 3.9e-7 on b2_r5)."""
import numpy as np
import pytest

import _f64_train_ref as T

TOL = 1e-10
BATCH_KEYS = ('states', 'states_delta', 'attrs', 'particle_nums', 'particle_dens')
CASES = [(b, w) for b in ('b4_r3', 'b2_r5') for w in ('seed0', 'trained')]
# Central differences at h = 2^-20 in one weight entry.  Truncation h^2 / 6 |f'''|: between two ReLU kinks the loss is a
# polynomial in the entry whose every further derivative costs at most a factor of the order of the activations times the
# weights it passes, generously 1e2 each, so 2^-40 / 6 x 1e4 = 1.5e-9 of the derivative.  Rounding: two evaluations of a loss of
# ~5e-4 (some 1e3 roundings of 2^-53 each on the path of one entry) divided by 2 h = 5e-4 x 1e-13 / 2e-6 = 3e-11 absolute,
# against gradient entries of 1e-5 and more: 3e-6.  Bound: 1e-5 of the tensor's largest gradient (FD_BOUND of
# test_f64_grad_host.py, by the same reasoning).
FD_H = 2.0 ** -20
FD_BOUND = 1e-5


def batch_of(golden, name):
    return [golden.train[name + '/' + k] for k in BATCH_KEYS]


def weights_of(golden, wset):
    return golden.weights_seed0 if wset == 'seed0' else golden.weights_trained


_cache = {}


def restated(golden, name, wset):
    if (name, wset) not in _cache:
        _cache[(name, wset)] = T.train_loss_and_grads64(weights_of(golden, wset), *batch_of(golden, name))
    return _cache[(name, wset)]


@pytest.mark.parametrize('name,wset', CASES)
def test_restatement_matches_the_reference_model_in_double(golden, name, wset):
    g = golden.train_f64
    p = '%s/%s/' % (name, wset)
    loss, terms, grads, _ = restated(golden, name, wset)
    assert abs(loss - float(g[p + 'loss'])) <= TOL * abs(float(g[p + 'loss']))
    assert np.abs(terms - g[p + 'loss_terms']).max() <= TOL * np.abs(g[p + 'loss_terms']).max()
    worst = 0.0
    for k in T.PARAMS:
        ref = g[p + 'grad/' + k]
        assert grads[k].dtype == np.float64 and grads[k].shape == ref.shape
        err = float(np.abs(grads[k] - ref).max() / max(np.abs(ref).max(), 1e-300))
        worst = max(worst, err)
        assert err <= TOL, (k, err)
    print('[f64-train-ref] %s %s: worst error %.2e of a tensor\'s largest gradient' % (name, wset, worst))


@pytest.mark.parametrize('name', ['b4_r3', 'b2_r5'])
def test_report_the_references_fp32_autograd_against_float64(golden, name):
    """train.npz holds the reference's fp32 gradients of the first iteration on the seed-0 weights: a figure, and a sanity
    bound far above fp32 rounding (a wrong restatement would be off by its own size)"""
    g64 = golden.train_f64
    worst = 0.0
    for k in T.PARAMS:
        ref = g64['%s/seed0/grad/%s' % (name, k)]
        err = float(np.abs(golden.train['%s/grad/%s' % (name, k)].astype(np.float64) - ref).max() / np.abs(ref).max())
        print('[f64-train-ref] %s reference fp32 autograd, %-45s %.3e' % (name, k, err))
        worst = max(worst, err)
    assert worst < 1e-4


def fd_entries(grads):
    """the largest entry of each of the nine weight tensors, and of three biases: a dozen"""
    keys = [k + '.weight' for k in T.KEYS] + [T.KEYS[1] + '.bias', T.KEYS[4] + '.bias', T.KEYS[6] + '.bias']
    return [(k, int(np.argmax(np.abs(grads[k])))) for k in keys]


@pytest.mark.parametrize('name,wset', [('b2_r5', 'seed0'), ('b2_r5', 'trained')])
def test_restatement_agrees_with_its_central_differences(golden, name, wset):
    batch = batch_of(golden, name)
    W0 = dict((k, v.numpy().copy()) for k, v in T.weights64(weights_of(golden, wset)).items())
    loss, _, grads, _, graphs0 = T.train_loss_and_grads64(W0, *batch, keep64=True, want_graphs=True)
    nums = batch[3]
    worst = 0.0
    for key, flat in fd_entries(grads):
        vals = []
        for sgn in (1.0, -1.0):
            W = dict((k, v.copy()) for k, v in W0.items())
            W[key].reshape(-1)[flat] += sgn * FD_H
            l, _, _, _, graphs = T.train_loss_and_grads64(W, *batch, keep64=True, want_graphs=True)
            for a, b in zip(graphs, graphs0):                       # the graph of the real rows is a constant of the derivative
                for j, n in enumerate(nums):
                    assert np.array_equal(a[j, :n], b[j, :n]), 'a neighbour list flips at h = %g in %s' % (FD_H, key)
            vals.append(l)
        cd = (vals[0] - vals[1]) / (2 * FD_H)
        res = abs(cd - grads[key].reshape(-1)[flat]) / np.abs(grads[key]).max()
        worst = max(worst, res)
        assert res < FD_BOUND, (key, flat, cd, grads[key].reshape(-1)[flat])
    print('[f64-train-ref] %s %s: central differences on 12 entries, worst residual %.3e of the tensor\'s largest gradient'
          % (name, wset, worst))

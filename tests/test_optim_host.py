"""CPU: the optimiser seam's host side -- the trainer's option checks, the four calls' signatures, and the numpy restatement the
GPU tests hold the device to (tests/_optim_ref.py) against torch.nn.utils.clip_grad_norm_ on random float64 blobs.

Bound: 1e-15 of the norm, of the factor and of the clipped gradient's largest entry.  Both sides are float64; they differ in the
order of one sum of 38 403 squares (numpy's pairwise sum against torch's vector_norm, and with the blob cut into the model's
tensors a norm of norms), a few units in the last place."""
import ctypes

import numpy as np
import pytest

import _optim_ref as R
from dyn_res_pile_manip_amd import _lib, train_gnn_dyn as TG, weights

TOL = 1e-15
N = _lib.DRP_N_WEIGHTS


def test_option_checks():
    for ok in ((1, None), (2, None), (1, 0.5), (7, 1e9), (1, float('inf')), (2.0, 3)):
        TG.check_optim_options(*ok)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match='accum_steps must be an integer >= 1'):
            TG.check_optim_options(bad, None)
    for bad in (0, 0.0, -1.0, float('nan'), float('-inf')):
        with pytest.raises(ValueError, match='clip_norm must be a number > 0'):
            TG.check_optim_options(1, bad)
    every = {option: 0 for option in TG.SCHEDULES}
    assert TG.check_train_options('mse', every, accum_steps=4, clip_norm=1.0).loss == 'mse'
    with pytest.raises(ValueError, match='accum_steps'):
        TG.check_train_options('mse', every, accum_steps=0)
    with pytest.raises(ValueError, match='clip_norm'):
        TG.check_train_options('sinkhorn', every, clip_norm=-2.0)
    with pytest.raises(ValueError, match='loss must be one of'):           # the older refusals come first
        TG.check_train_options('nope', every, accum_steps=0)
    with pytest.raises(ValueError, match='accum_steps'):                    # the command line's part has them too
        TG.check_train_options('mse', every, usage_only=True, accum_steps=0)


def test_cli_refuses_bad_options_as_usage_errors(capsys):
    for argv in (['--accum-steps', '0'], ['--clip-norm', '0'], ['--clip-norm', '-1']):
        with pytest.raises(SystemExit) as e:
            TG._cli(argv)
        assert e.value.code == 2
    assert 'clip_norm must be a number > 0' in capsys.readouterr().err


def test_signatures_of_the_four_calls():
    S = _lib.SIGNATURES
    dp, fp = _lib.c_double_p, _lib.c_float_p
    assert S['drp_train_accumulate'] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_double])
    assert S['drp_train_apply'] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_double, ctypes.c_double, dp, dp,
                                                   ctypes.POINTER(ctypes.c_int), fp])
    assert S['drp_train_get_state'] == (ctypes.c_int, [ctypes.c_void_p, fp, fp, ctypes.POINTER(ctypes.c_int64)])
    assert S['drp_train_set_state'] == (ctypes.c_int, [ctypes.c_void_p, fp, fp, ctypes.c_int64])


def _torch_clip(blob, max_norm, split):
    """torch's clip_grad_norm_ on the blob as one parameter, or cut into the model's tensors -> (total_norm, clipped blob)"""
    import torch
    if split:
        sizes = [int(np.prod(shape)) for _, shape in weights.STATE_DICT_KEYS]
        parts = np.split(blob, np.cumsum(sizes)[:-1])
    else:
        parts = [blob]
    params = []
    for p in parts:
        t = torch.zeros(p.shape, dtype=torch.float64, requires_grad=True)
        t.grad = torch.from_numpy(p.copy())
        params.append(t)
    total = torch.nn.utils.clip_grad_norm_(params, max_norm)
    return float(total), np.concatenate([t.grad.numpy() for t in params])


@pytest.mark.parametrize('split', [False, True], ids=['one-tensor', 'model-tensors'])
@pytest.mark.parametrize('seed', [0, 1, 2])
def test_restatement_against_torch_clip_grad_norm(seed, split):
    rng = np.random.default_rng(seed)
    g1, g2 = (rng.standard_normal(N).astype(np.float32) * np.float32(10.0 ** rng.integers(-4, 2)) for _ in range(2))
    acc = R.accumulate(R.accumulate(None, g1, 2), g2, 3)
    np.testing.assert_array_equal(acc, 2.0 * g1.astype(np.float64) + 3.0 * g2.astype(np.float64))
    scale = 1.0 / 5.0
    unclipped = R.norm(acc, scale)
    for max_norm in (0.5 * unclipped, 1e-3 * unclipped, 2.0 * unclipped):
        n, c, g = R.apply(acc, scale, max_norm)
        t_norm, t_grad = _torch_clip(scale * acc, max_norm, split)
        g64 = acc * (scale * c)
        figures = {'norm': abs(n - t_norm) / t_norm,
                   'clip': abs(c - min(1.0, max_norm / (t_norm + 1e-6))) / c,
                   'grad': float(np.abs(g64 - t_grad).max() / np.abs(t_grad).max())}
        print('[optim-host] seed %d %s max_norm/norm %.3g: %s' % (seed, 'split' if split else 'whole', max_norm / unclipped, figures))
        for k, v in figures.items():
            assert v <= TOL, (k, v)
        assert (c == 1.0) == (max_norm > unclipped)
        np.testing.assert_array_equal(g, g64.astype(np.float32))
    assert R.apply(acc, scale, None)[1] == 1.0
    np.testing.assert_array_equal(R.apply(acc, scale, None)[2], (acc * scale).astype(np.float32))

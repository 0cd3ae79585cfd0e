"""CPU: the float64 backward pass from given activations (tests/_rgr_train_ref.py: backward64_from_taps and
forward_layer_ratios) -- it restates autograd, an honest float32 run stays far inside its elementwise bound, and every
fault a kernel of csrc/k_rgr_bwd.h or csrc/k_rgr.h could plausibly make lands far outside it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _rgr_ref  # noqa: E402
import _rgr_train_ref as R  # noqa: E402

TOL = R.CW_TOL
LAM = 5e4
WG_SPLIT = (256, 32, 8, 2, 1)       # the kernels' fixed split-K per conv layer (capi_rgr_train.h: RGR_WG_SPLIT)
CS_CHUNK = 1024                     # rows per column-sum partial (k_rgr_bwd.h: RGR_CS_CHUNK)


def batch(B, n_out):
    x = np.stack([_rgr_ref.rand_input(900 + i, 1)[0] for i in range(B)]).astype(np.float32)
    x[-1, :, :, :7] = 0.0                                   # a blank strip: exact zeros at the left border
    rng = np.random.Generator(np.random.PCG64(B))
    if n_out == 1:
        return x, {'y': rng.uniform(20, 130, B).astype(np.float32), 'conf': rng.uniform(0.05, 1, B).astype(np.float32)}
    return x, {'label': (np.arange(B) % 6).astype(np.int32)}


_CASES = {}


def case(B, n_out):
    """(sd, x, targets, out, taps, g_ref, g_abs) on float64 taps, cached: the zero-unit weights, lam_reg > 0"""
    if (B, n_out) not in _CASES:
        sd = R.zero_units(R.fixture_state_dict(7, n_out))
        x, t = batch(B, n_out)
        out, taps = _rgr_ref.forward64(sd, x)
        g, ga = R.backward64_from_taps(sd, x, taps, out, lam_reg=LAM, **t)
        _CASES[(B, n_out)] = (sd, x, t, out, taps, g, ga)
    return _CASES[(B, n_out)]


@pytest.mark.parametrize('n_out', [1, 6])
def test_backward_from_taps_matches_autograd(n_out):
    sd, x, t, out, taps, g, ga = case(2, n_out)
    assert np.abs(taps['c3'][:, R.ZERO_CONV3_CHANNEL]).max() == 0 and np.abs(taps['f2'][:, R.ZERO_FC2_ROW]).max() == 0
    _, _, _, g_auto = R.loss_grad64(sd, x, lam_reg=LAM, **t)
    for k, v in g_auto.items():
        assert np.abs(g[k] - v).max() <= 1e-12 * np.abs(v).max(), k
    r = R.componentwise_ratio(g_auto, g, ga)
    assert max(r.values()) <= 1e-12, r


@pytest.mark.parametrize('B,n_out', [(2, 1), (1, 6)])
def test_float32_backward_inside_the_bound(B, n_out):
    """the same backward in torch float32 on float32 taps: its rounding against the bound, at TOL / 10"""
    import torch
    sd, x, t, _, _, _, _ = case(B, n_out)
    out, taps = R.forward_taps(sd, x, torch.float32)
    g32, _ = R.backward64_from_taps(sd, x, taps, out, lam_reg=LAM, dtype=torch.float32, bound=False, **t)
    g, ga = R.backward64_from_taps(sd, x, taps, out, lam_reg=LAM, **t)
    r = R.componentwise_ratio(g32, g, ga)
    rf = R.forward_layer_ratios(sd, x, taps, out)
    print('\n[grad-err] float32 stand-in B=%d n_out=%d, max |g - g_ref| / g_abs: %s' % (
        B, n_out, ', '.join('%s %.1e' % (k[6:], v) for k, v in r.items())))
    print('[fwd-err] float32 stand-in B=%d n_out=%d, per layer: %s' % (
        B, n_out, ', '.join('%s %.1e' % kv for kv in rf.items())))
    assert max(r.values()) <= TOL / 10 and max(rf.values()) <= TOL / 10


# ---- injected faults: each stands for one kernel detail --------------------------------------------------------------
def _rows_from(dz, k0):
    """dz [B,C,OH,OW] with its rows k >= k0 zeroed; k = (b, oh, ow), the device's NHWC row order"""
    import torch
    B, _, OH, OW = dz.shape
    return dz * (torch.arange(B * OH * OW).reshape(B, 1, OH, OW) < k0).to(dz.dtype)


def conv1_wgrad_loses_last_slab(orig):
    def f(a, dz, shape, l):
        if l == 0:
            K = dz.shape[0] * dz.shape[2] * dz.shape[3]
            kc = -(-(-(-K // WG_SPLIT[0])) // 32) * 32       # k_rgr_conv_wgrad's share: ceil(K / S), rounded up to 32
            dz = _rows_from(dz, (K - 1) // kc * kc)
        return orig(a, dz, shape, l)
    return f


def conv3_dgrad_loses_parity_11(orig):
    def f(dz, w, shape, l):
        r = orig(dz, w, shape, l)
        if l == 2:
            r[:, :, 1::2, 1::2] = 0.0
        return r
    return f


def conv2_dgrad_drops_border_row0(orig):
    def f(dz, w, shape, l):
        r = orig(dz, w, shape, l)
        if l == 1:
            r[:, :, 0, :] = 0.0
        return r
    return f


def leaky_rule_ge_zero(orig):
    return lambda a, name: (a >= 0).to(a.dtype) * 0.8 + 0.2


def fc_wgrad_drops_partial_group(orig):
    def f(dz, a, j):
        B = dz.shape[0]
        if j < 4 and B % 16:
            dz, a = dz[:B // 16 * 16], a[:B // 16 * 16]
        return orig(dz, a, j)
    return f


def conv1_bias_drops_last_chunk(orig):
    def f(dz, l):
        if l == 0:
            K = dz.shape[0] * dz.shape[2] * dz.shape[3]
            dz = _rows_from(dz, (K - 1) // CS_CHUNK * CS_CHUNK)
        return orig(dz, l)
    return f


def l1_sign_of_zero_is_one(orig):
    import torch
    return lambda w: torch.where(w >= 0, torch.ones_like(w), -torch.ones_like(w))


FAULTS = [('conv_wgrad', conv1_wgrad_loses_last_slab, 1, 1),
          ('conv_dgrad', conv3_dgrad_loses_parity_11, 2, 6),
          ('conv_dgrad', conv2_dgrad_drops_border_row0, 2, 1),
          ('leaky_mask', leaky_rule_ge_zero, 2, 6),
          ('fc_wgrad', fc_wgrad_drops_partial_group, 17, 1),
          ('conv_bias', conv1_bias_drops_last_chunk, 1, 6),
          ('l1_sign', l1_sign_of_zero_is_one, 2, 1)]


@pytest.mark.parametrize('attr,fault,B,n_out', FAULTS, ids=[f[1].__name__ for f in FAULTS])
def test_backward_fault_rejected(monkeypatch, attr, fault, B, n_out):
    sd, x, t, out, taps, g, ga = case(B, n_out)
    monkeypatch.setattr(R, attr, fault(getattr(R, attr)))
    gf, _ = R.backward64_from_taps(sd, x, taps, out, lam_reg=LAM, bound=False, **t)
    r = R.componentwise_ratio(gf, g, ga)
    k = max(r, key=r.get)
    print('\n[fault] %s (B=%d n_out=%d): %s %.1e' % (fault.__name__, B, n_out, k, r[k]))
    assert r[k] > 10 * TOL


def test_forward_fault_rejected(monkeypatch):
    """conv1's bounds check takes input row 0 for padding: the taps next to the padding go missing"""
    sd, x, t, out, taps, _, _ = case(1, 1)
    assert max(R.forward_layer_ratios(sd, x, taps, out).values()) <= 1e-12
    orig = R.conv_fwd

    def f(a, w, b, l):
        if l == 0:
            a = a.clone()
            a[:, :, 0, :] = 0.0
        return orig(a, w, b, l)
    monkeypatch.setattr(R, 'conv_fwd', f)
    r = R.forward_layer_ratios(sd, x, taps, out)
    print('\n[fault] conv1 forward reads row 0 as padding: c1 %.1e' % r['c1'])
    assert r['c1'] > 10 * TOL

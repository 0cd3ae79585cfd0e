"""Test-side restatement of the resolution regressor's training step (train/train_res_rgr.py:150-183) -- not the library's
code -- and how tests/golden/rgr_train.npz names its data:

  fixture_targets, fixture_state_dict, fixture_batch   the fixture's samples (regenerated, not stored) and seeded weights
  sample_index                                         which elements of a tensor the fixture records
  loss_grad64                                          loss terms and every gradient in float64 through torch autograd
  adam64                                               torch.optim.Adam's update restated in float64
  backward64_from_taps, componentwise_ratio            the backward pass in float64 from the device's own activations, with
                                                       an elementwise bound on its rounding
  forward_layer_ratios                                 each forward layer in float64 on the device's own input, bounded alike
  forward_taps                                         the network in another precision (the CPU float32 stand-in)
  zero_units                                           a conv3 channel and an FC2 row that output exactly 0
"""
import numpy as np

import _rgr_ref

RESOLUTIONS = (4, 8, 16, 32, 64, 128)
N_SAMPLES = 512         # strided samples kept per weight tensor; biases and the head are kept whole


def sample_index(key, n):
    layer = int(key.split('.')[1])
    if key.endswith('bias') or layer == 19:
        return np.arange(n)
    return np.arange(0, n, max(1, n // N_SAMPLES))


def fixture_targets(n):
    """per sample: regressor y (the opt_den value) and opt_y, classifier resolution"""
    rng = np.random.Generator(np.random.PCG64(20240))
    return {'y': rng.uniform(20.0, 130.0, n), 'opt_y': rng.uniform(-2.0, 1.0, n),
            'res': np.array(RESOLUTIONS)[rng.integers(0, 6, n)]}


def conf_of(opt_y):
    return np.minimum(np.exp(-np.asarray(opt_y, np.float64) - 1.0), 1.0).astype(np.float32)


def label_of(res):
    return np.array([RESOLUTIONS.index(int(r)) for r in np.asarray(res).reshape(-1)], np.int32)


def fixture_state_dict(seed, n_out):
    """res_regressor.random_state_dict(seed, n_out) with a few weights set to exactly 0: flat index 0 and the 6th recorded
    sample of every weight tensor"""
    from dyn_res_pile_manip_amd import res_regressor as rr
    sd = rr.random_state_dict(seed, n_out)
    for k, v in sd.items():
        if k.endswith('weight'):
            flat = v.reshape(-1)
            idx = sample_index(k, flat.size)
            flat[0] = 0.0
            flat[idx[5]] = 0.0
    return sd


def fixture_batch(z, idx, n_out):
    """(x [B,6,224,224], y, conf, label) of the fixture's samples idx; the regressor's targets or the classifier's label"""
    idx = np.asarray(idx).reshape(-1)
    x = np.stack([_rgr_ref.rand_input(int(z['xseed']) + int(i), 1)[0] for i in idx]).astype(np.float32)
    t = fixture_targets(int(z['n_train']) + int(z['n_valid']))
    if n_out == 1:
        return x, t['y'][idx].astype(np.float32), conf_of(t['opt_y'][idx]), None
    return x, None, None, label_of(t['res'][idx])


def loss_grad64(sd, x, y=None, conf=None, label=None, lam_reg=0.0, want_grad=True):
    """float64 restatement of one step's loss (:150-176) -> (loss, main, reg, {key: gradient in torch layout} or None)"""
    import torch
    import torch.nn.functional as F
    from dyn_res_pile_manip_amd import res_regressor as rr
    n_out = 1 if label is None else 6
    keys = [k for k, _ in rr.state_dict_keys(n_out)]
    P = {k: torch.tensor(np.asarray(sd[k], np.float64), requires_grad=want_grad) for k in keys}
    with torch.set_grad_enabled(want_grad):
        h = torch.from_numpy(np.asarray(x, np.float64))
        for i in (0, 2, 4, 6, 8):
            h = F.leaky_relu(F.conv2d(h, P['model.%d.weight' % i], P['model.%d.bias' % i], stride=2, padding=1), 0.2)
        h = h.flatten(1)
        for i in (11, 13, 15, 17):
            h = F.leaky_relu(F.linear(h, P['model.%d.weight' % i], P['model.%d.bias' % i]), 0.2)
        out = F.linear(h, P['model.19.weight'], P['model.19.bias'])
        if n_out == 1:
            yt = torch.from_numpy(np.asarray(y, np.float64)).reshape(-1, 1)
            ct = torch.from_numpy(np.asarray(conf, np.float64)).reshape(-1, 1)
            main = (F.mse_loss(out, yt, reduction='none') * ct).mean()
        else:
            main = F.cross_entropy(out, torch.from_numpy(np.asarray(label, np.int64)))
        ws = [P[k] for k in keys[0::2]]
        reg = sum(w.abs().sum() for w in ws) / sum(w.numel() for w in ws)
        loss = main + lam_reg * reg
    grads = None
    if want_grad:
        loss.backward()
        grads = {k: P[k].grad.numpy() for k in keys}
    return float(loss.detach()), float(main.detach()), float(reg.detach()), grads


def adam64(w, g, m, v, t, lr, beta1):
    """torch.optim.Adam's step t (1-based) in float64 -> (w, m, v)"""
    m = m + (g - m) * (1.0 - beta1)
    v = v * 0.999 + 0.001 * g * g
    denom = np.sqrt(v) / np.sqrt(1.0 - 0.999 ** t) + 1e-8
    return w - lr / (1.0 - beta1 ** t) * m / denom, m, v


# ---- the backward pass from the device's own activations, with an elementwise bound on its rounding ----------------------
# The building blocks below stand for one kernel detail each (l: conv layer 0..4; j: FC layer 0..3, 4 the head); they sit at
# module level so that a test can put a faulty one in place.  a: a post-activation, w: a weight in torch's layout.
TAPS = ('c1', 'c2', 'c3', 'c4', 'c5', 'f1', 'f2', 'f3', 'f4')
CONV_KEYS = (0, 2, 4, 6, 8)
FC_KEYS = (11, 13, 15, 17, 19)
CW_TOL = 1e-5           # the componentwise bound on max |g - g_ref| / g_abs (tests/test_rgr_backward_host.py, test_gpu_*)


def leaky_mask(a, name):
    """LeakyReLU(0.2)'s derivative read off the post-activation a of tap `name`: torch's rule (x > 0), 0.2 at exactly 0"""
    return (a > 0).to(a.dtype) * 0.8 + 0.2


def conv_fwd(a, w, b, l):
    import torch.nn.functional as F
    return F.conv2d(a, w, b, stride=2, padding=1)


def conv_wgrad(a, dz, shape, l):
    import torch
    return torch.nn.grad.conv2d_weight(a, shape, dz, stride=2, padding=1)


def conv_dgrad(dz, w, shape, l):
    import torch
    return torch.nn.grad.conv2d_input(shape, w, dz, stride=2, padding=1)


def conv_bias(dz, l):
    return dz.sum((0, 2, 3))


def fc_fwd(a, w, b, j):
    return a @ w.T + b


def fc_wgrad(dz, a, j):
    return dz.T @ a


def fc_dgrad(dz, w, j):
    return dz @ w


def fc_bias(dz, j):
    return dz.sum(0)


def l1_sign(w):
    """the L1 term's d|w|/dw: sign(0) = 0"""
    import torch
    return torch.sign(w)


def n_weights(n_out):
    from dyn_res_pile_manip_amd import res_regressor as rr
    return sum(int(np.prod(s)) for k, s in rr.state_dict_keys(n_out) if k.endswith('weight'))


def d_out64(out, y=None, conf=None, label=None):
    """dLoss/dOut [B, n_out] in float64 from the network's output: 2 conf (out - y) / B, or (softmax - onehot) / B"""
    o = np.asarray(out, np.float64)
    B = o.shape[0]
    if label is None:
        return 2.0 * np.asarray(conf, np.float64).reshape(B, 1) * (o - np.asarray(y, np.float64).reshape(B, 1)) / B
    mx = o.max(axis=1, keepdims=True)
    lse = mx + np.log(np.exp(o - mx).sum(axis=1, keepdims=True))
    oh = np.zeros_like(o)
    oh[np.arange(B), np.asarray(label).reshape(-1)] = 1.0
    return (np.exp(o - lse) - oh) / B


def _chain(W, A, M, d, coef, sgn, bound=False):
    """the backward pass through given weights W {key}, activations A (x, c1..c5, f1..f4), masks M {tap} and dOut d
    -> (gradients, their rounding bounds or None)"""
    g, gb = {}, {}
    dA, env = d, d.abs()
    for j in (4, 3, 2, 1, 0):
        k = 'model.%d.' % FC_KEYS[j]
        w = W[k + 'weight']
        dz = dA if j == 4 else M['f%d' % (j + 1)] * dA
        a = A['f%d' % j] if j else A['c5'].flatten(1)
        g[k + 'weight'] = fc_wgrad(dz, a, j) + coef * sgn(w)
        g[k + 'bias'] = fc_bias(dz, j)
        if bound:
            ez = env if j == 4 else M['f%d' % (j + 1)] * env
            gb[k + 'weight'] = fc_wgrad(dz.abs(), a.abs(), j) + fc_wgrad(ez * ez, a * a, j).sqrt() + coef * sgn(w).abs()
            gb[k + 'bias'] = fc_bias(dz.abs(), j) + fc_bias(ez * ez, j).sqrt()
            env = fc_dgrad(dz.abs(), w.abs(), j)
        dA = fc_dgrad(dz, w, j)
    dA = dA.reshape(A['c5'].shape)
    if bound:
        env = env.reshape(A['c5'].shape)
    for l in (4, 3, 2, 1, 0):
        k = 'model.%d.' % CONV_KEYS[l]
        w = W[k + 'weight']
        m = M['c%d' % (l + 1)]
        dz = m * dA
        a = A['c%d' % l] if l else A['x']
        g[k + 'weight'] = conv_wgrad(a, dz, w.shape, l) + coef * sgn(w)
        g[k + 'bias'] = conv_bias(dz, l)
        if bound:
            ez = m * env
            gb[k + 'weight'] = (conv_wgrad(a.abs(), dz.abs(), w.shape, l) + conv_wgrad(a * a, ez * ez, w.shape, l).sqrt() +
                                coef * sgn(w).abs())
            gb[k + 'bias'] = conv_bias(dz.abs(), l) + conv_bias(ez * ez, l).sqrt()
        if l:
            if bound:
                env = conv_dgrad(dz.abs(), w.abs(), a.shape, l)
            dA = conv_dgrad(dz, w, a.shape, l)
    return g, (gb if bound else None)


def backward64_from_taps(sd, x, taps, out, y=None, conf=None, label=None, lam_reg=0.0, dtype=None, bound=True):
    """The step's gradients (torch layouts, float64 numpy) from the given activations instead of a forward of its own:
    x [B,6,224,224], taps {'c1'..'f4'} post-activations in torch's layouts (Engine.rgr_tap), out [B,n_out].  The masks and
    dOut are read off those numbers, so against a device's own taps only the backward pass's rounding is left.
    -> (g_ref, g_abs).  g_abs bounds that rounding elementwise, to a small multiple of u = 2^-24:
      W_l: |dZ_l|^T |A_{l-1}| + sqrt((E_l^2)^T A_{l-1}^2) + lam/n_W |sign W_l|,   b_l: sum |dZ_l| + sqrt(sum E_l^2)
    The first term holds the layer's own sums (the split-K slabs, the sample groups, the column-sum chunks); the second the
    error its input dZ_l inherits from the dgrad that made it, E_l = m_l (|W_{l+1}|^T |dZ_{l+1}|) (|dOut| at the head), which
    enters the weight's sum with independent signs over samples and positions (a root-sum-square, not a sum of absolute
    values).  The absolute chain carried through every layer is a rigorous bound too, but it grows by about sqrt(fan-out)
    per layer against the signed chain (1e11 at conv1), so a slab or a border row dropped there would sit far below it.
    dtype (default float64) runs the chain in another precision (the CPU stand-in for an fp32 implementation); bound=False
    skips g_abs."""
    import torch
    dt = torch.float64 if dtype is None else dtype
    n_out = 1 if label is None else 6
    coef = lam_reg / n_weights(n_out)
    d = torch.from_numpy(d_out64(out, y, conf, label))
    A = {t: torch.from_numpy(np.asarray(taps[t], np.float64)) for t in TAPS}
    A['x'] = torch.from_numpy(np.asarray(x, np.float64))
    W = {k: torch.from_numpy(np.asarray(v, np.float64)) for k, v in sd.items()}
    M = {t: leaky_mask(A[t], t) for t in TAPS}
    with torch.no_grad():
        if dt != torch.float64:
            g, _ = _chain({k: v.to(dt) for k, v in W.items()}, {k: v.to(dt) for k, v in A.items()},
                          {k: v.to(dt) for k, v in M.items()}, d.to(dt), coef, l1_sign)
            gb = _chain(W, A, M, d, coef, l1_sign, True)[1] if bound else None
        else:
            g, gb = _chain(W, A, M, d, coef, l1_sign, bound)
    return ({k: v.to(torch.float64).numpy() for k, v in g.items()},
            {k: v.numpy() for k, v in gb.items()} if bound else None)


def componentwise_ratio(g, g_ref, g_abs, floor=1e-35):
    """{key: max over elements of |g - g_ref| / g_abs}; g_abs is floored where it underflows"""
    return {k: float((np.abs(np.asarray(g[k], np.float64).reshape(g_ref[k].shape) - g_ref[k]) /
                      np.maximum(g_abs[k], floor)).max()) for k in g_ref}


def forward_layer_ratios(sd, x, taps, out):
    """each forward layer against float64 on its own input from the given activations:
    ref_l = leaky(op(W_l, A_{l-1}) + b_l), bound |W_l| |A_{l-1}| + |b_l| -> {'c1'..'f4', 'out': max |A_l - ref_l| / bound}"""
    import torch
    import torch.nn.functional as F

    def t(v):
        return torch.from_numpy(np.asarray(v, np.float64))
    r = {}
    with torch.no_grad():
        prev = t(x)
        for i, name in enumerate(TAPS + ('out',)):
            k = 'model.%d.' % (CONV_KEYS + FC_KEYS)[i]
            w, b = t(sd[k + 'weight']), t(sd[k + 'bias'])
            if i < 5:
                ref, bnd = conv_fwd(prev, w, b, i), conv_fwd(prev.abs(), w.abs(), b.abs(), i)
            else:
                a = prev.flatten(1)
                ref, bnd = fc_fwd(a, w, b, i - 5), fc_fwd(a.abs(), w.abs(), b.abs(), i - 5)
            if name != 'out':
                ref = F.leaky_relu(ref, 0.2)
            got = t(taps[name] if name != 'out' else out)
            r[name] = float(((got - ref).abs() / bnd.clamp(min=1e-35)).max())
            prev = got
    return r


def forward_taps(sd, x, dtype):
    """the network in another precision through the same building blocks: (out, taps) as numpy arrays of that precision"""
    import torch
    import torch.nn.functional as F

    def t(v):
        return torch.from_numpy(np.asarray(v)).to(dtype)
    taps = {}
    with torch.no_grad():
        h = t(x)
        for l in range(5):
            k = 'model.%d.' % CONV_KEYS[l]
            h = F.leaky_relu(conv_fwd(h, t(sd[k + 'weight']), t(sd[k + 'bias']), l), 0.2)
            taps['c%d' % (l + 1)] = h.numpy()
        h = h.flatten(1)
        for j in range(5):
            k = 'model.%d.' % FC_KEYS[j]
            h = fc_fwd(h, t(sd[k + 'weight']), t(sd[k + 'bias']), j)
            if j < 4:
                h = F.leaky_relu(h, 0.2)
                taps['f%d' % (j + 1)] = h.numpy()
    return h.numpy(), taps


ZERO_CONV3_CHANNEL = 37
ZERO_FC2_ROW = 301


def zero_units(sd):
    """a copy of sd whose conv3 output channel ZERO_CONV3_CHANNEL and FC2 row ZERO_FC2_ROW have all-zero weights and bias:
    their post-activations are exactly 0, where LeakyReLU's derivative is 0.2"""
    sd = {k: np.array(v, np.float32, copy=True) for k, v in sd.items()}
    for k, i in (('model.4.', ZERO_CONV3_CHANNEL), ('model.13.', ZERO_FC2_ROW)):
        sd[k + 'weight'][i] = 0.0
        sd[k + 'bias'][i] = 0.0
    return sd

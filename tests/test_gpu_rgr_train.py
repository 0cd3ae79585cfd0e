"""GPU: training the resolution regressor on the device (drp_rgr_train_*, train/train_res_rgr.py) -- loss, gradients and Adam
against tests/golden/rgr_train.npz (the reference's train_res_cls with seeded weights) and the float64 restatement of
tests/_rgr_train_ref.py; modes, determinism, refusals, isolation from the PropNet state, the Python mirror."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _rgr_ref  # noqa: E402
import _rgr_train_ref as R  # noqa: E402

HEADS = {'rgr': 1, 'cls': 6}
# per-tensor bounds on max |g - g_ref| / max |g_ref|, 10x the worst measured on the MI355X or more: the fully connected
# layers and the head (measured <= 1.4e-6 against float64); the convolutions, whose gradients are badly conditioned sums
# over up to B x 12 544 positions (measured <= 1.9e-3 against float64, and the reference's own float32 run is off float64
# by 2e-3 .. 3e-2 there)
TOL_FC = 1e-4
TOL_CONV = 2e-2


@pytest.fixture(scope='module')
def z(golden):
    return golden.rgr_train


@pytest.fixture(scope='module')
def eng():
    from dyn_res_pile_manip_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def keys_of(n_out):
    from dyn_res_pile_manip_amd import res_regressor as rr
    return [k for k, _ in rr.state_dict_keys(n_out)]


def start(e, z, n_out, lam=None, lr=None):
    from dyn_res_pile_manip_amd import res_regressor as rr
    sd = R.fixture_state_dict(int(z['seed']), n_out)
    blob = rr.blob_from_state_dict(sd, n_out)
    e.rgr_load(blob, n_out)
    e.rgr_train_begin(float(z['lr']) if lr is None else lr, float(z['beta1']), float(z['lam_reg']) if lam is None else lam)
    return sd, blob


def step(e, batch, mode, want_grad=False):
    x, y, conf, label = batch
    return e.rgr_train_step(x, y=y, conf=conf, label=label, mode=mode, want_grad=want_grad)


def rand_batch(B, n_out, seed):
    x = np.stack([_rgr_ref.rand_input(5000 + seed * 100 + i, 1)[0] for i in range(B)]).astype(np.float32)
    rng = np.random.Generator(np.random.PCG64(seed))
    if n_out == 1:
        return x, rng.uniform(20, 130, B).astype(np.float32), rng.uniform(0.05, 1.0, B).astype(np.float32), None
    return x, None, None, rng.integers(0, 6, B).astype(np.int32)


# ---- against the reference -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['rgr', 'cls'])
def test_grad_matches_reference(eng, z, name):
    from dyn_res_pile_manip_amd import res_regressor as rr
    n_out = HEADS[name]
    sd, blob = start(eng, z, n_out)
    p = '%s_s0_' % name
    batch = R.fixture_batch(z, z[p + 'batch'], n_out)
    (loss, main, reg), g = step(eng, batch, 'grad', want_grad=True)
    lam = float(z['lam_reg'])
    np.testing.assert_allclose(main, float(z[p + 'main']), rtol=1e-5)
    np.testing.assert_allclose(reg, float(z[p + 'reg']), rtol=1e-9)
    np.testing.assert_allclose(loss, float(z[p + 'main']) + lam * float(z[p + 'reg']), rtol=1e-5)
    assert abs(loss - (main + lam * reg)) <= 1e-12 * abs(loss)
    gsd = rr.state_dict_from_blob(g, n_out)
    _, _, _, g64 = R.loss_grad64(sd, *batch, lam_reg=lam)
    census = []
    for j, k in enumerate(keys_of(n_out)):
        idx = R.sample_index(k, gsd[k].size)
        ref = z[p + 'g%d' % j]
        got = gsd[k].reshape(-1)[idx]
        scale = float(np.abs(ref).max())
        err = float(np.abs(got - ref).max())
        # the reference's own float32 error (CPU convolutions: up to ~1e-2 of the largest), measured against float64
        ref_err = float(np.abs(g64[k].reshape(-1)[idx] - ref).max())
        err64 = float(np.abs(gsd[k] - g64[k]).max()) / float(np.abs(g64[k]).max())
        gd = gsd[k].astype(np.float64)
        l1 = np.abs(gd).sum() / np.abs(g64[k]).sum() - 1.0
        l2 = np.sqrt((gd ** 2).sum()) / np.sqrt((g64[k] ** 2).sum()) - 1.0
        census.append((k, err / scale, ref_err / scale, err64, l1, l2))
    print('\n%s gradient census: max err / max|g_ref| vs the reference, the reference vs float64, the device vs float64'
          ' (all elements), L1 and L2 norm rel. diff vs float64:' % name)
    for c in census:
        print('  %-16s %.2e %.2e %.2e %+.2e %+.2e' % c)
    for j, (k, e, re, e64, l1, l2) in enumerate(census):
        tol = TOL_CONV if j < 10 else TOL_FC
        assert e <= max(tol, 2.0 * re), (k, e, re)
        assert e64 <= tol and abs(l1) <= tol and abs(l2) <= tol, (k, e64, l1, l2)
    # GRAD leaves the weights alone
    np.testing.assert_array_equal(eng.rgr_get_weights(), blob)


def adam_bound(t, beta1):
    """max |m_hat| / sqrt(v_hat) over any gradient history of t steps (Cauchy-Schwarz)"""
    a = np.array([(1 - beta1) * beta1 ** (t - 1 - i) for i in range(t)]) / (1 - beta1 ** t)
    b = np.array([0.001 * 0.999 ** (t - 1 - i) for i in range(t)]) / (1 - 0.999 ** t)
    return float(np.sqrt((a * a / b).sum()))


@pytest.mark.parametrize('name', ['rgr', 'cls'])
def test_update_matches_reference(eng, z, name):
    """three UPDATE steps on the fixture's batches.  Step 0 against the reference's weights elementwise; every step against
    Adam restated in float64 on the device's own gradient of that step (a GRAD call first: same kernels, same sums).  From
    step 1 on the weights differ from the reference's where a convolution's gradient was too small for either float32 run to
    get its sign (Adam moves such a weight by about lr either way); the trajectories then part (the loss by 3.8 % at step 2),
    so later steps' losses are held to the float64 restatement at the device's own weights."""
    from dyn_res_pile_manip_amd import res_regressor as rr
    n_out = HEADS[name]
    sd, blob = start(eng, z, n_out)
    lr, beta1 = float(z['lr']), float(z['beta1'])
    keys = keys_of(n_out)
    prev_dev = rr.state_dict_from_blob(blob, n_out)
    mv = {k: (0.0, 0.0) for k in keys}
    worst = [0.0, 0.0]
    for t in range(3):
        p = '%s_s%d_' % (name, t)
        batch = R.fixture_batch(z, z[p + 'batch'], n_out)
        _, g = step(eng, batch, 'grad', want_grad=True)
        (loss, main, reg), _ = step(eng, batch, 'update')
        if t == 0:
            np.testing.assert_allclose(main, float(z[p + 'main']), rtol=1e-5)
            np.testing.assert_allclose(reg, float(z[p + 'reg']), rtol=1e-9)
        else:                   # the loss of the weights the device holds (the trajectories part: measured 3.8 % at step 2)
            _, m64, r64, _ = R.loss_grad64(prev_dev, *batch, lam_reg=float(z['lam_reg']), want_grad=False)
            np.testing.assert_allclose(main, m64, rtol=1e-5)
            np.testing.assert_allclose(reg, r64, rtol=1e-9)
        cur = rr.state_dict_from_blob(eng.rgr_get_weights(), n_out)
        gd = rr.state_dict_from_blob(g, n_out)
        bound = lr * adam_bound(t + 1, beta1) * (1 + 1e-5)
        for j, k in enumerate(keys):
            idx = R.sample_index(k, cur[k].size)
            w0 = prev_dev[k].reshape(-1)[idx].astype(np.float64)
            w1 = cur[k].reshape(-1)[idx].astype(np.float64)
            ulp = 4 * np.spacing(np.abs(cur[k].reshape(-1)[idx]).astype(np.float32)).astype(np.float64)
            m, v = mv[k]
            pred, m, v = R.adam64(w0, gd[k].reshape(-1)[idx].astype(np.float64), m, v, t + 1, lr, beta1)
            mv[k] = (m, v)
            e = np.abs(w1 - pred)
            worst[0] = max(worst[0], float((e - ulp).max()) / lr)
            assert np.all(e <= 1e-3 * lr + ulp), (t, k, float(e.max()))
            assert np.all(np.abs(w1 - w0) <= bound + ulp), (t, k)
            if t == 0:
                gr = np.abs(z[p + 'g%d' % j])
                big = gr > (1e-3 if j >= 10 else 0.1) * gr.max()
                e = np.abs(w1 - z[p + 'w%d' % j])[big]
                worst[1] = max(worst[1], float((e - ulp[big]).max()) / lr if e.size else 0.0)
                assert np.all(e <= (2e-3 if j >= 10 else 5e-2) * lr + ulp[big]), (k, float(e.max()))
        prev_dev = cur
    print('\n%s update: worst |w - Adam64(own gradient)| / lr %.1e; step 0, |w - w_ref| / lr where |g_ref| is large %.1e'
          % (name, worst[0], worst[1]))
    # the valid phase after the three steps: EVAL
    w_before = eng.rgr_get_weights()
    vb = R.fixture_batch(z, z[name + '_valid_batch'], n_out)
    (loss, main, reg), _ = step(eng, vb, 'eval')
    _, m64, r64, _ = R.loss_grad64(prev_dev, *vb, lam_reg=float(z['lam_reg']), want_grad=False)
    np.testing.assert_allclose(main, m64, rtol=1e-5)
    np.testing.assert_array_equal(eng.rgr_get_weights(), w_before)


# ---- modes and numerics ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['rgr', 'cls'])
def test_training_forward_is_drp_rgr_forward(eng, z, name):
    n_out = HEADS[name]
    start(eng, z, n_out)
    batch = rand_batch(5, n_out, 1)
    out = eng.rgr_forward(batch[0])
    taps = {t: eng.rgr_tap(t) for t in ('c1', 'c3', 'c5', 'f1', 'f4')}
    (loss, main, reg), _ = step(eng, batch, 'eval')
    for t, v in taps.items():
        np.testing.assert_array_equal(eng.rgr_tap(t), v)
    o = out.astype(np.float64)
    if n_out == 1:
        ref = float(np.mean(batch[2].astype(np.float64) * (o[:, 0] - batch[1]) ** 2))
    else:
        mx = o.max(axis=1, keepdims=True)
        lse = mx[:, 0] + np.log(np.exp(o - mx).sum(axis=1))
        ref = float(np.mean(lse - o[np.arange(5), batch[3]]))
    np.testing.assert_allclose(main, ref, rtol=1e-12)


@pytest.mark.parametrize('B', [1, 16, 64])
def test_gradients_against_float64(eng, z, B):
    from dyn_res_pile_manip_amd import res_regressor as rr
    n_out = 6 if B == 16 else 1
    sd, _ = start(eng, z, n_out, lam=5e4)
    batch = rand_batch(B, n_out, B)
    (loss, main, reg), g = step(eng, batch, 'grad', want_grad=True)
    l64, m64, r64, g64 = R.loss_grad64(sd, *batch, lam_reg=5e4)
    np.testing.assert_allclose(main, m64, rtol=1e-5)
    np.testing.assert_allclose(reg, r64, rtol=1e-9)
    gsd = rr.state_dict_from_blob(g, n_out)
    census = []
    for k in keys_of(n_out):
        census.append((k, float(np.abs(gsd[k] - g64[k]).max()) / float(np.abs(g64[k]).max())))
    print('\nB=%d max err / max|g|: %s' % (B, ', '.join('%s %.1e' % c for c in census)))
    for j, (k, e) in enumerate(census):
        assert e <= (TOL_CONV if j < 10 else TOL_FC), (B, k, e)


# ---- componentwise against float64 from the device's own activations --------------------------------------------------
# R.backward64_from_taps restarts the backward in float64 at the device's taps and output, so the masks and dOut are the
# device's own and only the backward pass's rounding is left; it is held elementwise to TOL_CW times the bound g_abs
# (tests/_rgr_train_ref.py).  TOL_CW = 1e-5, 17x the worst measured on the MI355X (5.7e-7: the conv5 weight at B = 64; the
# edge cases <= 1.9e-7) and 80x below the weakest injected fault (8.3e-4: conv1's wgrad without its last split-K slab,
# tests/test_rgr_backward_host.py, where the CPU float32 stand-in sits at <= 3e-7).
TOL_CW = R.CW_TOL
LAM_CW = 5e4
SWEEP = ((64, 'rgr'), (63, 'cls'), (33, 'rgr'), (17, 'cls'), (16, 'rgr'), (5, 'cls'), (2, 'rgr'), (1, 'cls'))


def grad_with_taps(e, batch):
    """one GRAD step -> (loss triple, gradient state_dict, the step's taps, out of drp_rgr_forward on the same batch); the
    forward's taps are bit-equal to the step's"""
    from dyn_res_pile_manip_amd import res_regressor as rr
    loss, g = step(e, batch, 'grad', want_grad=True)
    taps = {t: e.rgr_tap(t) for t in R.TAPS}
    out = e.rgr_forward(batch[0])
    for t, v in taps.items():
        np.testing.assert_array_equal(e.rgr_tap(t), v, err_msg=t)
    return loss, rr.state_dict_from_blob(g, out.shape[1]), taps, out


def componentwise(sd, batch, taps, out, g, label):
    x, y, conf, lab = batch
    g_ref, g_abs = R.backward64_from_taps(sd, x, taps, out, y=y, conf=conf, label=lab, lam_reg=LAM_CW)
    r = R.componentwise_ratio(g, g_ref, g_abs)
    print('[grad-err] rgr componentwise %s: %s' % (label, ', '.join('%s %.1e' % (k[6:], v) for k, v in r.items())))
    return r, g_ref


def test_gradients_componentwise_batch_sweep(eng, z):
    """B from 64 down to 1 in one context (a stale slab or partial from a larger step would show), both heads"""
    worst = {}
    for B, name in SWEEP:
        n_out = HEADS[name]
        sd, _ = start(eng, z, n_out, lam=LAM_CW)
        batch = rand_batch(B, n_out, 300 + B)
        _, g, taps, out = grad_with_taps(eng, batch)
        r, _ = componentwise(sd, batch, taps, out, g, '%s B=%d' % (name, B))
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
            assert v <= TOL_CW, (B, name, k, v)
    print('[grad-err] rgr componentwise sweep worst: %s' % ', '.join('%s %.1e' % (k[6:], v) for k, v in worst.items()))


def _edge(name):
    """(n_out, state_dict, batch) of an edge case"""
    B = 6
    if name == 'zero':                  # a conv3 channel and an FC2 row with all-zero weights and bias: post-activation 0
        return 6, R.zero_units(R.fixture_state_dict(11, 6)), rand_batch(B, 6, 400)
    if name == 'blank':                 # one sample of x = 0
        x, y, conf, _ = rand_batch(B, 1, 401)
        x[2] = 0.0
        return 1, R.fixture_state_dict(11, 1), (x, y, conf, None)
    if name == 'saturated':             # head weights scaled until the logits spread by several hundred (in the test)
        return 6, R.fixture_state_dict(11, 6), (rand_batch(B, 6, 402)[0], None, None, np.arange(B, dtype=np.int32) % 6)
    x = rand_batch(B + 1, 1, 403)[0]    # 'extreme': conf from 1e-6 to 1, targets far from the output
    y = np.array([-5e3, 3e4, -2e2, 1e4, 900.0, -7e4, 2e5], np.float32)
    return 1, R.fixture_state_dict(11, 1), (x, y, np.logspace(-6, 0, B + 1).astype(np.float32), None)


@pytest.mark.parametrize('name', ['zero', 'blank', 'saturated', 'extreme'])
def test_gradients_componentwise_edges(eng, name):
    from dyn_res_pile_manip_amd import res_regressor as rr
    n_out, sd, batch = _edge(name)
    if name == 'saturated':
        eng.rgr_load(rr.blob_from_state_dict(sd, n_out), n_out)
        o = eng.rgr_forward(batch[0])
        sd['model.19.weight'] = sd['model.19.weight'] * np.float32(500.0 / float((o.max(axis=1) - o.min(axis=1)).min()))
    eng.rgr_load(rr.blob_from_state_dict(sd, n_out), n_out)
    eng.rgr_train_begin(1e-4, 0.9, LAM_CW)
    (loss, main, reg), g, taps, out = grad_with_taps(eng, batch)
    r, g_ref = componentwise(sd, batch, taps, out, g, name)
    assert max(r.values()) <= TOL_CW, r
    o = out.astype(np.float64)
    if n_out == 1:
        ref = float(np.mean(batch[2].astype(np.float64) * (o[:, 0] - batch[1]) ** 2))
    else:
        mx = o.max(axis=1, keepdims=True)
        ref = float(np.mean(mx[:, 0] + np.log(np.exp(o - mx).sum(axis=1)) - o[np.arange(o.shape[0]), batch[3]]))
    np.testing.assert_allclose(main, ref, rtol=1e-12)
    if name == 'zero':                  # the 0.2 rule is visible there: those units still pass a gradient on
        assert np.abs(taps['c3'][:, R.ZERO_CONV3_CHANNEL]).max() == 0 and np.abs(taps['f2'][:, R.ZERO_FC2_ROW]).max() == 0
        assert g_ref['model.4.bias'][R.ZERO_CONV3_CHANNEL] != 0 and g_ref['model.13.bias'][R.ZERO_FC2_ROW] != 0
    if name == 'blank':
        assert np.all(taps['c1'][2] == taps['c1'][2, :, :1, :1])  # leaky(bias) at every position
    if name == 'saturated':
        assert float((o.max(axis=1) - o.min(axis=1)).min()) >= 300.0, o


def test_refusals(z):
    from dyn_res_pile_manip_amd import res_regressor as rr
    from dyn_res_pile_manip_amd._lib import DrpError
    from dyn_res_pile_manip_amd.engine import Engine
    e = Engine(0)
    try:
        with pytest.raises(DrpError):
            e.rgr_train_begin(1e-4)                               # before drp_rgr_load
        sd = R.fixture_state_dict(int(z['seed']), 1)
        e.rgr_load(rr.blob_from_state_dict(sd, 1), 1)
        x, y, conf, _ = rand_batch(2, 1, 3)
        with pytest.raises(DrpError):
            e.rgr_train_step(x, y=y, conf=conf)                   # before drp_rgr_train_begin
        with pytest.raises(DrpError):
            e.rgr_train_set_lr(1e-3)
        e.rgr_train_begin(1e-4, 0.9, 0.0)
        w0 = e.rgr_get_weights()
        with pytest.raises(DrpError):
            e.rgr_train_step(x[:0], y=y[:0], conf=conf[:0])       # B = 0
        x65 = np.zeros((65, 6, 224, 224), np.float32)
        with pytest.raises(DrpError):
            e.rgr_train_step(x65, y=np.zeros(65, np.float32), conf=np.ones(65, np.float32))
        with pytest.raises(DrpError):
            e.rgr_train_step(x, y=y)                              # conf missing
        with pytest.raises(DrpError):
            e.rgr_train_step(x, y=y, conf=conf, label=np.zeros(2, np.int32))      # a label for the regressor
        with pytest.raises(DrpError):
            e.rgr_train_step(x, y=y, conf=conf, mode='update', want_grad=True)    # grad_out outside GRAD
        np.testing.assert_array_equal(e.rgr_get_weights(), w0)
        e.rgr_load(rr.blob_from_state_dict(R.fixture_state_dict(int(z['seed']), 6), 6), 6)
        with pytest.raises(DrpError):
            e.rgr_train_step(x, label=np.zeros(2, np.int32))      # drp_rgr_load ended the training
        e.rgr_train_begin(1e-4, 0.9, 0.0)
        with pytest.raises(DrpError):
            e.rgr_train_step(x, label=np.array([0, 6], np.int32))                 # label out of range
        with pytest.raises(DrpError):
            e.rgr_train_step(x, label=np.array([-1, 0], np.int32))
        with pytest.raises(DrpError):
            e.rgr_train_step(x, y=y, conf=conf)                   # y / conf for the classifier
        e.rgr_train_step(x, label=np.array([0, 5], np.int32), mode='eval')
    finally:
        e.close()


def test_determinism_and_modes_leave_state_alone(z):
    """two fresh contexts, 5 identical UPDATE steps: bit-identical weights -- one of them with EVAL and GRAD calls (and a
    forward) between the steps, so neither touches the weights or Adam's state"""
    from dyn_res_pile_manip_amd.engine import Engine
    res = []
    for interleave in (False, True):
        e = Engine(0)
        try:
            start(e, z, 6, lam=1e4)
            for i in range(5):
                b = rand_batch(8, 6, 40 + i)
                if interleave:
                    step(e, rand_batch(3, 6, 90 + i), 'eval')
                    step(e, rand_batch(5, 6, 95 + i), 'grad', want_grad=(i == 2))
                    e.rgr_forward(b[0][:2])
                step(e, b, 'update')
            res.append(e.rgr_get_weights())
        finally:
            e.close()
    np.testing.assert_array_equal(res[0], res[1])


def test_overfit_eight_samples(eng, z):
    start(eng, z, 1, lam=0.0, lr=1e-4)
    b = rand_batch(8, 1, 7)
    losses = [step(eng, b, 'update')[0][1] for _ in range(50)]
    final = step(eng, b, 'eval')[0][1]
    print('\noverfit mse: first %.4g, after 50 steps %.4g' % (losses[0], final))
    assert np.all(np.isfinite(losses)) and final < 3.0         # measured on the MI355X: 2495 -> 0.254


def test_updated_weights_serve_inference_and_state_dict_roundtrip(eng, z):
    from dyn_res_pile_manip_amd.res_regressor import MPCResCls
    from dyn_res_pile_manip_amd import res_regressor as rr
    from dyn_res_pile_manip_amd.engine import Engine
    m = MPCResCls(engine=eng)
    m.load_state_dict(R.fixture_state_dict(int(z['seed']), 6))
    x = rand_batch(3, 6, 11)[0]
    out0 = m(x)
    eng.rgr_train_begin(1e-4, 0.9, 0.0)
    step(eng, rand_batch(4, 6, 12), 'update')
    out1 = m(x)
    assert np.abs(out1 - out0).max() > 0
    sd = m.state_dict()
    assert list(sd.keys()) == keys_of(6)
    e2 = Engine(0)
    try:
        m2 = MPCResCls(engine=e2)
        m2.load_state_dict(sd)
        np.testing.assert_array_equal(m2(x), out1)
        np.testing.assert_array_equal(rr.blob_from_state_dict(sd, 6), eng.rgr_get_weights())
    finally:
        e2.close()


def test_propnet_state_unchanged_by_regressor_training(z):
    from dyn_res_pile_manip_amd import synthetic as syn, weights
    from dyn_res_pile_manip_amd.engine import Engine
    e = Engine(0)
    try:
        e.load_weights(weights.blob_from_state_dict(weights.random_state_dict(seed=0)), 0.08)
        rng = np.random.default_rng(0)
        B, T, N = 2, 2, 48
        states = np.zeros((B, T + 1, N, 3), np.float32)
        for b in range(B):
            s, _, _ = syn.make_pile(N, 1, seed=3 + b, kind='blob')
            for t in range(T + 1):
                states[b, t] = s[0] * 0.3 + [0, 0, 0.52]
        sdelta = (0.004 * rng.standard_normal((B, T, N, 3))).astype(np.float32)
        attrs = np.zeros((B, T + 1, N), np.float32)
        nums = np.full(B, N, np.int32)
        dens = np.array([300.0, 350.0], np.float32)
        e.train_begin(T, 1e-3, 0.9)
        e.train_step(states, sdelta, attrs, nums, dens, mode='update')
        w0 = e.get_weights()
        l0, _ = e.train_step(states, sdelta, attrs, nums, dens, mode='eval')
        start(e, z, 1, lam=1e3)
        for i in range(2):
            step(e, rand_batch(4, 1, 60 + i), 'update')
        np.testing.assert_array_equal(e.get_weights(), w0)
        l1, _ = e.train_step(states, sdelta, attrs, nums, dens, mode='eval')
        assert l1 == l0
        e.train_step(states, sdelta, attrs, nums, dens, mode='update')      # the PropNet optimiser carries on
    finally:
        e.close()


# ---- the Python mirror -----------------------------------------------------------------------------------------------
def _config(model_type, n, batch):
    return {'train_res_cls': {'model_type': model_type, 'num_data': n, 'train_valid_ratio': 0.75, 'state_h': 224,
                              'state_w': 224, 'res_dim': 6, 'batch_size': batch, 'num_worker': 0, 'n_epoch': 1,
                              'adam_beta1': 0.9, 'lr': 1e-5,
                              'lr_scheduler': {'type': 'StepLR', 'enabled': True, 'step_size': 1, 'gamma': 0.5,
                                               'factor': 0.1, 'patience': 10, 'threshold_mode': 'rel', 'cooldown': 0},
                              'lam_reg': 2e-4, 'log_per_iter': 1, 'ckp_per_iter': 1000}}


def test_train_res_cls_in_memory(eng, z):
    from dyn_res_pile_manip_amd import train_res_rgr as T
    from dyn_res_pile_manip_amd.res_regressor import MPCResRgrNoPool
    model = MPCResRgrNoPool(engine=eng)
    model.load_state_dict(R.fixture_state_dict(int(z['seed']), 1))
    w0 = eng.rgr_get_weights()

    def batch(seed):
        x, y, conf, _ = rand_batch(4, 1, seed)
        return {'input_img': x, 'optimal_den': y.reshape(4, 1, 1), 'conf': conf.reshape(4, 1)}
    logs, best = [], []
    res = T.train_res_cls(_config('regressor', 16, 4), model, {'train': [batch(70), batch(71), batch(72)],
                                                               'valid': [batch(73)]},
                          log=logs.append, on_best=best.append)
    assert [h[1] for h in res['history']] == ['train', 'valid'] and np.isfinite(res['best_valid_loss'])
    assert res['history'][1][3] == 0.5e-5                         # StepLR stepped after the train phase
    assert len(best) == 1 and set(best[0]) == set(keys_of(1)) and len(logs) == 4
    assert np.abs(eng.rgr_get_weights() - w0).max() > 0


def test_dataset_from_png_files(eng, z, tmp_path):
    pytest.importorskip('PIL')
    from PIL import Image
    from dyn_res_pile_manip_amd import train_res_rgr as T
    from dyn_res_pile_manip_amd.res_regressor import MPCResCls
    model = MPCResCls(engine=eng)
    model.load_state_dict(R.fixture_state_dict(int(z['seed']), 6))
    rng = np.random.default_rng(3)
    res = [4, 128, 16, 32]
    for i in range(4):
        d = tmp_path / str(i)
        d.mkdir()
        for nm in ('init', 'goal'):
            m = np.zeros((448, 448), np.uint8)
            cy, cx = rng.integers(100, 350, 2)
            m[cy - 60:cy + 60, cx - 40:cx + 40] = 255
            Image.fromarray(np.stack([m, m, m], axis=-1)).save(str(d / (nm + '.png')))
        np.save(str(d / 'opt_den.npy'), np.array([[float(res[i])]]))
    cfg = _config('classifier', 4, 3)
    ds = T.DatasetResRgr(str(tmp_path), cfg, 'train', engine=eng)
    assert len(ds) == 3 and [int(ds[i]['target'][0]) for i in range(3)] == [0, 5, 2]
    s0 = ds[0]['input_img']
    init = (np.asarray(Image.open(str(tmp_path / '0' / 'init.png')))[..., 2] == 255).astype(np.uint8)
    goal = (np.asarray(Image.open(str(tmp_path / '0' / 'goal.png')))[..., 2] == 255).astype(np.uint8)
    np.testing.assert_array_equal(s0, eng.rgr_stack(init, goal, 'cv5'))
    res_hist = T.train_res_cls(cfg, model, {'train': T.batches(ds, 3), 'valid': T.batches(
        T.DatasetResRgr(str(tmp_path), cfg, 'valid', engine=eng), 1)})
    assert np.isfinite(res_hist['best_valid_loss'])

"""GPU: the resolution regressor (model/res_regressor.py) on the device -- stack, forward, infer_param, determinism, refusals,
isolation from the PropNet state -- against tests/golden/rgr.npz (the reference's modules with seeded weights) and the
float64 restatement of tests/_rgr_ref.py."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _rgr_ref  # noqa: E402

TAPS = ('c1', 'c2', 'c3', 'c4', 'c5', 'f1', 'f2', 'f3', 'f4')


fixture_masks = _rgr_ref.fixture_masks


@pytest.fixture(scope='module')
def z(golden):
    return golden.rgr


@pytest.fixture(scope='module')
def sds(z):
    from dyn_res_pile_manip_amd import res_regressor as rr
    seed = int(z['seed'])
    return {1: rr.random_state_dict(seed, 1), 6: rr.random_state_dict(seed, 6)}


@pytest.fixture(scope='module')
def blobs(sds):
    from dyn_res_pile_manip_amd import res_regressor as rr
    return {n: rr.blob_from_state_dict(sd, n) for n, sd in sds.items()}


@pytest.fixture(scope='module')
def eng(blobs):
    from dyn_res_pile_manip_amd.engine import Engine
    e = Engine(0)
    e.rgr_load(blobs[1], 1)
    yield e
    e.close()


@pytest.fixture(scope='module')
def base_inputs(z):
    """the 3 fixture stacks (restated; tests/test_rgr_host.py holds them to the reference's) and the 2 random inputs"""
    return _rgr_ref.fixture_inputs(z)


def batch_of(base, B):
    """B distinct inputs: base sample i % 5 shifted by i // 5 columns"""
    return np.stack([np.roll(base[i % 5], i // 5, axis=2) for i in range(B)]).astype(np.float32)


# ---- stack ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['exact', 'cv5'])
@pytest.mark.parametrize('p', [0, 1, 2])
def test_stack_matches_restatement(eng, z, p, mode):
    from oracle import goal as og
    init, goal = fixture_masks(z, p)
    dt = og.distance_transform_edt if mode == 'exact' else og.distance_transform_cv5
    ref = _rgr_ref.stack(init, goal, lambda s: np.asarray(dt(s), np.float32))
    got = eng.rgr_stack(init, goal, mode)
    assert got.shape == (6, 224, 224)
    assert float(np.abs(got - ref).max()) <= 1e-6
    if mode == 'exact':           # the transform the fixture was captured with
        _rgr_ref.check_stack(got, z, p)
    # mask and exclusion channels: exact where a cell's footprint is uniform
    h, w = init.shape
    ty, tx = _rgr_ref.area_tab(h, 224), _rgr_ref.area_tab(w, 224)
    i32, g32 = init.astype(np.float32), goal.astype(np.float32)
    srcs = {0: i32, 1: g32, 4: i32 * (1 - g32), 5: g32 * (1 - i32)}
    n_uniform = 0
    for c, src in srcs.items():
        for dy in range(0, 224, 7):
            ys = [s for s, _ in ty[dy]]
            for dx in range(0, 224, 3):
                xs = [s for s, _ in tx[dx]]
                blk = src[np.ix_(ys, xs)]
                if blk.min() == blk.max():
                    n_uniform += 1
                    assert got[c, dy, dx] == ref[c, dy, dx], (c, dy, dx)
    assert n_uniform > 1000


def test_stack_integer_scale_is_block_mean(eng, z):
    init, goal = fixture_masks(z, 0)
    init, goal = init[:448, :448], goal[:448, :448]
    from oracle import goal as og
    ref = _rgr_ref.stack(init, goal, lambda s: np.asarray(og.distance_transform_edt(s), np.float32))
    got = eng.rgr_stack(init, goal, 'exact')
    assert float(np.abs(got - ref).max()) <= 1e-6
    blk = init.astype(np.float32).reshape(224, 2, 224, 2).mean(axis=(1, 3))
    np.testing.assert_array_equal(got[0], blk)


# ---- forward ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B', [1, 3, 16, 64])
def test_forward_taps_against_float64(eng, sds, base_inputs, B):
    x = batch_of(base_inputs, B)
    out = eng.rgr_forward(x)
    ref_out, ref_taps = _rgr_ref.forward64(sds[1], x)
    for t in TAPS:
        got = eng.rgr_tap(t)
        ref = ref_taps[t]
        assert got.shape == ref.shape, (t, got.shape, ref.shape)
        scale = float(np.abs(ref).max())
        assert scale > 1e-2, (t, scale)
        err = float(np.abs(got - ref).max())
        assert err <= 1e-5 * scale, (t, err, scale)
    assert float(np.abs(out - ref_out).max()) <= 2e-5 * float(np.abs(ref_out).max())


def test_forward_layers_componentwise_batch_sweep(eng, sds, blobs, base_inputs):
    """every tap and the output against float64 on the device's own input to that layer, elementwise to TOL times
    |W| |A_prev| + |b| (tests/_rgr_train_ref.py: forward_layer_ratios), B from 64 down to 1 in one context, both heads.
    Measured on the MI355X: <= 2.9e-7 (c2); the CPU float32 stand-in <= 2.1e-7, a conv1 that drops the taps next to the
    padding 5e-1 (tests/test_rgr_backward_host.py)"""
    import _rgr_train_ref as R
    tol = R.CW_TOL
    worst = {}
    try:
        for B, n_out in ((64, 1), (63, 6), (33, 1), (17, 6), (16, 1), (5, 6), (2, 1), (1, 6)):
            eng.rgr_load(blobs[n_out], n_out)
            x = batch_of(base_inputs, B)
            out = eng.rgr_forward(x)
            r = R.forward_layer_ratios(sds[n_out], x, {t: eng.rgr_tap(t) for t in TAPS}, out)
            print('[fwd-err] rgr componentwise B=%d n_out=%d: %s' % (
                B, n_out, ', '.join('%s %.1e' % kv for kv in r.items())))
            for k, v in r.items():
                worst[k] = max(worst.get(k, 0.0), v)
                assert v <= tol, (B, n_out, k, v)
    finally:
        eng.rgr_load(blobs[1], 1)
    print('[fwd-err] rgr componentwise sweep worst: %s' % ', '.join('%s %.1e' % kv for kv in worst.items()))


@pytest.mark.parametrize('n_out', [1, 6])
def test_forward_heads_match_fixture(eng, blobs, base_inputs, z, n_out):
    eng.rgr_load(blobs[n_out], n_out)
    try:
        out = eng.rgr_forward(base_inputs)
    finally:
        eng.rgr_load(blobs[1], 1)
    name = 'rgr' if n_out == 1 else 'cls'
    ref = np.concatenate([z['%s_out%d' % (name, p)] for p in range(3)] + [z['%s_rand_out' % name]])
    assert out.shape == ref.shape == (5, n_out)
    assert float(np.abs(out - ref).max()) <= 2e-5 * float(np.abs(ref).max())


# ---- infer_param -------------------------------------------------------------------------------------------------------
def test_infer_param_regressor(eng, sds, blobs, z, base_inputs):
    from dyn_res_pile_manip_amd.res_regressor import MPCResRgrNoPool
    model = MPCResRgrNoPool({'train_res_cls': {'state_h': 224, 'state_w': 224, 'res_dim': 1}}, engine=eng,
                            dt_mode='exact').cuda().eval()
    model.load_state_dict(sds[1])
    for p in range(3):
        init, goal = fixture_masks(z, p)
        y64 = float(_rgr_ref.forward64(sds[1], base_inputs[p:p + 1])[0][0, 0])
        n = model.infer_param(init.astype(np.float32), goal.astype(np.float32))
        assert isinstance(n, int)
        if abs(y64 - round(y64)) >= 1e-4:
            assert n == int(z['rgr_infer%d' % p]), (p, n, y64)
        assert abs(model.infer_output(init, goal)[0] - y64) <= 2e-5 * abs(y64)


def test_infer_param_classifier(eng, sds, blobs, z, base_inputs):
    from dyn_res_pile_manip_amd.res_regressor import MPCResCls
    model = MPCResCls(None, engine=eng, dt_mode='exact')
    model.load_state_dict(sds[6])
    try:
        for p in range(3):
            init, goal = fixture_masks(z, p)
            logits = _rgr_ref.forward64(sds[6], base_inputs[p:p + 1])[0][0]
            top = np.sort(logits)[::-1]
            res = model.infer_param(init, goal)
            assert res in (4, 8, 16, 32, 64, 128)
            if top[0] - top[1] >= 1e-5 * np.abs(logits).max():
                assert res == int(z['cls_infer%d' % p]), (p, res, logits)
    finally:
        eng.rgr_load(blobs[1], 1)


def test_model_forward_torch_and_large_batch(eng, sds, base_inputs):
    import torch
    from dyn_res_pile_manip_amd.res_regressor import MPCResRgrNoPool
    model = MPCResRgrNoPool(None, engine=eng)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sds[1].items()})
    x = batch_of(base_inputs, 70)             # above the device bound: split into pieces of 64
    y = model.forward(torch.from_numpy(x))
    assert isinstance(y, torch.Tensor) and tuple(y.shape) == (70, 1)
    np.testing.assert_array_equal(y.numpy()[66:], eng.rgr_forward(x[66:]))
    with pytest.raises(ValueError):
        model.infer_param(np.full((300, 300), 2, np.float32), np.zeros((300, 300), np.float32))
    with pytest.raises(ValueError):
        model.infer_param(np.zeros((300, 300)), np.zeros((300, 301)))


# ---- determinism -------------------------------------------------------------------------------------------------------
def test_bit_identical_across_runs_and_batches(eng, base_inputs):
    x = batch_of(base_inputs, 16)
    a = eng.rgr_forward(x)
    f4a = eng.rgr_tap('f4')
    b = eng.rgr_forward(x)
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(f4a, eng.rgr_tap('f4'))
    for i in range(16):
        one = eng.rgr_forward(x[i:i + 1])
        np.testing.assert_array_equal(one[0], a[i])
        np.testing.assert_array_equal(eng.rgr_tap('f4')[0], f4a[i])


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(blobs, base_inputs, z):
    from dyn_res_pile_manip_amd import _lib as L
    from dyn_res_pile_manip_amd.engine import Engine
    e = Engine(0)
    try:
        x1 = base_inputs[:1]
        with pytest.raises(L.DrpError, match='no weights'):
            e.rgr_forward(x1)
        init, goal = fixture_masks(z, 0)
        with pytest.raises(L.DrpError, match='no weights'):
            e.rgr_infer(init, goal)
        e.rgr_load(blobs[1], 1)
        ok = e.rgr_forward(x1)
        with pytest.raises(L.DrpError, match='floats'):
            e.rgr_load(blobs[1][:-1], 1)
        np.testing.assert_array_equal(e.rgr_forward(x1), ok)
        with pytest.raises(L.DrpError, match='n_out'):
            e.rgr_load(blobs[1], 2)
        with pytest.raises(L.DrpError, match='floats'):
            e.rgr_load(blobs[1], 6)
        np.testing.assert_array_equal(e.rgr_forward(x1), ok)
        for B in (0, 65):
            with pytest.raises(L.DrpError, match='batch'):
                e.rgr_forward(np.zeros((B, 6, 224, 224), np.float32))
            np.testing.assert_array_equal(e.rgr_forward(x1), ok)
        for shape in ((223, 300), (300, 200)):
            with pytest.raises(L.DrpError, match='smaller'):
                e.rgr_stack(np.zeros(shape, np.uint8), np.zeros(shape, np.uint8))
            assert e.rgr_infer(init, goal, 'exact').shape == (1,)
        m = np.ascontiguousarray(init, np.uint8)
        out = np.empty(1, np.float32)
        for mode in (2, -1):
            rc = e.lib.drp_rgr_infer(e.h, m.ctypes.data_as(L.c_uint8_p), m.ctypes.data_as(L.c_uint8_p), m.shape[0],
                                     m.shape[1], mode, out.ctypes.data_as(L.c_float_p))
            assert rc == -1 and b'distance transform mode' in e.lib.drp_last_error(e.h)
            assert e.rgr_infer(init, goal, 'cv5').shape == (1,)
        np.testing.assert_array_equal(e.rgr_forward(x1), ok)
        rc = e.lib.drp_rgr_forward(e.h, None, 1, out.ctypes.data_as(L.c_float_p))
        assert rc == -1
        np.testing.assert_array_equal(e.rgr_forward(x1), ok)
    finally:
        e.close()


# ---- isolation from the PropNet state ------------------------------------------------------------------------------
def test_propnet_rollout_unchanged_by_the_regressor(blobs, base_inputs):
    from dyn_res_pile_manip_amd import synthetic as syn, weights
    from dyn_res_pile_manip_amd.engine import Engine
    from oracle import propnet_sparse as osp
    e = Engine(0)
    try:
        e.load_weights(weights.blob_from_state_dict(weights.random_state_dict(seed=0)), 0.08)
        e.set_camera(osp.world2cam_affine(syn.demo_cam_extrinsics(), 24), 24.0, syn.demo_cam_params())
        e.set_goal_image(syn.goal_distance_image(syn.goal_mask('I')), 320, fps_init=0, mode='cv5')
        s0, dens, attr = syn.make_pile(64, 1, seed=0)
        acts = syn.sample_pushes(16, 5, seed=0)
        st0, rw0 = e.rollout(s0, attr, dens, acts, want_states=True, want_reward=True)
        e.rgr_load(blobs[1], 1)
        e.rgr_forward(batch_of(base_inputs, 4))
        st1, rw1 = e.rollout(s0, attr, dens, acts, want_states=True, want_reward=True)
        np.testing.assert_array_equal(st0, st1)
        np.testing.assert_array_equal(rw0, rw1)
    finally:
        e.close()

"""CPU: the float64 restatement of the regressor's training step (tests/_rgr_train_ref.py) against tests/golden/rgr_train.npz
(the reference's train_res_cls), the host learning-rate schedulers against torch.optim.lr_scheduler, and the dataset reader."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _rgr_train_ref as R  # noqa: E402

HEADS = {'rgr': 1, 'cls': 6}


@pytest.fixture(scope='module')
def z(golden):
    return golden.rgr_train


@pytest.mark.parametrize('name', ['rgr', 'cls'])
def test_restatement_reproduces_the_reference_step(z, name):
    from dyn_res_pile_manip_amd import res_regressor as rr
    n_out = HEADS[name]
    sd = R.fixture_state_dict(int(z['seed']), n_out)
    p = '%s_s0_' % name
    batch = R.fixture_batch(z, z[p + 'batch'], n_out)
    loss, main, reg, g = R.loss_grad64(sd, *batch, lam_reg=float(z['lam_reg']))
    np.testing.assert_allclose(main, float(z[p + 'main']), rtol=1e-5)
    np.testing.assert_allclose(reg, float(z[p + 'reg']), rtol=1e-12)
    np.testing.assert_allclose(loss, float(z[p + 'loss']), rtol=1e-3)        # the reference's reg is a float32 sum
    lr, beta1 = float(z['lr']), float(z['beta1'])
    for j, (k, _) in enumerate(rr.state_dict_keys(n_out)):
        idx = R.sample_index(k, g[k].size)
        ref = z[p + 'g%d' % j].astype(np.float64)
        # the reference ran in float32 on the CPU: its convolutions' gradients carry errors of 1e-3 .. 3e-2 of the
        # tensor's largest (measured: 2.6e-3 typical, 1.3e-2 and 3.0e-2 for the conv5 bias of the two heads), the fully
        # connected ones about 1e-6.  The device is held to the float64 restatement instead (tests/test_gpu_rgr_train.py).
        tol = 6e-2 if j < 10 else 1e-5
        assert np.abs(g[k].reshape(-1)[idx] - ref).max() <= tol * np.abs(ref).max(), k
        np.testing.assert_allclose(np.abs(g[k]).sum(), z[p + 'gl1'][j], rtol=tol)
        np.testing.assert_allclose(np.sqrt((g[k] ** 2).sum()), z[p + 'gl2'][j], rtol=tol)
        # Adam's first step, restated, on the reference's own gradient samples
        w0 = sd[k].reshape(-1)[idx].astype(np.float64)
        w1, _, _ = R.adam64(w0, ref, 0.0, 0.0, 1, lr, beta1)
        assert np.abs(w1 - z[p + 'w%d' % j]).max() <= 1e-3 * lr + 4 * np.spacing(np.float32(np.abs(w0).max() + lr)), k


def test_fixture_pins_sign_of_zero(z):
    """the zeroed weights stay in the fixture's samples, and the classifier's L1 gradient is visible there"""
    from dyn_res_pile_manip_amd import res_regressor as rr
    sd = R.fixture_state_dict(int(z['seed']), 6)
    for k, _ in rr.state_dict_keys(6)[0::2]:
        idx = R.sample_index(k, sd[k].size)
        assert sd[k].reshape(-1)[idx[5]] == 0.0 and sd[k].reshape(-1)[0] == 0.0
    coef = float(z['lam_reg']) / R.fixture_state_dict(int(z['seed']), 6)['model.11.weight'].size
    assert coef > 1e-2 * float(np.abs(z['cls_s0_g10']).max())      # the FC1 weight: the L1 share is not drowned


def _torch_sched(kind, **kw):
    import torch
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.Adam([p], lr=1e-3)
    s = getattr(torch.optim.lr_scheduler, kind)(opt, **kw)
    return opt, s


class _Opt(object):
    def __init__(self, lr):
        self.param_groups = [{'lr': lr}]

    def set_lr(self, lr):
        self.param_groups[0]['lr'] = lr


def test_step_lr_matches_torch():
    from dyn_res_pile_manip_amd import train_res_rgr as T
    opt, s = _torch_sched('StepLR', step_size=3, gamma=0.1)
    mine = _Opt(1e-3)
    ms = T.StepLR(mine, step_size=3, gamma=0.1)
    for _ in range(10):
        opt.step()
        s.step()
        ms.step()
        np.testing.assert_allclose(mine.param_groups[0]['lr'], opt.param_groups[0]['lr'], rtol=1e-12)


@pytest.mark.parametrize('threshold_mode,cooldown', [('rel', 0), ('abs', 2)])
def test_reduce_on_plateau_matches_torch(threshold_mode, cooldown):
    from dyn_res_pile_manip_amd import train_res_rgr as T
    opt, s = _torch_sched('ReduceLROnPlateau', mode='min', factor=0.5, patience=2, threshold_mode=threshold_mode,
                          cooldown=cooldown)
    mine = _Opt(1e-3)
    ms = T.ReduceLROnPlateau(mine, mode='min', factor=0.5, patience=2, threshold_mode=threshold_mode, cooldown=cooldown)
    metrics = [5.0, 4.0, 4.0, 3.9999, 4.1, 4.0, 3.0, 3.0, 3.0, 3.0, 3.0, 3.0, 2.0, 2.0, 2.0, 2.0, 2.0, 2.0, 2.0]
    for v in metrics:
        opt.step()
        s.step(v)
        ms.step(v)
        np.testing.assert_allclose(mine.param_groups[0]['lr'], opt.param_groups[0]['lr'], rtol=1e-12)
    assert mine.param_groups[0]['lr'] < 1e-3


def _write_sample(d, init, goal, opt_den, opt_y=None):
    from PIL import Image
    d.mkdir()
    Image.fromarray(init).save(str(d / 'init.png'))
    Image.fromarray(goal).save(str(d / 'goal.png'))
    np.save(str(d / 'opt_den.npy'), np.array([[opt_den]]))
    if opt_y is not None:
        np.save(str(d / 'opt_y.npy'), np.array([opt_y]))


def _cfg(model_type):
    return {'train_res_cls': {'model_type': model_type, 'num_data': 3, 'train_valid_ratio': 0.67, 'state_h': 224,
                              'state_w': 224}}


def test_dataset_targets_and_refusals(tmp_path):
    pytest.importorskip('PIL')
    from dyn_res_pile_manip_amd import train_res_rgr as T
    m = np.zeros((224, 224, 3), np.uint8)
    m[50:100, 60:120] = 255
    for i, (den, oy) in enumerate(((16.0, -0.5), (128.0, -2.0), (4.0, 0.7))):
        _write_sample(tmp_path / str(i), m, m, den, oy)
    ds = T.DatasetResRgr(str(tmp_path), _cfg('regressor'), 'train')
    assert len(ds) == 2 and len(T.DatasetResRgr(str(tmp_path), _cfg('regressor'), 'valid')) == 1
    t = [ds.targets(i) for i in range(2)]
    assert t[0]['optimal_den'].shape == (1, 1) and t[0]['conf'].shape == (1,)
    np.testing.assert_allclose(t[0]['conf'], [np.exp(-0.5)], rtol=1e-6)
    np.testing.assert_allclose(t[1]['conf'], [1.0])
    assert float(t[1]['optimal_den'][0, 0]) == 128.0
    dc = T.DatasetResRgr(str(tmp_path), _cfg('classifier'), 'train')
    assert [int(dc.targets(i)['target'][0]) for i in range(2)] == [2, 5]
    assert int(T.DatasetResRgr(str(tmp_path), _cfg('classifier'), 'valid').targets(0)['target'][0]) == 0
    bad = m.copy()
    bad[0, 0] = 128
    _write_sample(tmp_path / '3', bad, m, 8.0, 0.0)
    cfg = _cfg('classifier')
    cfg['train_res_cls']['num_data'] = 4
    cfg['train_res_cls']['train_valid_ratio'] = 1.0
    with pytest.raises(ValueError):
        T.DatasetResRgr(str(tmp_path), cfg, 'train').stack(3)         # refused before any device work
    with pytest.raises(AssertionError):
        T.DatasetResRgr(str(tmp_path), cfg, 'test')


def test_read_png_takes_bgr_channel_zero(tmp_path):
    pytest.importorskip('PIL')
    from PIL import Image
    from dyn_res_pile_manip_amd import train_res_rgr as T
    rgb = np.zeros((4, 4, 3), np.uint8)
    rgb[..., 2] = 255                       # blue: cv2's channel 0
    rgb[..., 0] = 7
    Image.fromarray(rgb).save(str(tmp_path / 'a.png'))
    assert np.all(T._read_png(str(tmp_path / 'a.png')) == 255)
    Image.fromarray(rgb[..., 0]).save(str(tmp_path / 'g.png'))
    assert np.all(T._read_png(str(tmp_path / 'g.png')) == 7)

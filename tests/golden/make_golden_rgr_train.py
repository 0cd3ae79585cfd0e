#!/usr/bin/env python3
"""Generate tests/golden/rgr_train.npz from the reference's regressor training (train/train_res_rgr.py:train_res_cls).

Runs ONLY in the build container (needs /root/reference).  Shims: make_golden.install_shims(), cv2.resize =
tests/_rgr_ref.resize_area, an empty torchvision and an empty skopt (imported by the dataset module, unused here).

train_res_cls itself runs, one epoch, on the CPU: its DatasetResRgr is replaced by an in-memory one (sample i: input
_rgr_ref.rand_input(XSEED + i, 1)[0], regressor targets opt_den = [[y_i]] and opt_y = [oy_i], classifier opt_den = [[res]]),
num_worker 0, batch 4, drop_last; 12 training samples (3 UPDATE steps, shuffled by the DataLoader under torch.manual_seed)
and 4 validation samples (one EVAL batch after the steps).  save_model is patched out; torch.optim.Adam is replaced by a
subclass that records, at every step, the gradients the reference's loss.backward() left (before the step) and the weights
after it; the reference's AverageMeter is replaced by one that records every loss.item().
Both heads, res_regressor.random_state_dict(SEED) weights with a few weights set to exactly 0 (pins sign(0) = 0 of the L1
term), lr 1e-4, lam_reg LAM (large enough for the L1 gradient to show next to the data gradient).

Recorded per head and step: the batch's sample indices, the loss (float32 item()), mse | ce (the reference's statements in
float32, through wrapped criteria), reg (float64 restatement of the
reference's sum |W| / n over the pre-step weights), per-tensor float64 gradient L1 / L2 norms, gradient samples and
post-step weight samples at _rgr_train_ref.sample_index positions (every element of each bias and of the head); and the
EVAL loss and mse | ce.  The reference's own reg is a float32 sum over 114 M values (about 1e-3 relative error); the
float64 one is the yardstick.  Usage:  python tests/golden/make_golden_rgr_train.py
"""
import io
import os
import sys
import types
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = '/root/reference'
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, HERE)

SEED = 11
XSEED = 1000
LR = 1e-4
LAM = 1e5
BETA1 = 0.9
B = 4
N_TRAIN, N_VALID = 12, 4
TORCH_SEED = 5


def main():
    import make_golden
    make_golden.install_shims()
    import _rgr_ref
    import _rgr_train_ref as R
    sys.modules['cv2'].resize = _rgr_ref.resize_area
    tv = types.ModuleType('torchvision')
    tv.models = types.ModuleType('torchvision.models')
    sys.modules['torchvision'] = tv
    sys.modules['torchvision.models'] = tv.models
    sys.modules['skopt'] = types.ModuleType('skopt')
    sys.path.insert(0, REF)
    import torch
    from model.res_regressor import MPCResRgrNoPool, MPCResCls
    import train.train_res_rgr as T
    from dyn_res_pile_manip_amd import res_regressor as rr

    torch.set_num_threads(8)
    targets = R.fixture_targets(N_TRAIN + N_VALID)
    out = {'seed': np.int64(SEED), 'xseed': np.int64(XSEED), 'lr': np.float64(LR), 'lam_reg': np.float64(LAM),
           'beta1': np.float64(BETA1), 'B': np.int64(B), 'n_train': np.int64(N_TRAIN), 'n_valid': np.int64(N_VALID)}

    for name, cls, n_out, model_type in (('rgr', MPCResRgrNoPool, 1, 'regressor'), ('cls', MPCResCls, 6, 'classifier')):
        cfg = {'dataset': {'global_scale': 24},
               'train_res_cls': {'model_type': model_type, 'num_data': N_TRAIN + N_VALID,
                                 'train_valid_ratio': N_TRAIN / (N_TRAIN + N_VALID), 'state_h': 224, 'state_w': 224,
                                 'res_dim': 6, 'batch_size': B, 'num_worker': 0, 'n_epoch': 1, 'adam_beta1': BETA1,
                                 'lr': LR, 'lr_scheduler': {'type': 'StepLR', 'enabled': False}, 'lam_reg': LAM,
                                 'log_per_iter': 1, 'ckp_per_iter': 10 ** 9}}
        seen = []

        class MemDataset(torch.utils.data.Dataset):
            def __init__(self, data_dir, config, phase):
                self.st = 0 if phase == 'train' else N_TRAIN
                self.n = N_TRAIN if phase == 'train' else N_VALID

            def __len__(self):
                return self.n

            def __getitem__(self, idx):
                i = idx + self.st
                seen.append(i)
                x = torch.from_numpy(_rgr_ref.rand_input(XSEED + i, 1)[0])
                if model_type == 'regressor':
                    opt_den = np.array([[targets['y'][i]]], np.float64)
                    opt_y = np.array([targets['opt_y'][i]], np.float64)
                    conf = np.minimum(np.exp(- opt_y - 1.0), 1.0)        # dataset/dataset_res_rgr.py, verbatim
                    return {'input_img': x, 'optimal_den': torch.from_numpy(opt_den).float(),
                            'conf': torch.from_numpy(conf).float()}
                opt_den = np.array([[float(targets['res'][i])]])
                resolutions = np.array([4, 8, 16, 32, 64, 128])
                target = (resolutions == opt_den[0]).nonzero()[0][0]
                return {'input_img': x, 'scores': torch.ones(1).float(),
                        'target': torch.from_numpy(np.array([target])).long()}

        sd = R.fixture_state_dict(SEED, n_out)
        model = cls(cfg)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        keys = [k for k, _ in rr.state_dict_keys(n_out)]
        params = dict(model.named_parameters())
        steps = []
        losses = []

        class RecAdam(torch.optim.Adam):
            def step(self, closure=None):
                rec = {'batch': np.array(seen[-B:], np.int64)}
                ws = [params[k].detach().double() for k in keys[0::2]]
                rec['reg'] = float(sum(w.abs().sum() for w in ws) / sum(w.numel() for w in ws))
                g = {k: params[k].grad.detach().numpy().copy() for k in keys}
                r = super().step(closure)
                w = {k: params[k].detach().numpy().copy() for k in keys}
                rec['g'], rec['w'] = g, w
                steps.append(rec)
                return r

        mains = []              # the reference's mse | ce of every batch, float32 as its statements compute them

        class RecMSE(object):
            def __init__(self, reduction='mean'):
                self.f = torch.nn.MSELoss(reduction=reduction)

            def __call__(self, out, target):
                e = self.f(out, target)
                confs = torch.stack([torch.from_numpy(R.conf_of([targets['opt_y'][i]])) for i in seen[-B:]])
                mains.append(float((e.detach() * confs).mean()))          # (MSELoss(...) * confs).mean(), :169
                return e

        class RecCE(object):
            def __init__(self):
                self.f = torch.nn.CrossEntropyLoss()

            def __call__(self, out, target):
                loss = self.f(out, target)
                mains.append(float(loss.detach()))
                return loss

        class RecMeter(object):
            def __init__(self):
                self.sum, self.count, self.avg = 0.0, 0, 0.0

            def update(self, val, n=1):
                losses.append(float(val))
                self.sum += val * n
                self.count += n
                self.avg = self.sum / self.count

        T.DatasetResRgr = MemDataset
        T.save_model = lambda *a, **k: None
        T.optim = types.SimpleNamespace(Adam=RecAdam)
        T.AverageMeter = RecMeter
        nn_proxy = types.SimpleNamespace(**{a: getattr(torch.nn, a) for a in ('KLDivLoss', 'HuberLoss')})
        nn_proxy.MSELoss, nn_proxy.CrossEntropyLoss = RecMSE, RecCE
        T.nn = nn_proxy
        torch.manual_seed(TORCH_SEED)
        T.train_res_cls(cfg, '/nonexistent', '/nonexistent', model, 0)
        assert len(steps) == N_TRAIN // B and len(losses) == N_TRAIN // B + N_VALID // B, (len(steps), len(losses))

        for t, rec in enumerate(steps):
            p = '%s_s%d_' % (name, t)
            out[p + 'batch'] = rec['batch']
            out[p + 'loss'] = np.float64(losses[t])
            out[p + 'main'] = np.float64(mains[t])
            out[p + 'reg'] = np.float64(rec['reg'])
            out[p + 'gl1'] = np.array([np.abs(rec['g'][k].astype(np.float64)).sum() for k in keys])
            out[p + 'gl2'] = np.array([np.sqrt((rec['g'][k].astype(np.float64) ** 2).sum()) for k in keys])
            for j, k in enumerate(keys):
                idx = R.sample_index(k, rec['g'][k].size)
                out[p + 'g%d' % j] = rec['g'][k].reshape(-1)[idx].astype(np.float32)
                out[p + 'w%d' % j] = rec['w'][k].reshape(-1)[idx].astype(np.float32)
            print(name, t, 'loss', losses[t], 'reg', rec['reg'], 'max|g|', ['%.3g' % np.abs(rec['g'][k]).max() for k in keys])
        out[name + '_valid_batch'] = np.arange(N_TRAIN, N_TRAIN + N_VALID, dtype=np.int64)
        out[name + '_valid_loss'] = np.float64(losses[-1])
        out[name + '_valid_main'] = np.float64(mains[-1])
        print(name, 'valid loss', losses[-1])

    path = os.path.join(HERE, 'rgr_train.npz')
    with zipfile.ZipFile(path, 'w', compression=zipfile.ZIP_DEFLATED) as z:
        for k in sorted(out):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(out[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()

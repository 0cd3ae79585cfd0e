"""Host mirror of the reference's regressor training script (`train/train_res_rgr.py`), laid out like train_gnn_dyn.py.

  DatasetResRgr(data_dir, config, phase)   dataset/dataset_res_rgr.py:15-120  init / goal PNGs -> the 6-channel stack (on the
                                           device, drp_rgr_stack with the chamfer transform, cv2's DIST_L2 mask 5), targets
  RgrAdam(model, lr, betas, lam_reg)       :66-68   torch.optim.Adam(model.parameters(), ...) whose state lives on the engine
  StepLR, ReduceLROnPlateau                :71-90   torch.optim.lr_scheduler's rules, on the host, driving RgrAdam's lr
  run_batch(model, optimizer, data, phase) :118-183 the loop body for one batch
  train_res_cls(config, model, ...)        :25-222  epochs over 'train' / 'valid' phases, best-model tracking

The forward, the loss (conf-weighted MSE or cross entropy, plus lam_reg * the weights' mean |W|), the backward pass and Adam
run in `drp_rgr_train_step` on the MI355X; nothing here computes the network on the host.
"""
import os

import numpy as np

from .train_gnn_dyn import AverageMeter, _np

RESOLUTIONS = (4, 8, 16, 32, 64, 128)


def _read_png(path):
    """channel 0 of cv2.imread(path) (BGR: the blue channel; a grey image's only channel) as uint8"""
    try:
        from PIL import Image
    except ImportError:
        try:
            import cv2
        except ImportError:
            raise ImportError('reading %s needs PIL or cv2' % path)
        img = cv2.imread(path)
        if img is None:
            raise IOError('cannot read %s' % path)
        return np.ascontiguousarray(img[..., 0])
    with Image.open(path) as im:
        a = np.asarray(im)
        if a.ndim == 2:
            if im.mode == 'P':
                a = np.asarray(im.convert('RGB'))[..., 2]
            return np.ascontiguousarray(a.astype(np.uint8))
        if a.shape[2] >= 3:
            return np.ascontiguousarray(a[..., 2].astype(np.uint8))      # RGB(A) -> BGR channel 0 = blue
        return np.ascontiguousarray(a[..., 0].astype(np.uint8))


def _binary(img, path):
    ok = (img == 0) | (img == 255)
    if not bool(np.all(ok)):
        raise ValueError('%s: the regressor\'s masks are binary images (0 / 255), found other values' % path)
    return (img == 255).astype(np.uint8)


class DatasetResRgr(object):
    """dataset/dataset_res_rgr.py:15-120: sample i of a phase is `data_dir/%d/` with i offset by the phase's start.  Returns
    {'input_img' [6,224,224], 'optimal_den' (1,1), 'conf' (1,)} (regressor) or {'input_img', 'scores' (1,), 'target' (1,)}
    (classifier), numpy.  conf = min(exp(-opt_y - 1), 1); target = the index of opt_den[0] in [4, 8, 16, 32, 64, 128].
    The stack needs a loaded model on `engine` (the model to be trained: drp_rgr_stack runs on its context) and is cached
    per index (cache=True), since it depends on the two images only."""

    def __init__(self, data_dir, config, phase, engine=None, cache=True):
        tc = config['train_res_cls']
        self.config = config
        self.num_data = tc['num_data']
        n_train = int(self.num_data * tc['train_valid_ratio'])
        if phase == 'train':
            self.epi_st_idx, self.n_episode = 0, n_train
        elif phase == 'valid':
            self.epi_st_idx, self.n_episode = n_train, self.num_data - n_train
        else:
            raise AssertionError('Unknown phase %s' % phase)
        self.data_dir = data_dir
        self.state_h, self.state_w = tc['state_h'], tc['state_w']
        self.model_type = tc['model_type']
        if self.model_type not in ('regressor', 'classifier'):
            raise AssertionError('Unknown model type %s' % self.model_type)
        self._engine = engine
        self._cache = {} if cache else None

    def __len__(self):
        return self.n_episode

    @property
    def engine(self):
        if self._engine is None:
            from .engine import default_engine
            self._engine = default_engine()
        return self._engine

    def _path(self, idx, name):
        return os.path.join(self.data_dir, '%d' % (idx + self.epi_st_idx), name)

    def stack(self, idx):
        if self._cache is not None and idx in self._cache:
            return self._cache[idx]
        init = _binary(_read_png(self._path(idx, 'init.png')), self._path(idx, 'init.png'))
        goal = _binary(_read_png(self._path(idx, 'goal.png')), self._path(idx, 'goal.png'))
        x = self.engine.rgr_stack(init, goal, 'cv5')
        if self._cache is not None:
            self._cache[idx] = x
        return x

    def targets(self, idx):
        """the sample's targets without its images"""
        optimal_den = np.load(self._path(idx, 'opt_den.npy'))
        if self.model_type == 'classifier':
            target = int((np.array(RESOLUTIONS) == optimal_den[0]).nonzero()[0][0])
            return {'scores': np.ones(1, np.float32), 'target': np.array([target], np.int64)}
        opt_y = np.load(self._path(idx, 'opt_y.npy'))
        conf = np.minimum(np.exp(-opt_y - 1.0), 1.0)
        return {'optimal_den': np.asarray(optimal_den, np.float32), 'conf': np.asarray(conf, np.float32)}

    def __getitem__(self, idx):
        d = self.targets(idx)
        d['input_img'] = self.stack(idx)
        return d


def collate(samples):
    """torch's default_collate for the dataset's dicts: every field stacked along a new batch axis"""
    return {k: np.stack([np.asarray(s[k]) for s in samples]) for k in samples[0]}


def batches(dataset, batch_size, shuffle=False, drop_last=True, rng=None):
    """DataLoader(dataset, batch_size, shuffle, drop_last=True) without workers: a list of collated batches"""
    order = np.arange(len(dataset))
    if shuffle:
        (rng if rng is not None else np.random).shuffle(order)
    n = len(order) // batch_size if drop_last else -(-len(order) // batch_size)
    return [collate([dataset[int(i)] for i in order[j * batch_size:(j + 1) * batch_size]]) for j in range(n)]


class RgrAdam(object):
    """torch.optim.Adam(model.parameters(), lr=lr, betas=(beta1, 0.999)) whose state lives on the model's engine, with the
    L1 weight lam_reg of the loss (train/train_res_rgr.py:66-68, :170-183)."""

    def __init__(self, model, lr, betas=(0.9, 0.999), lam_reg=0.0):
        if betas[1] != 0.999:
            raise NotImplementedError('beta2 is fixed at 0.999 as in the reference')
        model._check()
        self.model = model
        self.lam_reg = float(lam_reg)
        self.param_groups = [{'lr': float(lr)}]
        model.engine.rgr_train_begin(lr, betas[0], lam_reg)

    def set_lr(self, lr):
        self.param_groups[0]['lr'] = float(lr)
        self.model.engine.rgr_train_set_lr(lr)


class StepLR(object):
    """torch.optim.lr_scheduler.StepLR(optimizer, step_size, gamma): lr = base_lr * gamma ** (epoch // step_size), one
    step() per epoch"""

    def __init__(self, optimizer, step_size, gamma=0.1):
        self.optimizer, self.step_size, self.gamma = optimizer, int(step_size), float(gamma)
        self.last_epoch = 0

    def step(self):
        self.last_epoch += 1
        if self.last_epoch % self.step_size == 0:
            self.optimizer.set_lr(self.optimizer.param_groups[0]['lr'] * self.gamma)


class ReduceLROnPlateau(object):
    """torch.optim.lr_scheduler.ReduceLROnPlateau(optimizer, mode='min', factor, patience, threshold=1e-4, threshold_mode,
    cooldown, min_lr=0, eps=1e-8): step(metric) once per validation"""

    def __init__(self, optimizer, mode='min', factor=0.1, patience=10, threshold=1e-4, threshold_mode='rel', cooldown=0,
                 min_lr=0.0, eps=1e-8, verbose=False):
        if mode not in ('min', 'max') or threshold_mode not in ('rel', 'abs') or factor >= 1.0:
            raise ValueError('bad ReduceLROnPlateau settings')
        self.optimizer, self.mode, self.factor, self.patience = optimizer, mode, float(factor), int(patience)
        self.threshold, self.threshold_mode, self.cooldown = float(threshold), threshold_mode, int(cooldown)
        self.min_lr, self.eps = float(min_lr), float(eps)
        self.best = np.inf if mode == 'min' else -np.inf
        self.num_bad_epochs, self.cooldown_counter, self.last_epoch = 0, 0, 0

    def _better(self, a, best):
        if self.mode == 'min' and self.threshold_mode == 'rel':
            return a < best * (1.0 - self.threshold)
        if self.mode == 'min':
            return a < best - self.threshold
        if self.threshold_mode == 'rel':
            return a > best * (self.threshold + 1.0)
        return a > best + self.threshold

    def step(self, metrics):
        current = float(metrics)
        self.last_epoch += 1
        if self._better(current, self.best):
            self.best, self.num_bad_epochs = current, 0
        else:
            self.num_bad_epochs += 1
        if self.cooldown_counter > 0:
            self.cooldown_counter -= 1
            self.num_bad_epochs = 0
        if self.num_bad_epochs > self.patience:
            old = self.optimizer.param_groups[0]['lr']
            new = max(old * self.factor, self.min_lr)
            if old - new > self.eps:
                self.optimizer.set_lr(new)
            self.cooldown_counter, self.num_bad_epochs = self.cooldown, 0


def make_scheduler(config, optimizer):
    """:71-90 -> None, StepLR or ReduceLROnPlateau"""
    sc = config['train_res_cls']['lr_scheduler']
    if not sc['enabled']:
        return None
    if sc['type'] == 'ReduceLROnPlateau':
        return ReduceLROnPlateau(optimizer, mode='min', factor=sc['factor'], patience=sc['patience'],
                                 threshold_mode=sc['threshold_mode'], cooldown=sc['cooldown'])
    if sc['type'] == 'StepLR':
        return StepLR(optimizer, step_size=sc['step_size'], gamma=sc['gamma'])
    raise ValueError('unknown scheduler type: %s' % sc['type'])


def run_batch(model, optimizer, data, phase='train'):
    """The loop body at :118-183 -> (loss, mse | ce, reg) as python floats (the .item() values), before the update."""
    model._check()
    x = _np(data['input_img'])
    mode = 'update' if phase == 'train' else 'eval'
    if model.N_OUT == 1:
        y = _np(data['optimal_den']).reshape(x.shape[0], -1)[:, 0]                 # optimal_den[:, 0] of (1, 1)
        conf = _np(data['conf']).reshape(x.shape[0], -1)[:, 0]
        loss, _ = model.engine.rgr_train_step(x, y=y, conf=conf, mode=mode)
    else:
        label = _np(data['target'], np.int64).reshape(x.shape[0], -1)[:, 0]       # target[:, 0]
        loss, _ = model.engine.rgr_train_step(x, label=label, mode=mode)
    return loss


def train_res_cls(config, model, dataloaders, n_epoch=None, log=None, on_best=None):
    """train/train_res_rgr.py:25-222 without the file I/O: `dataloaders` = {'train': iterable of collated batches (a list,
    or a callable returning a fresh iterable per epoch, e.g. to reshuffle), 'valid': ...}.  Returns {'best_valid_loss',
    'history': [(epoch, phase, mean loss, lr)]}."""
    tc = config['train_res_cls']
    optimizer = RgrAdam(model, float(tc['lr']), betas=(tc['adam_beta1'], 0.999), lam_reg=float(tc['lam_reg']))
    scheduler = make_scheduler(config, optimizer)
    sc_type = tc['lr_scheduler']['type']
    main_name = 'ce' if model.N_OUT != 1 else 'mse'
    best_valid_loss = np.inf
    history = []
    for epoch in range(n_epoch if n_epoch is not None else tc['n_epoch']):
        for phase in ('train', 'valid'):
            model.train(phase == 'train')
            meter = AverageMeter()
            loader = dataloaders[phase]
            for i, data in enumerate(loader() if callable(loader) else loader):
                loss, main, reg = run_batch(model, optimizer, data, phase)
                meter.update(loss, _np(data['input_img']).shape[0])
                if log is not None and i % tc['log_per_iter'] == 0:
                    log('%s [%d][%d] LR: %.6f, loss: %.6f, %s: %.6f, reg: %.6f' % (
                        phase, epoch, i, optimizer.param_groups[0]['lr'], loss, main_name, main, reg))
            history.append((epoch, phase, float(meter.avg), optimizer.param_groups[0]['lr']))
            if phase == 'train' and scheduler is not None and sc_type == 'StepLR':
                scheduler.step()
            if phase == 'valid':
                if scheduler is not None and sc_type == 'ReduceLROnPlateau':
                    scheduler.step(meter.avg)
                if meter.avg < best_valid_loss:
                    best_valid_loss = meter.avg
                    if on_best is not None:
                        on_best(model.state_dict())            # save_model(model, net_best_dy), :218-220
    model.train(False)
    return {'best_valid_loss': float(best_valid_loss), 'history': history}

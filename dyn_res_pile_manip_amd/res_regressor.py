"""The resolution regressor on the device: mirrors of model/res_regressor.py's MPCResRgrNoPool (:106-177) and MPCResCls
(:15-104), the CNN the MPC loop asks for the particle count at every step (env/flex_env.py:981-998, :1083-1086).

The forward pass and the input stack (distance transforms, exclusions, INTER_AREA downscale) run in HIP on the engine's
context (include/drp.h, drp_rgr_*); this module checks and packs the state_dict and keeps the reference's call surface:

    rgr = MPCResRgrNoPool(config)
    rgr.load_state_dict(torch.load(path))
    rgr = rgr.cuda()
    particle_num = rgr.infer_param(fg_mask, subgoal_mask)

The models share the default engine (engine.default_engine) the way gnn_dyn.PropNetDiffDenModel does; the regressor's
weights and buffers are apart from the PropNet's on that context.
"""
import numpy as np

from . import _lib as L

STATE_SIZE = 224
RES_CHOICES = (4, 8, 16, 32, 64, 128)        # MPCResCls.infer_param (:102)
_CONV = ((0, 64, 6), (2, 128, 64), (4, 256, 128), (6, 512, 256), (8, 512, 512))      # (module index, out, in)
_FC = ((11, 4096, 25088), (13, 1024, 4096), (15, 256, 1024), (17, 64, 256))
_HEAD = 19
SLOPE = 0.2


def state_dict_keys(n_out):
    """[(key, shape)] in state_dict order for a head of n_out outputs (1: regressor, 6: classifier)."""
    keys = []
    for i, co, ci in _CONV:
        keys += [('model.%d.weight' % i, (co, ci, 4, 4)), ('model.%d.bias' % i, (co,))]
    for i, co, ci in _FC + ((_HEAD, n_out, 64),):
        keys += [('model.%d.weight' % i, (co, ci)), ('model.%d.bias' % i, (co,))]
    return keys


def n_floats(n_out):
    return int(sum(int(np.prod(s)) for _, s in state_dict_keys(n_out)))


def _to_numpy(v):
    if hasattr(v, 'detach'):
        v = v.detach().cpu().numpy()
    return np.asarray(v)


def blob_from_state_dict(sd, n_out, strict=True):
    """state_dict (torch tensors or numpy arrays) -> one float32 blob in state_dict order.  Every key must be present with
    its shape; strict=True also refuses keys the model does not have."""
    keys = state_dict_keys(n_out)
    names = set(k for k, _ in keys)
    if strict:
        extra = sorted(k for k in sd.keys() if k not in names)
        if extra:
            raise KeyError('unexpected key(s) in state_dict: %s' % ', '.join(extra))
    missing = [k for k, _ in keys if k not in sd]
    if missing:
        raise KeyError('missing key(s) in state_dict: %s' % ', '.join(missing))
    blob = np.empty(n_floats(n_out), np.float32)
    p = 0
    for k, shape in keys:
        v = _to_numpy(sd[k])
        if tuple(v.shape) != shape:
            raise ValueError('size mismatch for %s: got %s, the model has %s' % (k, tuple(v.shape), shape))
        n = int(np.prod(shape))
        blob[p:p + n] = v.reshape(-1)
        p += n
    return blob


def state_dict_from_blob(blob, n_out):
    blob = np.asarray(blob, np.float32).reshape(-1)
    if blob.size != n_floats(n_out):
        raise ValueError('blob of %d floats, %d expected' % (blob.size, n_floats(n_out)))
    sd, p = {}, 0
    for k, shape in state_dict_keys(n_out):
        n = int(np.prod(shape))
        sd[k] = blob[p:p + n].reshape(shape)
        p += n
    return sd


def random_state_dict(seed=0, n_out=1):
    """Deterministic weights for tests and tools (no trained checkpoint exists offline): numpy PCG64, every layer uniform in
    +-gain / sqrt(fan_in) with the LeakyReLU(0.2) gain sqrt(6 / 1.04), which keeps every layer's activations O(1); biases
    +-0.1 / sqrt(fan_in).  The trunk depends on the seed only (the head is drawn last).  The regressor's head bias is 75 and
    its weight gain 120, so its output on mask stacks lands in about 10 ... 140 (the label range of data_gen/res_rgr_data.py:424); the
    classifier's head is drawn like the other layers."""
    rng = np.random.Generator(np.random.PCG64(seed))
    gain = np.sqrt(6.0 / (1.0 + SLOPE * SLOPE))
    sd = {}

    def uni(shape, bound):
        return ((rng.random(shape, dtype=np.float32) * 2.0 - 1.0) * np.float32(bound)).astype(np.float32)

    for k, shape in state_dict_keys(n_out):
        fan_in = int(np.prod(shape[1:])) if len(shape) > 1 else None
        layer = int(k.split('.')[1])
        if k.endswith('weight'):
            g = gain
            if layer == _HEAD and n_out == 1:
                g = 120.0
            sd[k] = uni(shape, g / np.sqrt(fan_in))
        else:
            fan_in = int(np.prod(sd[k.replace('bias', 'weight')].shape[1:]))
            sd[k] = uni(shape, 0.1 / np.sqrt(fan_in))
            if layer == _HEAD and n_out == 1:
                sd[k] = sd[k] + np.float32(75.0)
    return sd


def masks_from_obs(obs, subgoal, global_scale):
    """The two masks of env/flex_env.py:994-996: the foreground of the rendered depth (obs[..., -1] / global_scale below
    0.599 / 0.8) and the subgoal's pixels (subgoal < 0.5), float32 0/1."""
    obs = np.asarray(obs)
    fg = (obs[..., -1] / global_scale < 0.599 / 0.8).astype(np.float32)
    goal = (np.asarray(subgoal) < 0.5).astype(np.float32)
    return fg, goal


def _mask_u8(m, name):
    m = _to_numpy(m)
    if m.ndim != 2:
        raise ValueError('%s must be a 2-D mask, got shape %s' % (name, m.shape))
    ok = (m == 0) | (m == 1)
    if not bool(np.all(ok)):
        raise ValueError('%s must hold only 0 and 1' % name)
    return np.ascontiguousarray(m, dtype=np.uint8)


class _ResModel(object):
    N_OUT = None

    def __init__(self, config=None, engine=None, dt_mode='cv5'):
        cfg = (config or {}).get('train_res_cls', {}) if isinstance(config, dict) else {}
        self.config = config
        self.state_h = int(cfg.get('state_h', STATE_SIZE))
        self.state_w = int(cfg.get('state_w', STATE_SIZE))
        self.res_dim = cfg.get('res_dim', None)
        if self.state_h != STATE_SIZE or self.state_w != STATE_SIZE:
            raise ValueError('state_h x state_w = %d x %d: the network is built for %d x %d (its flatten is 512 x 7 x 7)'
                             % (self.state_h, self.state_w, STATE_SIZE, STATE_SIZE))
        if dt_mode not in L.DIST_TRANSFORMS:
            raise ValueError('dt_mode %r: one of %s' % (dt_mode, sorted(L.DIST_TRANSFORMS)))
        self.dt_mode = dt_mode
        self._engine = engine
        self._loaded = False

    @property
    def engine(self):
        if self._engine is None:
            from .engine import default_engine
            self._engine = default_engine()
        return self._engine

    def load_state_dict(self, sd, strict=True):
        blob = blob_from_state_dict(sd, self.N_OUT, strict=strict)
        eng = self.engine
        eng.rgr_owner = None
        eng.rgr_load(blob, self.N_OUT)
        eng.rgr_owner = self          # a context holds one regressor's weights at a time
        self._loaded = True
        return self

    def _check(self):
        if not getattr(self, '_loaded', False):
            raise RuntimeError('%s: load_state_dict first' % type(self).__name__)
        if getattr(self.engine, 'rgr_owner', None) is not self:
            raise RuntimeError('%s: the engine holds another model\'s regressor weights now (load_state_dict again)'
                               % type(self).__name__)

    def forward(self, x):
        """x [B,6,224,224] (numpy or torch) -> [B,n_out] (the same kind; a torch result lives on the CPU)."""
        self._check()
        is_torch = hasattr(x, 'detach')
        a = np.ascontiguousarray(_to_numpy(x), dtype=np.float32)
        if a.ndim != 4 or a.shape[1:] != (6, STATE_SIZE, STATE_SIZE):
            raise ValueError('input of shape %s, [B, 6, %d, %d] expected' % (a.shape, STATE_SIZE, STATE_SIZE))
        # batches above the device bound go in pieces: outputs do not depend on the batch a sample travels in
        out = np.concatenate([self.engine.rgr_forward(a[i:i + L.RGR_BMAX]) for i in range(0, a.shape[0], L.RGR_BMAX)])
        if is_torch:
            import torch
            return torch.from_numpy(out)
        return out

    __call__ = forward

    def stack(self, init_img, goal_img):
        """The 6 x 224 x 224 input infer_param builds (:146-175), computed on the device."""
        self._check()
        a, b = self._masks(init_img, goal_img)
        return self.engine.rgr_stack(a, b, self.dt_mode)

    def _masks(self, init_img, goal_img):
        a, b = _mask_u8(init_img, 'init_img'), _mask_u8(goal_img, 'goal_img')
        if a.shape != b.shape:
            raise ValueError('init_img %s and goal_img %s differ in shape' % (a.shape, b.shape))
        return a, b

    def infer_output(self, init_img, goal_img):
        """the head's raw outputs [n_out] of infer_param"""
        self._check()
        a, b = self._masks(init_img, goal_img)
        return self.engine.rgr_infer(a, b, self.dt_mode)

    def state_dict(self, as_torch=False):
        """the device's current weights (training moves them) as {key: array} in state_dict order, torch layouts; torch
        tensors with as_torch=True"""
        self._check()
        sd = state_dict_from_blob(self.engine.rgr_get_weights(), self.N_OUT)
        if as_torch:
            import torch
            return {k: torch.from_numpy(v.copy()) for k, v in sd.items()}
        return sd

    def cuda(self, *args, **kwargs):
        return self

    def train(self, mode=True):
        """nn.Module.train: the network has no dropout or batch norm, nothing changes"""
        self.training = bool(mode)
        return self

    def eval(self):
        return self.train(False)

    def to(self, *args, **kwargs):
        return self


class MPCResRgrNoPool(_ResModel):
    """model/res_regressor.py:106-177: infer_param(init, goal) -> int(particle count)."""
    N_OUT = L.RGR_REGRESSOR

    def infer_param(self, init_img, goal_img):
        return int(self.infer_output(init_img, goal_img)[0])


class MPCResCls(_ResModel):
    """model/res_regressor.py:15-104: infer_param(init, goal) -> [4, 8, 16, 32, 64, 128][argmax of the 6 logits]."""
    N_OUT = L.RGR_CLASSIFIER

    def infer_param(self, init_img, goal_img):
        return RES_CHOICES[int(np.argmax(self.infer_output(init_img, goal_img)))]

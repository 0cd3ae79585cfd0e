"""Host mirror of the reference's training script body (`train/train_gnn_dyn.py`), row f4.

  collate_fn(data)                     :20-45   variable particle counts -> zero-padded batch
  collate_untracked(data)              the same, plus each sample's per-step target clouds (no counterpart: loss='chamfer')
  DeviceAdam(model, lr, betas)         :128-131 torch.optim.Adam(model.parameters(), ...) on the device
  run_batch(model, optimizer, data, phase)      :159-210 the loop body for one batch
  train(config, datasets, ...)         :134-246 epochs over 'train' / 'valid' phases, best-model tracking
  main(config, data_root, train_dir)   :45-130,196-228 the file-level part: seed, log dir, datasets and loaders
                                       (dataset_gnn_dyn.py), checkpoints, resume; `python -m dyn_res_pile_manip_amd.train_gnn_dyn`

The forward, the loss, the backward pass (state and weight gradients) and the Adam update run
in `drp_train_step` on the MI355X; nothing here computes on the host.  Data loading
(`dataset/dataset_gnn_dyn.py`: depth PNGs, pickled actions) is outside the path: `datasets`
is any pair of iterables of samples shaped like `ParticleDataset.__getitem__`'s return.
"""
import collections
import os

import numpy as np


def _np(x, dtype=np.float32):
    if hasattr(x, 'detach'):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=dtype)


class PaddedBatch(tuple):
    """What `collate_fn` returns: the reference's 6-tuple (states, states_delta, attr, particle_num,
    particle_den, color_imgs), plus the ragged layout it was built from."""
    offsets = None          # [B+1] running particle offset of each sample in the concatenated cloud
    actions = None          # [B, n_rollout, 4] float32, the raw pushes (sx, sy, ex, ey) of the samples' steps where the loader has
                            # them (dataset_gnn_dyn.get_batch / DeviceLoader): what impulses='actions' trains on
    depth_only = False      # True: the batch comes from depth frames alone (dataset_gnn_dyn.DepthDataset): states has only step 0
                            # and states_delta is zeros, so it trains with loss='chamfer', impulses='actions' and nothing else


def collate_fn(data):
    """Contract of train/train_gnn_dyn.py:20-45: samples with different particle counts become one batch
    zero-padded to the largest count -- states [B,T,n_max,3], states_delta [B,T-1,n_max,3], attr [B,T,n_max],
    particle_num [B] int32, particle_den [B] float32, color_imgs.

    Built as one ragged pack instead of a per-sample copy loop: the samples' particle axes are concatenated
    ([T, sum n, 3]), every particle gets its (sample, slot) address from the running offsets, and a single
    fancy-indexed store per field places the whole batch.  The offsets stay on the result (`.offsets`)."""
    counts = np.fromiter((int(d[3]) for d in data), dtype=np.int64, count=len(data))
    offsets = np.concatenate([[0], np.cumsum(counts)])
    B, n_max = len(data), int(counts.max())
    owner = np.repeat(np.arange(B), counts)                      # sample of every packed particle
    slot = np.arange(offsets[-1]) - offsets[owner]               # its index inside that sample
    def pack(field, time_axis_len=None):
        cloud = np.concatenate([_np(d[field]) for d in data], axis=1)           # [T, sum n(, 3)]
        out = np.zeros((B, cloud.shape[0], n_max) + cloud.shape[2:], dtype=np.float32)
        out[owner, :, slot] = np.moveaxis(cloud, 1, 0)
        return out
    imgs = None if data[0][5] is None else np.stack([np.asarray(d[5], dtype=np.float32) for d in data])
    batch = PaddedBatch((pack(0), pack(1), pack(2), counts.astype(np.int32),
                         np.asarray([d[4] for d in data], dtype=np.float32), imgs))
    batch.offsets = offsets
    return batch


def collate_untracked(data, actions=None):
    """collate_fn for untracked samples (dataset_gnn_dyn.drop_correspondence: the 6-tuple, then a list of n_rollout target clouds
    [m_t, 3]): the six fields as collate_fn gives them, then targets [B, H, M, 3] zero-padded to the largest cloud and
    target_nums [B, H] int32.  actions: the samples' pushes [B, H, 4], carried through as `.actions`."""
    batch = collate_fn(data)
    B, H = len(data), len(data[0][6])
    counts = np.array([[np.asarray(c).shape[0] for c in d[6]] for d in data], dtype=np.int64).reshape(B, H)
    flat = counts.reshape(-1)
    owner = np.repeat(np.arange(B * H), flat)                    # (sample, step) of every packed target row
    slot = np.arange(flat.sum()) - (np.cumsum(flat) - flat)[owner]
    targets = np.zeros((B * H, int(counts.max()), 3), dtype=np.float32)
    targets[owner, slot] = np.concatenate([_np(c).reshape(-1, 3) for d in data for c in d[6]], axis=0)
    out = PaddedBatch(tuple(batch) + (targets.reshape(B, H, -1, 3), counts.astype(np.int32)))
    out.offsets = batch.offsets
    if actions is not None:
        out.actions = np.asarray(actions, dtype=np.float32).reshape(B, H, 4)
    return out


class DeviceAdam(object):
    """torch.optim.Adam(model.parameters(), lr=lr, betas=(beta1, 0.999)) whose state lives in the
    model's engine (train/train_gnn_dyn.py:128-131)."""

    def __init__(self, model, lr, betas=(0.9, 0.999), n_rollout=5):
        if betas[1] != 0.999:
            raise NotImplementedError('beta2 is fixed at 0.999 as in the reference')
        self.model = model
        self.param_groups = [{'lr': float(lr)}]
        model.engine.train_begin(n_rollout, lr, betas[0])

    def set_lr(self, lr):
        self.param_groups[0]['lr'] = float(lr)
        self.model.engine.train_set_lr(lr)

    def state_dict(self):
        """Adam's moments and step count as the engine holds them (Engine.train_get_state): {'m', 'v': float32 [38403] in
        get_weights' layout, 'iter': int} -- with the weights, all a resumed run needs to continue with an uninterrupted one's bits"""
        m, v, it = self.model.engine.train_get_state()
        return {'m': m, 'v': v, 'iter': it}

    def load_state_dict(self, state):
        self.model.engine.train_set_state(state['m'], state['v'], int(state['iter']))


LOSSES = ('mse', 'chamfer')
# the one-to-one matching loss of Engine.cloud_match and its mix with the Chamfer distance (Engine.train_step_loss): they train as
# 'chamfer' does, on collate_untracked's batches.  The three older probe options refuse them (their refusals are pinned by
# tests); their float64 yardstick (Engine.train_grad_f64_match) is reached through an option of its own, match_probe_every /
# probe_batch_match
MATCH_LOSSES = ('match', 'chamfer+match')
# the entropy-regularised transport loss of Engine.cloud_transport (Engine.train_step_transport): fractional masses, so clouds of
# unequal counts share mass and every real row has a gradient.  It trains as the matching losses do and, like them, has no
# float64 yardstick: the probe options refuse it with their message
TRANSPORT_LOSSES = ('transport',)
UNTRACKED_LOSSES = ('chamfer',) + MATCH_LOSSES + TRANSPORT_LOSSES
# the Sinkhorn divergence of Engine.cloud_divergence (Engine.train_step_divergence): the transport loss with its entropic bias
# taken out -- its minimum over the prediction is the target cloud, not a shrunken copy of it -- and the loss to use on depth
# data.  It trains on the batches UNTRACKED_LOSSES train on and takes the transport loss's two options.  The three older probe
# options refuse it as they refuse the transport loss (their refusals are pinned by tests); its float64 yardstick
# (Engine.train_grad_f64_divergence) is reached through an option of its own, sinkhorn_probe_every / probe_batch_sinkhorn.  A
# tuple of its own: the four above are pinned by tests as they are
DIVERGENCE_LOSSES = ('sinkhorn',)
IMPULSES = ('data', 'actions')
DATA = ('particles', 'depth')
# eps_b = transport_eps_scale / particle_dens[b]: 1 / den is the squared fps_rad sampling radius, so scale 1 blurs the plan over
# one particle spacing -- a definition, not a tuned value
TRANSPORT_EPS_SCALE = 1.0
# the smallest of {10, 20, 50, 100, 200} at which the host reference's col_err is at most 1 % of the total mass on every case of
# tests/_untracked_ref.chamfer_cases() at scale 1 (DESIGN.md 9 has the table)
TRANSPORT_ITERS = 50
from ._lib import TRANSPORT_MAX_ITERS  # noqa: E402  (include/drp.h: DRP_TRANSPORT_MAX_ITERS)


def check_loss(loss, match_weight=0.5, transport_eps_scale=TRANSPORT_EPS_SCALE, transport_iters=TRANSPORT_ITERS):
    if callable(loss):                      # a loss of the caller's (Engine.train_step_custom): no option above is its
        return
    if loss not in LOSSES + MATCH_LOSSES + TRANSPORT_LOSSES + DIVERGENCE_LOSSES:
        raise ValueError('loss must be one of %s or %s or %s or %s, got %r' % (LOSSES, MATCH_LOSSES, TRANSPORT_LOSSES, DIVERGENCE_LOSSES, loss))
    if loss == 'chamfer+match' and not 0.0 < float(match_weight) < 1.0:
        raise ValueError('match_weight must lie in (0, 1), got %r' % (match_weight,))
    if loss in TRANSPORT_LOSSES + DIVERGENCE_LOSSES:
        if not 0.0 < float(transport_eps_scale) < float('inf'):
            raise ValueError('transport_eps_scale must be a positive finite number, got %r' % (transport_eps_scale,))
        if int(transport_iters) != transport_iters or not 1 <= int(transport_iters) <= TRANSPORT_MAX_ITERS:
            raise ValueError('transport_iters must be an integer in 1..%d, got %r' % (TRANSPORT_MAX_ITERS, transport_iters))


# the unbalanced Sinkhorn divergence (Engine.train_step_divergence(reach=...)): for a pile seen partly.  sinkhorn_reach_scale r:
# rho_b = r / particle_dens[b], transport_eps_scale's unit, so r = 4 is a reach of two particle spacings; None: balanced.
# sinkhorn_mass: the target cloud's total mass against the prediction's 1 -- 'unit': 1; 'count': target_nums[b, t] /
# particle_nums[b], equal mass per point, right when the targets are sampled at the particles' spacing (target_den_scale == 1).
# Its float64 yardstick (Engine.train_grad_f64_divergence(reach=...)) is reached through sinkhorn_reach_probe_every;
# sinkhorn_probe_every keeps refusing a reach (tests/test_divergence_unbalanced_host.py pins that)
SINKHORN_MASSES = ('unit', 'count')
SINKHORN_MIN_REACH_PER_EPS = 1.0 / 1024.0       # include/drp.h: rho >= eps / 1024
SINKHORN_MASS_RANGE = (0.125, 8.0)              # include/drp.h: 1/8 <= mass_q <= 8


def check_sinkhorn_options(loss, sinkhorn_reach_scale=None, sinkhorn_mass='unit', sinkhorn_probe_every=0,
                           transport_eps_scale=TRANSPORT_EPS_SCALE):
    """sinkhorn_reach_scale and sinkhorn_mass of run_batch() / train() / main(): DIVERGENCE_LOSSES' alone; 'count' needs a reach
    (balanced transport between unequal masses has no plan); sinkhorn_probe_every probes the balanced divergence and
    is refused with a reach -- refused, not skipped (a test pins it); sinkhorn_reach_probe_every probes the unbalanced one"""
    if sinkhorn_mass not in SINKHORN_MASSES:
        raise ValueError('sinkhorn_mass must be one of %s, got %r' % (SINKHORN_MASSES, sinkhorn_mass))
    if sinkhorn_reach_scale is None:
        if sinkhorn_mass != 'unit':
            raise ValueError('sinkhorn_mass=%r needs sinkhorn_reach_scale: balanced transport between unequal masses has no plan'
                             % (sinkhorn_mass,))
        return
    if loss not in DIVERGENCE_LOSSES:
        raise ValueError('sinkhorn_reach_scale and sinkhorn_mass need a loss of %s, got %r' % (DIVERGENCE_LOSSES, loss))
    r = float(sinkhorn_reach_scale)
    if not (r == float('inf') or (0.0 < r < float('inf') and r >= float(transport_eps_scale) * SINKHORN_MIN_REACH_PER_EPS)):
        raise ValueError('sinkhorn_reach_scale must be inf or a positive finite number of at least transport_eps_scale / 1024, got %r'
                         % (sinkhorn_reach_scale,))
    if r == float('inf') and sinkhorn_mass != 'unit':
        raise ValueError('sinkhorn_mass=%r needs a finite sinkhorn_reach_scale: balanced transport between unequal masses has no plan'
                         % (sinkhorn_mass,))
    if sinkhorn_probe_every > 0:
        raise ValueError('sinkhorn_probe_every: there is no float64 yardstick for the unbalanced divergence yet under this option '
                         '(sinkhorn_reach_scale=%r): sinkhorn_reach_probe_every reaches it' % (sinkhorn_reach_scale,))


def sinkhorn_reach(particle_dens, sinkhorn_reach_scale):
    """every sample's reach, float64 [B]: sinkhorn_reach_scale / particle_dens[b]"""
    return float(sinkhorn_reach_scale) / np.asarray(particle_dens, np.float64).reshape(-1)


def sinkhorn_mass_q(sinkhorn_mass, particle_nums, target_nums):
    """the target clouds' total masses, float64 [n_rollout, B], from particle_nums [B] and target_nums [B, n_rollout]"""
    tn = np.asarray(target_nums, np.float64)
    if sinkhorn_mass == 'unit':
        return np.ones(tn.T.shape)
    w = np.ascontiguousarray((tn / np.asarray(particle_nums, np.float64).reshape(-1, 1)).T)
    if not ((w >= SINKHORN_MASS_RANGE[0]) & (w <= SINKHORN_MASS_RANGE[1])).all():
        raise ValueError('sinkhorn_mass=\'count\': a target cloud has less than 1/8 or more than 8 times its prediction\'s points')
    return w


def transport_eps(particle_dens, transport_eps_scale=TRANSPORT_EPS_SCALE):
    """every sample's regularisation strength, float64 [B]: transport_eps_scale / particle_dens[b]"""
    return float(transport_eps_scale) / np.asarray(particle_dens, np.float64).reshape(-1)


def refuse_custom_probe(loss, option):
    """the five older probe options hold a built-in loss against its own float64 yardstick: a callable loss has none of those"""
    if callable(loss):
        raise ValueError('%s probes the built-in losses: a callable loss (%s) is probed through custom_probe_every'
                         % (option, getattr(loss, '__name__', repr(loss))))


def _check_schedule(row, loss, every, sinkhorn_reach_scale=None):
    """One probe schedule of train() / main() by its row of SCHEDULES; every: {option: its value} for the row's own option and
    its companions.  The schedule is a non-negative integer; given (> 0), it refuses a loss that is not the row's -- a callable
    one by name, for a built-in row --, any companion beside it, and a missing reach where the row needs one."""
    k = every[row.option]
    if int(k) != k or k < 0:
        raise ValueError('%s must be a non-negative integer, got %r' % (row.option, k))
    if k > 0:
        if row.losses is not None:
            refuse_custom_probe(loss, row.option)
        if any(every[c] > 0 for c in row.companions):
            raise ValueError('give %s alone, not with %s or %s' % (row.option, ', '.join(row.companions[:-1]), row.companions[-1]))
        if not callable(loss) if row.losses is None else loss not in row.losses:
            raise ValueError('%s needs %s, got %r: probe_every probes the losses of %s'
                             % (row.option, 'a callable loss' if row.losses is None else 'a loss of %s' % (row.losses,), loss, LOSSES))
        if row.needs_reach and sinkhorn_reach_scale is None:
            raise ValueError('%s needs sinkhorn_reach_scale: sinkhorn_probe_every probes the balanced divergence' % row.option)


def check_custom_probe_option(loss, custom_probe_every, grad_probe_every=0, probe_every=0, sinkhorn_probe_every=0, match_probe_every=0,
                              sinkhorn_reach_probe_every=0):
    """custom_probe_every of train() / main(): the probe schedule of a callable loss alone (probe_batch_custom), and no companion of
    the five other schedules -- each of which refuses a callable loss, naming it"""
    row = SCHEDULES['custom_probe_every']
    every = dict(zip(row.companions, (grad_probe_every, probe_every, sinkhorn_probe_every, match_probe_every,
                                      sinkhorn_reach_probe_every)), custom_probe_every=custom_probe_every)
    for option in row.companions:
        if every[option] > 0:
            refuse_custom_probe(loss, option)
    _check_schedule(row, loss, every)


def refuse_match_probe(loss):
    if loss in MATCH_LOSSES + TRANSPORT_LOSSES + DIVERGENCE_LOSSES:
        raise ValueError('there is no float64 yardstick for the matching loss yet: loss=%r cannot be probed '
                         '(probe_every, grad_probe_every, probe_batch)' % (loss,))


def check_depth_only(data, loss, impulses):
    """a batch made from depth frames alone has no tracked targets and no recorded impulses: anything but the Chamfer loss through
    the push would train on zeros"""
    if getattr(data, 'depth_only', False) and callable(loss) and impulses == 'actions':
        return                              # a loss of the caller's: what it reads of the batch is its own affair
    if getattr(data, 'depth_only', False) and not (loss in UNTRACKED_LOSSES + DIVERGENCE_LOSSES and impulses == 'actions'):
        raise ValueError('a depth-only batch (DepthDataset) holds no tracked states and no impulses: it needs loss=\'chamfer\' (or '
                         'one of %s) and impulses=\'actions\', got loss=%r, impulses=%r'
                         % (MATCH_LOSSES + TRANSPORT_LOSSES + DIVERGENCE_LOSSES, loss, impulses))


def resolve_data_options(data, loss, impulses):
    """main()'s / the command line's data, loss and impulses -> (loss, impulses).  None = not given: 'mse' and 'data' for
    data='particles'; data='depth' implies 'chamfer' and 'actions'; it takes a member of MATCH_LOSSES, TRANSPORT_LOSSES or
    DIVERGENCE_LOSSES in place of 'chamfer' and refuses anything else."""
    if data not in DATA:
        raise ValueError('data must be one of %s, got %r' % (DATA, data))
    if data == 'depth':
        if callable(loss):
            if impulses not in (None, 'actions'):
                raise ValueError('data=\'depth\' has no recorded impulses: impulses=%r contradicts the impulses=\'actions\' it implies'
                                 % (impulses,))
            return loss, 'actions'
        if loss not in (None,) + UNTRACKED_LOSSES + DIVERGENCE_LOSSES:
            raise ValueError('data=\'depth\' trains on untracked clouds: loss=%r contradicts the loss=\'chamfer\' it implies' % (loss,))
        if impulses not in (None, 'actions'):
            raise ValueError('data=\'depth\' has no recorded impulses: impulses=%r contradicts the impulses=\'actions\' it implies'
                             % (impulses,))
        return 'chamfer' if loss is None else loss, 'actions'
    return 'mse' if loss is None else loss, 'data' if impulses is None else impulses


def batch_actions(data):
    """the pushes [B, n_rollout, 4] a loader attached to a collated batch (impulses='actions')"""
    actions = getattr(data, 'actions', None)
    if actions is None:
        raise ValueError('impulses=\'actions\' needs a batch with .actions [B, n_rollout, 4] (ParticleDataset.get_batch, DeviceLoader, '
                         'UntrackedLoader attach it)')
    return _np(actions)


class _LossSpec(object):
    """A run's loss and its options, checked once (check_loss, check_sinkhorn_options): what run_batch, the probe_batch*
    functions and train() read instead of carrying the six values each."""

    def __init__(self, loss, match_weight=0.5, transport_eps_scale=TRANSPORT_EPS_SCALE, transport_iters=TRANSPORT_ITERS,
                 sinkhorn_reach_scale=None, sinkhorn_mass='unit', sinkhorn_probe_every=0):
        check_loss(loss, match_weight, transport_eps_scale, transport_iters)
        check_sinkhorn_options(loss, sinkhorn_reach_scale, sinkhorn_mass, sinkhorn_probe_every, transport_eps_scale)
        self.loss, self.match_weight, self.eps_scale, self.iters = loss, match_weight, transport_eps_scale, transport_iters
        self.reach_scale, self.mass = sinkhorn_reach_scale, sinkhorn_mass

    def eps(self, b):
        return transport_eps(b.dens, self.eps_scale)

    def reach_args(self, b):
        """the unbalanced divergence's keywords of the engine's calls on a batch; none without a reach"""
        if self.reach_scale is None:
            return {}
        return {'reach': sinkhorn_reach(b.dens, self.reach_scale), 'mass_q': sinkhorn_mass_q(self.mass, b.nums, b.tnums)}


class _Batch(object):
    """A collated batch as the engine's trainer calls take it, for a loss and an impulse source (both checked against the
    batch): states, states_delta (None where the batch has none), attrs, nums, dens; actions for impulses='actions', else None;
    sd: states_delta, None beside actions; targets, tnums for a loss that trains on target clouds, else None.  The model's
    weights are claimed for the context (models share the process's)."""

    def __init__(self, model, data, loss, impulses):
        if impulses not in IMPULSES:
            raise ValueError('impulses must be one of %s, got %r' % (IMPULSES, impulses))
        check_depth_only(data, loss, impulses)
        self.actions = batch_actions(data) if impulses == 'actions' else None
        self.states, self.attrs, self.nums, self.dens = _np(data[0]), _np(data[2]), _np(data[3], np.int32), _np(data[4])
        self.states_delta = None if data[1] is None else _np(data[1])
        self.sd = None if self.actions is not None else self.states_delta
        untracked = not callable(loss) and loss in UNTRACKED_LOSSES + DIVERGENCE_LOSSES
        self.targets, self.tnums = (_np(data[6]), _np(data[7], np.int32)) if untracked else (None, None)
        if hasattr(model, '_claim'):
            model._claim()

    def probe(self, model, states_delta, **kw):
        return model.engine.train_gradient_probe(self.states, states_delta, self.attrs, self.nums, self.dens, actions=self.actions,
                                                 **kw)


def run_batch(model, optimizer, data, phase='train', n_rollout=None, loss='mse', impulses='data', match_weight=0.5,
              transport_eps_scale=TRANSPORT_EPS_SCALE, transport_iters=TRANSPORT_ITERS, sinkhorn_reach_scale=None,
              sinkhorn_mass='unit', stats=None, mode=None):
    """The loop body at train/train_gnn_dyn.py:159-210 -> loss (python float, what loss.item() is there).  loss='chamfer': `data`
    is collate_untracked's (targets and target_nums behind the six fields) and each step's term is the Chamfer distance to its
    target cloud (Engine.train_step_untracked).  A batch marked depth_only (DepthDataset) is refused (ValueError) unless
    loss='chamfer' and impulses='actions'.  impulses='actions': every step's impulse is computed from the batch's pushes
    (`data.actions`) on the state the step reads instead of taken from states_delta (Engine.train_step_actions; the engine's
    camera must be set).  loss='match' / 'chamfer+match' (MATCH_LOSSES): collate_untracked's batches as for 'chamfer', each step's
    term the one-to-one matching distance to its target cloud, or (1 - match_weight) Chamfer + match_weight matching, with either
    impulse source (Engine.train_step_loss).  loss='transport' (TRANSPORT_LOSSES): the same batches and impulse sources, each
    step's term the entropy-regularised transport distance to its target cloud after transport_iters sweeps with
    eps_b = transport_eps_scale / particle_dens[b] (Engine.train_step_transport).  loss='sinkhorn' (DIVERGENCE_LOSSES): the same
    again with the Sinkhorn divergence as each step's term, under the same two options (Engine.train_step_divergence).
    sinkhorn_reach_scale (not None) and sinkhorn_mass: the unbalanced divergence with rho_b = sinkhorn_reach_scale /
    particle_dens[b] and the targets' masses of sinkhorn_mass_q (check_sinkhorn_options); `stats`, a dict, then receives
    'transported': the mean over the batch's problems of the share of the predicted mass the plan pairs with something.
    A CALLABLE loss: loss(pred, context) -> (value, d value / d pred) of losses.py, trained through Engine.train_step_custom
    with `data` itself as the context, on either impulse source and, with impulses='actions', on depth_only batches too.
    mode (None: 'update' for phase 'train', else 'eval'): 'grad' runs the same call with the weights untouched and the
    gradient left on the device for Engine.train_accumulate -- train()'s accum_steps / clip_norm path."""
    spec = _LossSpec(loss, match_weight, transport_eps_scale, transport_iters, sinkhorn_reach_scale, sinkhorn_mass)
    if mode is None:
        mode = 'update' if phase == 'train' else 'eval'
    b = _Batch(model, data, loss, impulses)
    if n_rollout is not None:
        assert b.states.shape[1] == n_rollout + 1       # :166 (n_history = 1)
    if hasattr(model, '_claim'):
        model._device_ahead = model._device_ahead or mode == 'update'
    engine, four, source = model.engine, (b.states, b.attrs, b.nums, b.dens), {'states_delta': b.sd, 'actions': b.actions}
    if callable(loss):
        return engine.train_step_custom(loss, *four, mode=mode, context=data, **source)[0]
    if loss in MATCH_LOSSES:
        return engine.train_step_loss(*four, b.targets, b.tnums, loss=loss, match_weight=match_weight, mode=mode, **source)[0]
    if loss in TRANSPORT_LOSSES + DIVERGENCE_LOSSES:
        step = engine.train_step_transport if loss in TRANSPORT_LOSSES else engine.train_step_divergence
        reach = spec.reach_args(b)
        if reach:
            reach['want_err'] = stats is not None
        out = step(*four, b.targets, b.tnums, spec.eps(b), int(spec.iters), mode=mode, **source, **reach)
        if reach and stats is not None:
            stats['transported'] = float(out[4].mean())
        return out[0]
    if b.actions is not None:
        return engine.train_step_actions(b.states, b.actions, b.attrs, b.nums, b.dens, b.targets, b.tnums, mode=mode)[0]
    if loss == 'chamfer':
        return engine.train_step_untracked(b.states, b.sd, b.attrs, b.nums, b.dens, b.targets, b.tnums, mode=mode)[0]
    return engine.train_step(b.states, b.sd, b.attrs, b.nums, b.dens, mode=mode)[0]


class AverageMeter(object):
    """utils.AverageMeter as the training loop uses it (:156, :205)."""

    def __init__(self):
        self.sum, self.count, self.avg = 0.0, 0, 0.0

    def update(self, val, n=1):
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count


def probe_batch(model, data, impulses='data', loss='mse'):
    """Engine.train_gradient_probe on a collated batch: the trainer's fp32 gradients against the float64 evaluation of the same
    batch on the device; weights, Adam state and iteration count are untouched.  loss='chamfer': `data` is collate_untracked's
    and the result also has 'min_margin' (Engine.train_gradient_probe).  A member of MATCH_LOSSES, TRANSPORT_LOSSES or
    DIVERGENCE_LOSSES is refused: no yardstick yet."""
    check_loss(loss)
    refuse_match_probe(loss)
    b = _Batch(model, data, loss, impulses)
    return b.probe(model, b.states_delta, **({'targets': b.targets, 'target_nums': b.tnums} if loss == 'chamfer' else {}))


def probe_batch_custom(model, data, loss, impulses='data'):
    """Engine.train_gradient_probe_custom on a collated batch with a callable loss, `data` itself as its context: the fp32 pair
    (train_predict, the loss, train_step_seeded) against the float64 pair; the result has 'loss_kind': 'custom' and 'seed_rel',
    the share of a finding that is the loss's own conditioning.  Weights, Adam state and iteration count are untouched."""
    if not callable(loss):
        raise ValueError('probe_batch_custom needs a callable loss, got %r' % (loss,))
    b = _Batch(model, data, loss, impulses)
    return model.engine.train_gradient_probe_custom(loss, b.states, b.attrs, b.nums, b.dens, states_delta=b.sd, actions=b.actions,
                                                    context=data)


def probe_batch_sinkhorn(model, data, impulses='data', transport_eps_scale=TRANSPORT_EPS_SCALE, transport_iters=TRANSPORT_ITERS,
                         sinkhorn_reach_scale=None, sinkhorn_mass='unit'):
    """Engine.train_gradient_probe with the Sinkhorn divergence on a collate_untracked batch: train_step_divergence(mode='grad')
    against Engine.train_grad_f64_divergence on the same batch, eps and sweeps as run_batch(loss='sinkhorn') takes them; the
    result has 'loss_kind': 'sinkhorn' and the float64 side's largest 'col_err' and 'self_err'.  Weights, Adam state and
    iteration count are untouched.  It works on depth_only batches with impulses='actions'.  probe_batch itself still refuses
    the loss: its refusal is pinned by tests/test_divergence_host.py and tests/test_gpu_train_divergence.py, and folding this
    call into probe_batch / probe_every waits for a change of those tests.  sinkhorn_reach_scale (not None) and sinkhorn_mass:
    the unbalanced divergence as run_batch takes it -- the reaches of sinkhorn_reach and the targets' masses of sinkhorn_mass_q
    -- against Engine.train_grad_f64_divergence(reach=, mass_q=); the result then also has 'reach': True, 'transported' and
    'transported_diff'."""
    spec = _LossSpec(DIVERGENCE_LOSSES[0], 0.5, transport_eps_scale, transport_iters, sinkhorn_reach_scale, sinkhorn_mass)
    b = _Batch(model, data, spec.loss, impulses)
    return b.probe(model, b.sd, targets=b.targets, target_nums=b.tnums, eps=spec.eps(b), iters=int(spec.iters), **spec.reach_args(b))


def probe_batch_match(model, data, impulses='data', loss='match', match_weight=0.5):
    """Engine.train_gradient_probe with a matching loss (a member of MATCH_LOSSES; match_weight: the mix's) on a
    collate_untracked batch: train_step_loss(mode='grad') against Engine.train_grad_f64_match on the fp32 side's own partners, so
    that 'rel' is arithmetic error on the same pairs; the result also has 'loss_kind', 'flipped', 'rows_flipped', 'cost_gap' --
    what the fp32 tape's drift did to the assignment -- and, only where a partner flipped, 'rel_own'.  Weights, Adam state and
    iteration count are untouched.  It works on depth_only batches with impulses='actions'.  probe_batch itself still refuses
    these losses: its refusal is pinned by tests/test_match_host.py and tests/test_gpu_train_match.py."""
    if loss not in MATCH_LOSSES:
        raise ValueError('probe_batch_match needs a loss of %s, got %r' % (MATCH_LOSSES, loss))
    check_loss(loss, match_weight)
    b = _Batch(model, data, loss, impulses)
    return b.probe(model, b.sd, targets=b.targets, target_nums=b.tnums, loss=loss, match_weight=float(match_weight))


# The six probe schedules of train() / main(), in the order their checks run.  option: the schedule's name; losses: the losses it
# probes (None: a callable loss); needs_reach: only beside sinkhorn_reach_scale; companions: the schedules its "give ... alone"
# refusal names, in the message's order; probe(model, data, impulses, spec) -> the probe's dict; suffix(pr, loss): what the
# schedule adds to the log line.  The two oldest rows are checked as a pair by check_probe_options, which has their own refusals.
_Schedule = collections.namedtuple('_Schedule', 'option losses needs_reach companions probe suffix')
_OLDER = ('grad_probe_every', 'probe_every')


def _probe_older(model, data, impulses, spec):
    return probe_batch(model, data, impulses, spec.loss)


def _probe_sinkhorn(model, data, impulses, spec):
    return probe_batch_sinkhorn(model, data, impulses, spec.eps_scale, spec.iters, spec.reach_scale, spec.mass)


def _suffix_older(pr, loss):
    return ', min_margin %.3e' % pr['min_margin'] if loss == 'chamfer' else ''


def _suffix_sinkhorn(pr, loss):
    return ', col_err %.3e, self_err %.3e' % (pr['col_err'], pr['self_err'])


SCHEDULES = collections.OrderedDict((row.option, row) for row in (
    _Schedule('custom_probe_every', None, False, _OLDER + ('sinkhorn_probe_every', 'match_probe_every', 'sinkhorn_reach_probe_every'),
              lambda model, data, impulses, spec: probe_batch_custom(model, data, spec.loss, impulses),
              lambda pr, loss: ', seed_rel %.3e' % pr['seed_rel']),
    _Schedule('grad_probe_every', ('mse',), False, (), _probe_older, _suffix_older),
    _Schedule('probe_every', LOSSES, False, (), _probe_older, _suffix_older),
    _Schedule('sinkhorn_probe_every', DIVERGENCE_LOSSES, False, _OLDER, _probe_sinkhorn, _suffix_sinkhorn),
    _Schedule('match_probe_every', MATCH_LOSSES, False, _OLDER + ('sinkhorn_probe_every',),
              lambda model, data, impulses, spec: probe_batch_match(model, data, impulses, spec.loss, spec.match_weight),
              lambda pr, loss: ', flipped %d, cost_gap %.3e' % (pr['flipped'], pr['cost_gap'])
              + (', rel_own %.3e' % pr['rel_own'] if 'rel_own' in pr else '')),
    _Schedule('sinkhorn_reach_probe_every', DIVERGENCE_LOSSES, True, _OLDER + ('sinkhorn_probe_every', 'match_probe_every'),
              _probe_sinkhorn, lambda pr, loss: _suffix_sinkhorn(pr, loss) + ', transported %.4f, transported_diff %.3e'
              % (pr['transported'], pr['transported_diff']))))


def check_match_probe_option(loss, match_probe_every, grad_probe_every=0, probe_every=0, sinkhorn_probe_every=0):
    """match_probe_every of train() / main(): the probe schedule of MATCH_LOSSES alone, and no companion of the three other
    schedules (check_probe_options has refused the two older ones for these losses already)"""
    _check_schedule(SCHEDULES['match_probe_every'], loss,
                    {'match_probe_every': match_probe_every, 'grad_probe_every': grad_probe_every, 'probe_every': probe_every,
                     'sinkhorn_probe_every': sinkhorn_probe_every})


def check_sinkhorn_probe_option(loss, sinkhorn_probe_every, grad_probe_every=0, probe_every=0):
    """sinkhorn_probe_every of train() / main(): the probe schedule of DIVERGENCE_LOSSES alone, and no companion of the two older
    schedules (check_probe_options has refused those for this loss already)"""
    _check_schedule(SCHEDULES['sinkhorn_probe_every'], loss,
                    {'sinkhorn_probe_every': sinkhorn_probe_every, 'grad_probe_every': grad_probe_every, 'probe_every': probe_every})


def check_sinkhorn_reach_probe_option(loss, sinkhorn_reach_probe_every, sinkhorn_reach_scale=None, grad_probe_every=0, probe_every=0,
                                      sinkhorn_probe_every=0, match_probe_every=0):
    """sinkhorn_reach_probe_every of train() / main(): the probe schedule of DIVERGENCE_LOSSES with a reach alone, and no
    companion of the four other schedules (sinkhorn_probe_every keeps refusing a reach: tests/test_divergence_unbalanced_host.py
    pins that)"""
    _check_schedule(SCHEDULES['sinkhorn_reach_probe_every'], loss,
                    {'sinkhorn_reach_probe_every': sinkhorn_reach_probe_every, 'grad_probe_every': grad_probe_every,
                     'probe_every': probe_every, 'sinkhorn_probe_every': sinkhorn_probe_every, 'match_probe_every': match_probe_every},
                    sinkhorn_reach_scale)


def check_probe_options(loss, grad_probe_every, probe_every):
    """the two probe schedules of train() / main(): grad_probe_every (the MSE yardstick alone) and probe_every (every loss of
    LOSSES; the matching losses have no float64 yardstick yet and refuse both)"""
    check_loss(loss)
    for option, every in (('grad_probe_every', grad_probe_every), ('probe_every', probe_every)):
        if every > 0:
            refuse_custom_probe(loss, option)
    if grad_probe_every > 0 or probe_every > 0:
        refuse_match_probe(loss)
    if grad_probe_every > 0 and probe_every > 0:
        raise ValueError('give grad_probe_every or probe_every, not both')
    if loss == 'chamfer' and grad_probe_every > 0:
        raise ValueError('grad_probe_every needs loss=\'mse\': the float64 yardstick of the gradients it pairs with is MSE-only; '
                         'probe_every probes every loss')


def check_optim_options(accum_steps=1, clip_norm=None):
    """accum_steps and clip_norm of train() / main(): an integer number of batches >= 1 per optimiser step, and None or a positive
    global-norm bound (inf: measured and logged, never clipped)"""
    if isinstance(accum_steps, bool) or int(accum_steps) != accum_steps or accum_steps < 1:
        raise ValueError('accum_steps must be an integer >= 1, got %r' % (accum_steps,))
    if clip_norm is not None and not float(clip_norm) > 0.0:
        raise ValueError('clip_norm must be a number > 0 (or None: no clipping), got %r' % (clip_norm,))


def check_train_options(loss, every, match_weight=0.5, transport_eps_scale=TRANSPORT_EPS_SCALE, transport_iters=TRANSPORT_ITERS,
                        sinkhorn_reach_scale=None, sinkhorn_mass='unit', usage_only=False, accum_steps=1, clip_norm=None):
    """Every option check of train() / main(), in the one order that decides which refusal a caller sees when two apply; every:
    {option: value} over SCHEDULES -> the run's _LossSpec.  usage_only: the command line's part -- what _cli() turns into a
    usage error before anything is read or written: the loss's own options, then the reach schedule.  accum_steps and clip_norm
    (check_optim_options) come last: every older refusal is seen as before."""
    def reach_probe():
        _check_schedule(SCHEDULES['sinkhorn_reach_probe_every'], loss, every, sinkhorn_reach_scale)
    if not usage_only:
        check_custom_probe_option(loss, every['custom_probe_every'], *(every[o] for o in SCHEDULES['custom_probe_every'].companions))
        check_probe_options(loss, every['grad_probe_every'], every['probe_every'])
        _check_schedule(SCHEDULES['sinkhorn_probe_every'], loss, every)
        _check_schedule(SCHEDULES['match_probe_every'], loss, every)
        reach_probe()
    spec = _LossSpec(loss, match_weight, transport_eps_scale, transport_iters, sinkhorn_reach_scale, sinkhorn_mass,
                     every['sinkhorn_probe_every'])
    if usage_only:
        reach_probe()
    check_optim_options(accum_steps, clip_norm)
    return spec


def train(config, model, dataloaders, n_epoch=None, log=None, on_best=None, ckp=None, first_epoch=0, grad_probe_every=0,
          loss='mse', impulses='data', probe_every=0, match_weight=0.5, transport_eps_scale=TRANSPORT_EPS_SCALE,
          transport_iters=TRANSPORT_ITERS, sinkhorn_probe_every=0, match_probe_every=0, sinkhorn_reach_scale=None,
          sinkhorn_mass='unit', sinkhorn_reach_probe_every=0, custom_probe_every=0, accum_steps=1, clip_norm=None,
          optimizer_state=None, on_optimizer=None):
    """train/train_gnn_dyn.py:134-246 without the file I/O: `dataloaders` = {'train': iterable of
    collated batches, 'valid': ...}.  Returns {'best_valid_loss', 'history': [(epoch, phase, rmse)]}.
    ckp(epoch, i, model): called after training batch i when i % ckp_per_iter == 0 (:217-218); first_epoch: the epoch
    a resumed run starts from (:136).  grad_probe_every = k > 0: every k-th training batch (i % k == 0) is probed before its
    update (probe_batch); the worst tensor's rel goes to the history as (epoch, 'grad_probe', rel) and to the log.
    loss='chamfer': the batches are collate_untracked's and every step's term is the Chamfer distance to its target cloud; the
    option grad_probe_every pairs with the MSE yardstick alone, so grad_probe_every > 0 is refused with it.  probe_every = k > 0:
    grad_probe_every's schedule and history entry for every loss and impulse source (probe_batch with the run's loss; with
    loss='chamfer' the log line also carries min_margin, the float64 side's smallest arg-min margin); giving both is refused.
    impulses='actions': the batches
    carry `.actions` and the model is trained through the push (run_batch); with real untracked data this is what makes
    n_rollout > 1 meaningful.  The engine's camera must be set (main does it).  loss in MATCH_LOSSES: run_batch's matching loss
    with match_weight; both probe options are refused with it.  loss in TRANSPORT_LOSSES: run_batch's transport loss with
    transport_eps_scale and transport_iters; the probe options are refused with it too.  loss in DIVERGENCE_LOSSES: the same
    with run_batch's Sinkhorn divergence.  sinkhorn_probe_every = k > 0: probe_every's schedule and history entry for a loss in
    DIVERGENCE_LOSSES (probe_batch_sinkhorn with the run's transport_eps_scale and transport_iters); the log line also carries
    col_err and self_err, the float64 side's largest certificates.  It is refused with any other loss and together with either
    older probe option, which keep refusing this loss: folding it into probe_every waits for a change of the tests that pin
    those refusals.  match_probe_every = k > 0: the same for a loss in MATCH_LOSSES (probe_batch_match with the run's
    match_weight); the log line also carries flipped and cost_gap -- the problems whose float64 optimum differs from the fp32
    side's partners, and how far from optimal in double those are -- and, where a partner flipped, rel_own.
    sinkhorn_reach_scale, sinkhorn_mass: run_batch's unbalanced divergence (check_sinkhorn_options: a loss in DIVERGENCE_LOSSES
    alone, 'count' only with a reach, no sinkhorn_probe_every beside a reach); the training log line then carries the batch's
    mean transported.  sinkhorn_reach_probe_every = k > 0: probe_every's schedule and history entry for a loss in
    DIVERGENCE_LOSSES with a reach (probe_batch_sinkhorn with the run's sinkhorn_reach_scale and sinkhorn_mass); the log line
    carries col_err, self_err, the float64 side's smallest transported and transported_diff.  It is refused without a reach,
    with any other loss and beside any of the four other probe options (check_sinkhorn_reach_probe_option).  A CALLABLE loss:
    run_batch's loss of the caller's, every batch its own context; the five probe options above refuse it, naming it.
    custom_probe_every = k > 0: probe_every's schedule and history entry for a callable loss (probe_batch_custom); the log line
    also carries seed_rel.  It is refused with a string loss and beside any other probe option (check_custom_probe_option).
    accum_steps = k, clip_norm = c (check_optim_options): with the defaults (1, None) the loop is the one above, call for call.
    Otherwise every training batch runs with mode='grad' on whichever call the run's loss uses (a callable loss included) and its
    gradient is accumulated on the device with weight B, its sample count (Engine.train_accumulate); after every k batches, and
    at the end of the phase for a remainder, one Adam step is taken on the sum times 1 / (the group's samples), clipped to the
    global norm c as torch's clip_grad_norm_ does (Engine.train_apply) -- the gradient of the mean loss over the group's
    samples.  clip_norm with accum_steps=1 is the same path with groups of one.  The log line of a batch that ends a group
    gets ', GradNorm %.6f, Clip %.4f' appended (a remainder group, applied behind the phase's last batch, logs a line of its
    own); an update skipped because its norm was not finite is logged once and counted in the result's 'skipped_updates' (a
    key the result has on this path only).  The probe schedules run as they do: they probe a batch before its pass.  ckp fires
    on its schedule even mid-group and then saves the weights as they stood before the open group.  The valid phase and the
    history's format are untouched.  optimizer_state: a DeviceAdam.state_dict() loaded before the first batch (a resumed run);
    on_optimizer(epoch, i, optimizer): called right behind every ckp call (main's --save-optimizer)."""
    every = {'grad_probe_every': grad_probe_every, 'probe_every': probe_every, 'sinkhorn_probe_every': sinkhorn_probe_every,
             'match_probe_every': match_probe_every, 'sinkhorn_reach_probe_every': sinkhorn_reach_probe_every,
             'custom_probe_every': custom_probe_every}
    spec = check_train_options(loss, every, match_weight, transport_eps_scale, transport_iters, sinkhorn_reach_scale, sinkhorn_mass,
                               accum_steps=accum_steps, clip_norm=clip_norm)
    if impulses not in IMPULSES:
        raise ValueError('impulses must be one of %s, got %r' % (IMPULSES, impulses))
    loss_kind = loss
    schedule = next((row for row in SCHEDULES.values() if every[row.option] > 0), None)         # (at most one of them is given)
    tc = config['train']
    n_rollout = tc['n_rollout']
    assert tc['n_history'] == 1
    optimizer = DeviceAdam(model, float(tc['lr']), betas=(tc['adam_beta1'], 0.999), n_rollout=n_rollout)
    if optimizer_state is not None:
        optimizer.load_state_dict(optimizer_state)
    grouped = int(accum_steps) > 1 or clip_norm is not None
    skipped = [0]

    def apply_group(n_samples, where):
        """one optimiser step on the open group's accumulated gradient -> the log line's suffix"""
        out = model.engine.train_apply(scale=1.0 / n_samples, max_norm=clip_norm)
        if hasattr(model, '_claim'):
            model._device_ahead = model._device_ahead or out['applied']
        if not out['applied']:
            skipped[0] += 1
            if log is not None:
                log('train %s update skipped: GradNorm %r is not finite, nothing moved' % (where, out['norm']))
        return ', GradNorm %.6f, Clip %.4f' % (out['norm'], out['clip'])

    best_valid_loss = np.inf
    history = []
    for epoch in range(int(first_epoch), n_epoch if n_epoch is not None else tc['n_epoch']):
        for phase in ('train', 'valid'):
            model.train(phase == 'train')
            meter = AverageMeter()
            group_batches, group_samples = 0, 0
            for i, data in enumerate(dataloaders[phase]):
                if schedule is not None and phase == 'train' and i % every[schedule.option] == 0:
                    pr = schedule.probe(model, data, impulses, spec)
                    history.append((epoch, 'grad_probe', float(pr['rel'])))
                    if log is not None:
                        log('grad_probe [%d][%d] worst %s rel %.3e (%s tape), loss diff %.3e'
                            % (epoch, i, pr['worst'], pr['rel'], pr['tape'], pr['loss_diff']) + schedule.suffix(pr, loss_kind))
                logged = log is not None and i % tc['log_per_iter'] == 0
                stats = {} if logged and sinkhorn_reach_scale is not None else None
                in_group = grouped and phase == 'train'
                loss = run_batch(model, optimizer, data, phase, n_rollout, loss=loss_kind, impulses=impulses, match_weight=match_weight,
                                 transport_eps_scale=transport_eps_scale, transport_iters=transport_iters,
                                 sinkhorn_reach_scale=sinkhorn_reach_scale, sinkhorn_mass=sinkhorn_mass, stats=stats,
                                 **({'mode': 'grad'} if in_group else {}))
                meter.update(loss, _np(data[0]).shape[0])
                applied = ''
                if in_group:
                    model.engine.train_accumulate(_np(data[0]).shape[0])
                    group_batches, group_samples = group_batches + 1, group_samples + _np(data[0]).shape[0]
                    if group_batches == int(accum_steps):
                        applied = apply_group(group_samples, '[%d][%d]' % (epoch, i))
                        group_batches, group_samples = 0, 0
                if logged:
                    log('%s [%d][%d] LR: %.6f, Loss: %.6f (%.6f)' % (phase, epoch, i, optimizer.param_groups[0]['lr'],
                                                                      np.sqrt(loss), np.sqrt(meter.avg))
                        + (', transported %.4f' % stats['transported'] if stats is not None else '') + applied)
                if ckp is not None and phase == 'train' and i % tc['ckp_per_iter'] == 0:
                    ckp(epoch, i, model)
                    if on_optimizer is not None:
                        on_optimizer(epoch, i, optimizer)
            if group_batches:                   # the phase's remainder: fewer than accum_steps batches, applied now
                applied = apply_group(group_samples, '[%d] (the last %d batches)' % (epoch, group_batches))
                if log is not None:
                    log('train [%d] the last %d batches applied%s' % (epoch, group_batches, applied))
            history.append((epoch, phase, float(np.sqrt(meter.avg))))
            if phase == 'valid' and meter.avg < best_valid_loss:
                best_valid_loss = meter.avg
                if on_best is not None:
                    on_best(model.state_dict())           # torch.save(model.state_dict(), net_best.pth), :244
    result = {'best_valid_loss': float(best_valid_loss), 'history': history}
    if grouped:
        result['skipped_updates'] = skipped[0]
    return result


def default_config():
    """config/train/gnn_dyn.yaml, the keys main() reads"""
    return {
        'dataset': {'global_scale': 24, 'n_episode': 2000, 'n_timestep': 10},
        'train': {'data_root': 'data/gnn_dyn_data', 'random_seed': 42, 'n_epoch': 2000, 'lr': 0.001, 'adam_beta1': 0.9,
                  'batch_size': 4, 'nf_hidden': 64, 'num_workers': 5, 'train_valid_ratio': 0.9, 'log_per_iter': 50,
                  'ckp_per_iter': 1000, 'n_history': 1, 'n_rollout': 5,
                  'particle': {'nf_effect': 64, 'resume': {'active': False, 'epoch': 0, 'iter': 0, 'folder': 'None'},
                               'adj_thresh': 0.08, 'add_delta': False}},
    }


def set_seed(seed):
    """utils.py:195-201"""
    import random
    import torch
    torch.manual_seed(seed)
    np.random.seed(seed)
    random.seed(seed)


def main(config, data_root=None, train_dir=None, cam=None, chunk=None, threads=8, n_epoch=None, engine=None, grad_probe_every=0,
         loss=None, impulses=None, probe_every=0, data='particles', target_den_scale=1.0, match_weight=0.5,
         transport_eps_scale=TRANSPORT_EPS_SCALE, transport_iters=TRANSPORT_ITERS, sinkhorn_probe_every=0, match_probe_every=0,
         sinkhorn_reach_scale=None, sinkhorn_mass='unit', sinkhorn_reach_probe_every=0, custom_probe_every=0, accum_steps=1,
         clip_norm=None, save_optimizer=False):
    """The file-level part of train/train_gnn_dyn.py:train() (:45-130, :196-228): seed, the log directory with config.yaml
    and log.txt, the 'train' / 'valid' ParticleDatasets and their DeviceLoaders, a fresh model (torch.nn.Linear's default
    initialisation) or the resumed checkpoint, net_epoch_%d_iter_%d.pth every ckp_per_iter training batches and
    net_best.pth, all in the state_dict layout PropNetDiffDenModel.load_state_dict reads.  cam = (cam_params,
    cam_extrinsic), by default the demo camera (synthetic.py; FleX is not available).  Returns train()'s result and
    the directory.  loss='chamfer': the recorded episodes' correspondence is dropped (dataset_gnn_dyn.drop_correspondence on
    every sample, seeded by train.random_seed) and the model is trained on the Chamfer distance to the untracked clouds.
    impulses='actions': the engine's camera is set from the dataset's extrinsics and global_scale and every step's impulse comes
    from the recorded push on the state the step reads (train).  probe_every, sinkhorn_probe_every, match_probe_every: train's.
    data='depth': the episodes need only their depth PNGs and actions.p (a recorded robot episode): the datasets are
    DepthDatasets (every frame of a window sampled from its depth image on the device, the later frames at target_den_scale
    times the state's density), which implies loss='chamfer' and impulses='actions'; a contradicting value is refused.  loss /
    impulses None: 'mse' / 'data', or what data implies.  loss in MATCH_LOSSES (with match_weight for the mix): as 'chamfer', on
    particles or depth; loss in TRANSPORT_LOSSES or DIVERGENCE_LOSSES (with transport_eps_scale and transport_iters) likewise.  chunk None: the
    dataset's default (64 samples; 16 for data='depth').  sinkhorn_reach_scale, sinkhorn_mass, sinkhorn_reach_probe_every: train's.
    A callable loss and custom_probe_every: train's (tracked batches, or with data='depth' the depth batches through the push).
    accum_steps, clip_norm: train's.  save_optimizer: every net_epoch_%d_iter_%d.pth gets an opt_epoch_%d_iter_%d.npz beside it
    (DeviceAdam.state_dict(): m, v, iter); off by default, so the files a run writes are what they were.  A resumed run loads the
    .npz of its checkpoint when it is there (whatever save_optimizer says) and then continues with Adam's moments and step count
    instead of zeros."""
    import time
    import yaml
    from . import synthetic, weights
    from .dataset_gnn_dyn import DepthDataset, DeviceLoader, ParticleDataset, UntrackedLoader
    from .gnn_dyn import PropNetDiffDenModel
    loss, impulses = resolve_data_options(data, loss, impulses)
    every = {'grad_probe_every': grad_probe_every, 'probe_every': probe_every, 'sinkhorn_probe_every': sinkhorn_probe_every,
             'match_probe_every': match_probe_every, 'sinkhorn_reach_probe_every': sinkhorn_reach_probe_every,
             'custom_probe_every': custom_probe_every}
    check_train_options(loss, every, match_weight, transport_eps_scale, transport_iters, sinkhorn_reach_scale, sinkhorn_mass,
                        accum_steps=accum_steps, clip_norm=clip_norm)
    tc = config['train']
    resume = tc['particle'].get('resume', {'active': False, 'epoch': 0, 'iter': 0})
    if cam is None:
        cam = (synthetic.demo_cam_params(), synthetic.demo_cam_extrinsics())
    set_seed(tc['random_seed'])
    if train_dir is None:
        root = 'data/gnn_dyn_model'
        train_dir = os.path.join(root, resume['folder'] if resume['active'] else time.strftime('%Y-%m-%d-%H-%M-%S'))
    os.makedirs(train_dir, exist_ok=True)
    with open(os.path.join(train_dir, 'config.yaml'), 'w') as f:
        yaml.safe_dump(config, f)
    log_name = 'log.txt' if not resume['active'] else 'log_resume_epoch_%d_iter_%d.txt' % (resume['epoch'], resume['iter'])
    data_root = data_root if data_root is not None else tc['data_root']
    if data == 'depth':
        datasets = {ph: DepthDataset(data_root, config, ph, cam, engine=engine, target_den_scale=target_den_scale)
                    for ph in ('train', 'valid')}
    else:
        datasets = {ph: ParticleDataset(data_root, config, ph, cam, engine=engine) for ph in ('train', 'valid')}
    loaders = {ph: DeviceLoader(datasets[ph], tc['batch_size'], shuffle=(ph == 'train'), chunk=chunk, threads=threads)
               for ph in ('train', 'valid')}
    if loss in UNTRACKED_LOSSES + DIVERGENCE_LOSSES and data != 'depth':
        loaders = {ph: UntrackedLoader(loaders[ph], seed=tc['random_seed'] + k, reseed=(ph == 'valid'))
                   for k, ph in enumerate(('train', 'valid'))}
    model = PropNetDiffDenModel(config, engine=engine)
    optimizer_state = None
    if impulses == 'actions':
        from .planners import world2cam_affine
        gs = float(config['dataset']['global_scale'])
        model.engine.set_camera(world2cam_affine(np.asarray(cam[1], dtype=np.float64)), gs, cam[0])
    if resume['active']:
        path = os.path.join(train_dir, 'net_epoch_%d_iter_%d.pth' % (resume['epoch'], resume['iter']))
        model.load_state_dict(weights.state_dict_from_blob(weights.load_checkpoint(path)))
        opt_path = os.path.join(train_dir, 'opt_epoch_%d_iter_%d.npz' % (resume['epoch'], resume['iter']))
        if os.path.exists(opt_path):
            with np.load(opt_path) as z:
                optimizer_state = {'m': z['m'], 'v': z['v'], 'iter': int(z['iter'])}
    else:
        model.load_state_dict(weights.random_state_dict(seed=tc['random_seed'], predictor_scale=1.0))
    with open(os.path.join(train_dir, log_name), 'w') as log_fout:
        def log(line):
            print(line)
            log_fout.write(line + '\n')
            log_fout.flush()

        def ckp(epoch, i, m):
            weights.save_checkpoint(m.state_dict(), os.path.join(train_dir, 'net_epoch_%d_iter_%d.pth' % (epoch, i)))

        def on_best(sd):
            weights.save_checkpoint(sd, os.path.join(train_dir, 'net_best.pth'))

        def on_optimizer(epoch, i, optimizer):
            np.savez(os.path.join(train_dir, 'opt_epoch_%d_iter_%d.npz' % (epoch, i)), **optimizer.state_dict())

        if optimizer_state is not None:
            log('resumed Adam\'s state after %d steps (opt_epoch_%d_iter_%d.npz)' % (optimizer_state['iter'], resume['epoch'], resume['iter']))

        result = train(config, model, loaders, n_epoch=n_epoch, log=log, on_best=on_best, ckp=ckp,
                       first_epoch=resume['epoch'] if resume['active'] and resume['epoch'] > 0 else 0,
                       loss=loss, impulses=impulses, match_weight=match_weight, transport_eps_scale=transport_eps_scale,
                       transport_iters=transport_iters, sinkhorn_reach_scale=sinkhorn_reach_scale, sinkhorn_mass=sinkhorn_mass,
                       accum_steps=accum_steps, clip_norm=clip_norm, optimizer_state=optimizer_state,
                       on_optimizer=on_optimizer if save_optimizer else None, **every)
        for epoch, phase, rmse in result['history']:
            if phase == 'grad_probe':                   # logged when it was taken
                continue
            log('%s [%d] Loss: %.6f' % (phase, epoch, rmse))
    return result, train_dir


def load_loss_fn(spec):
    """--loss-fn's 'package.module:attribute' -> the callable it names (importlib); anything else is refused"""
    import importlib
    module, sep, attribute = str(spec).partition(':')
    if not sep or not module or not attribute:
        raise ValueError('loss_fn must be given as package.module:attribute, got %r' % (spec,))
    fn = importlib.import_module(module)
    for part in attribute.split('.'):
        fn = getattr(fn, part)
    if not callable(fn):
        raise ValueError('loss_fn %r is not callable (%r)' % (spec, type(fn).__name__))
    return fn


def _cli(argv=None):
    import argparse
    import yaml
    ap = argparse.ArgumentParser(description='Train the particle dynamics model on recorded episodes (device data path '
                                             'and device trainer).')
    ap.add_argument('--config', help='config/train/gnn_dyn.yaml-style file (default: the reference\'s values)')
    ap.add_argument('--data-root', help='episode directory (default: train.data_root)')
    ap.add_argument('--train-dir', help='output directory (default: data/gnn_dyn_model/<time>)')
    ap.add_argument('--n-episode', type=int, help='override dataset.n_episode')
    ap.add_argument('--n-timestep', type=int, help='override dataset.n_timestep')
    ap.add_argument('--epochs', type=int, help='override train.n_epoch')
    ap.add_argument('--chunk', type=int, default=None, help='samples per device call (default 64; 16 with --data depth)')
    ap.add_argument('--threads', type=int, default=8, help='decoding threads (at most 16)')
    ap.add_argument('--grad-probe-every', type=int, default=0,
                    help='hold every k-th training batch\'s gradients against float64 before its update (0: never)')
    ap.add_argument('--probe-every', type=int, default=0,
                    help='the same for every --loss and --impulses; with --loss chamfer the log line carries the float64 side\'s '
                         'smallest arg-min margin')
    ap.add_argument('--sinkhorn-probe-every', type=int, default=0,
                    help='--loss sinkhorn: hold every k-th training batch\'s gradients against the float64 Sinkhorn divergence before '
                         'its update; the log line carries the float64 side\'s largest col_err and self_err (not with the two options above)')
    ap.add_argument('--match-probe-every', type=int, default=0,
                    help='--loss match, chamfer+match: hold every k-th training batch\'s gradients against the float64 matching loss on '
                         'the same pairs before its update; the log line carries the problems whose float64 optimum differs (flipped) '
                         'and the fp32 matching\'s distance from it (cost_gap) (not with the three options above)')
    ap.add_argument('--sinkhorn-reach-probe-every', type=int, default=0,
                    help='--loss sinkhorn --sinkhorn-reach-scale r: hold every k-th training batch\'s gradients against the float64 '
                         'unbalanced divergence before its update; the log line also carries the float64 side\'s smallest transported '
                         'share and its largest difference from the fp32 side\'s (not with the four options above)')
    ap.add_argument('--data', choices=DATA, default='particles',
                    help='depth: episodes of depth PNGs and actions.p alone; every frame of a window is sampled from its depth '
                         'image on the device.  Implies --loss chamfer --impulses actions')
    ap.add_argument('--target-den-scale', type=float, default=1.0,
                    help='--data depth: the target frames are sampled at this multiple of the state\'s particle density')
    ap.add_argument('--loss', choices=LOSSES + MATCH_LOSSES + TRANSPORT_LOSSES + DIVERGENCE_LOSSES, default=None,
                    help='(default mse) chamfer: drop the recorded correspondence and train on the Chamfer distance to the untracked '
                         'clouds; match: on the one-to-one matching distance to them; chamfer+match: on their mix (--match-weight); '
                         'transport: on the entropy-regularised transport distance to them (--transport-eps-scale, --transport-iters); '
                         'sinkhorn: on the Sinkhorn divergence to them, the transport distance without its pull inward (the same two '
                         'options): the one for depth data')
    ap.add_argument('--loss-fn', default=None, metavar='package.module:attribute',
                    help='train on a loss of your own instead of --loss: a function loss(pred, context) -> (value, gradient) as in '
                         'dyn_res_pile_manip_amd.losses (e.g. dyn_res_pile_manip_amd.losses:pseudo_huber_loss); context is the batch')
    ap.add_argument('--custom-probe-every', type=int, default=0,
                    help='--loss-fn: hold every k-th training batch\'s gradients against the float64 evaluation of the same loss before '
                         'its update; the log line carries seed_rel, the loss\'s own sensitivity to the fp32 prediction (not with the '
                         'five options above)')
    ap.add_argument('--match-weight', type=float, default=0.5,
                    help='--loss chamfer+match: (1 - w) Chamfer + w matching, w in (0, 1)')
    ap.add_argument('--transport-eps-scale', type=float, default=TRANSPORT_EPS_SCALE,
                    help='--loss transport, sinkhorn: eps = scale / particle density per sample (1: the plan blurs over one particle spacing)')
    ap.add_argument('--transport-iters', type=int, default=TRANSPORT_ITERS,
                    help='--loss transport, sinkhorn: Sinkhorn sweeps per problem, 1..%d' % TRANSPORT_MAX_ITERS)
    ap.add_argument('--sinkhorn-reach-scale', type=float, default=None,
                    help='--loss sinkhorn: the unbalanced divergence for a pile seen partly, reach = scale / particle density per sample '
                         '(the unit of --transport-eps-scale: 4 is a reach of two particle spacings); mass further than that from the '
                         'other cloud is given up, not moved (default: balanced)')
    ap.add_argument('--sinkhorn-mass', choices=SINKHORN_MASSES, default='unit',
                    help='--sinkhorn-reach-scale: the target cloud\'s total mass against the prediction\'s 1 -- unit: 1; count: its '
                         'point count over the prediction\'s, equal mass per point (targets sampled at the particles\' spacing)')
    ap.add_argument('--accum-steps', type=int, default=1, metavar='k',
                    help='one optimiser step per k training batches, on the gradient of the mean loss over their samples (accumulated '
                         'in float64 on the device); a remainder is applied at the end of the phase')
    ap.add_argument('--clip-norm', type=float, default=None, metavar='c',
                    help='clip every update\'s gradient to the global 2-norm c (torch\'s clip_grad_norm_); the log carries GradNorm and Clip')
    ap.add_argument('--save-optimizer', action='store_true',
                    help='write opt_epoch_E_iter_I.npz (Adam\'s m, v, iter) beside every net_epoch_E_iter_I.pth; a resumed run loads it when it is there')
    ap.add_argument('--impulses', choices=IMPULSES, default=None,
                    help='(default data) actions: compute every step\'s impulse from the recorded push on the state the model predicted')
    a = ap.parse_args(argv)
    if a.loss is not None and a.loss_fn is not None:
        ap.error('give --loss or --loss-fn, not both')
    try:
        if a.loss_fn is not None:
            a.loss = load_loss_fn(a.loss_fn)
        every = {option: getattr(a, option) for option in SCHEDULES}
        # (the callable's schedule on the loss as given; the rest on what --data makes of it)
        check_custom_probe_option(a.loss, a.custom_probe_every, *(every[o] for o in SCHEDULES['custom_probe_every'].companions))
        check_train_options(resolve_data_options(a.data, a.loss, a.impulses)[0], every, a.match_weight, a.transport_eps_scale,
                            a.transport_iters, a.sinkhorn_reach_scale, a.sinkhorn_mass, usage_only=True, accum_steps=a.accum_steps,
                            clip_norm=a.clip_norm)
    except ValueError as e:
        ap.error(str(e))
    config = default_config()
    if a.config:
        with open(a.config) as f:
            config = yaml.safe_load(f)
    if a.n_episode is not None:
        config['dataset']['n_episode'] = a.n_episode
    if a.n_timestep is not None:
        config['dataset']['n_timestep'] = a.n_timestep
    result, d = main(config, a.data_root, a.train_dir, chunk=a.chunk, threads=a.threads, n_epoch=a.epochs,
                     loss=a.loss, impulses=a.impulses, data=a.data, target_den_scale=a.target_den_scale, match_weight=a.match_weight,
                     transport_eps_scale=a.transport_eps_scale, transport_iters=a.transport_iters,
                     sinkhorn_reach_scale=a.sinkhorn_reach_scale, sinkhorn_mass=a.sinkhorn_mass, accum_steps=a.accum_steps,
                     clip_norm=a.clip_norm, save_optimizer=a.save_optimizer, **every)
    print('best valid loss %.6f, checkpoints in %s' % (np.sqrt(result['best_valid_loss']), d))


if __name__ == '__main__':
    _cli()

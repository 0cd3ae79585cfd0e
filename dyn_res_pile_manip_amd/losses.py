"""Losses for Engine.train_step_custom: Python functions in the place of the trainer's built-in loss kernels.

  loss_fn(pred, context) -> (value, grad)

pred [B, n_rollout, N, 3] is every step's predicted state (Engine.train_predict, or train_predict_f64: a loss_fn works on float32
and float64 arrays alike and answers in pred's dtype); value is a number, grad = d value / d pred in pred's shape -- COMPLETE: the
library applies no 1 / (n_rollout B) and no 1 / (3 n_b) behind it.  Rows n >= particle_nums[b] are padding: what pred holds
there is no part of any contract, so a loss must not read them, and its gradient there is ignored (the examples return 0).
context is whatever the caller hands train_step_custom; train_gnn_dyn.run_batch hands the collated batch, so context[0] is
states [B, n_rollout + 1, N, 3], context[3] particle_nums [B] and context[4] particle_dens [B].

  torch_loss(fn)              a loss written in torch -- fn(pred_tensor, context) -> scalar tensor -- through torch.autograd
  mse_loss                    the trainer's own tracked loss (train/train_gnn_dyn.py:184-186), as a worked example
  pseudo_huber_loss           a robust tracked loss: quadratic below one sampling spacing, linear beyond it

The loss runs on the host between two device calls; the model's forward, the reverse pass behind the seed, the weight gradients
and Adam stay on the device."""
import numpy as np


def _np(x, dtype):
    if hasattr(x, 'detach'):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=dtype)


def torch_loss(fn, device='cpu'):
    """fn(pred, context) -> scalar tensor, written in torch, as a loss_fn: pred becomes a leaf tensor of the array's dtype on
    `device`, the value is fn's, the gradient pred.grad after value.backward() (zeros where fn does not depend on pred)."""
    import torch

    def loss_fn(pred, context):
        pred = np.ascontiguousarray(pred)
        leaf = torch.from_numpy(pred.copy()).to(device).requires_grad_(True)
        value = fn(leaf, context)
        if value.dim() != 0:
            raise ValueError('a torch loss must return a scalar tensor, got shape %s' % (tuple(value.shape),))
        value.backward()
        grad = torch.zeros_like(leaf) if leaf.grad is None else leaf.grad
        return float(value.item()), grad.detach().cpu().numpy().astype(pred.dtype, copy=False)
    return loss_fn


def _tracked(pred, context):
    """-> (d = pred - target [B, H, N, 3] with the padded rows zeroed, inv [B, 1, 1, 1] = (1 / (H B)) / (3 n_b) -- the divisor
    3 n_b H B of the reference's MSE with the trainer's own two divisions --, the particle densities [B, 1, 1, 1]), all in pred's
    dtype"""
    pred = np.asarray(pred)
    dt = pred.dtype
    B, H, N, _ = pred.shape
    target = _np(context[0], dt)[:, 1:]
    nums = _np(context[3], np.int64).reshape(B)
    real = (np.arange(N)[None, :] < nums[:, None])[:, None, :, None]                 # [B, 1, N, 1]
    d = np.where(real, pred - target, dt.type(0))
    inv = (dt.type(1) / dt.type(H * B)) / (3 * nums).astype(dt)
    return d, inv.reshape(B, 1, 1, 1), _np(context[4], dt).reshape(B, 1, 1, 1)


def _sum_rows(x):
    """x [B, H, n] float64 -> [B, H]: every (sample, step)'s sum in the order the trainer's MSE kernel takes it (256 strided
    partial sums, a halving tree over each 64 of them, the four results in turn), so that mse_loss on float32 predictions
    returns the bits of the built-in loss; any fixed order would do for a loss of one's own"""
    n = x.shape[-1]
    k = -(-n // 256)
    pad = np.zeros(x.shape[:-1] + (k * 256,), np.float64)
    pad[..., :n] = x
    pad = pad.reshape(x.shape[:-1] + (k, 256))
    acc = np.zeros(x.shape[:-1] + (256,), np.float64)
    for q in range(k):
        acc = acc + pad[..., q, :]
    w = acc.reshape(x.shape[:-1] + (4, 64))
    for off in (32, 16, 8, 4, 2, 1):
        w = w[..., :off] + w[..., off:2 * off]
    w = w[..., 0]
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def _total(terms):
    """terms [B, H] float64 -> their sum step-major, then sample: the trainer's order"""
    total = 0.0
    for v in terms.T.reshape(-1):
        total += float(v)
    return total


def mse_loss(pred, context):
    """sum_t sum_b mse(pred[b, t, :n_b], states[b, t + 1, :n_b]) / (n_rollout B): the built-in tracked loss
    (train/train_gnn_dyn.py:184-186, :203) -> (value, d value / d pred).  On float32 predictions the gradient is formed with the
    built-in kernel's own operations, (2 d) inv, and the value summed in its order: a run trained through this function ends on
    the bits of a run with loss='mse'."""
    d, inv, _ = _tracked(pred, context)
    B, H = d.shape[:2]
    d64 = d.astype(np.float64).reshape(B, H, -1)
    terms = _sum_rows(d64 * d64) * inv.astype(np.float64).reshape(B, 1)
    return _total(terms), (d.dtype.type(2) * d) * inv


def pseudo_huber_loss(pred, context):
    """The MSE's robust relative: per coordinate delta^2 (sqrt(1 + d^2 / delta^2) - 1) in the place of d^2 -- quadratic for
    |d| << delta, linear beyond it, so one badly tracked particle does not dominate the batch -- summed over real rows and
    divided by 3 n_b n_rollout B as the MSE's terms are.  delta_b = 1 / sqrt(particle_dens[b]): one sampling spacing of the
    sample, the definition train_gnn_dyn.TRANSPORT_EPS_SCALE rests on -> (value, d value / d pred)"""
    d, inv, dens = _tracked(pred, context)
    B, H = d.shape[:2]
    delta2 = 1 / dens
    root = np.sqrt(1 + d * d / delta2)
    # delta^2 (root - 1) = d^2 / (root + 1): the same number without the cancellation at small d
    terms = _sum_rows((d * d / (root + 1)).astype(np.float64).reshape(B, H, -1)) * inv.astype(np.float64).reshape(B, 1)
    return _total(terms), d / root * inv

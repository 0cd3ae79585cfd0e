"""Costs for planning on a caller's objective: Python functions in the place of the planners' built-in goal-image reward
(Engine.gd_predict / gd_step_seeded, Engine.mpc_set_rewards, planners.PlannerGD.trajectory_optimization_ptcl_cost).

  cost(pred, context, want_grad) -> (values [B], grad [B, H, N, 3] or None)

pred [B, H, N, 3] is every step's predicted state of every row (Engine.gd_predict, mpc_get's states, or gd_predict_f64: a cost
works on float32 and float64 arrays alike and answers in pred's dtype).  Rows are independent: values[b] reads pred[b] only.
The reward of a row is -values[b]; the loss the GD planner minimises is values.sum(), so grad = d values.sum() / d pred =
d values[b] / d pred[b] row by row -- COMPLETE: the library scales nothing behind it.  With want_grad False (the sampling
planners) grad is None and need not be computed.  context is whatever the caller hands the planner.

  quadratic_cost(targets, step_weights)       a tracked target per step, seeds on every step
  keep_out_cost(center, radius, weight)       a smooth penalty, on every step, for particles inside a disc of the world plane
  cloud_divergence_cost(engine, target, ...)  Sinkhorn divergence of the final state to a target cloud: a density-aware goal
  cloud_chamfer_cost(engine, target, ...)     symmetric Chamfer distance of the final state to a target cloud
  sum_costs(*costs)                           the sum of costs
  torch_cost(fn)                              a cost written in torch -- fn(pred_tensor, context) -> [B] tensor -- through autograd

The cost runs on the host between two device calls; the rollout, the reverse pass behind the seed, Adam and the sampling
planners' updates stay on the device."""
import numpy as np


def _pred(pred):
    pred = np.asarray(pred)
    if pred.ndim != 4 or pred.shape[-1] != 3:
        raise ValueError('pred must be [B, H, N, 3], got %s' % (pred.shape,))
    if pred.dtype not in (np.float32, np.float64):
        pred = pred.astype(np.float64)
    return pred


def quadratic_cost(targets, step_weights=None):
    """values[b] = sum_t w_t mean_n |pred[b, t, n] - targets[t, n]|^2: targets [H, N, 3] (or [B, H, N, 3], a target per row),
    step_weights [H] (default: 1 on every step).  Its gradient is non-zero on every step whose weight is."""
    targets = np.asarray(targets, np.float64)

    def cost(pred, context=None, want_grad=True):
        pred = _pred(pred)
        dt = pred.dtype
        B, H, N, _ = pred.shape
        tg = targets.astype(dt)
        if tg.shape not in ((H, N, 3), (B, H, N, 3)):
            raise ValueError('targets %s against pred %s' % (tg.shape, pred.shape))
        w = np.ones((H,), dt) if step_weights is None else np.asarray(step_weights, dt).reshape(H)
        d = pred - tg
        scale = (w / dt.type(N)).reshape(1, H, 1, 1)
        values = (scale * d * d).sum(axis=(1, 2, 3))
        return values, ((2 * scale) * d).astype(dt, copy=False) if want_grad else None
    return cost


def keep_out_cost(center, radius, weight=1.0, world2cam=None, global_scale=1.0):
    """values[b] = weight * sum_t sum_n relu(1 - |x_n - center|^2 / radius^2)^2, x_n the particle's two coordinates in the world
    plane: zero with a zero gradient at the disc's edge and outside, smooth inside.  center [2] and radius are in world units.
    The predicted states are in the camera frame (s = (M [x, 0, -y, 1]) / global_scale, planners.py's gen_s_delta): world2cam
    [3, 4] and global_scale map them back -- the plane's two axes are columns 0 and 2 of M, orthonormal for a camera pose --;
    without world2cam the first two coordinates of pred are taken as they are."""
    center = np.asarray(center, np.float64).reshape(2)
    if not radius > 0:
        raise ValueError('radius must be positive, got %r' % (radius,))
    if world2cam is None:
        A = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
        off = np.zeros(2)
    else:
        M = np.asarray(world2cam, np.float64).reshape(3, 4)
        # x_world = M[:, 0] . (gs s - M[:, 3]),  y_world = -M[:, 2] . (gs s - M[:, 3])
        A = np.stack([M[:, 0], -M[:, 2]]) * float(global_scale)
        off = np.stack([M[:, 0], -M[:, 2]]) @ M[:, 3]

    def cost(pred, context=None, want_grad=True):
        pred = _pred(pred)
        dt = pred.dtype
        Ad, r2 = A.astype(dt), dt.type(radius * radius)
        xy = pred @ Ad.T - (off + center).astype(dt)                     # [B, H, N, 2]
        q = np.maximum(dt.type(1) - (xy * xy).sum(-1) / r2, dt.type(0))  # [B, H, N]
        values = dt.type(weight) * (q * q).sum(axis=(1, 2))
        if not want_grad:
            return values, None
        g_xy = (dt.type(-4 * weight) / r2) * q[..., None] * xy
        return values, (g_xy @ Ad).astype(dt, copy=False)
    return cost


def cloud_divergence_cost(engine, target, n_target=None, eps_scale=1.0, iters=50):
    """values[b] = Engine.cloud_divergence(pred[b, H-1], target): the Sinkhorn divergence of the FINAL predicted state to a
    target cloud [M, 3] (or [B, M, 3]; n_target: how many of its rows are points), zero only when the pile lies on the target
    -- a goal that knows how much material belongs where.  eps = eps_scale / context['dens'] (a number, or one per start column
    [n_batch]: 1 / dens is the squared sampling spacing, so eps_scale 1 blurs the plan over one spacing); without a context eps =
    eps_scale.  A float64
    pred goes through cloud_divergence_f64.  The gradient is non-zero on the final step only."""
    target = np.asarray(target, np.float32)

    def cost(pred, context=None, want_grad=True):
        pred = _pred(pred)
        B, H, N, _ = pred.shape
        q = np.broadcast_to(target if target.ndim == 3 else target[None], (B,) + target.shape[-2:])
        q = np.ascontiguousarray(q)
        n_q = None if n_target is None else np.broadcast_to(np.asarray(n_target, np.int32), (B,)).copy()
        dens = None if context is None else context.get('dens') if hasattr(context, 'get') else None
        # dens per start column [nb]: row = trajectory * nb + column, so the rows cycle through it
        eps = float(eps_scale) / np.resize(np.asarray(1.0 if dens is None else dens, np.float64), B)
        call = engine.cloud_divergence_f64 if pred.dtype == np.float64 else engine.cloud_divergence
        out = call(np.ascontiguousarray(pred[:, H - 1]), q, None, n_q, eps=eps, iters=int(iters), want_grad=want_grad)
        values = np.asarray(out['divergence']).astype(pred.dtype)
        if not want_grad:
            return values, None
        grad = np.zeros_like(pred)
        grad[:, H - 1] = out['grad']
        return values, grad
    return cost


def cloud_chamfer_cost(engine, target, n_target=None, weight=1.0):
    """values[b] = weight * Engine.cloud_chamfer(pred[b, H-1], target)['fwd' + 'bwd']: the symmetric squared Chamfer distance of
    the FINAL predicted state to a target cloud [M, 3] (or [B, M, 3]; n_target: how many of its rows are points) -- the host
    twin of the device-resident cloud goal (Engine.set_goal_cloud(kind='chamfer'), the counterpart of cloud_divergence_cost):
    on a float32 pred its values are that goal's numbers (the product with the weight formed in float64 and rounded once).  Its
    gradient is weight x the one-shot's fp32 gradient, formed in float64 and rounded again: the goal's kernel rounds weight x the
    double expression ONCE, so the two are the same numbers for a weight that is a power of two and may differ in the last place
    otherwise.  A float64 pred goes through cloud_chamfer_f64 (float64 gradient).  The gradient is non-zero on the final
    step only."""
    target = np.asarray(target, np.float32)
    w = np.float64(weight)

    def cost(pred, context=None, want_grad=True):
        pred = _pred(pred)
        B, H, N, _ = pred.shape
        q = np.broadcast_to(target if target.ndim == 3 else target[None], (B,) + target.shape[-2:])
        q = np.ascontiguousarray(q)
        n_q = None if n_target is None else np.broadcast_to(np.asarray(n_target, np.int32), (B,)).copy()
        call = engine.cloud_chamfer_f64 if pred.dtype == np.float64 else engine.cloud_chamfer
        out = call(np.ascontiguousarray(pred[:, H - 1], np.float32), q, None, n_q, want_grad=want_grad)
        values = (w * (np.asarray(out['fwd'], np.float64) + np.asarray(out['bwd'], np.float64))).astype(pred.dtype)
        if not want_grad:
            return values, None
        grad = np.zeros_like(pred)
        grad[:, H - 1] = (w * np.asarray(out['grad'], np.float64)).astype(pred.dtype)
        return values, grad
    return cost


def sum_costs(*costs):
    """the sum of costs: values and gradients added in the order given"""
    if not costs:
        raise ValueError('sum_costs needs at least one cost')

    def cost(pred, context=None, want_grad=True):
        values, grad = costs[0](pred, context, want_grad)
        for c in costs[1:]:
            v, g = c(pred, context, want_grad)
            values = values + v
            if want_grad:
                grad = grad + g
        return values, grad
    return cost


def torch_cost(fn, device='cpu'):
    """fn(pred, context) -> [B] tensor, written in torch, as a cost: pred becomes a leaf tensor of the array's dtype on `device`,
    the values are fn's, the gradient pred.grad after values.sum().backward() (zeros where fn does not depend on pred)."""
    import torch

    def cost(pred, context=None, want_grad=True):
        pred = np.ascontiguousarray(_pred(pred))
        leaf = torch.from_numpy(pred.copy()).to(device).requires_grad_(bool(want_grad))
        values = fn(leaf, context)
        if values.dim() != 1 or values.shape[0] != pred.shape[0]:
            raise ValueError('a torch cost must return one value per row [%d], got shape %s' % (pred.shape[0], tuple(values.shape)))
        out = values.detach().cpu().numpy().astype(pred.dtype, copy=False)
        if not want_grad:
            return out, None
        values.sum().backward()
        grad = torch.zeros_like(leaf) if leaf.grad is None else leaf.grad
        return out, grad.detach().cpu().numpy().astype(pred.dtype, copy=False)
    return cost


def check_cost_output(values, grad, shape, want_grad):
    """what a planner checks of a cost's answer before it reaches the device: values [B], grad [B, H, N, 3] when asked for"""
    values = np.asarray(values)
    if values.shape != (shape[0],):
        raise ValueError('the cost returned values of shape %s, expected (%d,)' % (values.shape, shape[0]))
    if want_grad:
        if grad is None or np.asarray(grad).shape != tuple(shape):
            raise ValueError('the cost returned a gradient of shape %s, expected %s'
                             % (None if grad is None else np.asarray(grad).shape, tuple(shape)))
    return values

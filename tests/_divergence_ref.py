"""TEST INFRASTRUCTURE of the Sinkhorn divergence (drp_cloud_divergence, drp_train_step_divergence; csrc/k_sinkhorn.h):
include/drp.h's definition in numpy float64, operation for operation, on tests/_transport_ref.py's sweeps and plan and
tests/_match_ref.py's fp32 cost.  The terms of every sum are added in ascending index.

  self64(x, eps, K)                the self problem of one cloud -> (h, S, C, d): K averaged Jacobi sweeps from h = 0, the symmetric
                                   plan, the cost matrix and the differences x_i - x_j it was formed from
  pair64(p, q, eps, K, scale)      one pair of real rows -> (value, gradient, f, g, h_p, h_q, col_err, self_err [2])
  divergence64(p, q, n_p, n_q, eps, K)    a padded batch
  train_divergence64(...)          the trainer's loss and weight gradients, shaped like _transport_ref.train_transport64

The device adds the same terms in another fixed order; every other operation is the same IEEE double operation
in the same order, and exp and log are each library's own."""
import numpy as np

import _transport_ref as T
from _match_ref import cost32


GRID_SPACING = 0.02


def grid_cloud(n, seed, shift=(0.0, 0.0, 0.0)):
    """the first n points of a square grid of spacing 0.02 in a plane, every coordinate moved by 0.002 x a standard normal draw
    -> [n, 3] float32: a pile's layer at the trainer's default eps = 0.02^2"""
    side = int(np.ceil(np.sqrt(n)))
    ij = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing='ij'), -1).reshape(-1, 2)[:n]
    x = np.concatenate([0.2 + GRID_SPACING * ij, np.full((n, 1), 0.5)], axis=1)
    return (x + 0.1 * GRID_SPACING * np.random.default_rng(seed).standard_normal((n, 3)) + np.asarray(shift)).astype(np.float32)


def _sum_asc(v):
    s = 0.0
    for x in np.asarray(v, np.float64).ravel():
        s += float(x)
    return s


def _rows_asc(X):
    """sum over axis 1 of X [n, m(, 3)], the terms added in ascending index"""
    s = np.zeros(X.shape[:1] + X.shape[2:])
    for j in range(X.shape[1]):
        s += X[:, j]
    return s


def _cost_and_diff(a, b, wide):
    """-> (C [n, m] float64, d [n, m, 3] float64 = a_i - b_j): the kernel's fp32 cost and fp32 differences widened, or with `wide`
    everything in float64 (central differences move a float64 point)"""
    if not wide:
        a32, b32 = np.asarray(a, np.float32), np.asarray(b, np.float32)
        return cost32(a32, b32).astype(np.float64), (a32[:, None, :] - b32[None, :, :]).astype(np.float64)
    d = np.asarray(a, np.float64)[:, None, :] - np.asarray(b, np.float64)[None, :, :]
    return d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2], d


def self64(x, eps, K, wide=False):
    C, d = _cost_and_diff(x, x, wide)
    n = C.shape[0]
    log_m = np.log(1.0 / n)
    h = np.zeros(n)
    for _ in range(int(K)):
        h = 0.5 * (h + (-eps * T._lse_rows((h[:, None] - C) / eps + log_m)))       # every h on the right: the previous sweep's
    S = ((1.0 / n) * (1.0 / n)) * np.exp((h[:, None] + h[None, :] - C) / eps)
    return h, S, C, d


def self_err64(S):
    return _sum_asc(np.abs(_rows_asc(S) - 1.0 / S.shape[0]))


def pair64(p, q, eps, K, scale=1.0, p64=None, want_plans=False):
    """one pair of real rows -> (value, grad [n, 3] float64 before the fp32 rounding, f, g, h_p, h_q, col_err, self_err [2])[+ (P,
    S_p)].  p64: the point the value is differentiated at where it is not the float32 p (central differences): costs and
    differences are then float64 throughout"""
    wide = p64 is not None
    pp = p64 if wide else p
    C, d = _cost_and_diff(pp, q, wide)
    n, m = C.shape
    f, g = T.sinkhorn64(C, eps, K)
    P = T.plan64(C, f, g, eps)
    h_p, S_p, _, d_pp = self64(pp, eps, K, wide)
    h_q, S_q, _, _ = self64(q, eps, K, wide)
    a, b = 1.0 / n, 1.0 / m
    cross = _sum_asc(np.concatenate([a * f, b * g]))
    value = scale * ((cross - _sum_asc(a * h_p) - _sum_asc(b * h_q)) / 3.0)
    grad = (2.0 * scale / 3.0) * (_rows_asc(P[:, :, None] * d) - _rows_asc(S_p[:, :, None] * d_pp))
    out = (value, grad, f, g, h_p, h_q, T.col_err64(P), np.array([self_err64(S_p), self_err64(S_q)]))
    return out + (P, S_p) if want_plans else out


def divergence64(p, q, n_p, n_q, eps, K, scale=1.0):
    """p [B, N, 3], q [B, M, 3] float32 with n_p, n_q real rows, eps a number or [B] -> {'divergence' [B], 'grad' [B, N, 3] float64
    (+0.0 on padding), 'f', 'h_p' [B, N], 'g', 'h_q' [B, M] (0 on padding), 'col_err' [B], 'self_err' [B, 2]}"""
    p, q = np.asarray(p, np.float32), np.asarray(q, np.float32)
    B, N, M = p.shape[0], p.shape[1], q.shape[1]
    eps = np.broadcast_to(np.asarray(eps, np.float64).reshape(-1), (B,))
    out = {'divergence': np.zeros(B), 'grad': np.zeros((B, N, 3)), 'f': np.zeros((B, N)), 'g': np.zeros((B, M)),
           'h_p': np.zeros((B, N)), 'h_q': np.zeros((B, M)), 'col_err': np.zeros(B), 'self_err': np.zeros((B, 2))}
    for b in range(B):
        n, m = int(n_p[b]), int(n_q[b])
        value, grad, f, g, h_p, h_q, ce, se = pair64(p[b, :n], q[b, :m], float(eps[b]), K, scale)
        out['divergence'][b], out['col_err'][b], out['self_err'][b] = value, ce, se
        out['grad'][b, :n], out['f'][b, :n], out['g'][b, :m], out['h_p'][b, :n], out['h_q'][b, :m] = grad, f, g, h_p, h_q
    return out


# ---- the trainer ---------------------------------------------------------------------------------------------------------
def train_divergence64(W, states, states_delta, attrs, particle_nums, particle_dens, targets, target_nums, plans, actions=None,
                       adj_thresh=0.08):
    """_transport_ref.train_transport64's loop with the term of (step t, sample b) replaced by the divergence.  plans[t][b] = (P
    [n_b, m_bt], S [n_b, n_b], value): what is differentiated is the surrogate (sum_ij P_ij |p_i - q_j|^2 - sum_ij S_ij |p_i -
    p_j|^2 / 2) / (3 n_rollout B) with P and S constants -- its derivative is the kernel's gradient -- and what is reported is
    value / (n_rollout B), from the duals -> (loss, terms [H, B], {key: gradient}, d loss / d predicted states [B, H, N, 3])"""
    import torch
    from oracle.propnet_dense import adjacency
    from _f64_grad_ref import _d, step, weights64
    from _f64_train_ref import PARAMS
    W = dict((k, v.clone().requires_grad_(True)) for k, v in weights64(W).items())
    st, at, dens = _d(states), _d(attrs), _d(particle_dens)
    if actions is None:
        sd_all = _d(states_delta)
    else:
        import _train_actions_ref as A
        ac = _d(actions)
    tg = _d(targets)
    nums = [int(n) for n in np.asarray(particle_nums)]
    tnums = np.asarray(target_nums)
    B, T1, N, _ = st.shape
    H = T1 - 1
    s_cur, a_cur = st[:, 0], at[:, 0]
    terms, preds = [], []
    for t in range(H):
        sd = sd_all[:, t] if actions is None else A.impulses64(s_cur, ac[:, t], nums)
        adj, _ = adjacency(s_cur.detach().float(), sd.detach().float(), adj_thresh)
        s_pred = step(W, a_cur, s_cur, sd, dens, adj.double())
        s_pred.retain_grad()
        preds.append(s_pred)
        row = []
        for b in range(B):
            n, m = nums[b], int(tnums[b, t])
            P, S, value = plans[t][b]
            d = s_pred[b, :n, None, :] - tg[b, t, None, :m, :]
            dd = s_pred[b, :n, None, :] - s_pred[b, None, :n, :]
            sur = ((torch.from_numpy(np.asarray(P, np.float64)) * (d ** 2).sum(-1)).sum()
                   - 0.5 * (torch.from_numpy(np.asarray(S, np.float64)) * (dd ** 2).sum(-1)).sum()) / 3.0
            row.append((sur - sur.detach() + float(value)) / (H * B))
        terms.append(torch.stack(row))
        s_cur = s_pred
    terms = torch.stack(terms)
    loss = terms.sum()
    loss.backward()
    grads = dict((k, W[k].grad.numpy().copy()) for k in PARAMS)
    g_state = np.stack([p.grad.numpy() if p.grad is not None else np.zeros((B, N, 3)) for p in preds], 1)
    return float(loss.item()), terms.detach().numpy(), grads, g_state
